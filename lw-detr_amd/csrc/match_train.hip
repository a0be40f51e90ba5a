// Training criterion for gfx950: the reference's SetCriterion in train() mode (models/lwdetr.py:218-506, models/matcher.py:50-111) -
// grouped Hungarian matching, the four classification loss forms, and the gradient with respect to the logits and boxes.
//   * match_assign_groups_kernel : the solver of match.hip (match_shared.h: lsa_lane_*) with one WAVE per (layer, image, group): the group
//                                  g of G solves the T_b targets of its image against the column slice [g nq/G, (g+1) nq/G) of the
//                                  target-major cost that match_cost_kernel wrote (the cost of a pair does not depend on the group).
//                                  The same fixed trip counts, hence the same guarantee on non-finite costs; pairs (layers, G, sumT).
//   * train_partials_kernel      : criterion_partials_kernel of match.hip with groups and four forms. A chunk of 32 queries rebuilds its
//                                  (b, q) -> target map from the pairs of the groups that overlap it. The position-supervised form needs
//                                  the image's largest matched IoU (lwdetr.py:309-310): every block of the image takes it over all
//                                  G T_b pairs in the same pass (a maximum does not depend on the order, so every block gets the same bits).
//   * train_finish_kernel        : the fixed-order f64 reduction; class_error over the G sumT matched rows, cardinality against T_b.
//   * train_backward_kernel      : one launch for all layers, the grid of the partials kernel: every block rebuilds its chunk's map, then
//                                  writes d loss / d logit for every (query, class) of the chunk and d loss / d box for every query of the
//                                  chunk (zero for unmatched queries). Each element is written exactly once by exactly one thread: no atomics.
//                                  The upstream gradient (layers, 5) is read on the device; 1 / num_boxes and mean(1) * nq are applied here.
// The per-element and per-pair derivatives (tr_elem, tr_pair) are __host__ __device__: lwdetr_criterion_grad_host runs them on host arrays.
//
// What is differentiated is the reference's graph: the IoU targets and IA-BCE's t are constants (detached, lwdetr.py:273-275, :285,
// :297-299, :318-320); the modulating weights are not. Rules at the kinks, torch's: d|x|/dx = sign(x) with sign(0) = 0; clamp(min = 0)
// passes the gradient where its argument is >= 0; max(a, b) / min(a, b) give all of it to the selected operand and half to each on a tie.
#include "match_shared.h"

namespace {

enum { TR_FOCAL = 0, TR_IABCE = 1, TR_VARIFOCAL = 2, TR_POSSUP = 3 };

struct GradLayers {
    void* logits[LWDETR_CRIT_MAX_LAYERS];
    void* boxes[LWDETR_CRIT_MAX_LAYERS];
};

LSA_HD float tr_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// One (query, class) term of loss_ce before the 1 / num_boxes scale, and (GRAD) its derivative with respect to the logit x.
// hit: the query is matched and the class is its target's label. tv (used when hit): forms 1, 2 the matched IoU, form 3 the matched IoU
// over the image's normaliser. The loss expressions of forms 0 and 1 are those of criterion_partials_kernel, token by token.
template <int FORM, bool GRAD> LSA_HD float tr_elem(float x, bool hit, float tv, float alpha, float& dx) {
    const float prob = tr_sigmoid(x);
    float loss;
    if (FORM == TR_FOCAL) {                                      // sigmoid_focal_loss, lwdetr.py:474-481, target one-hot of the matched label
        const float t = hit ? 1.f : 0.f;
        const float ce = (1.f - t) * x + fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x)));
        const float p_t = prob * t + (1.f - prob) * (1.f - t);
        const float omp = 1.f - p_t;
        loss = ce * (omp * omp);
        loss = (alpha * t + (1.f - alpha) * (1.f - t)) * loss;
        if (GRAD) {                                              // d ce = prob - t; d (1 - p_t) = -+ prob (1 - prob)
            const float ds = prob * (1.f - prob);
            const float dm = hit ? -ds : ds;
            dx = (alpha * t + (1.f - alpha) * (1.f - t)) * ((prob - t) * (omp * omp) + ce * (2.f * omp * dm));
        }
    } else if (FORM == TR_IABCE) {                               // IA-BCE, lwdetr.py:276-289
        float pw = 0.f, nw = prob * prob;
        if (hit) {
            const float tt = fmaxf(powf(prob, alpha) * powf(tv, 1.f - alpha), 0.01f);
            pw = tt;
            nw = 1.f - tt;
        }
        loss = -pw * logf(prob) - nw * logf(1.f - prob);
        if (GRAD) {                                              // t is detached (:285); neg_weights = prob ** 2 elsewhere is not
            if (hit) dx = nw * prob - pw * (1.f - prob);
            else dx = prob * prob * prob - 2.f * (prob * prob) * (1.f - prob) * logf(1.f - prob);
        }
    } else if (FORM == TR_VARIFOCAL) {                           // sigmoid_varifocal_loss, lwdetr.py:486-494, target = matched IoU at the label
        const float t = hit ? tv : 0.f;
        const float ce = (1.f - t) * x + fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x)));
        const bool posi = t > 0.f;
        const float d = prob - t;
        const float fw = posi ? t : (1.f - alpha) * (d * d);
        loss = ce * fw;
        if (GRAD) dx = posi ? t * d : d * fw + ce * ((1.f - alpha) * 2.f * d * (prob * (1.f - prob)));
    } else {                                                     // position_supervised_loss, lwdetr.py:497-506, target = IoU / image maximum
        const float t = hit ? tv : 0.f;
        const float ce = (1.f - t) * x + fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x)));
        const float d = t - prob;
        loss = ce * (d * d);
        const float at = t > 0.f ? alpha : 1.f - alpha;
        loss = at * loss;
        if (GRAD) dx = at * ((prob - t) * (d * d) + ce * (2.f * (prob - t) * (prob * (1.f - prob))));
    }
    return loss;
}

LSA_HD float tr_sign(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }
LSA_HD float tr_wgt(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }      // share of a in max(a, b)
LSA_HD float tr_wlt(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }      // share of a in min(a, b)

// A matched pair: IoU, sum |o - t| (lwdetr.py:371-374) and 1 - GIoU (:376-379) exactly as criterion_partials_kernel computes them, and (GRAD)
// d (g_l1 * l1 + g_gl * (1 - giou)) / d o through box_cxcywh_to_xyxy, box_iou and the enclosing box (util/box_ops.py:21-25, :36-73).
template <bool GRAD>
LSA_HD void tr_pair(const float* o, const float* t, float& iou, float& l1, float& gl, float g_l1, float g_gl, float* d) {
    const Xyxy a = cxcywh_to_xyxy(o[0], o[1], o[2], o[3]), b = cxcywh_to_xyxy(t[0], t[1], t[2], t[3]);
    float giou;
    box_iou_giou(a, b, iou, giou);
    l1 = fabsf(o[0] - t[0]) + fabsf(o[1] - t[1]) + fabsf(o[2] - t[2]) + fabsf(o[3] - t[3]);
    gl = 1.f - giou;
    if (!GRAD) return;
    const float aw = a.x1 - a.x0, ah = a.y1 - a.y0;
    const float area2 = (b.x1 - b.x0) * (b.y1 - b.y0);
    const float iwr = fminf(a.x1, b.x1) - fmaxf(a.x0, b.x0), ihr = fminf(a.y1, b.y1) - fmaxf(a.y0, b.y0);
    const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
    const float inter = iw * ih;
    const float uni = aw * ah + area2 - inter;
    const float ewr = fmaxf(a.x1, b.x1) - fminf(a.x0, b.x0), ehr = fmaxf(a.y1, b.y1) - fminf(a.y0, b.y0);
    const float ew = fmaxf(ewr, 0.f), eh = fmaxf(ehr, 0.f);
    const float area = ew * eh;
    const float g = -g_gl;                                       // d / d giou; giou = inter / uni - (area - uni) / area
    const float g_uni = g * (1.f / area - inter / (uni * uni));
    const float g_inter = g / uni - g_uni;                       // uni = area1 + area2 - inter
    const float g_area = -g * uni / (area * area);
    const float g_iw = iwr >= 0.f ? g_inter * ih : 0.f, g_ih = ihr >= 0.f ? g_inter * iw : 0.f;
    const float g_ew = ewr >= 0.f ? g_area * eh : 0.f, g_eh = ehr >= 0.f ? g_area * ew : 0.f;
    const float gx1 = g_iw * tr_wlt(a.x1, b.x1) + g_ew * tr_wgt(a.x1, b.x1) + g_uni * ah;
    const float gx0 = -(g_iw * tr_wgt(a.x0, b.x0)) - g_ew * tr_wlt(a.x0, b.x0) - g_uni * ah;
    const float gy1 = g_ih * tr_wlt(a.y1, b.y1) + g_eh * tr_wgt(a.y1, b.y1) + g_uni * aw;
    const float gy0 = -(g_ih * tr_wgt(a.y0, b.y0)) - g_eh * tr_wlt(a.y0, b.y0) - g_uni * aw;
    d[0] = gx0 + gx1 + g_l1 * tr_sign(o[0] - t[0]);
    d[1] = gy0 + gy1 + g_l1 * tr_sign(o[1] - t[1]);
    d[2] = (o[2] >= 0.f ? 0.5f * (gx1 - gx0) : 0.f) + g_l1 * tr_sign(o[2] - t[2]);
    d[3] = (o[3] >= 0.f ? 0.5f * (gy1 - gy0) : 0.f) + g_l1 * tr_sign(o[3] - t[3]);
}

// the scale of every loss_ce term: forms 0, 2, 3 are loss.mean(1).sum() / num_boxes * nq, form 1 is loss.sum() / num_boxes
LSA_HD float tr_ce_scale(int form, float up, int nq, float num_boxes) {
    return form == TR_IABCE ? up / num_boxes : up / (float)nq / num_boxes * (float)nq;
}

// =========================================================== grouped assignment ==========================================================
// prob = (layer * B + b) * G + g. The body is match_assign_kernel's on the column slice of group g; gw = nq / G columns.
template <int KPL>
__global__ __launch_bounds__(256) void match_assign_groups_kernel(const float* __restrict__ cost, const int32_t* __restrict__ offsets,
                                                                  int nlayers, int B, int nq, int G, int sumT, int maxT,
                                                                  int64_t* __restrict__ idx_q, int64_t* __restrict__ idx_t,
                                                                  int32_t* __restrict__ status, int32_t* __restrict__ steps) {
    extern __shared__ double lsa_smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int prob = blockIdx.x * (blockDim.x >> 6) + wave;
    if (prob >= nlayers * B * G) return;                         // whole waves leave; the kernel has no barrier
    const int lb = prob / G, grp = prob - lb * G;
    const int layer = lb / B, b = lb - layer * B;
    const int gw = nq / G;
    const int off = offsets[b], T = offsets[b + 1] - off;
    if (off < 0 || T < 0 || T > maxT || T > gw || (long)off + T > sumT) {      // offsets and the host's counts disagree: touch nothing
        if (lane == 0) { status[prob] = 2; if (steps) steps[prob] = 0; }
        return;
    }
    constexpr int NQP = KPL * LSA_WAVE;
    const int tpad = lsa_even(maxT);
    char* base = (char*)lsa_smem + (size_t)wave * ((size_t)tpad * 12 + (size_t)NQP * 8);
    volatile double* u = (volatile double*)base;
    volatile int* col4row = (volatile int*)(base + (size_t)tpad * 8);
    volatile int* path = col4row + tpad;
    volatile int* row4col = path + NQP;
    for (int i = lane; i < T; i += LSA_WAVE) { u[i] = 0.0; col4row[i] = -1; }
#pragma unroll
    for (int k = 0; k < KPL; ++k) { path[lane + LSA_WAVE * k] = -1; row4col[lane + LSA_WAVE * k] = -1; }

    LsaLane<KPL> s;
    lsa_lane_init(s);
    const float* cbase = cost + ((size_t)layer * sumT + off) * nq + (size_t)grp * gw;      // row stride nq, gw columns from here
    int nsteps = 0, bad = 0;
    for (int cur = 0; cur < T; ++cur) {
        lsa_lane_reset(s);
        double minv = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step <= cur && sink < 0; ++step) {
            const double ui = u[i];
            double best;
            int bestj;
            lsa_lane_scan(s, lane, gw, cbase + (size_t)i * nq, ui, minv, i, path, best, bestj, bad);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const double ob = __shfl_xor(best, m);
                const int oj = __shfl_xor(bestj, m);
                if (lsa_better(ob, oj, best, bestj)) { best = ob; bestj = oj; }
            }
            ++nsteps;
            minv = best;
            if (!(fabs(minv) <= DBL_MAX)) bad = 1;
            const int jsel = __builtin_amdgcn_readfirstlane(bestj);
            if (jsel >= gw) { bad = 1; break; }                  // unreachable: T <= gw leaves an unvisited column at every step
            lsa_lane_select(s, lane, jsel, i, path);
            const int r = row4col[jsel];
            if (r < 0) sink = jsel; else i = r;
        }
        if (sink < 0) { bad = 1; break; }                        // unreachable (see the head of match.hip)
        if (lane == 0) u[cur] = u[cur] + minv;
        lsa_lane_dual(s, lane, minv, row4col, u);
        int j = sink;
        for (int n = 0; n <= cur; ++n) {                         // flip the alternating path back to the root `cur`
            const int ii = path[j];
            if (ii < 0 || ii >= T) { bad = 1; break; }
            const int jn = col4row[ii];
            if (lane == 0) { row4col[j] = ii; col4row[ii] = j; }
            if (ii == cur || jn < 0) break;
            j = jn;
        }
    }
    // pairs in ascending query order inside the group, query indices offset by g * gw (matcher.py:104-110)
    const size_t obase = ((size_t)layer * G + grp) * sumT + off;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < KPL; ++k) {
        const int j = lane + LSA_WAVE * k;
        const int r = j < gw ? row4col[j] : -1;
        const bool has = r >= 0;
        const unsigned long long m = __ballot(has);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (has && cnt + pre < T) { idx_q[obase + cnt + pre] = (int64_t)grp * gw + j; idx_t[obase + cnt + pre] = r; }
        cnt += __popcll(m);
    }
    const int anybad = __any(bad);
    if (lane == 0) { status[prob] = anybad ? 1 : 0; if (steps) steps[prob] = nsteps; }
}

// =========================================================== the chunk's map =============================================================
// s_tgt[r] = packed target of query q0 + r or -1, s_iou[r] = its IoU with that target. Returns the image's largest matched IoU over all
// groups (form 3; 0 otherwise). Pairs of the groups that overlap the chunk are read (all groups for form 3). All 256 threads call it.
template <typename T, int FORM>
__device__ __forceinline__ float tr_build_map(const T* __restrict__ bx, const float* __restrict__ tboxes, const int64_t* __restrict__ idx_q,
                                              const int64_t* __restrict__ idx_t, int layer, int b, int nq, int q0, int nqc, int off, int Tb,
                                              int sumT, int G, int gw, int* s_tgt, float* s_iou, float* s_wmax) {
    const int tid = threadIdx.x;
    if (tid < CR_QCH) { s_tgt[tid] = -1; s_iou[tid] = 0.f; }
    __syncthreads();
    int g_lo = 0, g_hi = G - 1;
    if (FORM != TR_POSSUP) { g_lo = q0 / gw; g_hi = min((q0 + nqc - 1) / gw, G - 1); }
    const int npair = (g_hi - g_lo + 1) * Tb;
    float mx = 0.f;
    for (int p = tid; p < npair; p += CR_THREADS) {
        const int gi = p / Tb, pp = p - gi * Tb;
        const size_t at = ((size_t)layer * G + g_lo + gi) * sumT + off + pp;
        const long q = idx_q[at], t = idx_t[at];
        if (q < 0 || q >= nq || t < 0 || t >= Tb) continue;
        const bool mine = q >= q0 && q < q0 + nqc;
        if (FORM != TR_POSSUP && !mine) continue;
        const int g = off + (int)t;
        const size_t row = (size_t)b * nq + q;
        const float ocx = to_f32<T>(bx[row * 4 + 0]), ocy = to_f32<T>(bx[row * 4 + 1]), ow = to_f32<T>(bx[row * 4 + 2]),
                    oh = to_f32<T>(bx[row * 4 + 3]);
        const float tcx = tboxes[(size_t)g * 4 + 0], tcy = tboxes[(size_t)g * 4 + 1], tw = tboxes[(size_t)g * 4 + 2],
                    th = tboxes[(size_t)g * 4 + 3];
        float iou, giou;
        box_iou_giou(cxcywh_to_xyxy(ocx, ocy, ow, oh), cxcywh_to_xyxy(tcx, tcy, tw, th), iou, giou);
        if (FORM == TR_POSSUP) mx = fmaxf(mx, iou);
        if (mine) { s_tgt[(int)q - q0] = g; s_iou[(int)q - q0] = iou; }
    }
    if (FORM == TR_POSSUP) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
        if ((tid & 63) == 0) s_wmax[tid >> 6] = mx;
    }
    __syncthreads();
    if (FORM == TR_POSSUP) return fmaxf(fmaxf(s_wmax[0], s_wmax[1]), fmaxf(s_wmax[2], s_wmax[3]));
    return 0.f;
}

// =========================================================== losses ======================================================================
// grid (ceil(nq / 32), B, layers), 256 threads. partials as in match.hip: [((layer * B + b) * nchunks + chunk) * 5 + {ce, l1, 1 - giou, card, correct}]
template <typename T, int FORM>
__global__ __launch_bounds__(CR_THREADS) void train_partials_kernel(CritLayers L, int B, int nq, int C, const int64_t* __restrict__ labels,
                                                                    const float* __restrict__ tboxes, const int32_t* __restrict__ offsets,
                                                                    int sumT, const int64_t* __restrict__ idx_q,
                                                                    const int64_t* __restrict__ idx_t, int G, float alpha,
                                                                    float* __restrict__ partials) {
    __shared__ int s_tgt[CR_QCH];
    __shared__ float s_iou[CR_QCH], s_l1[CR_QCH], s_gl[CR_QCH];
    __shared__ float s_red[CR_THREADS / 64][3];
    __shared__ float s_wmax[CR_THREADS / 64];
    const int chunk = blockIdx.x, b = blockIdx.y, layer = blockIdx.z, tid = threadIdx.x;
    const int q0 = chunk * CR_QCH, nqc = min(CR_QCH, nq - q0);
    const int off = offsets[b];
    int Tb = offsets[b + 1] - off;
    if (off < 0 || Tb < 0 || (long)off + Tb > sumT) Tb = 0;
    const T* lg = (const T*)L.logits[layer];
    const T* bx = (const T*)L.boxes[layer];
    const float mx = tr_build_map<T, FORM>(bx, tboxes, idx_q, idx_t, layer, b, nq, q0, nqc, off, Tb, sumT, G, nq / G, s_tgt, s_iou, s_wmax);
    if (tid < CR_QCH) {
        float l1 = 0.f, gl = 0.f;
        const int g = s_tgt[tid];
        if (g >= 0) {
            const size_t row = (size_t)b * nq + q0 + tid;
            const float o[4] = {to_f32<T>(bx[row * 4 + 0]), to_f32<T>(bx[row * 4 + 1]), to_f32<T>(bx[row * 4 + 2]), to_f32<T>(bx[row * 4 + 3])};
            const float t[4] = {tboxes[(size_t)g * 4 + 0], tboxes[(size_t)g * 4 + 1], tboxes[(size_t)g * 4 + 2], tboxes[(size_t)g * 4 + 3]};
            float iou;
            tr_pair<false>(o, t, iou, l1, gl, 0.f, 0.f, nullptr);
        }
        s_l1[tid] = l1;
        s_gl[tid] = gl;
    }
    const float norm = mx + 1e-8f;                               // lwdetr.py:310
    const int wave = tid >> 6, lane = tid & 63;
    float acc = 0.f, card = 0.f, correct = 0.f;
    for (int r = wave; r < nqc; r += CR_THREADS / 64) {
        const int g = s_tgt[r];
        long lab = -1;
        if (g >= 0) { lab = labels[g]; lab = lab < 0 ? 0 : (lab >= C ? C - 1 : lab); }
        const float iou = FORM == TR_POSSUP ? s_iou[r] / norm : s_iou[r];
        const T* xrow = lg + ((size_t)b * nq + q0 + r) * C;
        float bv = -INFINITY;
        int bc = INT_MAX;
        for (int c = lane; c < C; c += 64) {
            const float x = to_f32<T>(xrow[c]);
            if (x > bv) { bv = x; bc = c; }
            float unused;
            acc += tr_elem<FORM, false>(x, c == lab, iou, alpha, unused);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {                      // row arg-max, first index on ties
            const float ov = __shfl_xor(bv, m);
            const int oc = __shfl_xor(bc, m);
            if (ov > bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
        }
        if (lane == 0) {
            card += bc != C - 1 ? 1.f : 0.f;                     // lwdetr.py:356
            if (g >= 0) correct += bc == (int)lab ? 1.f : 0.f;   // util/misc.py accuracy, top-1
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if (lane == 0) { s_red[wave][0] = acc; s_red[wave][1] = card; s_red[wave][2] = correct; }
    __syncthreads();
    if (tid == 0) {
        float ce = 0.f, cd = 0.f, co = 0.f, l1 = 0.f, gl = 0.f;
        for (int w = 0; w < CR_THREADS / 64; ++w) { ce += s_red[w][0]; cd += s_red[w][1]; co += s_red[w][2]; }
        for (int r = 0; r < CR_QCH; ++r) { l1 += s_l1[r]; gl += s_gl[r]; }
        float* o = partials + (((size_t)layer * B + b) * gridDim.x + chunk) * CR_NPART;
        o[0] = ce; o[1] = l1; o[2] = gl; o[3] = cd; o[4] = co;
    }
}

// c - a * b with the product rounded to f32 first (see match.hip: class_error is compared exactly)
__device__ __forceinline__ float tr_sub_rounded_product(float c, float a, float b) {
#pragma clang fp contract(off)
    const float p = a * b;
    return c - p;
}

// grid (layers), one wave: criterion_finish_kernel of match.hip with `nmatch` = G * sumT matched rows behind class_error
__global__ __launch_bounds__(64) void train_finish_kernel(const float* __restrict__ partials, CritLayers L,
                                                          const int32_t* __restrict__ offsets, int B, int nq, int nchunks, long nmatch,
                                                          int loss_form, float num_boxes, float* __restrict__ out) {
    const int layer = blockIdx.x, lane = threadIdx.x;
    double ce = 0.0, l1 = 0.0, gl = 0.0, co = 0.0, cerr = 0.0;
    for (int b = lane; b < B; b += 64) {
        const float* p = partials + ((size_t)layer * B + b) * nchunks * CR_NPART;
        double card = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            ce += (double)p[c * CR_NPART + 0]; l1 += (double)p[c * CR_NPART + 1]; gl += (double)p[c * CR_NPART + 2];
            card += (double)p[c * CR_NPART + 3]; co += (double)p[c * CR_NPART + 4];
        }
        cerr += fabs(card - (double)(offsets[b + 1] - offsets[b]));      // lwdetr.py:354-357: all nq rows against T_b
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        ce += __shfl_xor(ce, m); l1 += __shfl_xor(l1, m); gl += __shfl_xor(gl, m); co += __shfl_xor(co, m); cerr += __shfl_xor(cerr, m);
    }
    if (lane != 0) return;
    const double nb = (double)num_boxes;
    float* o = out + (size_t)layer * 5;
    o[0] = loss_form != TR_IABCE ? (float)(ce / (double)nq / nb * (double)nq) : (float)(ce / nb);
    float cls_err = 0.f;
    if (L.class_error[layer]) cls_err = nmatch > 0 ? tr_sub_rounded_product(100.f, (float)co, (float)(100.0 / (double)nmatch)) : 100.f;    // lwdetr.py:344
    o[1] = cls_err;
    o[2] = (float)(l1 / nb);
    o[3] = (float)(gl / nb);
    o[4] = (float)cerr / (float)B;
}

// =========================================================== backward ====================================================================
// grid (ceil(nq / 32), B, layers), 256 threads; grad_out (layers, 5) f32 on the device = d L / d {loss_ce, class_error, loss_bbox, loss_giou, card}
template <typename T, int FORM>
__global__ __launch_bounds__(CR_THREADS) void train_backward_kernel(CritLayers L, GradLayers Gr, int B, int nq, int C,
                                                                    const int64_t* __restrict__ labels, const float* __restrict__ tboxes,
                                                                    const int32_t* __restrict__ offsets, int sumT,
                                                                    const int64_t* __restrict__ idx_q, const int64_t* __restrict__ idx_t, int G,
                                                                    float alpha, float num_boxes, const float* __restrict__ grad_out) {
    __shared__ int s_tgt[CR_QCH];
    __shared__ float s_iou[CR_QCH];
    __shared__ float s_wmax[CR_THREADS / 64];
    const int chunk = blockIdx.x, b = blockIdx.y, layer = blockIdx.z, tid = threadIdx.x;
    const int q0 = chunk * CR_QCH, nqc = min(CR_QCH, nq - q0);
    const int off = offsets[b];
    int Tb = offsets[b + 1] - off;
    if (off < 0 || Tb < 0 || (long)off + Tb > sumT) Tb = 0;
    const T* lg = (const T*)L.logits[layer];
    const T* bx = (const T*)L.boxes[layer];
    T* glg = (T*)Gr.logits[layer];
    T* gbx = (T*)Gr.boxes[layer];
    const float mx = tr_build_map<T, FORM>(bx, tboxes, idx_q, idx_t, layer, b, nq, q0, nqc, off, Tb, sumT, G, nq / G, s_tgt, s_iou, s_wmax);
    const float up_ce = tr_ce_scale(FORM, grad_out[layer * 5 + 0], nq, num_boxes);
    const float up_l1 = grad_out[layer * 5 + 2] / num_boxes, up_gl = grad_out[layer * 5 + 3] / num_boxes;
    if (tid < nqc) {                                             // the chunk's box rows: matched ones get the pair's gradient, the others zero
        const size_t row = (size_t)b * nq + q0 + tid;
        float d[4] = {0.f, 0.f, 0.f, 0.f};
        const int g = s_tgt[tid];
        if (g >= 0) {
            const float o[4] = {to_f32<T>(bx[row * 4 + 0]), to_f32<T>(bx[row * 4 + 1]), to_f32<T>(bx[row * 4 + 2]), to_f32<T>(bx[row * 4 + 3])};
            const float t[4] = {tboxes[(size_t)g * 4 + 0], tboxes[(size_t)g * 4 + 1], tboxes[(size_t)g * 4 + 2], tboxes[(size_t)g * 4 + 3]};
            float iou, l1, gl;
            tr_pair<true>(o, t, iou, l1, gl, up_l1, up_gl, d);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) gbx[row * 4 + k] = from_f32<T>(d[k]);
    }
    const float norm = mx + 1e-8f;
    const int wave = tid >> 6, lane = tid & 63;
    for (int r = wave; r < nqc; r += CR_THREADS / 64) {
        const int g = s_tgt[r];
        long lab = -1;
        if (g >= 0) { lab = labels[g]; lab = lab < 0 ? 0 : (lab >= C ? C - 1 : lab); }
        const float iou = FORM == TR_POSSUP ? s_iou[r] / norm : s_iou[r];
        const size_t base = ((size_t)b * nq + q0 + r) * C;
        for (int c = lane; c < C; c += 64) {
            float dx = 0.f;
            tr_elem<FORM, true>(to_f32<T>(lg[base + c]), c == lab, iou, alpha, dx);
            glg[base + c] = from_f32<T>(up_ce * dx);
        }
    }
}

template <int FORM>
void grad_host_rows(const float* logits, int nq, int C, const int64_t* labels, const int* tgt, const float* iou, float norm, float alpha,
                    float scale, float* grad_logits) {
    for (int q = 0; q < nq; ++q) {
        long lab = -1;
        if (tgt[q] >= 0) { lab = labels[tgt[q]]; lab = lab < 0 ? 0 : (lab >= C ? C - 1 : lab); }
        const float tv = FORM == TR_POSSUP ? iou[q] / norm : iou[q];
        for (int c = 0; c < C; ++c) {
            float dx = 0.f;
            tr_elem<FORM, true>(logits[(size_t)q * C + c], c == lab, tv, alpha, dx);
            grad_logits[(size_t)q * C + c] = scale * dx;
        }
    }
}

int pack_grads(const lwdetr_crit_layer* grads, int nlayers, GradLayers& Gr) {
    if (!grads) return LWDETR_ERR_BAD_ARG;
    for (int l = 0; l < LWDETR_CRIT_MAX_LAYERS; ++l) {
        const bool on = l < nlayers;
        if (on && (!grads[l].logits || !grads[l].boxes)) return LWDETR_ERR_BAD_ARG;
        Gr.logits[l] = on ? const_cast<void*>(grads[l].logits) : nullptr;
        Gr.boxes[l] = on ? const_cast<void*>(grads[l].boxes) : nullptr;
    }
    return LWDETR_OK;
}

// LWDETR_OK when G groups split nq queries evenly into slices the solver can take and no image has more targets than a slice has columns
int check_groups(int nq, int groups, int maxT) {
    if (groups < 1 || nq < 1) return LWDETR_ERR_BAD_ARG;
    if (nq % groups != 0 || nq / groups > LWDETR_MATCH_MAX_NQ || maxT > nq / groups) return LWDETR_ERR_UNSUPPORTED;
    return LWDETR_OK;
}

}  // namespace

extern "C" int lwdetr_match_assign_groups(const float* cost, const int32_t* offsets, const int32_t* counts, int nlayers, int B, int nq,
                                          int groups, int64_t* idx_q, int64_t* idx_t, int32_t* status, int32_t* steps, void* hip_stream) {
    if (nlayers < 1 || nlayers > LWDETR_CRIT_MAX_LAYERS || B < 1 || nq < 1 || groups < 1 || !offsets || !counts || !status) return LWDETR_ERR_BAD_ARG;
    int maxT = 0;
    const long sumT = sum_counts(counts, B, &maxT);
    if (sumT < 0) return LWDETR_ERR_BAD_ARG;
    const int rc = check_groups(nq, groups, maxT);
    if (rc != LWDETR_OK) return rc;
    if (sumT > 0 && (!cost || !idx_q || !idx_t)) return LWDETR_ERR_BAD_ARG;
    const long nprob = (long)nlayers * B * groups;
    if (nprob > INT_MAX / 2) return LWDETR_ERR_UNSUPPORTED;
    const int kpl = lsa_kpl(nq / groups);
    const size_t per_wave = lsa_wave_bytes(maxT, kpl);
    const int waves = 4 * per_wave <= 48 * 1024 ? 4 : 2;        // 20 KB per wave at gw = T = 1024
    const dim3 grid((unsigned)((nprob + waves - 1) / waves)), block((unsigned)(waves * 64));
    const size_t smem = per_wave * waves;
    hipStream_t st = (hipStream_t)hip_stream;
#define LAUNCH_LSA(K) hipLaunchKernelGGL(match_assign_groups_kernel<K>, grid, block, smem, st, cost, offsets, nlayers, B, nq, groups, (int)sumT, \
                                         maxT, idx_q, idx_t, status, steps)
    switch (kpl) {
        case 1: LAUNCH_LSA(1); break;
        case 2: LAUNCH_LSA(2); break;
        case 5: LAUNCH_LSA(5); break;
        case 8: LAUNCH_LSA(8); break;
        default: LAUNCH_LSA(16); break;
    }
#undef LAUNCH_LSA
    return lwdetr_check_launch();
}

#define TR_DISPATCH(LAUNCH)                                                                                                          \
    switch (loss_form) {                                                                                                             \
        case TR_FOCAL: if (dtype == DT_F32) LAUNCH(float, TR_FOCAL); else if (dtype == DT_F16) LAUNCH(f16, TR_FOCAL); else LAUNCH(bf16, TR_FOCAL); break; \
        case TR_IABCE: if (dtype == DT_F32) LAUNCH(float, TR_IABCE); else if (dtype == DT_F16) LAUNCH(f16, TR_IABCE); else LAUNCH(bf16, TR_IABCE); break; \
        case TR_VARIFOCAL: if (dtype == DT_F32) LAUNCH(float, TR_VARIFOCAL); else if (dtype == DT_F16) LAUNCH(f16, TR_VARIFOCAL); else LAUNCH(bf16, TR_VARIFOCAL); break; \
        default: if (dtype == DT_F32) LAUNCH(float, TR_POSSUP); else if (dtype == DT_F16) LAUNCH(f16, TR_POSSUP); else LAUNCH(bf16, TR_POSSUP); break; \
    }

extern "C" int lwdetr_criterion_train_partials(const lwdetr_crit_layer* layers, int nlayers, int B, int nq, int C, const int64_t* labels,
                                               const float* tboxes, const int32_t* offsets, const int32_t* counts, const int64_t* idx_q,
                                               const int64_t* idx_t, int groups, int loss_form, float alpha, float* partials, int dtype,
                                               void* hip_stream) {
    CritLayers L;
    if (pack_layers(layers, nlayers, L) != LWDETR_OK || B < 1 || nq < 1 || C < 1 || !offsets || !counts || !partials) return LWDETR_ERR_BAD_ARG;
    if (dtype < DT_F32 || dtype > DT_BF16 || loss_form < TR_FOCAL || loss_form > TR_POSSUP || B > 65535) return LWDETR_ERR_UNSUPPORTED;
    int maxT = 0;
    const long sumT = sum_counts(counts, B, &maxT);
    if (sumT < 0 || (sumT > 0 && (!labels || !tboxes || !idx_q || !idx_t))) return LWDETR_ERR_BAD_ARG;
    const int rc = check_groups(nq, groups, maxT);
    if (rc != LWDETR_OK) return rc;
    const dim3 grid((unsigned)((nq + CR_QCH - 1) / CR_QCH), (unsigned)B, (unsigned)nlayers);
    hipStream_t st = (hipStream_t)hip_stream;
#define LAUNCH_PART(TT, F) hipLaunchKernelGGL((train_partials_kernel<TT, F>), grid, dim3(CR_THREADS), 0, st, L, B, nq, C, labels, tboxes, \
                                              offsets, (int)sumT, idx_q, idx_t, groups, alpha, partials)
    TR_DISPATCH(LAUNCH_PART)
#undef LAUNCH_PART
    return lwdetr_check_launch();
}

extern "C" int lwdetr_criterion_train_finish(const float* partials, const lwdetr_crit_layer* layers, const int32_t* offsets,
                                             const int32_t* counts, int nlayers, int B, int nq, int groups, int loss_form, float num_boxes,
                                             float* out, void* hip_stream) {
    CritLayers L;
    if (pack_layers(layers, nlayers, L) != LWDETR_OK || B < 1 || nq < 1 || groups < 1 || !partials || !offsets || !counts || !out ||
        !(num_boxes > 0.f))
        return LWDETR_ERR_BAD_ARG;
    if (loss_form < TR_FOCAL || loss_form > TR_POSSUP) return LWDETR_ERR_UNSUPPORTED;
    const long sumT = sum_counts(counts, B, nullptr);
    if (sumT < 0) return LWDETR_ERR_BAD_ARG;
    hipLaunchKernelGGL(train_finish_kernel, dim3((unsigned)nlayers), dim3(64), 0, (hipStream_t)hip_stream, partials, L, offsets, B, nq,
                       (nq + CR_QCH - 1) / CR_QCH, sumT * groups, loss_form, num_boxes, out);
    return lwdetr_check_launch();
}

extern "C" int lwdetr_criterion_backward(const lwdetr_crit_layer* layers, const lwdetr_crit_layer* grads, int nlayers, int B, int nq, int C,
                                         const int64_t* labels, const float* tboxes, const int32_t* offsets, const int32_t* counts,
                                         const int64_t* idx_q, const int64_t* idx_t, int groups, int loss_form, float alpha, float num_boxes,
                                         const float* grad_out, int dtype, void* hip_stream) {
    CritLayers L;
    GradLayers Gr;
    if (pack_layers(layers, nlayers, L) != LWDETR_OK || pack_grads(grads, nlayers, Gr) != LWDETR_OK || B < 1 || nq < 1 || C < 1 || !offsets ||
        !counts || !grad_out || !(num_boxes > 0.f))
        return LWDETR_ERR_BAD_ARG;
    if (dtype < DT_F32 || dtype > DT_BF16 || loss_form < TR_FOCAL || loss_form > TR_POSSUP || B > 65535) return LWDETR_ERR_UNSUPPORTED;
    int maxT = 0;
    const long sumT = sum_counts(counts, B, &maxT);
    if (sumT < 0 || (sumT > 0 && (!labels || !tboxes || !idx_q || !idx_t))) return LWDETR_ERR_BAD_ARG;
    const int rc = check_groups(nq, groups, maxT);
    if (rc != LWDETR_OK) return rc;
    const dim3 grid((unsigned)((nq + CR_QCH - 1) / CR_QCH), (unsigned)B, (unsigned)nlayers);
    hipStream_t st = (hipStream_t)hip_stream;
#define LAUNCH_BWD(TT, F) hipLaunchKernelGGL((train_backward_kernel<TT, F>), grid, dim3(CR_THREADS), 0, st, L, Gr, B, nq, C, labels, tboxes, \
                                             offsets, (int)sumT, idx_q, idx_t, groups, alpha, num_boxes, grad_out)
    TR_DISPATCH(LAUNCH_BWD)
#undef LAUNCH_BWD
    return lwdetr_check_launch();
}

extern "C" int lwdetr_criterion_grad_host(const float* logits, const float* boxes, int nq, int C, const int64_t* labels, const float* tboxes,
                                          int T, const int64_t* idx_q, const int64_t* idx_t, int npairs, int loss_form, float alpha,
                                          float num_boxes, const float* grad_out, float* grad_logits, float* grad_boxes) {
    if (!logits || !boxes || nq < 1 || C < 1 || T < 0 || npairs < 0 || !grad_out || !grad_logits || !grad_boxes || !(num_boxes > 0.f))
        return LWDETR_ERR_BAD_ARG;
    if (npairs > 0 && (!labels || !tboxes || !idx_q || !idx_t || T < 1)) return LWDETR_ERR_BAD_ARG;
    if (loss_form < TR_FOCAL || loss_form > TR_POSSUP) return LWDETR_ERR_UNSUPPORTED;
    std::vector<int> tgt(nq, -1);
    std::vector<float> iou(nq, 0.f);
    const float up_l1 = grad_out[2] / num_boxes, up_gl = grad_out[3] / num_boxes;
    for (size_t i = 0; i < (size_t)nq * 4; ++i) grad_boxes[i] = 0.f;
    float mx = 0.f;
    for (int p = 0; p < npairs; ++p) {
        const long q = idx_q[p], t = idx_t[p];
        if (q < 0 || q >= nq || t < 0 || t >= T) return LWDETR_ERR_BAD_ARG;
        float l1, gl, d[4];
        tr_pair<true>(boxes + (size_t)q * 4, tboxes + (size_t)t * 4, iou[q], l1, gl, up_l1, up_gl, d);
        tgt[q] = (int)t;
        mx = fmaxf(mx, iou[q]);
        for (int k = 0; k < 4; ++k) grad_boxes[(size_t)q * 4 + k] = d[k];
    }
    const float norm = mx + 1e-8f;
    const float scale = tr_ce_scale(loss_form, grad_out[0], nq, num_boxes);
    switch (loss_form) {
        case TR_FOCAL: grad_host_rows<TR_FOCAL>(logits, nq, C, labels, tgt.data(), iou.data(), norm, alpha, scale, grad_logits); break;
        case TR_IABCE: grad_host_rows<TR_IABCE>(logits, nq, C, labels, tgt.data(), iou.data(), norm, alpha, scale, grad_logits); break;
        case TR_VARIFOCAL: grad_host_rows<TR_VARIFOCAL>(logits, nq, C, labels, tgt.data(), iou.data(), norm, alpha, scale, grad_logits); break;
        default: grad_host_rows<TR_POSSUP>(logits, nq, C, labels, tgt.data(), iou.data(), norm, alpha, scale, grad_logits); break;
    }
    return LWDETR_OK;
}
