// Evaluation criterion for gfx950: Hungarian matcher and losses of the reference's SetCriterion, inference only, no gradient.
//   * match_cost_kernel        : C = w_bbox L1 + w_class (pos - neg) + w_giou (-GIoU) per (layer, image, own target, query), f32 in the
//                                reference's operation order (models/matcher.py:71-94, util/box_ops.py:21-25, :36-73), stored target-major
//                                so that a solver row is one contiguous run
//   * match_assign_kernel      : rectangular linear assignment, one WAVE per (layer, image): shortest augmenting paths with dual variables
//                                in f64 - the algorithm of scipy.optimize.linear_sum_assignment (Crouse 2016) on the transposed problem
//                                (rows = targets, columns = queries, as scipy transposes a tall matrix), hence the same optimum. Each lane
//                                owns the columns lane, lane + 64, ... (shortest, v, visited flags in registers); a step is one lane-local
//                                relaxation of the current row and one wave arg-min by shuffles, lowest index on ties. u, the row <-> column
//                                maps and the predecessors sit in the wave's slice of LDS; no barrier anywhere (a wave is in lockstep and
//                                its LDS operations complete in order; the arrays are volatile so none is cached in a register).
//                                EVERY loop has a trip count fixed by T and nq: T augmentations of at most (row + 1) steps (a search visits
//                                a new column per step and only `row` columns are assigned), the path walk at most (row + 1) links. No exit
//                                depends on a floating-point comparison alone, so NaN / inf costs terminate too and still leave a perfect
//                                matching of the T targets (a column chosen without ever having been relaxed takes the row being scanned as
//                                its predecessor, which keeps the predecessor chain valid); the status word says so.
//   * criterion_partials_kernel: per (layer, image, chunk of 32 queries): rebuilds the matched (b, q) -> target map of the chunk from the
//                                assignment, then one pass over the chunk's logits (a wave per query row, lanes over classes): the loss_ce
//                                terms (sigmoid focal loss lwdetr.py:458-483 / IA-BCE :266-290), the row arg-max (class_error, cardinality),
//                                and the matched pairs' L1 / GIoU terms; f32 sums of at most 32 * C terms, reduced in a fixed order
//   * criterion_finish_kernel  : adds the partials in a fixed order in f64, divides by num_boxes, composes mean(1) * nq for the focal form
// The solver's per-lane pieces (lsa_lane_*, match_shared.h) are __host__ __device__: lwdetr_match_assign_host runs the very same code with the 64 lanes
// emulated by a loop, so the solver is testable on a machine without a GPU.
#include "match_shared.h"

namespace {

// =========================================================== cost matrix =================================================================
// grid (sumT, ceil(nq / 256), layers): one packed target per block row, 256 queries per block
template <typename T>
__global__ __launch_bounds__(256) void match_cost_kernel(CritLayers L, int B, int nq, int C, const int64_t* __restrict__ labels,
                                                         const float* __restrict__ tboxes, const int32_t* __restrict__ offsets, int sumT,
                                                         float w_class, float w_bbox, float w_giou, float alpha, float* __restrict__ cost) {
    const int g = blockIdx.x, layer = blockIdx.z;
    const int q = blockIdx.y * 256 + threadIdx.x;
    int b = 0;                                                   // the image of packed target g: offsets[b] <= g < offsets[b + 1]
    for (int i = 0; i < B; ++i) b = offsets[i + 1] <= g ? i + 1 : b;
    if (b >= B || g < offsets[b] || g >= sumT || q >= nq) return;
    long lab = labels[g];
    lab = lab < 0 ? 0 : (lab >= C ? C - 1 : lab);
    const T* lg = (const T*)L.logits[layer];
    const T* bx = (const T*)L.boxes[layer];
    const size_t row = (size_t)b * nq + q;
    const float x = to_f32<T>(lg[row * C + lab]);
    const float ocx = to_f32<T>(bx[row * 4 + 0]), ocy = to_f32<T>(bx[row * 4 + 1]), ow = to_f32<T>(bx[row * 4 + 2]),
                oh = to_f32<T>(bx[row * 4 + 3]);
    const float tcx = tboxes[(size_t)g * 4 + 0], tcy = tboxes[(size_t)g * 4 + 1], tw = tboxes[(size_t)g * 4 + 2], th = tboxes[(size_t)g * 4 + 3];
    // matcher.py:86-88
    const float p = sigmoid_f32(x);
    const float neg = (1.f - alpha) * (p * p) * (-logf(1.f - p + 1e-8f));
    const float om = 1.f - p;
    const float pos = alpha * (om * om) * (-logf(p + 1e-8f));
    const float c_class = pos - neg;
    // matcher.py:91 (cdist p = 1)
    const float c_bbox = fabsf(ocx - tcx) + fabsf(ocy - tcy) + fabsf(ow - tw) + fabsf(oh - th);
    float iou, giou;
    box_iou_giou(cxcywh_to_xyxy(ocx, ocy, ow, oh), cxcywh_to_xyxy(tcx, tcy, tw, th), iou, giou);
    cost[((size_t)layer * sumT + g) * nq + q] = w_bbox * c_bbox + w_class * c_class + w_giou * (-giou);      // matcher.py:94
}

// =========================================================== assignment ==================================================================
template <int KPL>
__global__ __launch_bounds__(256) void match_assign_kernel(const float* __restrict__ cost, const int32_t* __restrict__ offsets, int nlayers,
                                                           int B, int nq, int sumT, int maxT, int64_t* __restrict__ idx_q,
                                                           int64_t* __restrict__ idx_t, int32_t* __restrict__ status,
                                                           int32_t* __restrict__ steps) {
    extern __shared__ double lsa_smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int prob = blockIdx.x * (blockDim.x >> 6) + wave;
    if (prob >= nlayers * B) return;                             // whole waves leave; the kernel has no barrier
    const int layer = prob / B, b = prob - layer * B;
    const int off = offsets[b], T = offsets[b + 1] - off;
    if (off < 0 || T < 0 || T > maxT || T > nq || (long)off + T > sumT) {      // offsets and the host's counts disagree: touch nothing
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
    const float* cbase = cost + ((size_t)layer * sumT + off) * nq;
    int nsteps = 0, bad = 0;
    for (int cur = 0; cur < T; ++cur) {
        lsa_lane_reset(s);
        double minv = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step <= cur && sink < 0; ++step) {
            const double ui = u[i];
            double best;
            int bestj;
            lsa_lane_scan(s, lane, nq, cbase + (size_t)i * nq, ui, minv, i, path, best, bestj, bad);
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
            if (jsel >= nq) { bad = 1; break; }                  // unreachable: T <= nq leaves an unvisited column at every step
            lsa_lane_select(s, lane, jsel, i, path);
            const int r = row4col[jsel];
            if (r < 0) sink = jsel; else i = r;
        }
        if (sink < 0) { bad = 1; break; }                        // unreachable (see the head of the file)
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
    // pairs in ascending query order (scipy's row order for the untransposed problem)
    const size_t obase = (size_t)layer * sumT + off;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < KPL; ++k) {
        const int j = lane + LSA_WAVE * k;
        const int r = j < nq ? row4col[j] : -1;
        const bool has = r >= 0;
        const unsigned long long m = __ballot(has);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (has && cnt + pre < T) { idx_q[obase + cnt + pre] = j; idx_t[obase + cnt + pre] = r; }
        cnt += __popcll(m);
    }
    const int anybad = __any(bad);
    if (lane == 0) { status[prob] = anybad ? 1 : 0; if (steps) steps[prob] = nsteps; }
}

// =========================================================== losses ======================================================================
// grid (ceil(nq / 32), B, layers), 256 threads. partials[((layer * B + b) * nchunks + chunk) * 5 + {ce, l1, 1 - giou, card, correct}]
template <typename T, int FORM>
__global__ __launch_bounds__(CR_THREADS) void criterion_partials_kernel(CritLayers L, int B, int nq, int C, const int64_t* __restrict__ labels,
                                                                        const float* __restrict__ tboxes, const int32_t* __restrict__ offsets,
                                                                        int sumT, const int64_t* __restrict__ idx_q,
                                                                        const int64_t* __restrict__ idx_t, float alpha,
                                                                        float* __restrict__ partials) {
    __shared__ int s_tgt[CR_QCH];
    __shared__ float s_iou[CR_QCH], s_l1[CR_QCH], s_gl[CR_QCH];
    __shared__ float s_red[CR_THREADS / 64][3];
    const int chunk = blockIdx.x, b = blockIdx.y, layer = blockIdx.z, tid = threadIdx.x;
    const int q0 = chunk * CR_QCH, nqc = min(CR_QCH, nq - q0);
    const int off = offsets[b];
    int Tb = offsets[b + 1] - off;
    if (off < 0 || Tb < 0 || (long)off + Tb > sumT) Tb = 0;
    const T* lg = (const T*)L.logits[layer];
    const T* bx = (const T*)L.boxes[layer];
    if (tid < CR_QCH) { s_tgt[tid] = -1; s_iou[tid] = 0.f; s_l1[tid] = 0.f; s_gl[tid] = 0.f; }
    __syncthreads();
    for (int p = tid; p < Tb; p += CR_THREADS) {                 // the chunk's slice of the matched (b, q) -> target map
        const long q = idx_q[(size_t)layer * sumT + off + p], t = idx_t[(size_t)layer * sumT + off + p];
        if (q >= q0 && q < q0 + nqc && t >= 0 && t < Tb) {
            const int g = off + (int)t;
            const size_t row = (size_t)b * nq + q;
            const float ocx = to_f32<T>(bx[row * 4 + 0]), ocy = to_f32<T>(bx[row * 4 + 1]), ow = to_f32<T>(bx[row * 4 + 2]),
                        oh = to_f32<T>(bx[row * 4 + 3]);
            const float tcx = tboxes[(size_t)g * 4 + 0], tcy = tboxes[(size_t)g * 4 + 1], tw = tboxes[(size_t)g * 4 + 2],
                        th = tboxes[(size_t)g * 4 + 3];
            float iou, giou;
            box_iou_giou(cxcywh_to_xyxy(ocx, ocy, ow, oh), cxcywh_to_xyxy(tcx, tcy, tw, th), iou, giou);
            const int r = (int)q - q0;
            s_tgt[r] = g;
            s_iou[r] = iou;
            s_l1[r] = fabsf(ocx - tcx) + fabsf(ocy - tcy) + fabsf(ow - tw) + fabsf(oh - th);       // lwdetr.py:371-374
            s_gl[r] = 1.f - giou;                                                                     // lwdetr.py:376-379
        }
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    float acc = 0.f, card = 0.f, correct = 0.f;
    for (int r = wave; r < nqc; r += CR_THREADS / 64) {
        const int g = s_tgt[r];
        long lab = -1;
        if (g >= 0) { lab = labels[g]; lab = lab < 0 ? 0 : (lab >= C ? C - 1 : lab); }
        const float iou = s_iou[r];
        const T* xrow = lg + ((size_t)b * nq + q0 + r) * C;
        float bv = -INFINITY;
        int bc = INT_MAX;
        for (int c = lane; c < C; c += 64) {
            const float x = to_f32<T>(xrow[c]);
            if (x > bv) { bv = x; bc = c; }
            const float prob = sigmoid_f32(x);
            const bool hit = c == lab;
            float loss;
            if (FORM == 0) {                                     // sigmoid_focal_loss, lwdetr.py:474-481, target one-hot of the matched label
                const float t = hit ? 1.f : 0.f;
                const float ce = (1.f - t) * x + fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x)));
                const float p_t = prob * t + (1.f - prob) * (1.f - t);
                const float omp = 1.f - p_t;
                loss = ce * (omp * omp);
                loss = (alpha * t + (1.f - alpha) * (1.f - t)) * loss;
            } else {                                             // IA-BCE, lwdetr.py:276-289
                float pw = 0.f, nw = prob * prob;
                if (hit) {
                    const float tt = fmaxf(powf(prob, alpha) * powf(iou, 1.f - alpha), 0.01f);
                    pw = tt;
                    nw = 1.f - tt;
                }
                loss = -pw * logf(prob) - nw * logf(1.f - prob);
            }
            acc += loss;
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

// c - a * b with the product rounded to f32 first, as torch evaluates `100 - correct.mul_(100 / n)` (util/misc.py accuracy): class_error is
// compared exactly, and a fused multiply-add lands on the other side of a rounding tie (19 of 65 correct)
__device__ __forceinline__ float sub_rounded_product(float c, float a, float b) {
#pragma clang fp contract(off)
    const float p = a * b;
    return c - p;
}

// grid (layers), one wave: lane l adds the images l, l + 64, ... chunk by chunk in f64, then a butterfly in a fixed order
__global__ __launch_bounds__(64) void criterion_finish_kernel(const float* __restrict__ partials, CritLayers L,
                                                              const int32_t* __restrict__ offsets, int B, int nq, int nchunks, int sumT,
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
        cerr += fabs(card - (double)(offsets[b + 1] - offsets[b]));      // lwdetr.py:354-357
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        ce += __shfl_xor(ce, m); l1 += __shfl_xor(l1, m); gl += __shfl_xor(gl, m); co += __shfl_xor(co, m); cerr += __shfl_xor(cerr, m);
    }
    if (lane != 0) return;
    const double nb = (double)num_boxes;
    float* o = out + (size_t)layer * 5;
    o[0] = loss_form == 0 ? (float)(ce / (double)nq / nb * (double)nq) : (float)(ce / nb);        // lwdetr.py:483 * :339 / :290
    float cls_err = 0.f;
    if (L.class_error[layer]) cls_err = sumT > 0 ? sub_rounded_product(100.f, (float)co, (float)(100.0 / (double)sumT)) : 100.f;    // lwdetr.py:344
    o[1] = cls_err;
    o[2] = (float)(l1 / nb);
    o[3] = (float)(gl / nb);
    o[4] = (float)cerr / (float)B;                                                                  // F.l1_loss mean over images
}

}  // namespace

extern "C" int lwdetr_match_cost(const lwdetr_crit_layer* layers, int nlayers, int B, int nq, int C, const int64_t* labels,
                                 const float* tboxes, const int32_t* offsets, const int32_t* counts, float w_class, float w_bbox,
                                 float w_giou, float alpha, float* cost, int dtype, void* hip_stream) {
    CritLayers L;
    if (pack_layers(layers, nlayers, L) != LWDETR_OK || B < 1 || nq < 1 || C < 1 || !offsets || !counts) return LWDETR_ERR_BAD_ARG;
    if (dtype < DT_F32 || dtype > DT_BF16) return LWDETR_ERR_UNSUPPORTED;
    const long sumT = sum_counts(counts, B, nullptr);
    if (sumT < 0) return LWDETR_ERR_BAD_ARG;
    if (sumT == 0) return LWDETR_OK;
    if (!labels || !tboxes || !cost) return LWDETR_ERR_BAD_ARG;
    const int qb = (nq + 255) / 256;
    if (qb > 65535) return LWDETR_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)sumT, (unsigned)qb, (unsigned)nlayers);
    hipStream_t st = (hipStream_t)hip_stream;
#define LAUNCH_COST(TT) hipLaunchKernelGGL(match_cost_kernel<TT>, grid, dim3(256), 0, st, L, B, nq, C, labels, tboxes, offsets, (int)sumT, \
                                           w_class, w_bbox, w_giou, alpha, cost)
    if (dtype == DT_F32) LAUNCH_COST(float); else if (dtype == DT_F16) LAUNCH_COST(f16); else LAUNCH_COST(bf16);
#undef LAUNCH_COST
    return lwdetr_check_launch();
}

extern "C" int lwdetr_match_assign(const float* cost, const int32_t* offsets, const int32_t* counts, int nlayers, int B, int nq,
                                   int64_t* idx_q, int64_t* idx_t, int32_t* status, int32_t* steps, void* hip_stream) {
    if (nlayers < 1 || nlayers > LWDETR_CRIT_MAX_LAYERS || B < 1 || nq < 1 || !offsets || !counts || !status) return LWDETR_ERR_BAD_ARG;
    if (nq > LWDETR_MATCH_MAX_NQ) return LWDETR_ERR_UNSUPPORTED;
    int maxT = 0;
    const long sumT = sum_counts(counts, B, &maxT);
    if (sumT < 0) return LWDETR_ERR_BAD_ARG;
    if (maxT > nq) return LWDETR_ERR_UNSUPPORTED;
    if (sumT > 0 && (!cost || !idx_q || !idx_t)) return LWDETR_ERR_BAD_ARG;
    const int kpl = lsa_kpl(nq);
    const size_t per_wave = lsa_wave_bytes(maxT, kpl);
    const int waves = 4 * per_wave <= 48 * 1024 ? 4 : 2;        // 20 KB per wave at nq = T = 1024
    const int nprob = nlayers * B;
    const dim3 grid((unsigned)((nprob + waves - 1) / waves)), block((unsigned)(waves * 64));
    const size_t smem = per_wave * waves;
    hipStream_t st = (hipStream_t)hip_stream;
#define LAUNCH_LSA(K) hipLaunchKernelGGL(match_assign_kernel<K>, grid, block, smem, st, cost, offsets, nlayers, B, nq, (int)sumT, maxT, idx_q, \
                                         idx_t, status, steps)
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

extern "C" int lwdetr_match_assign_host(const float* cost, int nq, int T, int64_t* idx_q, int64_t* idx_t, int32_t* status,
                                        int32_t* steps) {
    if (nq < 1 || T < 0 || (T > 0 && (!cost || !idx_q || !idx_t))) return LWDETR_ERR_BAD_ARG;
    if (nq > LWDETR_MATCH_MAX_NQ || T > nq) return LWDETR_ERR_UNSUPPORTED;
    switch (lsa_kpl(nq)) {
        case 1: lsa_host<1>(cost, nq, T, idx_q, idx_t, status, steps); break;
        case 2: lsa_host<2>(cost, nq, T, idx_q, idx_t, status, steps); break;
        case 5: lsa_host<5>(cost, nq, T, idx_q, idx_t, status, steps); break;
        case 8: lsa_host<8>(cost, nq, T, idx_q, idx_t, status, steps); break;
        default: lsa_host<16>(cost, nq, T, idx_q, idx_t, status, steps); break;
    }
    return LWDETR_OK;
}

extern "C" long lwdetr_criterion_partials_floats(int nlayers, int B, int nq) {
    if (nlayers < 1 || B < 1 || nq < 1) return 0;
    return (long)nlayers * B * ((nq + CR_QCH - 1) / CR_QCH) * CR_NPART;
}

extern "C" int lwdetr_criterion_partials(const lwdetr_crit_layer* layers, int nlayers, int B, int nq, int C, const int64_t* labels,
                                         const float* tboxes, const int32_t* offsets, const int32_t* counts, const int64_t* idx_q,
                                         const int64_t* idx_t, int loss_form, float alpha, float* partials, int dtype, void* hip_stream) {
    CritLayers L;
    if (pack_layers(layers, nlayers, L) != LWDETR_OK || B < 1 || nq < 1 || C < 1 || !offsets || !counts || !partials) return LWDETR_ERR_BAD_ARG;
    if (dtype < DT_F32 || dtype > DT_BF16 || loss_form < 0 || loss_form > 1 || B > 65535) return LWDETR_ERR_UNSUPPORTED;
    const long sumT = sum_counts(counts, B, nullptr);
    if (sumT < 0 || (sumT > 0 && (!labels || !tboxes || !idx_q || !idx_t))) return LWDETR_ERR_BAD_ARG;
    const dim3 grid((unsigned)((nq + CR_QCH - 1) / CR_QCH), (unsigned)B, (unsigned)nlayers);
    hipStream_t st = (hipStream_t)hip_stream;
#define LAUNCH_PART(TT, F) hipLaunchKernelGGL((criterion_partials_kernel<TT, F>), grid, dim3(CR_THREADS), 0, st, L, B, nq, C, labels, tboxes, \
                                              offsets, (int)sumT, idx_q, idx_t, alpha, partials)
    if (loss_form == 0) {
        if (dtype == DT_F32) LAUNCH_PART(float, 0); else if (dtype == DT_F16) LAUNCH_PART(f16, 0); else LAUNCH_PART(bf16, 0);
    } else {
        if (dtype == DT_F32) LAUNCH_PART(float, 1); else if (dtype == DT_F16) LAUNCH_PART(f16, 1); else LAUNCH_PART(bf16, 1);
    }
#undef LAUNCH_PART
    return lwdetr_check_launch();
}

extern "C" int lwdetr_criterion_finish(const float* partials, const lwdetr_crit_layer* layers, const int32_t* offsets,
                                       const int32_t* counts, int nlayers, int B, int nq, int loss_form, float num_boxes, float* out,
                                       void* hip_stream) {
    CritLayers L;
    if (pack_layers(layers, nlayers, L) != LWDETR_OK || B < 1 || nq < 1 || !partials || !offsets || !counts || !out || !(num_boxes > 0.f))
        return LWDETR_ERR_BAD_ARG;
    if (loss_form < 0 || loss_form > 1) return LWDETR_ERR_UNSUPPORTED;
    const long sumT = sum_counts(counts, B, nullptr);
    if (sumT < 0) return LWDETR_ERR_BAD_ARG;
    hipLaunchKernelGGL(criterion_finish_kernel, dim3((unsigned)nlayers), dim3(64), 0, (hipStream_t)hip_stream, partials, L, offsets, B, nq,
                       (nq + CR_QCH - 1) / CR_QCH, (int)sumT, loss_form, num_boxes, out);
    return lwdetr_check_launch();
}
