// COCO box evaluation for gfx950: the arithmetic of pycocotools' COCOeval (iouType 'bbox') behind datasets/coco_eval.py:26-78, :219-264.
//   * cocoeval_match_kernel : COCOeval.computeIoU + evaluateImg for one batch. A WORKGROUP per image: its threads map the labels to dense
//                             categories, rank every detection inside its (image, category) list (descending score, stable in the detection
//                             index: argsort(-score, kind='mergesort'), first maxDets[-1] = 100 kept) by counting, then its four WAVES take the
//                             image's categories. The 4 area ranges x 10 IoU thresholds = 40 greedy matchings of a category sit on lanes 0..39
//                             of the wave (lane = area * 10 + threshold); each lane walks detections by ground truths serially and recomputes
//                             the IoU of a pair (maskApi.c bbIou) instead of keeping a (100, 256) f64 table in LDS - a pair that does not
//                             overlap costs two subtractions, only an overlapping one pays the f64 division. The matched / ignored flags of a
//                             detection are one __ballot each: bit (area * 10 + threshold) of a 40-bit mask.
//   * cocoeval_npig_kernel  : the number of non-ignored ground truths per (category, area range) over the evaluated images (integer atomics)
//   * cocoeval_curves_kernel: COCOeval.accumulate. A workgroup per (category, area, maxDet, threshold) walks the category's segment of the
//                             score-ordered store in chunks of 256 with an integer carry: running tp / fp by ballots, rc = tp / npig,
//                             pr = tp / (fp + tp + eps). searchsorted(rc, recThrs, 'left') is found from the other side: rc only steps where a
//                             true positive sits, and the element at which it steps over recall thresholds is their index. The right-to-left
//                             running maximum of pr is a maximum per threshold bucket (integer atomicMax on the bit pattern of the non-negative
//                             f64: order-independent) and a suffix maximum over the 101 buckets.
// All geometry and curve arithmetic is f64 in COCOeval's operation order with FP CONTRACTION OFF for the whole file: an FMA in
// `da + ga - w * h` changes the last bit of an IoU and with it a threshold decision. The greedy decisions and the recall look-ups are
// comparisons of these values, so same order and same rounding give the same result. No floating-point atomics, no host synchronisation.
// EVERY loop has a trip count fixed by the counts (K, the group sizes, the segment lengths, 101): NaN / inf boxes and scores terminate.
// The per-lane pieces (ce_*) are __host__ __device__: lwdetr_cocoeval_match_host runs the very same code with the lanes emulated by a loop.
#include "common.h"
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

#define CE_HD __host__ __device__ __forceinline__

namespace {

constexpr int CE_MAXD = LWDETR_COCOEVAL_MAX_DETS;
constexpr int CE_MAXG = LWDETR_COCOEVAL_MAX_GROUP;
constexpr int CE_MAXC = LWDETR_COCOEVAL_MAX_CATS;
constexpr int CE_KEEP = LWDETR_COCOEVAL_KEEP;
constexpr int CE_NT = LWDETR_COCOEVAL_NTHR;
constexpr int CE_NA = LWDETR_COCOEVAL_NAREA;
constexpr int CE_NR = LWDETR_COCOEVAL_NREC;
constexpr int CE_LANES = CE_NA * CE_NT;
constexpr int CE_GW = CE_MAXG / 64;                 // 64-bit words of a lane's "gt already matched" set
typedef unsigned long long u64;

struct CeThr { double v[CE_NT]; };
struct CeRec { double v[CE_NR]; };

// Params.areaRng of cocoeval.py: [0, 1e5^2], [0, 32^2], [32^2, 96^2], [96^2, 1e5^2], both ends inclusive
CE_HD double ce_area_lo(int a) { return a == 2 ? 1024.0 : (a == 3 ? 9216.0 : 0.0); }
CE_HD double ce_area_hi(int a) { return a == 1 ? 1024.0 : (a == 2 ? 9216.0 : 1e10); }

// the label of the f32 record -> dense category; anything that is no id of the ground truth's category list is dropped (getAnnIds(catIds))
CE_HD int ce_dense_cat(float label, const int32_t* lut, int lut_size) {
    if (!(label >= 0.f && label < (float)lut_size)) return -1;
    const int id = (int)label;
    if ((float)id != label || id >= lut_size) return -1;
    return lut[id];
}
// is detection e listed before detection d? argsort(-score, kind='mergesort'): descending score, equal scores by index, NaN last
CE_HD bool ce_before(float se, int e, float sd, int d) {
    const bool ne = se != se, nd = sd != sd;
    if (ne || nd) return ne == nd ? e < d : nd;
    return se > sd || (se == sd && e < d);
}

struct CeDet { double x, y, w, h, area; };
// convert_to_xywh (datasets/coco_eval.py:176-178) subtracts on the f32 tensor; .tolist() then widens; loadRes: area = bb[2] * bb[3]
CE_HD CeDet ce_det_xywh(const float* rec) {
    const float w = rec[4] - rec[2], h = rec[5] - rec[3];
    CeDet d;
    d.x = (double)rec[2]; d.y = (double)rec[3]; d.w = (double)w; d.h = (double)h;
    d.area = d.w * d.h;
    return d;
}
// maskApi.c bbIou, operation by operation
CE_HD double ce_iou(const CeDet& d, const double* g, bool crowd) {
    const double ga = g[2] * g[3];
    const double w = fmin(d.w + d.x, g[2] + g[0]) - fmax(d.x, g[0]);
    if (w <= 0) return 0.0;
    const double h = fmin(d.h + d.y, g[3] + g[1]) - fmax(d.y, g[1]);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = crowd ? d.area : d.area + ga - i;
    return i / u;
}
CE_HD bool ce_gt_ignored(const double* garea, const uint8_t* gcrowd, int g, double lo, double hi) {
    const double ar = garea[g];
    return gcrowd[g] != 0 || ar < lo || ar > hi;
}
// One detection of one (area range, threshold) matching: the body of evaluateImg's `for dind, d in enumerate(dt)`. COCOeval walks the gts
// sorted non-ignored first (stable) and breaks at the first ignored one once a non-ignored match is held; that is two passes in dataset
// order, the second (ignored gts) only when the first found nothing. gtm = the lane's set of gts matched at this threshold.
CE_HD void ce_lane_step(const CeDet& d, const double* gbox, const double* garea, const uint8_t* gcrowd, int G, double lo, double hi,
                        double thr, u64 (&gtm)[CE_GW], bool& matched, bool& ignored) {
    const double cap = 1 - 1e-10;
    double iou = cap < thr ? cap : thr;                          // min([t, 1 - 1e-10])
    int m = -1;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && m >= 0) break;
#pragma unroll
        for (int w = 0; w < CE_GW; ++w) {
            const int n = G - w * 64 < 64 ? G - w * 64 : 64;
            for (int j = 0; j < n; ++j) {
                const int g = w * 64 + j;
                const bool crowd = gcrowd[g] != 0;
                if ((int)ce_gt_ignored(garea, gcrowd, g, lo, hi) != pass) continue;
                if (((gtm[w] >> j) & 1ull) && !crowd) continue;  // already matched at this threshold, and no crowd
                const double v = ce_iou(d, gbox + (size_t)g * 4, crowd);
                if (v < iou) continue;                           // strictly less: an equal IoU moves the match to the later gt
                iou = v;
                m = g;
            }
        }
    }
    matched = m >= 0;
    if (matched) {
        ignored = ce_gt_ignored(garea, gcrowd, m, lo, hi);       // a matched detection inherits the gt's ignore flag
#pragma unroll
        for (int w = 0; w < CE_GW; ++w)
            if (w == (m >> 6)) gtm[w] |= 1ull << (m & 63);
    } else {
        ignored = d.area < lo || d.area > hi;                    // unmatched: ignored when its own area is outside the range
    }
}
// the group (row, k) of the ground-truth table, or an empty one when the table is inconsistent (the host refuses such a table; a kernel
// that met one touches nothing outside it)
CE_HD void ce_group(const lwdetr_coco_gt& gt, int row, int k, int& off, int& G) {
    const size_t gi = (size_t)row * gt.n_cats + k;
    off = gt.grp_off[gi];
    G = gt.grp_off[gi + 1] - off;
    if (off < 0 || G < 0 || G > CE_MAXG || (long)off + G > gt.n_ann) { off = 0; G = 0; }
}

// ============================================================ per-image matching ==========================================================
__global__ __launch_bounds__(256) void cocoeval_match_kernel(lwdetr_coco_gt gt, const float* __restrict__ dets, const int32_t* __restrict__ rows,
                                                             int K, CeThr thr, int32_t* __restrict__ out_cat, float* __restrict__ out_score,
                                                             int32_t* __restrict__ out_rank, int64_t* __restrict__ out_matched,
                                                             int64_t* __restrict__ out_ignored) {
    __shared__ float s_score[CE_MAXD];
    __shared__ int s_cat[CE_MAXD];
    __shared__ int s_rank[CE_MAXD];
    __shared__ int s_cnt[CE_MAXC];
    __shared__ volatile int s_list[4][CE_KEEP];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int row = rows[b];
    const bool row_ok = row >= 0 && row < gt.n_images;           // an image that is not in the table keeps nothing (the host raises)
    const float* recs = dets + (size_t)b * K * 6;
    for (int c = tid; c < gt.n_cats; c += 256) s_cnt[c] = 0;
    for (int d = tid; d < K; d += 256) {
        s_score[d] = recs[(size_t)d * 6];
        s_cat[d] = row_ok ? ce_dense_cat(recs[(size_t)d * 6 + 1], gt.cat_lut, gt.lut_size) : -1;
    }
    __syncthreads();
    for (int d = tid; d < K; d += 256) {
        const int cat = s_cat[d];
        const float sd = s_score[d];
        int rank = 0;
        if (cat >= 0)
            for (int e = 0; e < K; ++e) rank += (s_cat[e] == cat && ce_before(s_score[e], e, sd, d)) ? 1 : 0;
        const bool kept = cat >= 0 && cat < gt.n_cats && rank < CE_KEEP;
        s_rank[d] = kept ? rank : -1;
        const size_t o = (size_t)b * K + d;
        out_score[o] = sd;
        out_cat[o] = kept ? cat : -1;
        out_rank[o] = kept ? rank : -1;
        if (kept) atomicAdd(&s_cnt[cat], 1);
        else { out_matched[o] = 0; out_ignored[o] = 0; }
    }
    __syncthreads();
    // no barrier from here on: a wave is in lockstep, its LDS operations complete in order, and s_list is volatile
    const int a = lane / CE_NT, t = lane - a * CE_NT;
    const bool active = lane < CE_LANES;
    const double lo = ce_area_lo(a), hi = ce_area_hi(a), th = active ? thr.v[t] : 0.0;
    for (int k = wave; k < gt.n_cats; k += 4) {
        const int nd = s_cnt[k];
        if (nd <= 0 || nd > CE_KEEP) continue;                   // wave-uniform
        for (int d = lane; d < K; d += 64)
            if (s_cat[d] == k && s_rank[d] >= 0) s_list[wave][s_rank[d]] = d;
        __builtin_amdgcn_wave_barrier();
        int off, G;
        ce_group(gt, row, k, off, G);
        u64 gtm[CE_GW];
#pragma unroll
        for (int w = 0; w < CE_GW; ++w) gtm[w] = 0ull;
        for (int i = 0; i < nd; ++i) {
            const int d = s_list[wave][i];
            const CeDet det = ce_det_xywh(recs + (size_t)d * 6);
            bool matched = false, ignored = false;
            if (active) ce_lane_step(det, gt.box + (size_t)off * 4, gt.area + off, gt.crowd + off, G, lo, hi, th, gtm, matched, ignored);
            const u64 mm = __ballot(matched), ii = __ballot(ignored);
            if (lane == 0) {
                out_matched[(size_t)b * K + d] = (int64_t)mm;
                out_ignored[(size_t)b * K + d] = (int64_t)ii;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// the same batch on host arrays, lanes and threads emulated
void match_host(const lwdetr_coco_gt& gt, const float* dets, const int32_t* rows, int B, int K, const double* thrs, int32_t* out_cat,
                float* out_score, int32_t* out_rank, int64_t* out_matched, int64_t* out_ignored) {
    std::vector<int> cat(K), rank(K), list(CE_KEEP);
    for (int b = 0; b < B; ++b) {
        const int row = rows[b];
        const bool row_ok = row >= 0 && row < gt.n_images;
        const float* recs = dets + (size_t)b * K * 6;
        for (int d = 0; d < K; ++d) cat[d] = row_ok ? ce_dense_cat(recs[(size_t)d * 6 + 1], gt.cat_lut, gt.lut_size) : -1;
        for (int d = 0; d < K; ++d) {
            const float sd = recs[(size_t)d * 6];
            int r = 0;
            if (cat[d] >= 0)
                for (int e = 0; e < K; ++e) r += (cat[e] == cat[d] && ce_before(recs[(size_t)e * 6], e, sd, d)) ? 1 : 0;
            const bool kept = cat[d] >= 0 && cat[d] < gt.n_cats && r < CE_KEEP;
            rank[d] = kept ? r : -1;
            const size_t o = (size_t)b * K + d;
            out_score[o] = sd;
            out_cat[o] = kept ? cat[d] : -1;
            out_rank[o] = rank[d];
            out_matched[o] = 0;
            out_ignored[o] = 0;
        }
        for (int k = 0; k < gt.n_cats && row_ok; ++k) {
            int nd = 0;
            for (int d = 0; d < K; ++d)
                if (cat[d] == k && rank[d] >= 0) { list[rank[d]] = d; ++nd; }
            if (nd == 0) continue;
            int off, G;
            ce_group(gt, row, k, off, G);
            for (int lane = 0; lane < CE_LANES; ++lane) {
                const int a = lane / CE_NT, t = lane - a * CE_NT;
                u64 gtm[CE_GW];
                for (int w = 0; w < CE_GW; ++w) gtm[w] = 0ull;
                for (int i = 0; i < nd; ++i) {
                    const int d = list[i];
                    const CeDet det = ce_det_xywh(recs + (size_t)d * 6);
                    bool matched = false, ignored = false;
                    ce_lane_step(det, gt.box + (size_t)off * 4, gt.area + off, gt.crowd + off, G, ce_area_lo(a), ce_area_hi(a), thrs[t], gtm,
                                 matched, ignored);
                    const size_t o = (size_t)b * K + d;
                    if (matched) out_matched[o] |= (int64_t)(1ull << lane);
                    if (ignored) out_ignored[o] |= (int64_t)(1ull << lane);
                }
            }
        }
    }
}

// ============================================================ non-ignored gt counts =======================================================
// grid (n evaluated images), 64 threads: npig[k * 4 + a] += 1 per annotation of the image that is not ignored in area range a
__global__ __launch_bounds__(64) void cocoeval_npig_kernel(lwdetr_coco_gt gt, const int32_t* __restrict__ rows, int32_t* __restrict__ npig) {
    const int row = rows[blockIdx.x];
    if (row < 0 || row >= gt.n_images) return;
    int beg = gt.grp_off[(size_t)row * gt.n_cats], end = gt.grp_off[(size_t)(row + 1) * gt.n_cats];
    if (beg < 0 || end > gt.n_ann) return;
    for (int g = beg + (int)threadIdx.x; g < end; g += 64) {
        const int k = gt.cat[g];
        if (k < 0 || k >= gt.n_cats) continue;
#pragma unroll
        for (int a = 0; a < CE_NA; ++a)
            if (!ce_gt_ignored(gt.area, gt.crowd, g, ce_area_lo(a), ce_area_hi(a))) atomicAdd(&npig[k * CE_NA + a], 1);
    }
}

// ============================================================ curves =====================================================================
// number of thresholds <= x (thresholds ascending): searchsorted(recThrs, x, side='right'); at most 7 halvings of 101
__device__ __forceinline__ int ce_count_le(const CeRec& rec, double x) {
    int lo = 0, hi = CE_NR;
    for (int s = 0; s < 7; ++s) {
        const int mid = (lo + hi) >> 1;
        if (lo < hi) { if (rec.v[mid] <= x) lo = mid + 1; else hi = mid; }
    }
    return lo;
}

// grid (n_cats * 4 * 3 * 10), 256 threads. The store is ordered by (category, descending score, image, in-image order); seg_off (n_cats + 1)
// are the categories' segments. precision / scores (10, 101, K, 4, 3), recall (10, K, 4, 3), pre-filled with -1 by the caller.
__global__ __launch_bounds__(256) void cocoeval_curves_kernel(const int64_t* __restrict__ seg_off, const float* __restrict__ score,
                                                              const int32_t* __restrict__ rank, const int64_t* __restrict__ matched,
                                                              const int64_t* __restrict__ ignored, const int32_t* __restrict__ npig,
                                                              CeRec rec, int n_cats, long n_store, double* __restrict__ precision,
                                                              double* __restrict__ scores, double* __restrict__ recall) {
    __shared__ u64 s_max[CE_NR];
    __shared__ int s_has[CE_NR];
    __shared__ float s_sc[CE_NR];
    __shared__ int s_w[2][4][3];
    const int grp = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int t = grp % CE_NT, m = (grp / CE_NT) % 3, a = (grp / (CE_NT * 3)) % CE_NA, k = grp / (CE_NT * 3 * CE_NA);
    if (k >= n_cats) return;
    const int np = npig[k * CE_NA + a];
    if (np <= 0) return;                                         // block-uniform: the group stays -1
    const int maxdet = m == 0 ? 1 : (m == 1 ? 10 : 100);
    const int bit = a * CE_NT + t;
    long s0 = seg_off[k], s1 = seg_off[k + 1];
    if (s0 < 0 || s1 > n_store || s1 < s0) { s0 = 0; s1 = 0; }
    for (int r = tid; r < CE_NR; r += 256) { s_max[r] = 0ull; s_has[r] = 0; s_sc[r] = 0.f; }
    __syncthreads();
    const double dnp = (double)np;
    const u64 lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    long ctp = 0, cfp = 0, cnd = 0;                              // the carry: counts before this chunk
    int par = 0;
    for (long base = s0; base < s1; base += 256, par ^= 1) {
        const long i = base + tid;
        const bool part = i < s1 && rank[i] >= 0 && rank[i] < maxdet;
        bool mt = false, ig = false;
        if (part) { mt = ((u64)matched[i] >> bit) & 1ull; ig = ((u64)ignored[i] >> bit) & 1ull; }
        const bool tpv = part && mt && !ig, fpv = part && !mt && !ig;
        const u64 bt = __ballot(tpv), bf = __ballot(fpv), bp = __ballot(part);
        if (lane == 0) { s_w[par][wave][0] = __popcll(bt); s_w[par][wave][1] = __popcll(bf); s_w[par][wave][2] = __popcll(bp); }
        __syncthreads();                                         // s_w is double-buffered: one barrier per chunk
        long tp = ctp, fp = cfp, nb = cnd, ttp = 0, tfp = 0, tnd = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int wt = s_w[par][w][0], wf = s_w[par][w][1], wp = s_w[par][w][2];
            if (w < wave) { tp += wt; fp += wf; nb += wp; }
            ttp += wt; tfp += wf; tnd += wp;
        }
        if (part) {
            nb += __popcll(bp & lt);                             // participants before this one
            tp += __popcll(bt & lt) + (tpv ? 1 : 0);             // inclusive running counts (np.cumsum)
            fp += __popcll(bf & lt) + (fpv ? 1 : 0);
            const double dtp = (double)tp;
            const double rc = dtp / dnp;
            const double pr = dtp / ((double)(fp + tp) + 2.220446049250313e-16);
            const int c = ce_count_le(rec, rc);                  // the recall thresholds whose index is <= i
            if (c > 0) atomicMax(&s_max[c - 1], (u64)__double_as_longlong(pr));
            const bool first = nb == 0;
            const double rc_prev = (double)(tp - (tpv ? 1 : 0)) / dnp;
            if (first || rc > rc_prev) {                         // rc steps here: i is the 'left' index of the thresholds in (rc_prev, rc]
                const int c0 = first ? 0 : ce_count_le(rec, rc_prev);
                const float sc = score[i];
                for (int r = 0; r < CE_NR; ++r)
                    if (r >= c0 && r < c) { s_has[r] = 1; s_sc[r] = sc; }
            }
        }
        ctp += ttp; cfp += tfp; cnd += tnd;
    }
    __syncthreads();
    for (int r = tid; r < CE_NR; r += 256) {
        double q = 0.0, ss = 0.0;
        if (s_has[r]) {                                    // else: no index with rc >= thr, precision and score stay 0
            u64 best = 0ull;
            for (int r2 = r; r2 < CE_NR; ++r2) best = s_max[r2] > best ? s_max[r2] : best;
            q = __longlong_as_double((long long)best);
            ss = (double)s_sc[r];
        }
        const size_t o = ((((size_t)t * CE_NR + r) * n_cats + k) * CE_NA + a) * 3 + m;
        precision[o] = q;
        scores[o] = ss;
    }
    if (tid == 0) recall[(((size_t)t * n_cats + k) * CE_NA + a) * 3 + m] = cnd > 0 ? (double)ctp / dnp : 0.0;
}

int check_gt(const lwdetr_coco_gt* gt) {
    if (!gt || gt->n_images < 0 || gt->n_cats < 1 || gt->lut_size < 0 || gt->n_ann < 0 || gt->max_group < 0) return LWDETR_ERR_BAD_ARG;
    if (!gt->grp_off || !gt->cat_lut || (gt->n_ann > 0 && (!gt->box || !gt->area || !gt->crowd || !gt->cat))) return LWDETR_ERR_BAD_ARG;
    if (gt->n_cats > CE_MAXC || gt->max_group > CE_MAXG) return LWDETR_ERR_UNSUPPORTED;
    return LWDETR_OK;
}
int check_match(const lwdetr_coco_gt* gt, const void* dets, const void* rows, int B, int K, const double* thrs, const void* o0,
                const void* o1, const void* o2, const void* o3, const void* o4) {
    const int rc = check_gt(gt);
    if (rc != LWDETR_OK) return rc;
    if (B < 0 || K < 0 || !thrs) return LWDETR_ERR_BAD_ARG;
    if (K > CE_MAXD) return LWDETR_ERR_UNSUPPORTED;
    if (B > 0 && K > 0 && (!dets || !rows || !o0 || !o1 || !o2 || !o3 || !o4)) return LWDETR_ERR_BAD_ARG;
    return LWDETR_OK;
}

}  // namespace

extern "C" int lwdetr_cocoeval_match(const lwdetr_coco_gt* gt, const float* dets, const int32_t* rows, int B, int K, const double* iou_thrs,
                                     int32_t* out_cat, float* out_score, int32_t* out_rank, int64_t* out_matched, int64_t* out_ignored,
                                     void* hip_stream) {
    const int rc = check_match(gt, dets, rows, B, K, iou_thrs, out_cat, out_score, out_rank, out_matched, out_ignored);
    if (rc != LWDETR_OK) return rc;
    if (B == 0 || K == 0) return LWDETR_OK;
    CeThr thr;
    for (int t = 0; t < CE_NT; ++t) thr.v[t] = iou_thrs[t];
    hipLaunchKernelGGL(cocoeval_match_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)hip_stream, *gt, dets, rows, K, thr, out_cat,
                       out_score, out_rank, out_matched, out_ignored);
    return lwdetr_check_launch();
}

extern "C" int lwdetr_cocoeval_match_host(const lwdetr_coco_gt* gt, const float* dets, const int32_t* rows, int B, int K,
                                          const double* iou_thrs, int32_t* out_cat, float* out_score, int32_t* out_rank,
                                          int64_t* out_matched, int64_t* out_ignored) {
    const int rc = check_match(gt, dets, rows, B, K, iou_thrs, out_cat, out_score, out_rank, out_matched, out_ignored);
    if (rc != LWDETR_OK) return rc;
    if (B == 0 || K == 0) return LWDETR_OK;
    match_host(*gt, dets, rows, B, K, iou_thrs, out_cat, out_score, out_rank, out_matched, out_ignored);
    return LWDETR_OK;
}

extern "C" int lwdetr_cocoeval_npig(const lwdetr_coco_gt* gt, const int32_t* rows, int n_rows, int32_t* npig, void* hip_stream) {
    const int rc = check_gt(gt);
    if (rc != LWDETR_OK) return rc;
    if (n_rows < 0 || !npig || (n_rows > 0 && !rows)) return LWDETR_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)hip_stream;
    if (hipMemsetAsync(npig, 0, sizeof(int32_t) * (size_t)gt->n_cats * CE_NA, st) != hipSuccess) return LWDETR_ERR_LAUNCH;
    if (n_rows == 0) return LWDETR_OK;
    hipLaunchKernelGGL(cocoeval_npig_kernel, dim3((unsigned)n_rows), dim3(64), 0, st, *gt, rows, npig);
    return lwdetr_check_launch();
}

extern "C" int lwdetr_cocoeval_curves(const int64_t* seg_off, const float* score, const int32_t* rank, const int64_t* matched,
                                      const int64_t* ignored, const int32_t* npig, const double* rec_thrs, int n_cats, long n_store,
                                      double* precision, double* scores, double* recall, void* hip_stream) {
    if (n_cats < 1 || n_store < 0 || !seg_off || !npig || !rec_thrs || !precision || !scores || !recall) return LWDETR_ERR_BAD_ARG;
    if (n_store > 0 && (!score || !rank || !matched || !ignored)) return LWDETR_ERR_BAD_ARG;
    if (n_cats > CE_MAXC) return LWDETR_ERR_UNSUPPORTED;
    CeRec rec;
    for (int r = 0; r < CE_NR; ++r) rec.v[r] = rec_thrs[r];
    for (int r = 1; r < CE_NR; ++r)
        if (!(rec.v[r - 1] <= rec.v[r])) return LWDETR_ERR_BAD_ARG;      // the look-up halves an ascending list
    hipLaunchKernelGGL(cocoeval_curves_kernel, dim3((unsigned)(n_cats * CE_NA * 3 * CE_NT)), dim3(256), 0, (hipStream_t)hip_stream, seg_off,
                       score, rank, matched, ignored, npig, rec, n_cats, n_store, precision, scores, recall);
    return lwdetr_check_launch();
}
