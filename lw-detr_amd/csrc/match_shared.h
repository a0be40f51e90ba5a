// Pieces shared by match.hip (evaluation criterion) and match_train.hip (training criterion): the box arithmetic of util/box_ops.py in
// f32, the per-lane pieces of the assignment solver (lsa_lane_*, __host__ __device__) with its host instantiation, and the packing of the
// host-side layer array. Everything has internal linkage: each of the two objects compiles its own copy.
#pragma once
#include "common.h"
#include <cfloat>
#include <climits>
#include <vector>
#define LSA_HD __host__ __device__ __forceinline__

namespace {

constexpr int LSA_WAVE = 64;
constexpr int CR_QCH = LWDETR_CRIT_QCHUNK;
constexpr int CR_THREADS = 256;
constexpr int CR_NPART = 5;                 // ce, l1, 1 - giou, rows with arg-max != C - 1, matched rows with arg-max == label

struct CritLayers {
    const void* logits[LWDETR_CRIT_MAX_LAYERS];
    const void* boxes[LWDETR_CRIT_MAX_LAYERS];
    int class_error[LWDETR_CRIT_MAX_LAYERS];
};

// ---- box arithmetic of util/box_ops.py in f32, operation by operation ------------------------------------------------------------------
struct Xyxy { float x0, y0, x1, y1; };
LSA_HD Xyxy cxcywh_to_xyxy(float cx, float cy, float w, float h) {        // box_ops.py:21-25 (w.clamp(min=0))
    const float wc = fmaxf(w, 0.f), hc = fmaxf(h, 0.f);
    Xyxy r;
    r.x0 = cx - 0.5f * wc; r.y0 = cy - 0.5f * hc; r.x1 = cx + 0.5f * wc; r.y1 = cy + 0.5f * hc;
    return r;
}
LSA_HD void box_iou_giou(const Xyxy& a, const Xyxy& b, float& iou, float& giou) {      // box_ops.py:36-73
    const float area1 = (a.x1 - a.x0) * (a.y1 - a.y0), area2 = (b.x1 - b.x0) * (b.y1 - b.y0);
    const float iw = fmaxf(fminf(a.x1, b.x1) - fmaxf(a.x0, b.x0), 0.f), ih = fmaxf(fminf(a.y1, b.y1) - fmaxf(a.y0, b.y0), 0.f);
    const float inter = iw * ih;
    const float uni = area1 + area2 - inter;
    iou = inter / uni;
    const float ew = fmaxf(fmaxf(a.x1, b.x1) - fminf(a.x0, b.x0), 0.f), eh = fmaxf(fmaxf(a.y1, b.y1) - fminf(a.y0, b.y0), 0.f);
    const float area = ew * eh;
    giou = iou - (area - uni) / area;
}
__device__ __forceinline__ float sigmoid_f32(float x) { return 1.f / (1.f + expf(-x)); }

template <int KPL> struct LsaLane {          // the columns lane, lane + 64, ..., lane + 64 (KPL - 1) of one problem
    double shortest[KPL];
    double v[KPL];
    unsigned visited;
};

LSA_HD double lsa_inf() { return __builtin_huge_val(); }
// total order of the arg-min: smaller value, equal values by lower column index (a is never NaN: `shortest` only takes values that compared less)
LSA_HD bool lsa_better(double a, int aj, double b, int bj) { return a < b || (a == b && aj < bj); }

template <int KPL> LSA_HD void lsa_lane_init(LsaLane<KPL>& s) {
#pragma unroll
    for (int k = 0; k < KPL; ++k) s.v[k] = 0.0;
}
template <int KPL> LSA_HD void lsa_lane_reset(LsaLane<KPL>& s) {
#pragma unroll
    for (int k = 0; k < KPL; ++k) s.shortest[k] = lsa_inf();
    s.visited = 0u;
}
// one step of the search: relax the lane's unvisited columns through row i, return the lane's best (value, column)
template <int KPL>
LSA_HD void lsa_lane_scan(LsaLane<KPL>& s, int lane, int nq, const float* crow, double ui, double minv, int i, volatile int* path,
                          double& best, int& bestj, int& bad) {
    best = lsa_inf();
    bestj = INT_MAX;
#pragma unroll
    for (int k = 0; k < KPL; ++k) {
        const int j = lane + LSA_WAVE * k;
        if (j < nq && !((s.visited >> k) & 1u)) {
            const float c = crow[j];
            if (!(fabsf(c) <= FLT_MAX)) bad = 1;
            const double r = minv + (double)c - ui - s.v[k];
            if (r < s.shortest[k]) { s.shortest[k] = r; path[j] = i; }
            if (lsa_better(s.shortest[k], j, best, bestj)) { best = s.shortest[k]; bestj = j; }
        }
    }
}
// the owner of the chosen column marks it visited; a column that was never relaxed in this search (only possible with non-finite costs)
// takes the row being scanned as predecessor, so that every visited column's predecessor chain ends at the search's root
template <int KPL> LSA_HD void lsa_lane_select(LsaLane<KPL>& s, int lane, int jsel, int i, volatile int* path) {
    if ((jsel & (LSA_WAVE - 1)) != lane) return;
#pragma unroll
    for (int k = 0; k < KPL; ++k)
        if (k == (jsel >> 6)) {
            s.visited |= 1u << k;
            if (!(s.shortest[k] < lsa_inf())) path[jsel] = i;
        }
}
// dual update of the visited columns and of the rows they are assigned to (before the augmentation rewires them)
template <int KPL>
LSA_HD void lsa_lane_dual(LsaLane<KPL>& s, int lane, double minv, const volatile int* row4col, volatile double* u) {
#pragma unroll
    for (int k = 0; k < KPL; ++k)
        if ((s.visited >> k) & 1u) {
            const int j = lane + LSA_WAVE * k;
            const double d = minv - s.shortest[k];
            const int r = row4col[j];
            if (r >= 0) u[r] = u[r] + d;
            s.v[k] -= d;
        }
}

LSA_HD int lsa_even(int n) { return (n + 1) & ~1; }
static size_t lsa_wave_bytes(int maxT, int kpl) { return (size_t)lsa_even(maxT) * 12 + (size_t)kpl * LSA_WAVE * 8; }

// the same solver with the 64 lanes emulated (one problem, host memory)
template <int KPL> void lsa_host(const float* cost, int nq, int T, int64_t* idx_q, int64_t* idx_t, int32_t* status, int32_t* steps) {
    constexpr int NQP = KPL * LSA_WAVE;
    std::vector<LsaLane<KPL>> lanes(LSA_WAVE);
    std::vector<double> u(T > 0 ? T : 1, 0.0);
    std::vector<int> col4row(T > 0 ? T : 1, -1), path(NQP, -1), row4col(NQP, -1);
    for (auto& s : lanes) lsa_lane_init(s);
    int nsteps = 0, bad = 0;
    for (int cur = 0; cur < T; ++cur) {
        for (auto& s : lanes) lsa_lane_reset(s);
        double minv = 0.0;
        int i = cur, sink = -1;
        for (int step = 0; step <= cur && sink < 0; ++step) {
            const double ui = u[i];
            double best = lsa_inf();
            int bestj = INT_MAX;
            for (int lane = 0; lane < LSA_WAVE; ++lane) {
                double lb;
                int lj;
                lsa_lane_scan(lanes[lane], lane, nq, cost + (size_t)i * nq, ui, minv, i, path.data(), lb, lj, bad);
                if (lsa_better(lb, lj, best, bestj)) { best = lb; bestj = lj; }
            }
            ++nsteps;
            minv = best;
            if (!(fabs(minv) <= DBL_MAX)) bad = 1;
            const int jsel = bestj;
            if (jsel >= nq) { bad = 1; break; }
            for (int lane = 0; lane < LSA_WAVE; ++lane) lsa_lane_select(lanes[lane], lane, jsel, i, path.data());
            const int r = row4col[jsel];
            if (r < 0) sink = jsel; else i = r;
        }
        if (sink < 0) { bad = 1; break; }
        u[cur] = u[cur] + minv;
        for (int lane = 0; lane < LSA_WAVE; ++lane) lsa_lane_dual(lanes[lane], lane, minv, row4col.data(), u.data());
        int j = sink;
        for (int n = 0; n <= cur; ++n) {
            const int ii = path[j];
            if (ii < 0 || ii >= T) { bad = 1; break; }
            const int jn = col4row[ii];
            row4col[j] = ii; col4row[ii] = j;
            if (ii == cur || jn < 0) break;
            j = jn;
        }
    }
    int cnt = 0;
    for (int j = 0; j < nq && cnt < T; ++j)
        if (row4col[j] >= 0) { idx_q[cnt] = j; idx_t[cnt] = row4col[j]; ++cnt; }
    if (status) *status = bad ? 1 : 0;
    if (steps) *steps = nsteps;
}

int lsa_kpl(int nq) {
    const int need = (nq + LSA_WAVE - 1) / LSA_WAVE;
    for (int k : {1, 2, 5, 8, 16}) if (need <= k) return k;
    return 0;
}

int pack_layers(const lwdetr_crit_layer* layers, int nlayers, CritLayers& L) {
    if (!layers || nlayers < 1 || nlayers > LWDETR_CRIT_MAX_LAYERS) return LWDETR_ERR_BAD_ARG;
    for (int l = 0; l < LWDETR_CRIT_MAX_LAYERS; ++l) {
        const bool on = l < nlayers;
        if (on && (!layers[l].logits || !layers[l].boxes)) return LWDETR_ERR_BAD_ARG;
        L.logits[l] = on ? layers[l].logits : nullptr;
        L.boxes[l] = on ? layers[l].boxes : nullptr;
        L.class_error[l] = on ? layers[l].class_error : 0;
    }
    return LWDETR_OK;
}
// sum of the host's counts (-1: a negative count or more than 2^31 - 1 targets), and their maximum
long sum_counts(const int32_t* counts, int B, int* maxT) {
    long s = 0;
    int mx = 0;
    for (int b = 0; b < B; ++b) {
        if (counts[b] < 0) return -1;
        s += counts[b];
        mx = counts[b] > mx ? counts[b] : mx;
    }
    if (maxT) *maxT = mx;
    return s > INT_MAX ? -1 : s;
}

}  // namespace
