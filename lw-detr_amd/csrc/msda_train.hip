// Differentiable deformable cross-attention for training, for gfx950: fused forward and backward of
//   loc = ref_xy + off / P * ref_wh * 0.5,  a = softmax_{L*P}(logits),  out[b, q, m*D + c] = sum_{l,p} a * bilinear(value)
// (reference models/ops/modules/ms_deform_attn.py:113-142 between the Linears, with the sampling rules of lwdetr_msda_forward). The forward
// saves nothing; the backward recomputes locations and weights with the same functions (this object is built without contraction, so they
// are the same bits) and runs two kernels, neither with a floating-point atomic:
//   * msda_train_bwd_q_kernel walks the (b, q, head) items. A group of D / 8 lanes owns one item (8 channels per lane, 16-byte corner loads), the
//     channel sums of d/d(loc) and d/d(weight) are xor-shuffle butterflies, the sum over points stays in the lane, and the sum over heads that
//     grad_ref needs goes through shared memory in head order: a workgroup always holds whole queries. It also leaves one record per sample in
//     the workspace: the sample's top-left pixel index and its four corner weights times the attention weight.
//   * msda_train_bwd_v_kernel owns value pixels. A one-wave workgroup holds the f32 gradient of one (image, head, band of value rows) in shared
//     memory, reads that (image, head)'s records level by level in query order, 512 at a time, queues the samples that touch its band (a ballot
//     and a prefix count keep the queue in query order), and adds them one after the other - the lanes of a step are the (corner, channel) pairs
//     of ONE sample, so no two of them meet in an element and the order of the additions into an element is the query order, whatever the
//     launch. The band is stored once, rounded.
// Every arithmetic step is f32; every output element is rounded once, on its store.
#include "common.h"

#include <atomic>
#include <math.h>
#include <type_traits>

namespace {

#define MT_HD __host__ __device__ __forceinline__

// ------------------------------------------------------------------ the per-sample functions, shared by the kernels and the host evaluation
constexpr int MT_NO_SAMPLE = -(1 << 30);               // record of a sample outside the map: below every band
constexpr int MT_MAX_LP = 16, MT_MAX_L = 4, MT_MAX_D = 64, MT_MAX_M = 256;
constexpr int MT_SLAB_FLOATS = 2048;                   // 8 KB of f32 gradient per one-wave workgroup of the pixel kernel

struct MtGeom { int hl, wl; float lh, lw; bool inside, c[4]; };

MT_HD float mt_loc(float ref_c, float off, float ref_s, int P) { return ref_c + off / (float)P * ref_s * 0.5f; }
MT_HD float mt_weight(float logit, float mx, float sum) { return expf(logit - mx) / sum; }

// corner k: bit 0 = right column, bit 1 = lower row. A sample outside the map (a non-finite location among them) has no corner.
MT_HD MtGeom mt_geom(float loc_x, float loc_y, int H, int W) {
    MtGeom g;
    const float h_raw = loc_y * H - 0.5f, w_raw = loc_x * W - 0.5f;
    g.inside = h_raw > -1.f && w_raw > -1.f && h_raw < (float)H && w_raw < (float)W;
    const float h_im = g.inside ? h_raw : 0.f, w_im = g.inside ? w_raw : 0.f;
    const float hf = floorf(h_im), wf = floorf(w_im);
    g.hl = (int)hf; g.wl = (int)wf; g.lh = h_im - hf; g.lw = w_im - wf;
    const bool t = g.hl >= 0, l = g.wl >= 0, b = g.hl + 1 <= H - 1, r = g.wl + 1 <= W - 1;
    g.c[0] = g.inside && t && l; g.c[1] = g.inside && t && r; g.c[2] = g.inside && b && l; g.c[3] = g.inside && b && r;
    return g;
}
MT_HD void mt_corner_weights(const MtGeom& g, float (&w)[4]) {
    const float hh = 1.f - g.lh, hw = 1.f - g.lw;
    w[0] = hh * hw; w[1] = hh * g.lw; w[2] = g.lh * hw; w[3] = g.lh * g.lw;
}
// one channel of one sample: v[k] is the corner's value (0 where the corner is outside the map or masked), tg the output gradient.
// ga: d out / d a; gx, gy: d out / d loc (in units of the normalised location).
MT_HD void mt_sample_grad(const MtGeom& g, int H, int W, float a, const float (&v)[4], float tg, float& ga, float& gx, float& gy) {
    const float hh = 1.f - g.lh, hw = 1.f - g.lw, tgv = tg * a;
    float gh = 0.f, gw = 0.f;
    gh -= hw * v[0]; gw -= hh * v[0];
    gh -= g.lw * v[1]; gw += hh * v[1];
    gh += hw * v[2]; gw -= g.lh * v[2];
    gh += g.lw * v[3]; gw += g.lh * v[3];
    ga += tg * (hh * hw * v[0] + hh * g.lw * v[1] + g.lh * hw * v[2] + g.lh * g.lw * v[3]);
    gx += (float)W * gw * tgv;
    gy += (float)H * gh * tgv;
}
MT_HD float mt_d_off(float g, float ref_s, int P) { return g * ref_s * 0.5f / (float)P; }
MT_HD float mt_d_size(float g, float off, int P) { return g * off * 0.5f / (float)P; }
MT_HD float mt_d_logit(float a, float ga, float dot) { return a * (ga - dot); }

// ------------------------------------------------------------------------------------------------------------------- launch-form record
// 0 .. 8: msda_train_fwd (dtype x form), 9 .. 17: msda_train_bwd_q, 18 .. 26: msda_train_bwd_v (dtype x pairs per lane 1 / 2 / 4 for D <= 16 / 32 / 64); form 0 = (L, P) = (1, 2), 1 = (2, 4), 2 = run-time.
constexpr int TP_COUNT = 27;
std::atomic<long> g_train_path[TP_COUNT];
const char* const kTrainPathNames[TP_COUNT] = {
    "msda_train_fwd_f32_l1p2", "msda_train_fwd_f32_l2p4", "msda_train_fwd_f32_gen", "msda_train_fwd_f16_l1p2", "msda_train_fwd_f16_l2p4",
    "msda_train_fwd_f16_gen", "msda_train_fwd_bf16_l1p2", "msda_train_fwd_bf16_l2p4", "msda_train_fwd_bf16_gen",
    "msda_train_bwd_q_f32_l1p2", "msda_train_bwd_q_f32_l2p4", "msda_train_bwd_q_f32_gen", "msda_train_bwd_q_f16_l1p2", "msda_train_bwd_q_f16_l2p4",
    "msda_train_bwd_q_f16_gen", "msda_train_bwd_q_bf16_l1p2", "msda_train_bwd_q_bf16_l2p4", "msda_train_bwd_q_bf16_gen",
    "msda_train_bwd_v_f32_e1", "msda_train_bwd_v_f32_e2", "msda_train_bwd_v_f32_e4", "msda_train_bwd_v_f16_e1", "msda_train_bwd_v_f16_e2",
    "msda_train_bwd_v_f16_e4", "msda_train_bwd_v_bf16_e1", "msda_train_bwd_v_bf16_e2", "msda_train_bwd_v_bf16_e4"};
template <typename T> constexpr int mp_dtype_of() { return std::is_same<T, float>::value ? 0 : std::is_same<T, f16>::value ? 1 : 2; }
inline int train_path_done(int path, int rc) {
    if (rc == LWDETR_OK && path >= 0 && path < TP_COUNT) g_train_path[path].fetch_add(1, std::memory_order_relaxed);
    return rc;
}

struct TrainParams {
    const void* value; long ld_v; const void* off; long ld_off; const void* lg; long ld_lg; const float* ref; const unsigned char* mask;
    const int64_t* shapes; const int64_t* lsi;
    int B, S, M, D, L, Q, P;
    void* out;                                                             // forward
    const void* go; void* g_value; void* g_off; void* g_lg; float* g_ref;  // backward
    float* rec_w; int* rec_base;                                           // workspace: 4 corner weights and the top-left pixel per sample
    int gs, qpb, band, pshift;
};

template <typename T> __device__ __forceinline__ void load8(const T* p, float (&f)[8]) {
    const typename Vec<T>::v8 v = *(const typename Vec<T>::v8*)p;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = to_f32<T>(v[e]);
}
template <> __device__ __forceinline__ void load8<float>(const float* p, float (&f)[8]) {       // two 16-byte pieces: a row of a Linear's output is 16-byte aligned
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[e] = a[e]; f[4 + e] = b[e]; }
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float (&f)[8]) {
    typename Vec<T>::v8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = from_f32<T>(f[e]);
    *(typename Vec<T>::v8*)p = o;
}
template <> __device__ __forceinline__ void store8<float>(float* p, const float (&f)[8]) {
    f32x4 a, b;
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] = f[e]; b[e] = f[4 + e]; }
    *(f32x4*)p = a; *(f32x4*)(p + 4) = b;
}

// maximum and sum of exponentials of the L*P logits of one (row, head): the forward and the backward call this one function
template <typename T, int LPC> __device__ __forceinline__ void mt_softmax_stats(const T* lgp, int LP, float& mx, float& sum) {
    mx = -INFINITY; sum = 0.f;
    if (LPC > 0) {
#pragma unroll
        for (int i = 0; i < LPC; ++i) mx = fmaxf(mx, to_f32<T>(lgp[i]));
#pragma unroll
        for (int i = 0; i < LPC; ++i) sum += expf(to_f32<T>(lgp[i]) - mx);
    } else {
        for (int i = 0; i < LP; ++i) mx = fmaxf(mx, to_f32<T>(lgp[i]));
        for (int i = 0; i < LP; ++i) sum += expf(to_f32<T>(lgp[i]) - mx);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ forward
// One lane owns 8 channels of one (b, q, head).
template <typename T, int TL, int TP>
__global__ __launch_bounds__(256) void msda_train_fwd_kernel(TrainParams p) {
    const int DC = p.D >> 3;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)p.B * p.Q * p.M * DC) return;
    const int dc = (int)(idx % DC);
    const long item = idx / DC;
    const int m = (int)(item % p.M);
    const long row = item / p.M;
    const int b = (int)(row / p.Q);
    const int L = TL > 0 ? TL : p.L, P = TP > 0 ? TP : p.P, LP = L * P;
    const T* offp = (const T*)p.off + row * p.ld_off + (long)m * LP * 2;
    const T* lgp = (const T*)p.lg + row * p.ld_lg + (long)m * LP;
    float mx, sum;
    mt_softmax_stats<T, TL * TP>(lgp, LP, mx, sum);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int l = 0; l < (TL > 0 ? TL : MT_MAX_L); ++l) {
        if (l >= L) break;
        const int H = (int)p.shapes[2 * l], W = (int)p.shapes[2 * l + 1];
        const float* rf = p.ref + (row * L + l) * 4;
        const float cx = rf[0], cy = rf[1], bw = rf[2], bh = rf[3];
        const long s0 = (long)b * p.S + p.lsi[l];
        const T* vbase = (const T*)p.value + s0 * p.ld_v + (long)m * p.D + dc * 8;
        const unsigned char* mk = p.mask ? p.mask + s0 : nullptr;
#pragma unroll
        for (int pt = 0; pt < (TP > 0 ? TP : 8); ++pt) {
            if (pt >= P) break;
            const int i = l * P + pt;
            const float ox = to_f32<T>(offp[2 * i]), oy = to_f32<T>(offp[2 * i + 1]);
            const MtGeom g = mt_geom(mt_loc(cx, ox, bw, P), mt_loc(cy, oy, bh, P), H, W);
            const float a = mt_weight(to_f32<T>(lgp[i]), mx, sum);
            float cw[4];
            mt_corner_weights(g, cw);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long pix = (long)(g.hl + (k >> 1)) * W + g.wl + (k & 1);
                if (g.c[k] && !(mk && mk[pix])) {
                    float v[8];
                    load8<T>(vbase + pix * p.ld_v, v);
                    const float w = cw[k] * a;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += w * v[e];
                }
            }
        }
    }
    store8<T>((T*)p.out + row * ((long)p.M * p.D) + (long)m * p.D + dc * 8, acc);
}

// ------------------------------------------------------------------------------------------------------------- backward, the query side
// Workgroup = qpb whole queries; a group of gs lanes (a power of two >= D / 8, inside one wave) owns one (query, head) at a time.
// Shared memory: [256 / gs][16] d/d(weight) of the item a group works on, then [qpb * M][L][4] per-head sums for grad_ref.
template <typename T, int TL, int TP>
__global__ __launch_bounds__(256) void msda_train_bwd_q_kernel(TrainParams p) {
    extern __shared__ float smem[];
    const int GS = p.gs, SLOTS = 256 / GS;
    const int slot = threadIdx.x / GS, gl = threadIdx.x & (GS - 1);
    const int L = TL > 0 ? TL : p.L, P = TP > 0 ? TP : p.P, LP = L * P;
    const long nrows = (long)p.B * p.Q;
    const long row0 = (long)blockIdx.x * p.qpb;
    const int nitems = p.qpb * p.M;
    float* stash = smem + slot * MT_MAX_LP;
    float* part = smem + SLOTS * MT_MAX_LP;
    const bool active = gl * 8 < p.D;                       // D = 24, 40, 48, 56: the last lanes of a group carry no channel
    const int ch = active ? gl * 8 : 0;
    const long wo = (long)p.M * p.D;
    for (int base = 0; base < nitems; base += SLOTS) {      // the same trip count in every lane: the shuffles below need whole groups
        const int it = base + slot;
        const int m = it % p.M;
        const long row = row0 + it / p.M;
        const bool live = it < nitems && row < nrows;
        const long r = live ? row : nrows - 1;              // a dead group shadows the last row and stores nothing
        const int b = (int)(r / p.Q), q = (int)(r % p.Q);
        const T* offp = (const T*)p.off + r * p.ld_off + (long)m * LP * 2;
        const T* lgp = (const T*)p.lg + r * p.ld_lg + (long)m * LP;
        float mx, sum;
        mt_softmax_stats<T, TL * TP>(lgp, LP, mx, sum);
        float tg[8];
        load8<T>((const T*)p.go + r * wo + (long)m * p.D + ch, tg);
        T* g_off = (T*)p.g_off + (r * p.M + m) * (long)(LP * 2);
        T* g_lg = (T*)p.g_lg + (r * p.M + m) * (long)LP;
        float dot = 0.f;
#pragma unroll
        for (int l = 0; l < (TL > 0 ? TL : MT_MAX_L); ++l) {
            if (l >= L) break;
            const int H = (int)p.shapes[2 * l], W = (int)p.shapes[2 * l + 1];
            const float* rf = p.ref + (r * L + l) * 4;
            const float cx = rf[0], cy = rf[1], bw = rf[2], bh = rf[3];
            const long s0 = (long)b * p.S + p.lsi[l];
            const T* vbase = (const T*)p.value + s0 * p.ld_v + (long)m * p.D + ch;
            const unsigned char* mk = p.mask ? p.mask + s0 : nullptr;
            const long rec0 = (((long)b * p.M + m) * L + l) * ((long)p.Q * P) + (long)q * P;
            float rx = 0.f, ry = 0.f, rw = 0.f, rh = 0.f;
#pragma unroll
            for (int pt = 0; pt < (TP > 0 ? TP : 8); ++pt) {
                if (pt >= P) break;
                const int i = l * P + pt;
                const float ox = to_f32<T>(offp[2 * i]), oy = to_f32<T>(offp[2 * i + 1]);
                const MtGeom g = mt_geom(mt_loc(cx, ox, bw, P), mt_loc(cy, oy, bh, P), H, W);
                const float a = mt_weight(to_f32<T>(lgp[i]), mx, sum);
                float ga = 0.f, gx = 0.f, gy = 0.f;
                if (g.inside && active) {
                    float v[4][8];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const long pix = (long)(g.hl + (k >> 1)) * W + g.wl + (k & 1);
                        if (g.c[k] && !(mk && mk[pix])) load8<T>(vbase + pix * p.ld_v, v[k]);
                        else {
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[k][e] = 0.f;
                        }
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float vv[4] = {v[0][e], v[1][e], v[2][e], v[3][e]};
                        mt_sample_grad(g, H, W, a, vv, tg[e], ga, gx, gy);
                    }
                }
                for (int o = GS >> 1; o >= 1; o >>= 1) {                       // a butterfly: every lane of the group ends with the same bits
                    ga += __shfl_xor(ga, o); gx += __shfl_xor(gx, o); gy += __shfl_xor(gy, o);
                }
                if (live && gl == 0) {
                    float cw[4];
                    mt_corner_weights(g, cw);
                    float* rwp = p.rec_w + (rec0 + pt) * 4;
#pragma unroll
                    for (int k = 0; k < 4; ++k) rwp[k] = g.c[k] ? cw[k] * a : 0.f;
                    p.rec_base[rec0 + pt] = g.inside ? g.hl * W + g.wl : MT_NO_SAMPLE;
                    g_off[2 * i] = from_f32<T>(mt_d_off(gx, bw, P));
                    g_off[2 * i + 1] = from_f32<T>(mt_d_off(gy, bh, P));
                    stash[i] = ga;
                }
                dot += a * ga;
                rx += gx; ry += gy; rw += mt_d_size(gx, ox, P); rh += mt_d_size(gy, oy, P);
            }
            if (live && gl == 0) {
                float* pp = part + ((long)it * L + l) * 4;
                pp[0] = rx; pp[1] = ry; pp[2] = rw; pp[3] = rh;
            }
        }
        if (live && gl == 0)
            for (int i = 0; i < LP; ++i) g_lg[i] = from_f32<T>(mt_d_logit(mt_weight(to_f32<T>(lgp[i]), mx, sum), stash[i], dot));
    }
    __syncthreads();
    const int L4 = L * 4;
    for (int t = threadIdx.x; t < p.qpb * L4; t += 256) {   // grad_ref: the heads of a query, in head order
        const int qi = t / L4, rem = t - qi * L4;
        const long row = row0 + qi;
        if (row >= nrows) continue;
        float s = 0.f;
        for (int m = 0; m < p.M; ++m) s += part[((long)(qi * p.M + m)) * L4 + rem];
        p.g_ref[row * L4 + rem] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------- backward, the pixel side
// Shared memory of the one-wave workgroup: the band [band][D] f32, then a queue of up to 64 samples that touch the band - record index and
// top-left pixel, the 4 corner weights, the D output-gradient values. The wave reads 512 records per step (eight independent loads per
// lane), appends the hits of each 64 in lane order - a ballot and a prefix count, so the queue is in query order - and when the queue is
// full it fetches the weights and gradient rows of all its samples at once (one memory latency per 64 samples, not per sample) and then adds the
// samples one after the other, reading sample h + 1's operands from shared memory while sample h is added: the lanes of a step are the
// (corner, channel) pairs of ONE sample.
constexpr int MT_QUEUE = 64, MT_SCAN = 8;

// NJ: (corner, channel) pairs per lane, 4 D / 64 rounded up to 1, 2 or 4 - the per-sample step is instruction bound, so D <= 16 gets the one-pair form
template <typename T, int NJ>
__global__ __launch_bounds__(64) void msda_train_bwd_v_kernel(TrainParams p) {
    extern __shared__ float slab[];                          // [band][D] | queue
    const int lane = threadIdx.x, D = p.D;
    const int nb = (p.S + p.band - 1) / p.band;
    const int sb = blockIdx.x % nb, m = (blockIdx.x / nb) % p.M, b = blockIdx.x / (nb * p.M);
    const long s0 = (long)sb * p.band, s1 = s0 + p.band < p.S ? s0 + p.band : p.S;
    const int nslab = (int)(s1 - s0) * D;
    int* qn = (int*)(slab + p.band * D);
    int* qbase = qn + MT_QUEUE;
    float* qw = (float*)(qbase + MT_QUEUE);                  // [64][4]
    float* qtg = qw + MT_QUEUE * 4;                          // [64][D]
    for (int i = lane; i < nslab; i += 64) slab[i] = 0.f;
    int ek[NJ], ec[NJ]; bool ev[NJ];                            // this lane's (corner, channel) pairs of a sample
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = lane + 64 * j;
        ev[j] = e < 4 * D; ek[j] = ev[j] ? e / D : 0; ec[j] = ev[j] ? e % D : 0;
    }
    const long wo = (long)p.M * D;
    const T* go = (const T*)p.go + (long)b * p.Q * wo + (long)m * D;
    const long nrec = (long)p.Q * p.P;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int l = 0; l < p.L; ++l) {
        const int H = (int)p.shapes[2 * l], W = (int)p.shapes[2 * l + 1];
        const long lsi = p.lsi[l];
        const long a0 = s0 > lsi ? s0 : lsi, a1 = s1 < lsi + (long)H * W ? s1 : lsi + (long)H * W;
        if (a0 >= a1) continue;                              // this level has no pixel in the band
        const int p0 = (int)(a0 - lsi), p1 = (int)(a1 - lsi), slab_px = (int)(a0 - s0) - p0;
        const long recb = (((long)b * p.M + m) * p.L + l) * nrec;
        const int* rb = p.rec_base + recb;
        const f32x4* rw = (const f32x4*)(p.rec_w + recb * 4);
        int qcount = 0;                                      // wave-uniform
        auto flush = [&]() {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (lane < qcount) {
                const f32x4 w = rw[qn[lane]];
#pragma unroll
                for (int k = 0; k < 4; ++k) qw[lane * 4 + k] = w[k];
            }
            for (int e0 = lane; e0 < qcount * D; e0 += 64 * 8) {          // eight independent loads per lane before the first is stored
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int e = e0 + 64 * u, ee = e < qcount * D ? e : 0, h = ee / D, c = ee - h * D;
                    v[u] = to_f32<T>(go[(long)(qn[h] >> p.pshift) * wo + c]);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (e0 + 64 * u < qcount * D) qtg[e0 + 64 * u] = v[u];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            // one sample per step, in query order; sample h + 1's pixel, weights and gradient row are read while sample h is added
            int base_n = qbase[0];
            float wn[NJ], tgn[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) { wn[j] = qw[ek[j]]; tgn[j] = qtg[ec[j]]; }
            for (int h = 0; h < qcount; ++h) {
                const int base = base_n, nx = h + 1 < qcount ? h + 1 : h;
                float w[NJ], tg[NJ];
#pragma unroll
                for (int j = 0; j < NJ; ++j) { w[j] = wn[j]; tg[j] = tgn[j]; }
                base_n = qbase[nx];
#pragma unroll
                for (int j = 0; j < NJ; ++j) { wn[j] = qw[nx * 4 + ek[j]]; tgn[j] = qtg[nx * D + ec[j]]; }
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int pi = base + (ek[j] & 1) + (ek[j] >> 1) * W;
                    if (ev[j] && pi >= p0 && pi < p1 && w[j] != 0.f) slab[(slab_px + pi) * D + ec[j]] += w[j] * tg[j];
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");    // the next sample's lanes may read what other lanes wrote here
            }
            qcount = 0;
        };
        for (long c0 = 0; c0 < nrec; c0 += 64 * MT_SCAN) {
            int bs[MT_SCAN];
#pragma unroll
            for (int j = 0; j < MT_SCAN; ++j) {
                const long n = c0 + j * 64 + lane;
                bs[j] = n < nrec ? rb[n] : MT_NO_SAMPLE;
            }
#pragma unroll
            for (int j = 0; j < MT_SCAN; ++j) {
                const bool hit = bs[j] != MT_NO_SAMPLE && bs[j] + W + 1 >= p0 && bs[j] < p1;
                const unsigned long long hm = __ballot(hit);
                const int cnt = __popcll(hm);
                if (qcount + cnt > MT_QUEUE) flush();
                if (hit) {
                    const int r = qcount + __popcll(hm & below);
                    qn[r] = (int)(c0 + j * 64 + lane); qbase[r] = bs[j];
                }
                qcount += cnt;
            }
        }
        flush();
    }
    const unsigned char* mk = p.mask ? p.mask + (long)b * p.S : nullptr;
    T* gv = (T*)p.g_value + ((long)b * p.S) * wo + (long)m * D;
    for (int i = lane; i < nslab; i += 64) {
        const int px = i / D, c = i - px * D;
        const long s = s0 + px;
        gv[s * wo + c] = from_f32<T>(mk && mk[s] ? 0.f : slab[i]);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------- host
int form_of(int L, int P) { return L == 1 && P == 2 ? 0 : L == 2 && P == 4 ? 1 : 2; }
bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }
size_t esize(int dtype) { return dtype == DT_F32 ? 4 : 2; }

// LWDETR_ERR_UNSUPPORTED / LWDETR_ERR_BAD_ARG of the header, in this order; touches no runtime
int check_desc(const lwdetr_msda_train_desc* d) {
    if (!d) return LWDETR_ERR_BAD_ARG;
    if (d->B < 1 || d->S < 1 || d->M < 1 || d->D < 1 || d->L < 1 || d->Q < 1 || d->P < 1) return LWDETR_ERR_BAD_ARG;
    if (d->dtype != DT_F32 && d->dtype != DT_F16 && d->dtype != DT_BF16) return LWDETR_ERR_UNSUPPORTED;
    if (d->D % 8 != 0 || d->D > MT_MAX_D || d->L > MT_MAX_L || !(d->P == 1 || d->P == 2 || d->P == 4 || d->P == 8) || d->L * d->P > MT_MAX_LP ||
        d->M > MT_MAX_M)
        return LWDETR_ERR_UNSUPPORTED;
    if (!d->value || !d->offsets || !d->logits || !d->ref || !d->shapes || !d->level_start) return LWDETR_ERR_BAD_ARG;
    const size_t es = esize(d->dtype);
    const long mlp = (long)d->M * d->L * d->P;
    if (d->value_ld < (long)d->M * d->D || d->offsets_ld < 2 * mlp || d->logits_ld < mlp) return LWDETR_ERR_BAD_ARG;
    if (!al16(d->value) || (d->value_ld * es) % 16 != 0) return LWDETR_ERR_BAD_ARG;
    if ((uintptr_t)d->offsets % es != 0 || (uintptr_t)d->logits % es != 0 || (uintptr_t)d->ref % 4 != 0 || (uintptr_t)d->shapes % 8 != 0 ||
        (uintptr_t)d->level_start % 8 != 0)
        return LWDETR_ERR_BAD_ARG;
    if ((long)d->B * d->Q * d->M * (d->D / 8) > 0x7fffffffL * 256 || (long)d->Q * d->P > 0x7fffffffL) return LWDETR_ERR_BAD_ARG;
    return LWDETR_OK;
}

TrainParams params_of(const lwdetr_msda_train_desc* d) {
    TrainParams p = {};
    p.value = d->value; p.ld_v = d->value_ld; p.off = d->offsets; p.ld_off = d->offsets_ld; p.lg = d->logits; p.ld_lg = d->logits_ld;
    p.ref = d->ref; p.mask = d->mask; p.shapes = d->shapes; p.lsi = d->level_start;
    p.B = d->B; p.S = d->S; p.M = d->M; p.D = d->D; p.L = d->L; p.Q = d->Q; p.P = d->P;
    return p;
}

template <typename T> int launch_fwd(TrainParams p, hipStream_t st) {
    const long n = (long)p.B * p.Q * p.M * (p.D >> 3);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const int form = form_of(p.L, p.P);
    if (form == 0) hipLaunchKernelGGL((msda_train_fwd_kernel<T, 1, 2>), grid, block, 0, st, p);
    else if (form == 1) hipLaunchKernelGGL((msda_train_fwd_kernel<T, 2, 4>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((msda_train_fwd_kernel<T, 0, 0>), grid, block, 0, st, p);
    return train_path_done(mp_dtype_of<T>() * 3 + form, lwdetr_check_launch());
}

template <typename T> int launch_bwd(TrainParams p, hipStream_t st) {
    int gs = 1;
    while (gs * 8 < p.D) gs <<= 1;
    const int slots = 256 / gs;
    p.gs = gs;
    p.qpb = slots / p.M > 0 ? slots / p.M : 1;
    const long rows = (long)p.B * p.Q, blocks = (rows + p.qpb - 1) / p.qpb;
    const size_t smem_q = ((size_t)slots * MT_MAX_LP + (size_t)p.qpb * p.M * p.L * 4) * sizeof(float);
    const int form = form_of(p.L, p.P);
    {
        const dim3 grid((unsigned)blocks), block(256);
        if (form == 0) hipLaunchKernelGGL((msda_train_bwd_q_kernel<T, 1, 2>), grid, block, smem_q, st, p);
        else if (form == 1) hipLaunchKernelGGL((msda_train_bwd_q_kernel<T, 2, 4>), grid, block, smem_q, st, p);
        else hipLaunchKernelGGL((msda_train_bwd_q_kernel<T, 0, 0>), grid, block, smem_q, st, p);
        const int rc = train_path_done(9 + mp_dtype_of<T>() * 3 + form, lwdetr_check_launch());
        if (rc != LWDETR_OK) return rc;
    }
    p.band = MT_SLAB_FLOATS / p.D;
    p.pshift = p.P == 1 ? 0 : p.P == 2 ? 1 : p.P == 4 ? 2 : 3;
    const long nb = ((long)p.S + p.band - 1) / p.band;
    const size_t smem_v = ((size_t)p.band * p.D + MT_QUEUE * (6 + p.D)) * sizeof(float);           // the band, then the queue
    const dim3 grid_v((unsigned)(nb * p.M * p.B)), block_v(64);
    const int nj = p.D <= 16 ? 0 : p.D <= 32 ? 1 : 2;
    if (nj == 0) hipLaunchKernelGGL((msda_train_bwd_v_kernel<T, 1>), grid_v, block_v, smem_v, st, p);
    else if (nj == 1) hipLaunchKernelGGL((msda_train_bwd_v_kernel<T, 2>), grid_v, block_v, smem_v, st, p);
    else hipLaunchKernelGGL((msda_train_bwd_v_kernel<T, 4>), grid_v, block_v, smem_v, st, p);
    return train_path_done(18 + mp_dtype_of<T>() * 3 + nj, lwdetr_check_launch());
}

}  // namespace

extern "C" {

// See include/lwdetr_hip.h for the contract.
int lwdetr_msda_train_forward(const lwdetr_msda_train_desc* desc, void* out, void* hip_stream) {
    const int rc = check_desc(desc);
    if (rc != LWDETR_OK) return rc;
    if (!out || !al16(out)) return LWDETR_ERR_BAD_ARG;
    TrainParams p = params_of(desc);
    p.out = out;
    hipStream_t st = (hipStream_t)hip_stream;
    switch (desc->dtype) {
        case DT_F32: return launch_fwd<float>(p, st);
        case DT_F16: return launch_fwd<f16>(p, st);
        default: return launch_fwd<bf16>(p, st);
    }
}

long lwdetr_msda_train_workspace_bytes(const lwdetr_msda_train_desc* desc) {
    if (check_desc(desc) != LWDETR_OK) return 0;
    return (long)desc->B * desc->M * desc->L * desc->Q * desc->P * 20;       // 4 f32 corner weights + 1 int32 pixel index per sample
}

int lwdetr_msda_train_backward(const lwdetr_msda_train_desc* desc, const void* grad_out, void* grad_value, void* grad_offsets, void* grad_logits,
                               float* grad_ref, void* workspace, long workspace_bytes, void* hip_stream) {
    const int rc = check_desc(desc);
    if (rc != LWDETR_OK) return rc;
    if (!grad_out || !grad_value || !grad_offsets || !grad_logits || !grad_ref || !workspace) return LWDETR_ERR_BAD_ARG;
    const size_t es = esize(desc->dtype);
    if (!al16(grad_out) || !al16(workspace) || (uintptr_t)grad_value % es != 0 || (uintptr_t)grad_offsets % es != 0 ||
        (uintptr_t)grad_logits % es != 0 || (uintptr_t)grad_ref % 4 != 0)
        return LWDETR_ERR_BAD_ARG;
    const long nrec = (long)desc->B * desc->M * desc->L * desc->Q * desc->P;
    const long nb = ((long)desc->S + MT_SLAB_FLOATS / desc->D - 1) / (MT_SLAB_FLOATS / desc->D);
    if (workspace_bytes < nrec * 20 || nb * desc->M * desc->B > 0x7fffffffL) return LWDETR_ERR_BAD_ARG;
    TrainParams p = params_of(desc);
    p.go = grad_out; p.g_value = grad_value; p.g_off = grad_offsets; p.g_lg = grad_logits; p.g_ref = grad_ref;
    p.rec_w = (float*)workspace; p.rec_base = (int*)((float*)workspace + nrec * 4);
    hipStream_t st = (hipStream_t)hip_stream;
    switch (desc->dtype) {
        case DT_F32: return launch_bwd<float>(p, st);
        case DT_F16: return launch_bwd<f16>(p, st);
        default: return launch_bwd<bf16>(p, st);
    }
}

int lwdetr_msda_train_backward_host(const float* value, long value_ld, const unsigned char* mask, const int64_t* shapes, const int64_t* level_start,
                                    int D, int L, int P, const float* offsets, const float* logits, const float* ref, const float* grad_out,
                                    float* grad_value, long grad_value_ld, float* grad_offsets, float* grad_logits, float* grad_ref) {
    if (!value || !shapes || !level_start || !offsets || !logits || !ref || !grad_out || !grad_value || !grad_offsets || !grad_logits || !grad_ref)
        return LWDETR_ERR_BAD_ARG;
    if (D < 1 || L < 1 || P < 1 || value_ld < D || grad_value_ld < D) return LWDETR_ERR_BAD_ARG;
    if (L * P > MT_MAX_LP) return LWDETR_ERR_UNSUPPORTED;
    const int LP = L * P;
    float mx = -INFINITY, sum = 0.f, ga_all[MT_MAX_LP], dot = 0.f;
    for (int i = 0; i < LP; ++i) mx = fmaxf(mx, logits[i]);
    for (int i = 0; i < LP; ++i) sum += expf(logits[i] - mx);
    for (int l = 0; l < L; ++l) {
        const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
        const float cx = ref[4 * l], cy = ref[4 * l + 1], bw = ref[4 * l + 2], bh = ref[4 * l + 3];
        const long s0 = level_start[l];
        float rx = 0.f, ry = 0.f, rw = 0.f, rh = 0.f;
        for (int pt = 0; pt < P; ++pt) {
            const int i = l * P + pt;
            const float ox = offsets[2 * i], oy = offsets[2 * i + 1];
            const MtGeom g = mt_geom(mt_loc(cx, ox, bw, P), mt_loc(cy, oy, bh, P), H, W);
            const float a = mt_weight(logits[i], mx, sum);
            float cw[4], ga = 0.f, gx = 0.f, gy = 0.f;
            mt_corner_weights(g, cw);
            long px[4];
            bool use[4];
            for (int k = 0; k < 4; ++k) {
                px[k] = s0 + (long)(g.hl + (k >> 1)) * W + g.wl + (k & 1);
                use[k] = g.c[k] && !(mask && mask[px[k]]);
            }
            for (int c = 0; c < D; ++c) {
                float v[4];
                for (int k = 0; k < 4; ++k) v[k] = use[k] ? value[px[k] * value_ld + c] : 0.f;
                if (g.inside) mt_sample_grad(g, H, W, a, v, grad_out[c], ga, gx, gy);
                for (int k = 0; k < 4; ++k)
                    if (use[k]) grad_value[px[k] * grad_value_ld + c] += (cw[k] * a) * grad_out[c];
            }
            grad_offsets[2 * i] = mt_d_off(gx, bw, P);
            grad_offsets[2 * i + 1] = mt_d_off(gy, bh, P);
            ga_all[i] = ga;
            dot += a * ga;
            rx += gx; ry += gy; rw += mt_d_size(gx, ox, P); rh += mt_d_size(gy, oy, P);
        }
        grad_ref[4 * l] += rx; grad_ref[4 * l + 1] += ry; grad_ref[4 * l + 2] += rw; grad_ref[4 * l + 3] += rh;
    }
    for (int i = 0; i < LP; ++i) grad_logits[i] = mt_d_logit(mt_weight(logits[i], mx, sum), ga_all[i], dot);
    return LWDETR_OK;
}

int lwdetr_msda_train_path_counts(long* out, int n) {
    for (int i = 0; out && i < n && i < TP_COUNT; ++i) out[i] = g_train_path[i].load(std::memory_order_relaxed);
    return TP_COUNT;
}
const char* lwdetr_msda_train_path_name(int i) { return i >= 0 && i < TP_COUNT ? kTrainPathNames[i] : nullptr; }

}  // extern "C"
