// Differentiable fused softmax(c Q K^T) V for gfx950: the ViT attention core of the reference's TRAINING step (models/backbone/vit.py:130-137),
// forward and backward, without the N x N score / weight tensors that autograd keeps there.
//
//   forward : o_q = sum_k a_qk v_k, a = softmax_k(c q_q . k_k); writes o and lse_q = log sum_k exp(s_qk) (f32, natural log)
//   backward: D_q = do_q . o_q, p_qk = exp(s_qk - lse_q), dv_k = sum_q p_qk do_q, ds_qk = p_qk (do_q . v_k - D_q),
//             dq_q = c sum_k ds_qk k_k, dk_k = c sum_q ds_qk q_q            (p is recomputed from q, k and lse: nothing of size N x N exists)
//
// The scaled score is ONE f32 product, fl(c fl(q . k)), in the forward and in both backward kernels, and the MFMA chains that form q . k sum in
// the same order in all of them: the backward sees the forward's score bit for bit, so the rounding of a large score (|s| u) cancels against the
// same rounding inside lse instead of showing up in p. That is why this object is built with -ffp-contract=off (Makefile): HIP's __fmul_rn is a
// plain product, and hipcc otherwise fuses it with the subtraction that follows into one FMA in the backward but not in the forward.
//
// Operands are strided (base + b*sb + n*sn + h*sh + d, elements), so q / k / v are views qkv[:, :, i] of the reference's (B, N, 3, heads, hd)
// tensor and dq / dk / dv are views of one gradient buffer of that shape; o / do are (B, N, heads*hd) with a row stride. Every output element
// is written by the call; there are no atomics on any output, and every sum has one fixed order: two calls give the same bits.
//
// Structure. Waves are independent (no LDS, no barriers, as attn_kernel of attention.hip): one wave owns one 16-row block of one
// (batch, head) and walks the other axis in steps of at_kt(hd) 16-row tiles (64 rows a step at hd 16 / 32, 32 at hd 64; masks, clamps and
// MFMAs work on the 16-row tile); a 256-thread workgroup is four such waves of consecutive blocks, so a 49-key window costs four waves of
// whichever workgroups they fall into, and a 1600-key sequence spreads over 100 waves per head.
// All products are 16x16 MFMAs through Mma<T>::k16 (common.h): v_mfma_f32_16x16x16_{f16,bf16} for the 16-bit types and four exact
// v_mfma_f32_16x16x4_f32 for f32 - no down-conversion of f32 operands; scores, p, ds and all accumulators are f32, p and ds are rounded to T
// only as operands of their second MFMA. The first product of every pair is oriented so that its accumulator (row 4g + r in the registers,
// column on the lane) is already the B operand of the second, which sums over that row index:
//   forward / dQ  (wave owns 16 queries, loops over keys):   S^T = K Q^T, dP^T = V dO^T  ->  O^T += V^T P^T,  dQ^T += K^T dS^T
//   dK / dV       (wave owns 16 keys, loops over queries):   S = Q K^T,  dP = dO V^T     ->  dV^T += dO^T P,  dK^T += Q^T dS
// Row operands are 4-element vector loads; the transposed operands (V^T, K^T, dO^T, Q^T) are gathered element-wise through L1 / L2.
//
// Launch forms - a function of N only (hd and dtype select the instantiation, not the form):
//   forward               attn_train_fwd_<dt>_hd<HD>            every N
//   backward, N <= 256    attn_train_bwd_one_<dt>_hd<HD>        ONE launch: wave i computes D in registers, dQ of query block i, then dK / dV of
//                                                               key block i (the whole (sequence, head) is <= 16 waves and its operands stay in L1 / L2)
//   backward, N >  256    attn_train_bwd_dot_<dt>               D = rowsum(dO o) into the workspace (B * heads * N floats), then
//                         attn_train_bwd_dkdv_<dt>_hd<HD>       a wave per key block, and
//                         attn_train_bwd_dq_<dt>_hd<HD>         a wave per query block: both recompute p
// The one-launch form recomputes D per (block, tile) pair - one more row operand per tile - and saves two launch boundaries and the round trip
// of D. kAttnTrainOneLaunchMaxN = 256 covers every window of the recipes (49 ... 196 keys) and no global block (784 ...); the threshold itself
// was chosen, not measured.
#include "common.h"
#include <atomic>
#include <cmath>
#include <cstdio>
#include <type_traits>

namespace {

constexpr int kAttnTrainOneLaunchMaxN = 256;

struct ATParams {
    const void *q, *k, *v, *o, *d_o;
    void *out, *dq, *dk, *dv;
    float* lse;
    float* D;
    long q_sb, q_sn, q_sh, k_sb, k_sn, k_sh, v_sb, v_sn, v_sh, o_ld, do_ld;
    long dq_sb, dq_sn, dq_sh, dk_sb, dk_sn, dk_sh, dv_sb, dv_sn, dv_sh;
    int B, heads, N, nblk;
    long nwaves;
    float scale;
};

// 16-row MFMA tiles per loop step: the loads and score MFMAs of a step are independent of one another, and the forward reduces its row maximum
// once per step. 64 rows a step at hd 16 / 32, 32 at hd 64 (register budget). Tiles of a ragged last step that lie wholly past N are clamped
// loads with p = 0.
constexpr int at_kt(int hd) { return hd == 64 ? 2 : 4; }

// reductions over the four lane groups g on the VALU (v_permlane16_swap / v_permlane32_swap, as attention.hip) instead of ds_bpermute
__device__ __forceinline__ float at_gmax(float v) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float at_gsum(float v) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

template <typename T> __device__ __forceinline__ typename Vec<T>::v4 at_row4(const T* p) { return *(const typename Vec<T>::v4*)p; }
// transposed operand: element r <- X[min(row0 + r, last)][col]
template <typename T> __device__ __forceinline__ typename Vec<T>::v4 at_gather4(const T* base, long sn, int row0, int last, int col) {
    typename Vec<T>::v4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = row0 + r < last ? row0 + r : last;
        v[r] = base[(long)row * sn + col];
    }
    return v;
}
// The loops run their whole steps (every row < N) without clamps and masks, so that the addresses are affine in the step and hipcc keeps them
// as pointers it increments; only the ragged last step (TAIL) clamps rows to N - 1 and masks.
template <typename T, bool TAIL> __device__ __forceinline__ typename Vec<T>::v4 at_gather4t(const T* base, long sn, int row0, int last, int col) {
    if (TAIL) return at_gather4<T>(base, sn, row0, last, col);
    typename Vec<T>::v4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = base[(long)(row0 + r) * sn + col];
    return v;
}
template <bool TAIL> __device__ __forceinline__ int at_row(int row, int last) { return TAIL && row > last ? last : row; }

// exp(x), x <= ~0. 16-bit types: v_exp_f32 of fl(x log2 e) - the weight is rounded to 2^-11 / 2^-8 next, the |x| u of the product is far below it.
// f32: the product's rounding is put back (x log2 e = t + e exactly, to first order exp2(t + e) = exp2(t) (1 + e ln 2)), which leaves the
// instruction's own ~1 ulp whatever |x| is, at a third of the instructions of the library's expf. x = -inf gives NaN here: callers select.
template <typename T> __device__ __forceinline__ float at_exp(float x) {
    const float t = x * 1.44269502f;
    const float y = __builtin_amdgcn_exp2f(t);
    if (!std::is_same<T, float>::value) return y;
    const float e = fmaf(x, 1.92596303e-8f, fmaf(x, 1.44269502f, -t));
    return fmaf(y, e * 0.693147181f, y);
}
template <typename T> __device__ __forceinline__ float at_dot4(typename Vec<T>::v4 a, typename Vec<T>::v4 b, float acc) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = fmaf(to_f32<T>(a[e]), to_f32<T>(b[e]), acc);
    return acc;
}

struct ATWave { int b, h, blk, lane, l15, g; bool live; };
__device__ __forceinline__ ATWave at_wave(const ATParams& p) {
    ATWave w;
    w.lane = threadIdx.x & 63; w.l15 = w.lane & 15; w.g = w.lane >> 4;
    const long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    w.live = gw < p.nwaves;
    const long prob = gw / p.nblk;
    w.blk = (int)(gw - prob * p.nblk);
    w.b = (int)(prob / p.heads); w.h = (int)(prob - (long)w.b * p.heads);
    return w;
}

template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_train_fwd_kernel(const ATParams p) {
    typedef typename Vec<T>::v4 V4;
    constexpr int DC = HD / 16, KT = at_kt(HD);
    const ATWave w = at_wave(p);
    if (!w.live) return;
    const int l15 = w.l15, g = w.g, N = p.N, last = N - 1, q0 = w.blk * 16;
    const T* Qb = (const T*)p.q + w.b * p.q_sb + w.h * p.q_sh;
    const T* Kb = (const T*)p.k + w.b * p.k_sb + w.h * p.k_sh;
    const T* Vb = (const T*)p.v + w.b * p.v_sb + w.h * p.v_sh;
    const int qrow = q0 + l15 < last ? q0 + l15 : last;
    V4 qf[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) qf[c] = at_row4<T>(Qb + (long)qrow * p.q_sn + c * 16 + g * 4);
    f32x4 o[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, lsum = 0.f;       // running maximum of query l15 (equal in its four lanes), this lane's share of the denominator
    auto step = [&](const int k0, auto tail) {
        constexpr bool TAIL = decltype(tail)::value;
        f32x4 s[KT];                                               // S^T[key k0 + 16t + 4g + r][query l15]
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int krow = at_row<TAIL>(k0 + t * 16 + l15, last);
            s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < DC; ++c) s[t] = Mma<T>::k16(at_row4<T>(Kb + (long)krow * p.k_sn + c * 16 + g * 4), qf[c], s[t]);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[t][r] = s[t][r] * p.scale;
                mx = fmaxf(mx, !TAIL || k0 + t * 16 + g * 4 + r < N ? s[t][r] : -INFINITY);
            }
        const float mnew = fmaxf(m, at_gmax(mx));                  // finite: key k0 exists
        const float alpha = m == -INFINITY ? 0.f : at_exp<T>(m - mnew);   // the first step
        V4 pf[KT];
        float ps = 0.f;
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            f32x4 pr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = at_exp<T>(s[t][r] - mnew);
                pr[r] = !TAIL || k0 + t * 16 + g * 4 + r < N ? e : 0.f;
                ps += pr[r];
            }
            pf[t] = cvt4<T>(pr);
        }
        lsum = fmaf(lsum, alpha, ps);
        m = mnew;
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            o[c] *= alpha;
#pragma unroll
            for (int t = 0; t < KT; ++t)                           // O^T[d = 16c + 4g + r][query l15]
                o[c] = Mma<T>::k16(at_gather4t<T, TAIL>(Vb, p.v_sn, k0 + t * 16 + g * 4, last, c * 16 + l15), pf[t], o[c]);
        }
    };
    int k0 = 0;
    for (; k0 + 16 * KT <= N; k0 += 16 * KT) step(k0, std::false_type{});
    if (k0 < N) step(k0, std::true_type{});
    const float l = at_gsum(lsum);
    if (q0 + l15 < N) {
        const float inv = 1.f / l;
        T* orow = (T*)p.out + ((long)w.b * N + q0 + l15) * p.o_ld + w.h * HD;
#pragma unroll
        for (int c = 0; c < DC; ++c) *(V4*)(orow + c * 16 + g * 4) = cvt4<T>(o[c] * inv);
        if (g == 0) p.lse[((long)w.b * p.heads + w.h) * N + q0 + l15] = m + logf(l);
    }
}

// dQ of query block w.blk. FUSED: D is formed here from dO and o; otherwise read from the workspace.
template <typename T, int HD, bool FUSED>
__device__ __forceinline__ void attn_train_dq_part(const ATParams& p, const ATWave& w) {
    typedef typename Vec<T>::v4 V4;
    constexpr int DC = HD / 16, KT = at_kt(HD);
    const int l15 = w.l15, g = w.g, N = p.N, last = N - 1, q0 = w.blk * 16;
    const T* Qb = (const T*)p.q + w.b * p.q_sb + w.h * p.q_sh;
    const T* Kb = (const T*)p.k + w.b * p.k_sb + w.h * p.k_sh;
    const T* Vb = (const T*)p.v + w.b * p.v_sb + w.h * p.v_sh;
    const int qrow = q0 + l15 < last ? q0 + l15 : last;
    const T* dorow = (const T*)p.d_o + ((long)w.b * N + qrow) * p.do_ld + w.h * HD;
    const long stat = ((long)w.b * p.heads + w.h) * N + qrow;
    V4 qf[DC], dof[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) {
        qf[c] = at_row4<T>(Qb + (long)qrow * p.q_sn + c * 16 + g * 4);
        dof[c] = at_row4<T>(dorow + c * 16 + g * 4);
    }
    const float lse = p.lse[stat];
    float Dq;
    if (FUSED) {
        const T* orow = (const T*)p.o + ((long)w.b * N + qrow) * p.o_ld + w.h * HD;
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < DC; ++c) d = at_dot4<T>(dof[c], at_row4<T>(orow + c * 16 + g * 4), d);
        Dq = at_gsum(d);
    } else {
        Dq = p.D[stat];
    }
    f32x4 acc[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto step = [&](const int k0, auto tail) {
        constexpr bool TAIL = decltype(tail)::value;
        V4 dsf[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int krow = at_row<TAIL>(k0 + t * 16 + l15, last);
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};   // S^T, dP^T [key k0 + 16t + 4g + r][query l15]
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                s = Mma<T>::k16(at_row4<T>(Kb + (long)krow * p.k_sn + c * 16 + g * 4), qf[c], s);
                dp = Mma<T>::k16(at_row4<T>(Vb + (long)krow * p.v_sn + c * 16 + g * 4), dof[c], dp);
            }
            f32x4 ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = at_exp<T>(s[r] * p.scale - lse);
                const float pr = !TAIL || k0 + t * 16 + g * 4 + r < N ? e : 0.f;
                ds[r] = pr * (dp[r] - Dq);
            }
            dsf[t] = cvt4<T>(ds);
        }
#pragma unroll
        for (int c = 0; c < DC; ++c)
#pragma unroll
            for (int t = 0; t < KT; ++t)                           // dQ^T[d = 16c + 4g + r][query l15]
                acc[c] = Mma<T>::k16(at_gather4t<T, TAIL>(Kb, p.k_sn, k0 + t * 16 + g * 4, last, c * 16 + l15), dsf[t], acc[c]);
    };
    int k0 = 0;
    for (; k0 + 16 * KT <= N; k0 += 16 * KT) step(k0, std::false_type{});
    if (k0 < N) step(k0, std::true_type{});
    if (q0 + l15 < N) {
        T* row = (T*)p.dq + w.b * p.dq_sb + (long)(q0 + l15) * p.dq_sn + w.h * p.dq_sh;
#pragma unroll
        for (int c = 0; c < DC; ++c) *(V4*)(row + c * 16 + g * 4) = cvt4<T>(acc[c] * p.scale);
    }
}

// dK and dV of key block w.blk
template <typename T, int HD, bool FUSED>
__device__ __forceinline__ void attn_train_dkdv_part(const ATParams& p, const ATWave& w) {
    typedef typename Vec<T>::v4 V4;
    constexpr int DC = HD / 16, KT = at_kt(HD);
    const int l15 = w.l15, g = w.g, N = p.N, last = N - 1, k0 = w.blk * 16;
    const T* Qb = (const T*)p.q + w.b * p.q_sb + w.h * p.q_sh;
    const T* Kb = (const T*)p.k + w.b * p.k_sb + w.h * p.k_sh;
    const T* Vb = (const T*)p.v + w.b * p.v_sb + w.h * p.v_sh;
    const T* dOb = (const T*)p.d_o + (long)w.b * N * p.do_ld + w.h * HD;
    const T* Ob = (const T*)p.o + (long)w.b * N * p.o_ld + w.h * HD;
    const long stat0 = ((long)w.b * p.heads + w.h) * N;
    const int krow = k0 + l15 < last ? k0 + l15 : last;
    V4 kf[DC], vf[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) {
        kf[c] = at_row4<T>(Kb + (long)krow * p.k_sn + c * 16 + g * 4);
        vf[c] = at_row4<T>(Vb + (long)krow * p.v_sn + c * 16 + g * 4);
    }
    f32x4 dk[DC], dv[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) { dk[c] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[c] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    auto step = [&](const int q0, auto tail) {
        constexpr bool TAIL = decltype(tail)::value;
        V4 pf[KT], dsf[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int qrow = at_row<TAIL>(q0 + t * 16 + l15, last);
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};   // S, dP [query q0 + 16t + 4g + r][key l15]
            float dpart = 0.f;
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                const V4 dor = at_row4<T>(dOb + (long)qrow * p.do_ld + c * 16 + g * 4);
                s = Mma<T>::k16(at_row4<T>(Qb + (long)qrow * p.q_sn + c * 16 + g * 4), kf[c], s);
                dp = Mma<T>::k16(dor, vf[c], dp);
                if (FUSED) dpart = at_dot4<T>(dor, at_row4<T>(Ob + (long)qrow * p.o_ld + c * 16 + g * 4), dpart);
            }
            float Drow = 0.f;
            if (FUSED) Drow = at_gsum(dpart);                        // D of query q0 + 16t + l15, in the same order as attn_train_dq_part forms it
            f32x4 pr, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qi = q0 + t * 16 + g * 4 + r;
                const int qc = at_row<TAIL>(qi, last);
                const float Dq = FUSED ? __shfl(Drow, g * 4 + r) : p.D[stat0 + qc];
                const float pe = at_exp<T>(s[r] * p.scale - p.lse[stat0 + qc]);
                pr[r] = !TAIL || qi < N ? pe : 0.f;
                ds[r] = pr[r] * (dp[r] - Dq);
            }
            pf[t] = cvt4<T>(pr); dsf[t] = cvt4<T>(ds);
        }
#pragma unroll
        for (int c = 0; c < DC; ++c)
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                dv[c] = Mma<T>::k16(at_gather4t<T, TAIL>(dOb, p.do_ld, q0 + t * 16 + g * 4, last, c * 16 + l15), pf[t], dv[c]);    // dV^T[d = 16c + 4g + r][key l15]
                dk[c] = Mma<T>::k16(at_gather4t<T, TAIL>(Qb, p.q_sn, q0 + t * 16 + g * 4, last, c * 16 + l15), dsf[t], dk[c]);    // dK^T
            }
    };
    int q0 = 0;
    for (; q0 + 16 * KT <= N; q0 += 16 * KT) step(q0, std::false_type{});
    if (q0 < N) step(q0, std::true_type{});
    if (k0 + l15 < N) {
        T* krow_o = (T*)p.dk + w.b * p.dk_sb + (long)(k0 + l15) * p.dk_sn + w.h * p.dk_sh;
        T* vrow_o = (T*)p.dv + w.b * p.dv_sb + (long)(k0 + l15) * p.dv_sn + w.h * p.dv_sh;
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            *(V4*)(krow_o + c * 16 + g * 4) = cvt4<T>(dk[c] * p.scale);
            *(V4*)(vrow_o + c * 16 + g * 4) = cvt4<T>(dv[c]);
        }
    }
}

template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_train_bwd_one_kernel(const ATParams p) {
    const ATWave w = at_wave(p);
    if (!w.live) return;
    attn_train_dq_part<T, HD, true>(p, w);
    attn_train_dkdv_part<T, HD, true>(p, w);
}
template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_train_bwd_dq_kernel(const ATParams p) {
    const ATWave w = at_wave(p);
    if (!w.live) return;
    attn_train_dq_part<T, HD, false>(p, w);
}
template <typename T, int HD>
__global__ __launch_bounds__(256) void attn_train_bwd_dkdv_kernel(const ATParams p) {
    const ATWave w = at_wave(p);
    if (!w.live) return;
    attn_train_dkdv_part<T, HD, false>(p, w);
}
// D[b, h, n] = sum_d dO[b, n, h*hd + d] o[b, n, h*hd + d], one thread per row, d ascending
template <typename T>
__global__ __launch_bounds__(256) void attn_train_bwd_dot_kernel(const ATParams p, int hd) {
    typedef typename Vec<T>::v4 V4;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long rows = (long)p.B * p.heads * p.N;
    if (i >= rows) return;
    const long bh = i / p.N;
    const int n = (int)(i - bh * p.N);
    const int b = (int)(bh / p.heads), h = (int)(bh - (long)b * p.heads);
    const T* dor = (const T*)p.d_o + ((long)b * p.N + n) * p.do_ld + h * hd;
    const T* orow = (const T*)p.o + ((long)b * p.N + n) * p.o_ld + h * hd;
    float d = 0.f;
    for (int c = 0; c < hd; c += 4) d = at_dot4<T>(*(const V4*)(dor + c), *(const V4*)(orow + c), d);
    p.D[i] = d;
}

// ---- launch-form record (lwdetr_attn_train_path_counts): one slot per instantiation the launchers below can name
constexpr int ATP_FWD = 0, ATP_ONE = 9, ATP_DOT = 18, ATP_DKDV = 21, ATP_DQ = 30, ATP_SLOTS = 39;
constexpr int atp_hd(int hd) { return hd == 16 ? 0 : (hd == 32 ? 1 : 2); }
template <typename T> constexpr int atp_dt() { return std::is_same<T, float>::value ? 0 : (std::is_same<T, f16>::value ? 1 : 2); }
struct ATPathTable {
    char names[ATP_SLOTS][40];
    ATPathTable() {
        const char* dts[3] = {"f32", "f16", "bf16"};
        const int hds[3] = {16, 32, 64};
        for (int dt = 0; dt < 3; ++dt) {
            snprintf(names[ATP_DOT + dt], sizeof names[0], "attn_train_bwd_dot_%s", dts[dt]);
            for (int h = 0; h < 3; ++h) {
                snprintf(names[ATP_FWD + dt * 3 + h], sizeof names[0], "attn_train_fwd_%s_hd%d", dts[dt], hds[h]);
                snprintf(names[ATP_ONE + dt * 3 + h], sizeof names[0], "attn_train_bwd_one_%s_hd%d", dts[dt], hds[h]);
                snprintf(names[ATP_DKDV + dt * 3 + h], sizeof names[0], "attn_train_bwd_dkdv_%s_hd%d", dts[dt], hds[h]);
                snprintf(names[ATP_DQ + dt * 3 + h], sizeof names[0], "attn_train_bwd_dq_%s_hd%d", dts[dt], hds[h]);
            }
        }
    }
};
const ATPathTable& at_paths() { static const ATPathTable t; return t; }
std::atomic<long> g_at_path[ATP_SLOTS];
inline int at_done(int slot, int rc) {                   // counted only when the launch check succeeded
    if (rc == LWDETR_OK) g_at_path[slot].fetch_add(1, std::memory_order_relaxed);
    return rc;
}

inline bool at_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool at_st16(long stride, int esz) { return (stride * esz) % 16 == 0; }

int at_check_desc(const lwdetr_attn_train_desc* d, int dtype) {
    if (!d || !d->q || !d->k || !d->v || !d->o || !d->lse) return LWDETR_ERR_BAD_ARG;
    if (d->B < 1 || d->heads < 1 || d->N < 1) return LWDETR_ERR_BAD_ARG;
    if (!std::isfinite(d->scale) || !(d->scale > 0.f)) return LWDETR_ERR_BAD_ARG;
    if (dtype < DT_F32 || dtype > DT_BF16 || (d->hd != 16 && d->hd != 32 && d->hd != 64)) return LWDETR_ERR_UNSUPPORTED;
    const int esz = dtype == DT_F32 ? 4 : 2;
    if (!at_al16(d->q) || !at_al16(d->k) || !at_al16(d->v) || !at_al16(d->o) || ((uintptr_t)d->lse & 3)) return LWDETR_ERR_BAD_ARG;
    const long st[10] = {d->q_sb, d->q_sn, d->q_sh, d->k_sb, d->k_sn, d->k_sh, d->v_sb, d->v_sn, d->v_sh, d->o_ld};
    for (long s : st)
        if (!at_st16(s, esz)) return LWDETR_ERR_BAD_ARG;
    if (((long)d->B * d->heads * ((d->N + 15) / 16) + 3) / 4 > 0x7fffffffL) return LWDETR_ERR_UNSUPPORTED;
    return LWDETR_OK;
}

void at_fill(ATParams& p, const lwdetr_attn_train_desc* d) {
    p = ATParams{};
    p.q = d->q; p.k = d->k; p.v = d->v; p.o = d->o; p.out = d->o; p.lse = d->lse;
    p.q_sb = d->q_sb; p.q_sn = d->q_sn; p.q_sh = d->q_sh; p.k_sb = d->k_sb; p.k_sn = d->k_sn; p.k_sh = d->k_sh;
    p.v_sb = d->v_sb; p.v_sn = d->v_sn; p.v_sh = d->v_sh; p.o_ld = d->o_ld;
    p.B = d->B; p.heads = d->heads; p.N = d->N; p.nblk = (d->N + 15) / 16;
    p.nwaves = (long)d->B * d->heads * p.nblk;
    p.scale = d->scale;
}

template <typename T, int HD>
int at_forward(const ATParams& p, hipStream_t st) {
    const unsigned grid = (unsigned)((p.nwaves + 3) / 4);
    hipLaunchKernelGGL((attn_train_fwd_kernel<T, HD>), dim3(grid), dim3(256), 0, st, p);
    return at_done(ATP_FWD + atp_dt<T>() * 3 + atp_hd(HD), lwdetr_check_launch());
}
template <typename T, int HD>
int at_backward(const ATParams& p, hipStream_t st) {
    const unsigned grid = (unsigned)((p.nwaves + 3) / 4);
    const int slot = atp_dt<T>() * 3 + atp_hd(HD);
    if (p.N <= kAttnTrainOneLaunchMaxN) {
        hipLaunchKernelGGL((attn_train_bwd_one_kernel<T, HD>), dim3(grid), dim3(256), 0, st, p);
        return at_done(ATP_ONE + slot, lwdetr_check_launch());
    }
    const long rows = (long)p.B * p.heads * p.N;
    hipLaunchKernelGGL((attn_train_bwd_dot_kernel<T>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, p, HD);
    int rc = at_done(ATP_DOT + atp_dt<T>(), lwdetr_check_launch());
    if (rc != LWDETR_OK) return rc;
    hipLaunchKernelGGL((attn_train_bwd_dkdv_kernel<T, HD>), dim3(grid), dim3(256), 0, st, p);
    rc = at_done(ATP_DKDV + slot, lwdetr_check_launch());
    if (rc != LWDETR_OK) return rc;
    hipLaunchKernelGGL((attn_train_bwd_dq_kernel<T, HD>), dim3(grid), dim3(256), 0, st, p);
    return at_done(ATP_DQ + slot, lwdetr_check_launch());
}
template <typename T>
int at_dispatch(const ATParams& p, int hd, bool backward, hipStream_t st) {
    switch (hd) {
        case 16: return backward ? at_backward<T, 16>(p, st) : at_forward<T, 16>(p, st);
        case 32: return backward ? at_backward<T, 32>(p, st) : at_forward<T, 32>(p, st);
        default: return backward ? at_backward<T, 64>(p, st) : at_forward<T, 64>(p, st);
    }
}
int at_dispatch_dtype(const ATParams& p, int hd, int dtype, bool backward, hipStream_t st) {
    switch (dtype) {
        case DT_F32: return at_dispatch<float>(p, hd, backward, st);
        case DT_F16: return at_dispatch<f16>(p, hd, backward, st);
        default: return at_dispatch<bf16>(p, hd, backward, st);
    }
}

}  // namespace

extern "C" int lwdetr_attn_train_path_counts(long* out, int n) {
    for (int i = 0; out && i < n && i < ATP_SLOTS; ++i) out[i] = g_at_path[i].load(std::memory_order_relaxed);
    return ATP_SLOTS;
}
extern "C" const char* lwdetr_attn_train_path_name(int i) { return i >= 0 && i < ATP_SLOTS ? at_paths().names[i] : nullptr; }

extern "C" int lwdetr_attn_train_forward(const lwdetr_attn_train_desc* d, int dtype, void* hip_stream) {
    const int rc = at_check_desc(d, dtype);
    if (rc != LWDETR_OK) return rc;
    ATParams p;
    at_fill(p, d);
    return at_dispatch_dtype(p, d->hd, dtype, false, (hipStream_t)hip_stream);
}

extern "C" long lwdetr_attn_train_workspace_bytes(int B, int heads, int N, int hd, int dtype) {
    (void)hd; (void)dtype;
    if (B < 1 || heads < 1 || N < 1) return 0;
    return N <= kAttnTrainOneLaunchMaxN ? 0 : (long)B * heads * N * (long)sizeof(float);
}

extern "C" int lwdetr_attn_train_backward(const lwdetr_attn_train_desc* d, const void* d_o, long do_ld, void* dq, void* dk, void* dv,
                                          long dq_sb, long dq_sn, long dq_sh, long dk_sb, long dk_sn, long dk_sh, long dv_sb, long dv_sn,
                                          long dv_sh, void* workspace, int dtype, void* hip_stream) {
    if (!d_o || !dq || !dk || !dv) return LWDETR_ERR_BAD_ARG;
    const int rc = at_check_desc(d, dtype);
    if (rc != LWDETR_OK) return rc;
    const int esz = dtype == DT_F32 ? 4 : 2;
    if (!at_al16(d_o) || !at_al16(dq) || !at_al16(dk) || !at_al16(dv)) return LWDETR_ERR_BAD_ARG;
    const long st[10] = {do_ld, dq_sb, dq_sn, dq_sh, dk_sb, dk_sn, dk_sh, dv_sb, dv_sn, dv_sh};
    for (long s : st)
        if (!at_st16(s, esz)) return LWDETR_ERR_BAD_ARG;
    if (d->N > kAttnTrainOneLaunchMaxN && (!workspace || ((uintptr_t)workspace & 3))) return LWDETR_ERR_BAD_ARG;
    ATParams p;
    at_fill(p, d);
    p.d_o = d_o; p.do_ld = do_ld; p.dq = dq; p.dk = dk; p.dv = dv; p.D = (float*)workspace;
    p.dq_sb = dq_sb; p.dq_sn = dq_sn; p.dq_sh = dq_sh; p.dk_sb = dk_sb; p.dk_sn = dk_sn; p.dk_sh = dk_sh;
    p.dv_sb = dv_sb; p.dv_sn = dv_sn; p.dv_sh = dv_sh;
    return at_dispatch_dtype(p, d->hd, dtype, true, (hipStream_t)hip_stream);
}
