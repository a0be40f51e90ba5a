// Two-stage query selection under training (reference models/transformer.py:224-264 with group_detr groups):
//   lwdetr_two_stage_scores           score[g, r] = max_c (LayerNorm(x_r W_eo[g]^T + b_eo[g]) W_cls[g]^T + b_cls[g])_c for every group and encoder
//                                     token in ONE launch; y and the logits never reach memory
//   lwdetr_two_stage_gather           the selected rows of memory / proposals, and the inverse table (B, S, G) -> q or -1
//   lwdetr_two_stage_scatter_backward grad_memory from the selected rows' gradients: one wave per token row, groups added in ascending g
// No atomics anywhere: a second call returns the same bits. Contract: include/lwdetr_hip.h.
//
// Scoring kernel. A workgroup of 4 waves owns 64 rows of one group (grid = row tiles x G, so a training batch of 50-100 row tiles still covers
// 256 CUs 13 times over); each wave owns 16 rows for the whole pipeline, so nothing but the weights is shared. Both GEMMs are issued TRANSPOSED,
// D^T = W x^T: the weight rows are the MFMA's A operand and the token rows its B operand. The result fragment of the first GEMM then holds, per
// lane, row (lane & 15) and the four consecutive channels 16 t + 4 (lane >> 4) + 0..3 - which is exactly the B-operand fragment of a k16 MFMA
// over channel chunk t. LayerNorm therefore runs in registers (row statistics: in-lane sums in a fixed order, then xor-butterflies over lanes
// 16 and 32 apart - commutative, so every lane of a row holds the same bits and a row's result does not depend on where in a tile it sits) and
// the class GEMM consumes y straight from registers, rounded to T once. Its result fragment holds 4 classes of row (lane & 15) per lane: the
// row maximum is an in-lane running maximum over class tiles and one butterfly.
// The weights stream through a double-buffered LDS slab with one barrier per step: W_eo in k-chunks of 64 bytes per output channel (the whole
// f32 matrix at d = 384 is 576 KiB), W_cls in tiles of 16 classes x d. Slab rows are padded by 16 bytes, which spreads the 16 lanes of a
// quarter-wave over all 64 banks.
#include "common.h"

#include <atomic>
#include <type_traits>

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int TS_ROWS = 64, TS_THREADS = 256;
constexpr int TS_MAX_G = 16, TS_MAX_NCLS = 384, TS_MAX_D_SEL = 4096;
constexpr float TS_EPS = 1e-5f;

constexpr int TSP_COUNT = 12;
std::atomic<long> g_ts_path[TSP_COUNT];
const char* const kTsPathNames[TSP_COUNT] = {
    "ts_scores_f32_d256", "ts_scores_f32_d384", "ts_scores_f16_d256", "ts_scores_f16_d384", "ts_scores_bf16_d256", "ts_scores_bf16_d384",
    "ts_gather_f32", "ts_gather_f16", "ts_gather_bf16", "ts_scatter_f32", "ts_scatter_f16", "ts_scatter_bf16",
};
template <typename T> constexpr int ts_dtype_of() { return std::is_same<T, float>::value ? 0 : std::is_same<T, f16>::value ? 1 : 2; }
inline int ts_path_done(int path, int rc) {
    if (rc == LWDETR_OK && path >= 0 && path < TSP_COUNT) g_ts_path[path].fetch_add(1, std::memory_order_relaxed);
    return rc;
}

struct ScoreParams {
    const void* memory;
    long ld;
    const unsigned char* rowvalid;
    const void *w_eo, *b_eo, *ln_w, *ln_b, *w_cls, *b_cls;
    float* scores;
    long rows;
    int ncls;
};

// the first GEMM's 16-byte operand piece: 4 f32 (k16, four exact 16x16x4 MFMAs) or 8 halves (k32)
template <typename T> struct Op1 {
    typedef typename Vec<T>::v8 type;
    static __device__ __forceinline__ f32x4 mma(u32x4 a, u32x4 b, f32x4 c) {
        return Mma<T>::k32(__builtin_bit_cast(type, a), __builtin_bit_cast(type, b), c);
    }
};
template <> struct Op1<float> {
    typedef f32x4 type;
    static __device__ __forceinline__ f32x4 mma(u32x4 a, u32x4 b, f32x4 c) {
        return Mma<float>::k16(__builtin_bit_cast(f32x4, a), __builtin_bit_cast(f32x4, b), c);
    }
};

template <typename T, int D>
__global__ __launch_bounds__(TS_THREADS) void two_stage_scores_kernel(ScoreParams p) {
    constexpr int ES = (int)sizeof(T);
    constexpr int E = 16 / ES;                 // elements per 16-byte piece
    constexpr int KC = 4 * E;                  // k-values per chunk of the first GEMM (16 f32 / 32 halves): 64 bytes per weight row
    constexpr int NCH = D / KC;
    constexpr int NT = D / 16;                 // 16-channel tiles of y
    constexpr int RS1 = 80;                    // slab row of the first GEMM: 64 bytes + 16 pad
    constexpr int BUF = D * RS1;               // one slab buffer
    constexpr int PPT1 = D * 4 / TS_THREADS;   // 16-byte pieces per thread and chunk
    constexpr int RS2 = D * ES + 16;           // slab row of the class GEMM: one class's d weights + 16 pad
    constexpr int PPR2 = D * ES / 16;          // pieces per class row
    constexpr int PPT2 = 16 * PPR2 / TS_THREADS;
    static_assert(16 * RS2 <= BUF, "a class tile must fit a slab buffer");
    static_assert(D % 64 == 0 && (16 * PPR2) % TS_THREADS == 0, "uniform piece counts");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
    const int g = blockIdx.y;
    const long r = (long)blockIdx.x * TS_ROWS + wave * 16 + j;
    const bool live = r < p.rows && p.rowvalid[r] != 0;
    const T* xrow = (const T*)p.memory + (live ? r : 0) * p.ld + q * E;
    const T* W = (const T*)p.w_eo + (long)g * D * D;

    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    u32x4 wreg[PPT1], xcur, xnext;
    const u32x4 zero4 = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int u = 0; u < PPT1; ++u) {
        const int pi = tid + TS_THREADS * u;
        wreg[u] = *(const u32x4*)(W + (long)(pi >> 2) * D + (pi & 3) * E);
    }
#pragma unroll
    for (int u = 0; u < PPT1; ++u) {
        const int pi = tid + TS_THREADS * u;
        *(u32x4*)(lds + (pi >> 2) * RS1 + (pi & 3) * 16) = wreg[u];
    }
    xcur = live ? *(const u32x4*)xrow : zero4;
    xnext = zero4;
    __syncthreads();

#pragma unroll 1
    for (int c = 0; c < NCH; ++c) {
        const bool more = c + 1 < NCH;
        if (more) {
#pragma unroll
            for (int u = 0; u < PPT1; ++u) {
                const int pi = tid + TS_THREADS * u;
                wreg[u] = *(const u32x4*)(W + (long)(pi >> 2) * D + (c + 1) * KC + (pi & 3) * E);
            }
            xnext = live ? *(const u32x4*)(xrow + (c + 1) * KC) : zero4;
        }
        const unsigned char* buf = lds + (c & 1) * BUF + j * RS1 + q * 16;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const u32x4 w = *(const u32x4*)(buf + t * 16 * RS1);
            acc[t] = Op1<T>::mma(w, xcur, acc[t]);
        }
        if (more) {
            unsigned char* nb = lds + ((c + 1) & 1) * BUF;
#pragma unroll
            for (int u = 0; u < PPT1; ++u) {
                const int pi = tid + TS_THREADS * u;
                *(u32x4*)(nb + (pi >> 2) * RS1 + (pi & 3) * 16) = wreg[u];
            }
            xcur = xnext;
        }
        __syncthreads();
    }

    // first class tile on its way while LayerNorm runs (both buffers are free after the loop's last barrier)
    const T* Wc = (const T*)p.w_cls + (long)g * p.ncls * D;
    const int nct = (p.ncls + 15) >> 4;
    u32x4 creg[PPT2];
#pragma unroll
    for (int u = 0; u < PPT2; ++u) {
        const int pi = tid + TS_THREADS * u, cls = pi / PPR2, part = pi - cls * PPR2;
        creg[u] = cls < p.ncls ? *(const u32x4*)(Wc + (long)cls * D + part * E) : zero4;
    }

    // bias, LayerNorm over the row: this lane holds channels 16 t + 4 q + i of row j
    const T* be = (const T*)p.b_eo + (long)g * D;
    const T* lw = (const T*)p.ln_w + (long)g * D;
    const T* lb = (const T*)p.ln_b + (long)g * D;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const typename Vec<T>::v4 b4 = *(const typename Vec<T>::v4*)(be + t * 16 + q * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[t][i] += to_f32<T>(b4[i]);
            s += acc[t][i];
        }
    }
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    const float mean = s * (1.f / D);
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float dlt = acc[t][i] - mean;
            v = fmaf(dlt, dlt, v);
        }
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    const float rstd = 1.f / sqrtf(v * (1.f / D) + TS_EPS);
    typename Vec<T>::v4 y[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const typename Vec<T>::v4 w4 = *(const typename Vec<T>::v4*)(lw + t * 16 + q * 4);
        const typename Vec<T>::v4 b4 = *(const typename Vec<T>::v4*)(lb + t * 16 + q * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) y[t][i] = from_f32<T>(fmaf((acc[t][i] - mean) * rstd, to_f32<T>(w4[i]), to_f32<T>(b4[i])));
    }

#pragma unroll
    for (int u = 0; u < PPT2; ++u) {
        const int pi = tid + TS_THREADS * u, cls = pi / PPR2, part = pi - cls * PPR2;
        *(u32x4*)(lds + cls * RS2 + part * 16) = creg[u];
    }
    __syncthreads();

    const T* bc = (const T*)p.b_cls + (long)g * p.ncls;
    float best = -INFINITY;
#pragma unroll 1
    for (int ct = 0; ct < nct; ++ct) {
        const bool more = ct + 1 < nct;
        if (more) {
#pragma unroll
            for (int u = 0; u < PPT2; ++u) {
                const int pi = tid + TS_THREADS * u, cls = pi / PPR2, part = pi - cls * PPR2, cc = (ct + 1) * 16 + cls;
                creg[u] = cc < p.ncls ? *(const u32x4*)(Wc + (long)cc * D + part * E) : zero4;
            }
        }
        const unsigned char* buf = lds + (ct & 1) * BUF + j * RS2 + q * 4 * ES;
        f32x4 l0 = f32x4{0.f, 0.f, 0.f, 0.f}, l1 = l0;         // two chains: a k16 MFMA waits for the previous one on the same accumulator
#pragma unroll
        for (int t = 0; t < NT; t += 2) {
            const typename Vec<T>::v4 w0 = *(const typename Vec<T>::v4*)(buf + t * 16 * ES);
            const typename Vec<T>::v4 w1 = *(const typename Vec<T>::v4*)(buf + (t + 1) * 16 * ES);
            l0 = Mma<T>::k16(w0, y[t], l0);
            l1 = Mma<T>::k16(w1, y[t + 1], l1);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cc = ct * 16 + q * 4 + i;
            if (cc < p.ncls) best = fmaxf(best, (l0[i] + l1[i]) + to_f32<T>(bc[cc]));
        }
        if (more) {
            unsigned char* nb = lds + ((ct + 1) & 1) * BUF;
#pragma unroll
            for (int u = 0; u < PPT2; ++u) {
                const int pi = tid + TS_THREADS * u, cls = pi / PPR2, part = pi - cls * PPR2;
                *(u32x4*)(nb + cls * RS2 + part * 16) = creg[u];
            }
        }
        __syncthreads();
    }
    best = fmaxf(best, __shfl_xor(best, 16));
    best = fmaxf(best, __shfl_xor(best, 32));
    if (q == 0 && r < p.rows) p.scores[(long)g * p.rows + r] = best;
}

// ------------------------------------------------------------------------------------------------------------------- selection
struct SelParams {
    const void* memory;
    long ld;
    const unsigned char* rowvalid;
    const float* props;
    const int64_t* idx;
    void* x_sel;
    float* props_sel;
    int* inv;
    const void* gx;
    void* gm;
    int B, S, G, nq, d;
};

__global__ void ts_inv_fill_kernel(int* inv, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) inv[i] = -1;
}

// one wave per selected row (b, g, q); an index outside [0, S) selects nothing: zeros, no table entry
template <typename T> __global__ __launch_bounds__(256) void ts_gather_kernel(SelParams p) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6), total = (long)p.B * p.G * p.nq;
    if (item >= total) return;
    const int qi = (int)(item % p.nq);
    const long bg = item / p.nq;
    const int g = (int)(bg % p.G), b = (int)(bg / p.G);
    const int64_t s = p.idx[((long)g * p.B + b) * p.nq + qi];
    const bool ok = s >= 0 && s < p.S;
    const long row = (long)b * p.S + (ok ? s : 0);
    const bool valid = ok && p.rowvalid[row] != 0;
    const T* src = (const T*)p.memory + row * p.ld;
    T* dst = (T*)p.x_sel + item * p.d;
    for (int c = lane; c < p.d; c += 64) dst[c] = valid ? src[c] : from_f32<T>(0.f);
    if (lane < 4) p.props_sel[item * 4 + lane] = ok ? p.props[row * 4 + lane] : 0.f;
    if (lane == 0 && ok) p.inv[row * p.G + g] = qi;
}

// one wave per token row: the groups that selected it, in ascending g, f32, one rounding
template <typename T> __global__ __launch_bounds__(256) void ts_scatter_kernel(SelParams p) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6), total = (long)p.B * p.S;
    if (row >= total) return;
    const int b = (int)(row / p.S);
    const bool valid = p.rowvalid[row] != 0;
    int qs[TS_MAX_G];
#pragma unroll
    for (int g = 0; g < TS_MAX_G; ++g) {
        const int qv = g < p.G ? p.inv[row * p.G + g] : -1;
        qs[g] = valid && qv >= 0 && qv < p.nq ? qv : -1;
    }
    const T* gx = (const T*)p.gx;
    T* out = (T*)p.gm + row * p.d;
    for (int c = lane; c < p.d; c += 64) {
        float a = 0.f;
#pragma unroll
        for (int g = 0; g < TS_MAX_G; ++g)
            if (qs[g] >= 0) a += to_f32<T>(gx[(((long)b * p.G + g) * p.nq + qs[g]) * p.d + c]);
        out[c] = from_f32<T>(a);
    }
}

// ------------------------------------------------------------------------------------------------------------------------ host
bool al16(const void* p) { return (uintptr_t)p % 16 == 0; }
size_t esize(int dtype) { return dtype == DT_F32 ? 4 : 2; }
bool dtype_ok(int dtype) { return dtype == DT_F32 || dtype == DT_F16 || dtype == DT_BF16; }

int scores_check(const void* memory, long ld, const unsigned char* rowvalid, const void* w_eo, const void* b_eo, const void* ln_w, const void* ln_b,
                 const void* w_cls, const void* b_cls, const float* scores, long rows, int d, int ncls, int G, int dtype) {
    if (!dtype_ok(dtype)) return LWDETR_ERR_UNSUPPORTED;
    if ((d != 256 && d != 384) || ncls < 1 || ncls > TS_MAX_NCLS || G < 1 || G > TS_MAX_G || rows < 0) return LWDETR_ERR_BAD_ARG;
    if (!memory || !rowvalid || !w_eo || !b_eo || !ln_w || !ln_b || !w_cls || !b_cls || !scores) return LWDETR_ERR_BAD_ARG;
    if (ld < d || (ld * esize(dtype)) % 16 != 0) return LWDETR_ERR_BAD_ARG;
    if (!al16(memory) || !al16(w_eo) || !al16(b_eo) || !al16(ln_w) || !al16(ln_b) || !al16(w_cls) || (uintptr_t)b_cls % esize(dtype) != 0 ||
        (uintptr_t)scores % 4 != 0)
        return LWDETR_ERR_BAD_ARG;
    if ((rows + TS_ROWS - 1) / TS_ROWS > 0x7fffffffL) return LWDETR_ERR_BAD_ARG;
    return LWDETR_OK;
}

int sel_check(int B, int S, int G, int nq, int d, int dtype) {
    if (!dtype_ok(dtype)) return LWDETR_ERR_UNSUPPORTED;
    if (B < 1 || S < 1 || nq < 1 || nq > S || G < 1 || G > TS_MAX_G || d < 1 || d > TS_MAX_D_SEL) return LWDETR_ERR_BAD_ARG;
    if (((long)B * S + 3) / 4 > 0x7fffffffL || ((long)B * S * G + 255) / 256 > 0x7fffffffL) return LWDETR_ERR_BAD_ARG;
    return LWDETR_OK;
}

template <typename T, int D> int launch_scores(const ScoreParams& p, int G, hipStream_t st) {
    const dim3 grid((unsigned)((p.rows + TS_ROWS - 1) / TS_ROWS), (unsigned)G), block(TS_THREADS);
    hipLaunchKernelGGL((two_stage_scores_kernel<T, D>), grid, block, 0, st, p);
    return ts_path_done(ts_dtype_of<T>() * 2 + (D == 384), lwdetr_check_launch());
}
template <typename T> int launch_scores_d(const ScoreParams& p, int d, int G, hipStream_t st) {
    return d == 256 ? launch_scores<T, 256>(p, G, st) : launch_scores<T, 384>(p, G, st);
}

template <typename T> int launch_gather(const SelParams& p, hipStream_t st) {
    const long n = (long)p.B * p.S * p.G, items = (long)p.B * p.G * p.nq;
    hipLaunchKernelGGL(ts_inv_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p.inv, n);
    int rc = lwdetr_check_launch();
    if (rc != LWDETR_OK) return rc;
    hipLaunchKernelGGL((ts_gather_kernel<T>), dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, p);
    return ts_path_done(6 + ts_dtype_of<T>(), lwdetr_check_launch());
}
template <typename T> int launch_scatter(const SelParams& p, hipStream_t st) {
    const long rows = (long)p.B * p.S;
    hipLaunchKernelGGL((ts_scatter_kernel<T>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, p);
    return ts_path_done(9 + ts_dtype_of<T>(), lwdetr_check_launch());
}

}  // namespace

extern "C" {

int lwdetr_two_stage_scores_check(const void* memory, long ld, const unsigned char* rowvalid, const void* w_eo, const void* b_eo, const void* ln_w,
                                  const void* ln_b, const void* w_cls, const void* b_cls, const float* scores, long rows, int d, int ncls, int G,
                                  int dtype) {
    return scores_check(memory, ld, rowvalid, w_eo, b_eo, ln_w, ln_b, w_cls, b_cls, scores, rows, d, ncls, G, dtype);
}

int lwdetr_two_stage_scores(const void* memory, long ld, const unsigned char* rowvalid, const void* w_eo, const void* b_eo, const void* ln_w,
                            const void* ln_b, const void* w_cls, const void* b_cls, float* scores, long rows, int d, int ncls, int G, int dtype,
                            void* hip_stream) {
    const int rc = scores_check(memory, ld, rowvalid, w_eo, b_eo, ln_w, ln_b, w_cls, b_cls, scores, rows, d, ncls, G, dtype);
    if (rc != LWDETR_OK || rows == 0) return rc;
    ScoreParams p = {memory, ld, rowvalid, w_eo, b_eo, ln_w, ln_b, w_cls, b_cls, scores, rows, ncls};
    hipStream_t st = (hipStream_t)hip_stream;
    switch (dtype) {
        case DT_F32: return launch_scores_d<float>(p, d, G, st);
        case DT_F16: return launch_scores_d<f16>(p, d, G, st);
        default: return launch_scores_d<bf16>(p, d, G, st);
    }
}

int lwdetr_two_stage_gather_check(const void* memory, long ld, const unsigned char* rowvalid, const float* props, const int64_t* idx,
                                  const void* x_sel, const float* props_sel, const int* inv, int B, int S, int G, int nq, int d, int dtype) {
    const int rc = sel_check(B, S, G, nq, d, dtype);
    if (rc != LWDETR_OK) return rc;
    if (!memory || !rowvalid || !props || !idx || !x_sel || !props_sel || !inv) return LWDETR_ERR_BAD_ARG;
    if (ld < d) return LWDETR_ERR_BAD_ARG;
    const size_t es = esize(dtype);
    if ((uintptr_t)memory % es != 0 || (uintptr_t)x_sel % es != 0 || (uintptr_t)props % 4 != 0 || (uintptr_t)props_sel % 4 != 0 ||
        (uintptr_t)idx % 8 != 0 || (uintptr_t)inv % 4 != 0)
        return LWDETR_ERR_BAD_ARG;
    return LWDETR_OK;
}

int lwdetr_two_stage_gather(const void* memory, long ld, const unsigned char* rowvalid, const float* props, const int64_t* idx, void* x_sel,
                            float* props_sel, int* inv, int B, int S, int G, int nq, int d, int dtype, void* hip_stream) {
    const int rc = lwdetr_two_stage_gather_check(memory, ld, rowvalid, props, idx, x_sel, props_sel, inv, B, S, G, nq, d, dtype);
    if (rc != LWDETR_OK) return rc;
    SelParams p = {};
    p.memory = memory; p.ld = ld; p.rowvalid = rowvalid; p.props = props; p.idx = idx; p.x_sel = x_sel; p.props_sel = props_sel; p.inv = inv;
    p.B = B; p.S = S; p.G = G; p.nq = nq; p.d = d;
    hipStream_t st = (hipStream_t)hip_stream;
    switch (dtype) {
        case DT_F32: return launch_gather<float>(p, st);
        case DT_F16: return launch_gather<f16>(p, st);
        default: return launch_gather<bf16>(p, st);
    }
}

int lwdetr_two_stage_scatter_backward_check(const void* grad_x_sel, const int* inv, const unsigned char* rowvalid, const void* grad_memory, int B,
                                            int S, int G, int nq, int d, int dtype) {
    const int rc = sel_check(B, S, G, nq, d, dtype);
    if (rc != LWDETR_OK) return rc;
    if (!grad_x_sel || !inv || !rowvalid || !grad_memory) return LWDETR_ERR_BAD_ARG;
    const size_t es = esize(dtype);
    if ((uintptr_t)grad_x_sel % es != 0 || (uintptr_t)grad_memory % es != 0 || (uintptr_t)inv % 4 != 0) return LWDETR_ERR_BAD_ARG;
    return LWDETR_OK;
}

int lwdetr_two_stage_scatter_backward(const void* grad_x_sel, const int* inv, const unsigned char* rowvalid, void* grad_memory, int B, int S, int G,
                                      int nq, int d, int dtype, void* hip_stream) {
    const int rc = lwdetr_two_stage_scatter_backward_check(grad_x_sel, inv, rowvalid, grad_memory, B, S, G, nq, d, dtype);
    if (rc != LWDETR_OK) return rc;
    SelParams p = {};
    p.gx = grad_x_sel; p.inv = const_cast<int*>(inv); p.rowvalid = rowvalid; p.gm = grad_memory;
    p.B = B; p.S = S; p.G = G; p.nq = nq; p.d = d;
    hipStream_t st = (hipStream_t)hip_stream;
    switch (dtype) {
        case DT_F32: return launch_scatter<float>(p, st);
        case DT_F16: return launch_scatter<f16>(p, st);
        default: return launch_scatter<bf16>(p, st);
    }
}

int lwdetr_two_stage_path_counts(long* out, int n) {
    for (int i = 0; out && i < n && i < TSP_COUNT; ++i) out[i] = g_ts_path[i].load(std::memory_order_relaxed);
    return TSP_COUNT;
}
const char* lwdetr_two_stage_path_name(int i) { return i >= 0 && i < TSP_COUNT ? kTsPathNames[i] : nullptr; }

}  // extern "C"
