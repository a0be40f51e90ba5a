// The tail of a training step over many tensors at once: gradient-norm clip, per-tensor AdamW and the model EMA (reference engine.py:76-83:
// torch.nn.utils.clip_grad_norm_, torch.optim.AdamW over one parameter group per parameter, util/utils.py:20-29 ModelEma.update).
//
// Work is described by two tables in device memory (include/lwdetr_hip.h): one lwdetr_mt_tensor record per tensor and one lwdetr_mt_chunk per
// piece of at most LWDETR_MT_CHUNK = 1024 elements. A chunk is the work of ONE WAVE, not of a workgroup: 64 lanes x 4 floats x 4 rounds, so
// a 256-thread workgroup takes four chunks and a 4-element tensor (two thirds of the reference's tensors hold <= 1024 elements) costs a wave.
// Nothing here synchronises inside a workgroup except the one-workgroup norm reducer.
//
// Lane l of a chunk owns the elements r * 256 + 4 l + {0..3}, r = 0..3, on every path. Where every pointer of the record that the launch
// touches is 16-byte aligned (chunk offsets are multiples of 1024 elements, so the tensor's base decides) a full quad moves as one 16-byte
// access; a full chunk issues all of its loads (up to 20 per lane) before the first use. Any other quad - a view at an odd element offset,
// the tail of a tensor - goes element by element over the same indices, so a sum of squares does not depend on the path taken.
//
// Arithmetic: f32, FP contraction off for the whole object (Makefile; the pragma below covers builds that do not pass the flag), so the host
// form computes the same bits. AdamW follows torch's non-capturable single-tensor path operation by operation (lerp in ATen's two-branch
// form, addcmul as a + value * (b * b), addcdiv as a + value * (m / denom)) with one exception: sqrt(v) / bc2_sqrt is sqrt(v) * (1 / bc2_sqrt)
// with the reciprocal taken once per chunk - one sqrt and one division per element. The EMA is fl(fl(d e) + fl((1 - d) x)).
// No floating-point atomics: sumsq stores one partial per chunk, norm_finish adds them in f64 in a fixed order.
#include "common.h"
#include <atomic>
#include <math.h>
#include <vector>

#pragma clang fp contract(off)

namespace {

enum { MT_WAVE = 64, MT_WAVES = 4, MT_THREADS = MT_WAVE * MT_WAVES, MT_ROUNDS = 4, MT_ROUND_ELEMS = MT_WAVE * 4, MT_MAX_BLOCKS = 2048,
       MT_FINISH_THREADS = 256 };
static_assert(MT_ROUNDS * MT_ROUND_ELEMS == LWDETR_MT_CHUNK, "a chunk is 4 rounds of 64 lanes x 4 floats");
enum { MT_L_SUMSQ = 0, MT_L_FINISH, MT_L_STEP, MT_L_COUNT };
const char* const kMtLaunchNames[MT_L_COUNT] = {"mt_sumsq", "mt_norm_finish", "mt_step"};
std::atomic<long> g_mt_launches[MT_L_COUNT];

enum { MODE_SCALE = 0, MODE_ADAM, MODE_ADAM_EMA, MODE_EMA, MODE_SET };

struct MtCtx { float coef, coef_lo, decay_mul, neg_step, rbc2, w1, beta2, w2, eps, d, omd; };

// ATen's lerp (aten/src/ATen/native/Lerp.h): the form that is exact at the nearer end
__host__ __device__ inline float mt_lerp(float a, float b, float w) {
    const float diff = b - a;
    return fabsf(w) < 0.5f ? a + w * diff : b - diff * (1.f - w);
}
// g * clip_coef with the coefficient held as hi + lo (mt_norm_clip): one fused multiply-add over the small product, so the clipped gradient
// is the correctly rounded product with the f64 coefficient - an f32 coefficient costs an ulp here, which its square doubles in exp_avg_sq.
// Without a clip buffer hi = 1, lo = 0 and the result is g.
__host__ __device__ inline float mt_clip(float g, const MtCtx& c) { return fmaf(g, c.coef, g * c.coef_lo); }
__host__ __device__ inline void mt_adamw(float& p, float g, float& m, float& v, const MtCtx& c) {
    const float gc = mt_clip(g, c);
    p = p * c.decay_mul;                                    // decay_mul = 1 where weight_decay = 0: the product is p
    m = mt_lerp(m, gc, c.w1);
    v = v * c.beta2 + c.w2 * (gc * gc);
    const float denom = sqrtf(v) * c.rbc2 + c.eps;
    p = p + c.neg_step * (m / denom);
}
__host__ __device__ inline float mt_ema(float e, float x, float d, float omd) {
    const float a = d * e;
    const float b = omd * x;
    return a + b;
}
// ModelEma on an int64 buffer: the f32 result of decay * e + (1 - decay) * m copied into the buffer, which truncates toward zero
// (e = 5, m = 6 -> 5; e = 0, m = 4000 -> 1). Out-of-range and NaN give INT64_MIN, what the x86 conversion the reference runs through gives.
__host__ __device__ inline int64_t mt_ema_i64(int64_t e, int64_t x, float d, float omd) {
    const float r = mt_ema((float)e, (float)x, d, omd);
    if (!(r > -9.2233720368547758e18f && r < 9.2233720368547758e18f)) return INT64_MIN;
    return (int64_t)r;
}

template <int MODE> struct MtUse {
    static constexpr bool adam = MODE == MODE_ADAM || MODE == MODE_ADAM_EMA;
    static constexpr bool rp = MODE != MODE_SCALE, wp = adam;
    static constexpr bool rg = MODE == MODE_SCALE || adam, wg = MODE == MODE_SCALE;
    static constexpr bool mv = adam;
    static constexpr bool re = MODE == MODE_ADAM_EMA || MODE == MODE_EMA, we = re || MODE == MODE_SET;
};
template <int MODE> __host__ __device__ inline void mt_elem(float& p, float& g, float& m, float& v, float& e, const MtCtx& c) {
    if (MODE == MODE_SCALE) g = mt_clip(g, c);
    if (MtUse<MODE>::adam) mt_adamw(p, g, m, v, c);
    if (MtUse<MODE>::re) e = mt_ema(e, p, c.d, c.omd);
    if (MODE == MODE_SET) e = p;
}
template <int MODE> __host__ __device__ inline void mt_quad(f32x4& P, f32x4& G, f32x4& M, f32x4& V, f32x4& E, const MtCtx& c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float p = P[k], g = G[k], m = M[k], v = V[k], e = E[k];
        mt_elem<MODE>(p, g, m, v, e, c);
        P[k] = p; G[k] = g; M[k] = m; V[k] = v; E[k] = e;
    }
}
__host__ __device__ inline f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__host__ __device__ inline void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// one lane's share of one chunk: p .. e already point at the chunk's first element (null where the mode does not touch the array)
template <int MODE>
__host__ __device__ inline void mt_chunk_mode(float* p, float* g, float* m, float* v, float* e, int count, int lane, bool vec, const MtCtx& c) {
    typedef MtUse<MODE> U;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (vec && count == LWDETR_MT_CHUNK) {
        f32x4 P[MT_ROUNDS], G[MT_ROUNDS], M[MT_ROUNDS], V[MT_ROUNDS], E[MT_ROUNDS];
#pragma unroll
        for (int r = 0; r < MT_ROUNDS; ++r) {
            const int i = r * MT_ROUND_ELEMS + lane * 4;
            P[r] = U::rp ? ld4(p + i) : zero;
            G[r] = U::rg ? ld4(g + i) : zero;
            M[r] = U::mv ? ld4(m + i) : zero;
            V[r] = U::mv ? ld4(v + i) : zero;
            E[r] = U::re ? ld4(e + i) : zero;
        }
#pragma unroll
        for (int r = 0; r < MT_ROUNDS; ++r) {
            const int i = r * MT_ROUND_ELEMS + lane * 4;
            mt_quad<MODE>(P[r], G[r], M[r], V[r], E[r], c);
            if (U::wp) st4(p + i, P[r]);
            if (U::wg) st4(g + i, G[r]);
            if (U::mv) { st4(m + i, M[r]); st4(v + i, V[r]); }
            if (U::we) st4(e + i, E[r]);
        }
        return;
    }
    for (int r = 0; r < MT_ROUNDS; ++r) {
        const int i = r * MT_ROUND_ELEMS + lane * 4;
        const int n = count - i < 4 ? count - i : 4;
        if (n <= 0) break;
        if (vec && n == 4) {
            f32x4 P = U::rp ? ld4(p + i) : zero, G = U::rg ? ld4(g + i) : zero, M = U::mv ? ld4(m + i) : zero, V = U::mv ? ld4(v + i) : zero,
                  E = U::re ? ld4(e + i) : zero;
            mt_quad<MODE>(P, G, M, V, E, c);
            if (U::wp) st4(p + i, P);
            if (U::wg) st4(g + i, G);
            if (U::mv) { st4(m + i, M); st4(v + i, V); }
            if (U::we) st4(e + i, E);
        } else {
            for (int k = 0; k < n; ++k) {
                float pp = U::rp ? p[i + k] : 0.f, gg = U::rg ? g[i + k] : 0.f, mm = U::mv ? m[i + k] : 0.f, vv = U::mv ? v[i + k] : 0.f,
                      ee = U::re ? e[i + k] : 0.f;
                mt_elem<MODE>(pp, gg, mm, vv, ee, c);
                if (U::wp) p[i + k] = pp;
                if (U::wg) g[i + k] = gg;
                if (U::mv) { m[i + k] = mm; v[i + k] = vv; }
                if (U::we) e[i + k] = ee;
            }
        }
    }
}

__host__ __device__ inline uintptr_t mt_bits(const void* a) { return reinterpret_cast<uintptr_t>(a); }
__host__ __device__ inline float* mt_at(void* base, int64_t off) { return base ? static_cast<float*>(base) + off : nullptr; }

// a chunk whose record or range does not hold together takes no part (lwdetr_mt_check refuses such tables on the host before they are used)
__host__ __device__ inline int mt_chunk_count(const lwdetr_mt_tensor& t, const lwdetr_mt_chunk& ck) {
    if (ck.offset < 0 || ck.offset >= t.numel || ck.count <= 0) return 0;
    const int64_t left = t.numel - ck.offset;
    int n = ck.count < LWDETR_MT_CHUNK ? ck.count : LWDETR_MT_CHUNK;
    if ((int64_t)n > left) n = (int)left;
    return n;
}

__host__ __device__ inline void mt_chunk_step(const lwdetr_mt_tensor& t, const lwdetr_mt_chunk& ck, int lane, const lwdetr_mt_hyper& h,
                                              unsigned flags, float coef, float coef_lo) {
    const int count = mt_chunk_count(t, ck);
    if (count <= 0) return;
    const bool ema = (flags & LWDETR_MT_EMA) != 0, set = (flags & LWDETR_MT_EMA_SET) != 0;
    if (t.kind == LWDETR_MT_EMA_I64) {
        if (!(ema || set) || !t.p || !t.ema) return;
        const int64_t* x = static_cast<const int64_t*>(t.p) + ck.offset;
        int64_t* e = static_cast<int64_t*>(t.ema) + ck.offset;
        for (int i = lane; i < count; i += MT_WAVE) e[i] = set ? x[i] : mt_ema_i64(e[i], x[i], h.ema_decay, h.ema_one_minus_decay);
        return;
    }
    if (t.kind != LWDETR_MT_PARAM && t.kind != LWDETR_MT_EMA_F32) return;
    const bool grads = t.kind == LWDETR_MT_PARAM && !t.skip && t.g;
    const bool scale = (flags & LWDETR_MT_SCALE_GRADS) && grads;
    const bool adam = (flags & LWDETR_MT_ADAMW) && grads && t.p && t.m && t.v;
    const bool avg = (ema || set) && t.p && t.ema;
    if (!(scale || adam || avg)) return;
    uintptr_t bits = 0;
    if (scale || adam) bits |= mt_bits(t.g);
    if (adam) bits |= mt_bits(t.p) | mt_bits(t.m) | mt_bits(t.v);
    if (avg) bits |= mt_bits(t.p) | mt_bits(t.ema);
    const bool vec = (bits & 15) == 0;
    MtCtx c;
    c.coef = coef; c.coef_lo = coef_lo; c.decay_mul = t.decay_mul; c.neg_step = t.neg_step_size; c.rbc2 = adam ? 1.f / t.bc2_sqrt : 0.f;
    c.w1 = h.one_minus_beta1; c.beta2 = h.beta2; c.w2 = h.one_minus_beta2; c.eps = h.eps; c.d = h.ema_decay; c.omd = h.ema_one_minus_decay;
    float *p = mt_at(t.p, ck.offset), *g = mt_at(t.g, ck.offset), *m = mt_at(t.m, ck.offset), *v = mt_at(t.v, ck.offset),
          *e = mt_at(t.ema, ck.offset);
    if (scale) mt_chunk_mode<MODE_SCALE>(p, g, m, v, e, count, lane, vec, c);
    else if (adam && avg && ema) mt_chunk_mode<MODE_ADAM_EMA>(p, g, m, v, e, count, lane, vec, c);
    else if (adam) mt_chunk_mode<MODE_ADAM>(p, g, m, v, e, count, lane, vec, c);
    else if (ema) mt_chunk_mode<MODE_EMA>(p, g, m, v, e, count, lane, vec, c);
    else mt_chunk_mode<MODE_SET>(p, g, m, v, e, count, lane, vec, c);
}

// one lane's sum of the squares of its elements of the chunk, rounds outer, the quad inner, on both paths
__host__ __device__ inline float mt_chunk_sumsq(const lwdetr_mt_tensor& t, const lwdetr_mt_chunk& ck, int lane) {
    const int count = mt_chunk_count(t, ck);
    if (count <= 0 || t.kind != LWDETR_MT_PARAM || t.skip || !t.g) return 0.f;
    const float* g = static_cast<const float*>(t.g) + ck.offset;
    const bool vec = (mt_bits(t.g) & 15) == 0;
    float s = 0.f;
    if (vec && count == LWDETR_MT_CHUNK) {
        f32x4 G[MT_ROUNDS];
#pragma unroll
        for (int r = 0; r < MT_ROUNDS; ++r) G[r] = ld4(g + r * MT_ROUND_ELEMS + lane * 4);
#pragma unroll
        for (int r = 0; r < MT_ROUNDS; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) s = s + G[r][k] * G[r][k];
        return s;
    }
    for (int r = 0; r < MT_ROUNDS; ++r) {
        const int i = r * MT_ROUND_ELEMS + lane * 4;
        const int n = count - i < 4 ? count - i : 4;
        if (n <= 0) break;
        for (int k = 0; k < n; ++k) s = s + g[i + k] * g[i + k];
    }
    return s;
}

// clamp(max_norm / (total_norm + 1e-6), max = 1) with torch's NaN rule: a NaN passes through the clamp
// (the quotient is taken in f64 from the unrounded norm; norm_clip = {total_norm, clip_coef, clip_coef's f32 remainder, 0})
__host__ __device__ inline void mt_norm_clip(double sumsq, double max_norm, float* out) {
    const double tn = sqrt(sumsq);
    double c = max_norm / (tn + 1e-6);
    if (c > 1.0) c = 1.0;
    const float hi = (float)c;
    out[0] = (float)tn;
    out[1] = hi;
    out[2] = (float)(c - (double)hi);          // what f32 drops of the coefficient (0 when it clamps to 1, NaN with a NaN)
    out[3] = 0.f;
}

__global__ __launch_bounds__(MT_THREADS) void mt_sumsq_kernel(const lwdetr_mt_tensor* __restrict__ tensors, int ntensors,
                                                              const lwdetr_mt_chunk* __restrict__ chunks, int nchunks,
                                                              float* __restrict__ partials) {
    const int lane = threadIdx.x & (MT_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = (int)gridDim.x * MT_WAVES;
    for (int c = (int)blockIdx.x * MT_WAVES + wave; c < nchunks; c += nwaves) {
        const lwdetr_mt_chunk ck = chunks[c];
        float s = 0.f;
        if ((unsigned)ck.tensor < (unsigned)ntensors) s = mt_chunk_sumsq(tensors[ck.tensor], ck, lane);
#pragma unroll
        for (int o = MT_WAVE / 2; o > 0; o >>= 1) s = s + __shfl_down(s, o, MT_WAVE);
        if (lane == 0) partials[c] = s;
    }
}

__global__ __launch_bounds__(MT_FINISH_THREADS) void mt_norm_finish_kernel(const float* __restrict__ partials, int nchunks, double max_norm,
                                                                           float* __restrict__ norm_clip) {
    __shared__ double sm[MT_FINISH_THREADS];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < nchunks; i += MT_FINISH_THREADS) acc = acc + (double)partials[i];
    sm[tid] = acc;
    __syncthreads();
    for (int o = MT_FINISH_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) sm[tid] = sm[tid] + sm[tid + o];
        __syncthreads();
    }
    if (tid == 0) mt_norm_clip(sm[0], max_norm, norm_clip);
}

__global__ __launch_bounds__(MT_THREADS) void mt_step_kernel(const lwdetr_mt_tensor* __restrict__ tensors, int ntensors,
                                                             const lwdetr_mt_chunk* __restrict__ chunks, int nchunks, lwdetr_mt_hyper h,
                                                             unsigned flags, const float* __restrict__ norm_clip) {
    const int lane = threadIdx.x & (MT_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = (int)gridDim.x * MT_WAVES;
    const float coef = norm_clip ? norm_clip[1] : 1.f, coef_lo = norm_clip ? norm_clip[2] : 0.f;
    for (int c = (int)blockIdx.x * MT_WAVES + wave; c < nchunks; c += nwaves) {
        const lwdetr_mt_chunk ck = chunks[c];
        if ((unsigned)ck.tensor >= (unsigned)ntensors) continue;
        mt_chunk_step(tensors[ck.tensor], ck, lane, h, flags, coef, coef_lo);
    }
}

int mt_check_flags(unsigned flags, const lwdetr_mt_hyper* hyper, const float* norm_clip) {
    const unsigned all = LWDETR_MT_SCALE_GRADS | LWDETR_MT_ADAMW | LWDETR_MT_EMA | LWDETR_MT_EMA_SET;
    if (flags == 0 || (flags & ~all)) return LWDETR_ERR_BAD_ARG;
    if ((flags & LWDETR_MT_EMA) && (flags & LWDETR_MT_EMA_SET)) return LWDETR_ERR_BAD_ARG;
    if ((flags & LWDETR_MT_SCALE_GRADS) && !norm_clip) return LWDETR_ERR_BAD_ARG;
    if ((flags & (LWDETR_MT_ADAMW | LWDETR_MT_EMA)) && !hyper) return LWDETR_ERR_BAD_ARG;
    if ((flags & LWDETR_MT_SCALE_GRADS) && flags != LWDETR_MT_SCALE_GRADS) return LWDETR_ERR_UNSUPPORTED;   // the fused form scales in registers
    if ((flags & LWDETR_MT_ADAMW) && (flags & LWDETR_MT_EMA_SET)) return LWDETR_ERR_UNSUPPORTED;
    return LWDETR_OK;
}
int mt_launched(int which, int rc) {
    if (rc == LWDETR_OK) g_mt_launches[which].fetch_add(1, std::memory_order_relaxed);
    return rc;
}
unsigned mt_blocks(int nchunks) {
    const int b = (nchunks + MT_WAVES - 1) / MT_WAVES;
    return (unsigned)(b < MT_MAX_BLOCKS ? b : MT_MAX_BLOCKS);
}

}  // namespace

extern "C" int lwdetr_mt_check(const lwdetr_mt_tensor* tensors, int ntensors, const lwdetr_mt_chunk* chunks, int nchunks) {
    if (!tensors || !chunks || ntensors <= 0 || nchunks <= 0) return LWDETR_ERR_BAD_ARG;
    for (int i = 0; i < ntensors; ++i) {
        const lwdetr_mt_tensor& t = tensors[i];
        if (t.numel <= 0 || t.kind < LWDETR_MT_PARAM || t.kind > LWDETR_MT_EMA_I64) return LWDETR_ERR_BAD_ARG;
        if (t.kind == LWDETR_MT_EMA_I64 && ((mt_bits(t.p) | mt_bits(t.ema)) & 7)) return LWDETR_ERR_BAD_ARG;
        if (t.kind != LWDETR_MT_EMA_I64 && ((mt_bits(t.p) | mt_bits(t.g) | mt_bits(t.m) | mt_bits(t.v) | mt_bits(t.ema)) & 3)) return LWDETR_ERR_BAD_ARG;
    }
    // the chunks tile every tensor exactly once, in order: nothing is left out and nothing is done twice
    int c = 0;
    for (int i = 0; i < ntensors; ++i) {
        int64_t off = 0;
        while (off < tensors[i].numel) {
            if (c >= nchunks) return LWDETR_ERR_BAD_ARG;
            const lwdetr_mt_chunk& ck = chunks[c++];
            const int64_t left = tensors[i].numel - off;
            const int64_t want = left < LWDETR_MT_CHUNK ? left : LWDETR_MT_CHUNK;
            if (ck.tensor != i || ck.offset != off || (int64_t)ck.count != want) return LWDETR_ERR_BAD_ARG;
            off += want;
        }
    }
    return c == nchunks ? LWDETR_OK : LWDETR_ERR_BAD_ARG;
}

extern "C" int lwdetr_mt_sumsq(const lwdetr_mt_tensor* tensors, int ntensors, const lwdetr_mt_chunk* chunks, int nchunks, float* partials,
                               void* hip_stream) {
    if (!tensors || !chunks || !partials || ntensors <= 0 || nchunks <= 0) return LWDETR_ERR_BAD_ARG;
    hipLaunchKernelGGL(mt_sumsq_kernel, dim3(mt_blocks(nchunks)), dim3(MT_THREADS), 0, (hipStream_t)hip_stream, tensors, ntensors, chunks,
                       nchunks, partials);
    return mt_launched(MT_L_SUMSQ, lwdetr_check_launch());
}

extern "C" int lwdetr_mt_norm_finish(const float* partials, int nchunks, double max_norm, float* norm_clip, void* hip_stream) {
    if (!partials || !norm_clip || nchunks <= 0 || !(max_norm > 0.0)) return LWDETR_ERR_BAD_ARG;
    hipLaunchKernelGGL(mt_norm_finish_kernel, dim3(1), dim3(MT_FINISH_THREADS), 0, (hipStream_t)hip_stream, partials, nchunks, max_norm,
                       norm_clip);
    return mt_launched(MT_L_FINISH, lwdetr_check_launch());
}

extern "C" int lwdetr_mt_step(const lwdetr_mt_tensor* tensors, int ntensors, const lwdetr_mt_chunk* chunks, int nchunks,
                              const lwdetr_mt_hyper* hyper, unsigned flags, const float* norm_clip, void* hip_stream) {
    if (!tensors || !chunks || ntensors <= 0 || nchunks <= 0) return LWDETR_ERR_BAD_ARG;
    const int rc = mt_check_flags(flags, hyper, norm_clip);
    if (rc != LWDETR_OK) return rc;
    const lwdetr_mt_hyper h = hyper ? *hyper : lwdetr_mt_hyper{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    hipLaunchKernelGGL(mt_step_kernel, dim3(mt_blocks(nchunks)), dim3(MT_THREADS), 0, (hipStream_t)hip_stream, tensors, ntensors, chunks,
                       nchunks, h, flags, norm_clip);
    return mt_launched(MT_L_STEP, lwdetr_check_launch());
}

extern "C" int lwdetr_mt_norm_host(const lwdetr_mt_tensor* tensors, int ntensors, const lwdetr_mt_chunk* chunks, int nchunks, double max_norm,
                                   float* norm_clip) {
    if (!norm_clip || !(max_norm > 0.0)) return LWDETR_ERR_BAD_ARG;
    const int rc = lwdetr_mt_check(tensors, ntensors, chunks, nchunks);
    if (rc != LWDETR_OK) return rc;
    std::vector<float> partials(nchunks);
    for (int c = 0; c < nchunks; ++c) {
        float s[MT_WAVE];
        for (int lane = 0; lane < MT_WAVE; ++lane) s[lane] = mt_chunk_sumsq(tensors[chunks[c].tensor], chunks[c], lane);
        for (int o = MT_WAVE / 2; o > 0; o >>= 1)
            for (int lane = 0; lane < o; ++lane) s[lane] = s[lane] + s[lane + o];
        partials[c] = s[0];
    }
    double sm[MT_FINISH_THREADS];
    for (int tid = 0; tid < MT_FINISH_THREADS; ++tid) {
        double acc = 0.0;
        for (int i = tid; i < nchunks; i += MT_FINISH_THREADS) acc = acc + (double)partials[i];
        sm[tid] = acc;
    }
    for (int o = MT_FINISH_THREADS / 2; o > 0; o >>= 1)
        for (int tid = 0; tid < o; ++tid) sm[tid] = sm[tid] + sm[tid + o];
    mt_norm_clip(sm[0], max_norm, norm_clip);
    return LWDETR_OK;
}

extern "C" int lwdetr_mt_step_host(const lwdetr_mt_tensor* tensors, int ntensors, const lwdetr_mt_chunk* chunks, int nchunks,
                                   const lwdetr_mt_hyper* hyper, unsigned flags, const float* norm_clip) {
    int rc = lwdetr_mt_check(tensors, ntensors, chunks, nchunks);
    if (rc != LWDETR_OK) return rc;
    rc = mt_check_flags(flags, hyper, norm_clip);
    if (rc != LWDETR_OK) return rc;
    const lwdetr_mt_hyper h = hyper ? *hyper : lwdetr_mt_hyper{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float coef = norm_clip ? norm_clip[1] : 1.f, coef_lo = norm_clip ? norm_clip[2] : 0.f;
    for (int c = 0; c < nchunks; ++c)
        for (int lane = 0; lane < MT_WAVE; ++lane) mt_chunk_step(tensors[chunks[c].tensor], chunks[c], lane, h, flags, coef, coef_lo);
    return LWDETR_OK;
}

extern "C" int lwdetr_mt_launch_counts(long* out, int n) {
    for (int i = 0; out && i < n && i < MT_L_COUNT; ++i) out[i] = g_mt_launches[i].load(std::memory_order_relaxed);
    return MT_L_COUNT;
}
extern "C" const char* lwdetr_mt_launch_name(int i) { return i >= 0 && i < MT_L_COUNT ? kMtLaunchNames[i] : nullptr; }
