// Training-forward glue that has no GEMM in it: the channels-first LayerNorm at the end of a projector stage (reference
// models/backbone/projector.py:21-47) and the query sine embedding of the decoder (models/transformer.py:42-68), forward and backward.
// f32 / f16 / bf16 I/O, f32 arithmetic, one rounding per output element; no floating-point atomic, every sum has one fixed order.
//
// LayerNorm2d. x is (B, C, H*W). A workgroup owns LN_PX = 64 consecutive pixels of one image; lane = pixel, so every NCHW access is 64
// consecutive elements of one channel row. Its four waves take the channels c = wave, wave + 4, ...; a pixel's sum over C is the four waves'
// partial sums added in wave order. The statistics are two passes (mean, then the mean of (x - mean)^2) over a tile that the first pass
// left in L2. The token layout (B, H*W, C) has lanes along C: a 64-channel x 64-pixel chunk goes through an LDS tile with rows of 65 words
// (a column read or write then touches 32 different banks per half wave), so both sides stay coalesced.
// Backward: dx = rstd (g - mean_c g - xhat mean_c(g xhat)), g = dy w. dw_c / db_c: every workgroup reduces its 64 pixels with a butterfly
// and writes one partial per channel; ln2d_finish_kernel adds the partials in ascending workgroup order.
//
// Sine embed. One wave per box row, lanes along the 4 * dim output columns. The argument is formed in revolutions, r = box / dim_t, from
// a host table of 1 / dim_t split into two floats: the product's rounding error is recovered with an FMA, the integer part is removed
// exactly, and sinf / cosf see |theta| <= pi whatever the box magnitude.
#include "common.h"

#include <atomic>

namespace {

constexpr int LN_PX = 64, LN_WAVES = 4, LN_THREADS = 256, LN_CH = 64, LN_LD = LN_PX + 1;
constexpr int LN_MAX_C = 1024, SE_MAX_DIM = 256;

enum { TG_LN_FWD_NCHW = 0, TG_LN_FWD_TOK, TG_LN_BWD_NCHW, TG_LN_BWD_TOK, TG_SINE_FWD, TG_SINE_BWD, TG_KINDS };
constexpr int TGP_COUNT = TG_KINDS * 3;
const char* const kTgPathNames[TGP_COUNT] = {
    "ln2d_fwd_nchw_f32", "ln2d_fwd_nchw_f16", "ln2d_fwd_nchw_bf16", "ln2d_fwd_tok_f32", "ln2d_fwd_tok_f16", "ln2d_fwd_tok_bf16",
    "ln2d_bwd_nchw_f32", "ln2d_bwd_nchw_f16", "ln2d_bwd_nchw_bf16", "ln2d_bwd_tok_f32", "ln2d_bwd_tok_f16", "ln2d_bwd_tok_bf16",
    "sine_fwd_f32", "sine_fwd_f16", "sine_fwd_bf16", "sine_bwd_f32", "sine_bwd_f16", "sine_bwd_bf16"};
std::atomic<long> g_tg_path[TGP_COUNT];

int tg_path_done(int kind, int dtype, int rc) {
    if (rc == LWDETR_OK) g_tg_path[kind * 3 + dtype].fetch_add(1, std::memory_order_relaxed);
    return rc;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- LayerNorm2d
struct LnParams {
    const void* x;
    const float* w;
    const float* b;
    void* y;
    float* mean;
    float* rstd;
    const void* dy;
    void* dx;
    float* part;
    int C;
    long HW;
    float eps;
};

template <typename T, bool TOK> __global__ __launch_bounds__(LN_THREADS) void ln2d_fwd_kernel(LnParams p) {
    __shared__ float red[LN_WAVES][LN_PX];
    __shared__ float tile[TOK ? LN_CH * LN_LD : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = p.C;
    const long HW = p.HW, b = blockIdx.y, px0 = (long)blockIdx.x * LN_PX, px = px0 + lane;
    const bool ok = px < HW;
    const T* xb = (const T*)p.x + b * C * HW;
    const float inv_c = 1.f / (float)C;

    float a = 0.f;
    if (ok)
        for (int c = wave; c < C; c += LN_WAVES) a += to_f32(xb[(long)c * HW + px]);
    red[wave][lane] = a;
    __syncthreads();
    const float mean = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) * inv_c;
    __syncthreads();
    a = 0.f;
    if (ok)
        for (int c = wave; c < C; c += LN_WAVES) {
            const float d = to_f32(xb[(long)c * HW + px]) - mean;
            a += d * d;
        }
    red[wave][lane] = a;
    __syncthreads();
    const float var = (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]) * inv_c;
    const float rstd = 1.f / sqrtf(var + p.eps);
    if (wave == 0 && ok) {
        p.mean[b * HW + px] = mean;
        p.rstd[b * HW + px] = rstd;
    }
    if (!TOK) {
        T* yb = (T*)p.y + b * C * HW;
        if (ok)
            for (int c = wave; c < C; c += LN_WAVES)
                yb[(long)c * HW + px] = from_f32<T>((to_f32(xb[(long)c * HW + px]) - mean) * rstd * p.w[c] + p.b[c]);
    } else {
        T* yb = (T*)p.y + b * HW * C;
        for (int c0 = 0; c0 < C; c0 += LN_CH) {
            __syncthreads();
#pragma unroll 4
            for (int i = 0; i < LN_CH / LN_WAVES; ++i) {
                const int cl = wave * (LN_CH / LN_WAVES) + i, c = c0 + cl;
                float v = 0.f;
                if (ok && c < C) v = (to_f32(xb[(long)c * HW + px]) - mean) * rstd * p.w[c] + p.b[c];
                tile[cl * LN_LD + lane] = v;
            }
            __syncthreads();
            const int c = c0 + lane;
            for (int pl = wave; pl < LN_PX; pl += LN_WAVES) {
                const long po = px0 + pl;
                if (po < HW && c < C) yb[po * C + c] = from_f32<T>(tile[lane * LN_LD + pl]);
            }
        }
    }
}

// PASS 0: the per-pixel sums over C of g and g xhat, and the workgroup's per-channel partials of dw / db. PASS 1: dx.
template <typename T, bool TOK, int PASS>
__device__ __forceinline__ void ln2d_bwd_pass(const LnParams& p, float* tile, long b, long px0, int lane, int wave, bool ok, float mean, float rstd,
                                              float m1, float m2, float& s1, float& s2, long wg) {
    const int C = p.C;
    const long HW = p.HW, px = px0 + lane;
    const T* xb = (const T*)p.x + b * C * HW;
    for (int c0 = 0; c0 < C; c0 += LN_CH) {
        if (TOK) {
            __syncthreads();
            const T* dyb = (const T*)p.dy + b * HW * C;
            const int c = c0 + lane;
            for (int pl = wave; pl < LN_PX; pl += LN_WAVES) {
                const long po = px0 + pl;
                tile[lane * LN_LD + pl] = (po < HW && c < C) ? to_f32(dyb[po * C + c]) : 0.f;
            }
            __syncthreads();
        }
        for (int i = 0; i < LN_CH / LN_WAVES; ++i) {
            const int cl = wave * (LN_CH / LN_WAVES) + i, c = c0 + cl;
            if (c >= C) break;                                      // wave-uniform
            float dyv = 0.f, xh = 0.f;
            if (ok) {
                dyv = TOK ? tile[cl * LN_LD + lane] : to_f32(((const T*)p.dy)[(b * C + c) * HW + px]);
                xh = (to_f32(xb[(long)c * HW + px]) - mean) * rstd;
            }
            const float g = dyv * p.w[c];
            if (PASS == 0) {
                s1 += g;
                s2 += g * xh;
                const float pw = wave_sum(dyv * xh), pb = wave_sum(dyv);
                if (lane == 0) {
                    p.part[(wg * 2 + 0) * C + c] = pw;
                    p.part[(wg * 2 + 1) * C + c] = pb;
                }
            } else if (ok) {
                ((T*)p.dx)[(b * C + c) * HW + px] = from_f32<T>(rstd * ((g - m1) - xh * m2));
            }
        }
    }
}

template <typename T, bool TOK> __global__ __launch_bounds__(LN_THREADS) void ln2d_bwd_kernel(LnParams p) {
    __shared__ float red1[LN_WAVES][LN_PX];
    __shared__ float red2[LN_WAVES][LN_PX];
    __shared__ float tile[TOK ? LN_CH * LN_LD : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long HW = p.HW, b = blockIdx.y, px0 = (long)blockIdx.x * LN_PX, px = px0 + lane;
    const long wg = b * gridDim.x + blockIdx.x;
    const bool ok = px < HW;
    const float mean = ok ? p.mean[b * HW + px] : 0.f, rstd = ok ? p.rstd[b * HW + px] : 0.f;
    float s1 = 0.f, s2 = 0.f;
    ln2d_bwd_pass<T, TOK, 0>(p, tile, b, px0, lane, wave, ok, mean, rstd, 0.f, 0.f, s1, s2, wg);
    red1[wave][lane] = s1;
    red2[wave][lane] = s2;
    __syncthreads();
    const float inv_c = 1.f / (float)p.C;
    const float m1 = (((red1[0][lane] + red1[1][lane]) + red1[2][lane]) + red1[3][lane]) * inv_c;
    const float m2 = (((red2[0][lane] + red2[1][lane]) + red2[2][lane]) + red2[3][lane]) * inv_c;
    ln2d_bwd_pass<T, TOK, 1>(p, tile, b, px0, lane, wave, ok, mean, rstd, m1, m2, s1, s2, wg);
}

// dw[c] / db[c]: the workgroups' partials in ascending workgroup order
__global__ void ln2d_finish_kernel(const float* part, float* dw, float* db, long nwg, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float aw = 0.f, ab = 0.f;
    for (long g = 0; g < nwg; ++g) {
        aw += part[(g * 2 + 0) * C + c];
        ab += part[(g * 2 + 1) * C + c];
    }
    dw[c] = aw;
    db[c] = ab;
}

// ----------------------------------------------------------------------------------------------------------------- sine embed
struct SeParams {
    const void* boxes;
    long ld;
    const float* inv_hi;
    const float* inv_lo;
    void* out;
    const void* gout;
    void* gboxes;
    long rows;
    int dim;
};

// theta in [-pi, pi] with sin / cos equal to those of 2 pi v (ih + il)
__device__ __forceinline__ float se_theta(float v, float ih, float il) {
    const float r = v * ih;
    const float e = fmaf(v, ih, -r) + v * il;
    const float f = (r - rintf(r)) + e;
    return fmaf(f, 6.2831855f, f * -1.7484555e-7f);                  // 2 pi = 6.2831855 - 1.7484555e-7
}

// output block -> box coordinate: y, x, w, h
__device__ __forceinline__ int se_coord(int blk) { return blk == 0 ? 1 : (blk == 1 ? 0 : blk); }

template <typename T> __global__ __launch_bounds__(256) void sine_fwd_kernel(SeParams p) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const T* bx = (const T*)p.boxes + row * p.ld;
    const float v[4] = {to_f32(bx[0]), to_f32(bx[1]), to_f32(bx[2]), to_f32(bx[3])};
    T* out = (T*)p.out + row * 4 * p.dim;
    for (int col = lane; col < 4 * p.dim; col += 64) {
        const int blk = col / p.dim, j = col - blk * p.dim, cc = se_coord(blk);
        const float val = cc == 0 ? v[0] : (cc == 1 ? v[1] : (cc == 2 ? v[2] : v[3]));
        const float th = se_theta(val, p.inv_hi[j], p.inv_lo[j]);
        out[col] = from_f32<T>((j & 1) ? cosf(th) : sinf(th));
    }
}

template <typename T> __global__ __launch_bounds__(256) void sine_bwd_kernel(SeParams p) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;                                       // wave-uniform: the shuffles below see whole waves
    const T* bx = (const T*)p.boxes + row * p.ld;
    const float v[4] = {to_f32(bx[0]), to_f32(bx[1]), to_f32(bx[2]), to_f32(bx[3])};
    const T* go = (const T*)p.gout + row * 4 * p.dim;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int col = lane; col < 4 * p.dim; col += 64) {
        const int blk = col / p.dim, j = col - blk * p.dim, cc = se_coord(blk);
        const float val = cc == 0 ? v[0] : (cc == 1 ? v[1] : (cc == 2 ? v[2] : v[3]));
        const float ih = p.inv_hi[j];
        const float th = se_theta(val, ih, p.inv_lo[j]);
        const float t = to_f32(go[col]) * (6.2831855f * ih) * ((j & 1) ? -sinf(th) : cosf(th));
        a0 += cc == 0 ? t : 0.f;
        a1 += cc == 1 ? t : 0.f;
        a2 += cc == 2 ? t : 0.f;
        a3 += cc == 3 ? t : 0.f;
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3);
    if (lane == 0) {
        T* gb = (T*)p.gboxes + row * 4;
        gb[0] = from_f32<T>(a0); gb[1] = from_f32<T>(a1); gb[2] = from_f32<T>(a2); gb[3] = from_f32<T>(a3);
    }
}

// ------------------------------------------------------------------------------------------------------------------------ host
size_t esize(int dtype) { return dtype == DT_F32 ? 4 : 2; }
bool dtype_ok(int dtype) { return dtype == DT_F32 || dtype == DT_F16 || dtype == DT_BF16; }
bool aligned(const void* p, size_t a) { return (uintptr_t)p % a == 0; }
long ln_tiles(long HW) { return (HW + LN_PX - 1) / LN_PX; }

int ln_check(int B, int C, long HW, int dtype) {
    if (!dtype_ok(dtype)) return LWDETR_ERR_UNSUPPORTED;
    if (B < 1 || B > 65535 || C < 1 || C > LN_MAX_C || HW < 1 || ln_tiles(HW) > 0x7fffffffL) return LWDETR_ERR_BAD_ARG;
    return LWDETR_OK;
}

template <typename T> int launch_ln_fwd(const LnParams& p, int B, int tokens, int dtype, hipStream_t st) {
    const dim3 grid((unsigned)ln_tiles(p.HW), (unsigned)B), block(LN_THREADS);
    if (tokens) hipLaunchKernelGGL((ln2d_fwd_kernel<T, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((ln2d_fwd_kernel<T, false>), grid, block, 0, st, p);
    return tg_path_done(tokens ? TG_LN_FWD_TOK : TG_LN_FWD_NCHW, dtype, lwdetr_check_launch());
}

template <typename T> int launch_ln_bwd(const LnParams& p, int B, int tokens, int dtype, float* dw, float* db, hipStream_t st) {
    const dim3 grid((unsigned)ln_tiles(p.HW), (unsigned)B), block(LN_THREADS);
    if (tokens) hipLaunchKernelGGL((ln2d_bwd_kernel<T, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((ln2d_bwd_kernel<T, false>), grid, block, 0, st, p);
    int rc = lwdetr_check_launch();
    if (rc != LWDETR_OK) return rc;
    hipLaunchKernelGGL(ln2d_finish_kernel, dim3((unsigned)((p.C + 255) / 256)), dim3(256), 0, st, (const float*)p.part, dw, db,
                       ln_tiles(p.HW) * B, p.C);
    return tg_path_done(tokens ? TG_LN_BWD_TOK : TG_LN_BWD_NCHW, dtype, lwdetr_check_launch());
}

int se_check(const void* boxes, long ld, const float* inv_hi, const float* inv_lo, long rows, int dim, int dtype) {
    if (!dtype_ok(dtype)) return LWDETR_ERR_UNSUPPORTED;
    if (rows < 0 || dim < 2 || dim > SE_MAX_DIM || (dim & 1) || ld < 4 || (rows + 3) / 4 > 0x7fffffffL) return LWDETR_ERR_BAD_ARG;
    if (!boxes || !inv_hi || !inv_lo || !aligned(boxes, esize(dtype)) || !aligned(inv_hi, 4) || !aligned(inv_lo, 4)) return LWDETR_ERR_BAD_ARG;
    return LWDETR_OK;
}

}  // namespace

extern "C" {

int lwdetr_ln2d_forward(const void* x, const float* w, const float* b, void* y, float* mean, float* rstd, int B, int C, long HW, float eps,
                        int tokens, int dtype, void* hip_stream) {
    const int rc = ln_check(B, C, HW, dtype);
    if (rc != LWDETR_OK) return rc;
    const size_t es = esize(dtype);
    if (!x || !w || !b || !y || !mean || !rstd || !aligned(x, es) || !aligned(y, es) || !aligned(w, 4) || !aligned(b, 4) || !aligned(mean, 4) ||
        !aligned(rstd, 4) || !(eps >= 0.f))
        return LWDETR_ERR_BAD_ARG;
    LnParams p = {};
    p.x = x; p.w = w; p.b = b; p.y = y; p.mean = mean; p.rstd = rstd; p.C = C; p.HW = HW; p.eps = eps;
    hipStream_t st = (hipStream_t)hip_stream;
    switch (dtype) {
        case DT_F32: return launch_ln_fwd<float>(p, B, tokens, dtype, st);
        case DT_F16: return launch_ln_fwd<f16>(p, B, tokens, dtype, st);
        default: return launch_ln_fwd<bf16>(p, B, tokens, dtype, st);
    }
}

long lwdetr_ln2d_workspace_floats(int B, int C, long HW) {
    if (B < 1 || C < 1 || HW < 1) return 0;
    return ln_tiles(HW) * B * 2 * C;
}

int lwdetr_ln2d_backward(const void* x, const float* w, const float* mean, const float* rstd, const void* dy, void* dx, float* dw, float* db,
                         float* ws, long ws_floats, int B, int C, long HW, int tokens, int dtype, void* hip_stream) {
    const int rc = ln_check(B, C, HW, dtype);
    if (rc != LWDETR_OK) return rc;
    const size_t es = esize(dtype);
    if (!x || !w || !mean || !rstd || !dy || !dx || !dw || !db || !ws || !aligned(x, es) || !aligned(dy, es) || !aligned(dx, es) || !aligned(w, 4) ||
        !aligned(mean, 4) || !aligned(rstd, 4) || !aligned(dw, 4) || !aligned(db, 4) || !aligned(ws, 4))
        return LWDETR_ERR_BAD_ARG;
    if (ws_floats < lwdetr_ln2d_workspace_floats(B, C, HW)) return LWDETR_ERR_BAD_ARG;
    LnParams p = {};
    p.x = x; p.w = w; p.mean = const_cast<float*>(mean); p.rstd = const_cast<float*>(rstd); p.dy = dy; p.dx = dx; p.part = ws; p.C = C; p.HW = HW;
    hipStream_t st = (hipStream_t)hip_stream;
    switch (dtype) {
        case DT_F32: return launch_ln_bwd<float>(p, B, tokens, dtype, dw, db, st);
        case DT_F16: return launch_ln_bwd<f16>(p, B, tokens, dtype, dw, db, st);
        default: return launch_ln_bwd<bf16>(p, B, tokens, dtype, dw, db, st);
    }
}

int lwdetr_sine_embed_forward(const void* boxes, long ld, const float* inv_hi, const float* inv_lo, void* out, long rows, int dim, int dtype,
                              void* hip_stream) {
    const int rc = se_check(boxes, ld, inv_hi, inv_lo, rows, dim, dtype);
    if (rc != LWDETR_OK) return rc;
    if (!out || !aligned(out, esize(dtype))) return LWDETR_ERR_BAD_ARG;
    if (rows == 0) return LWDETR_OK;
    SeParams p = {};
    p.boxes = boxes; p.ld = ld; p.inv_hi = inv_hi; p.inv_lo = inv_lo; p.out = out; p.rows = rows; p.dim = dim;
    hipStream_t st = (hipStream_t)hip_stream;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    switch (dtype) {
        case DT_F32: hipLaunchKernelGGL(sine_fwd_kernel<float>, grid, block, 0, st, p); break;
        case DT_F16: hipLaunchKernelGGL(sine_fwd_kernel<f16>, grid, block, 0, st, p); break;
        default: hipLaunchKernelGGL(sine_fwd_kernel<bf16>, grid, block, 0, st, p); break;
    }
    return tg_path_done(TG_SINE_FWD, dtype, lwdetr_check_launch());
}

int lwdetr_sine_embed_backward(const void* boxes, long ld, const float* inv_hi, const float* inv_lo, const void* grad_out, void* grad_boxes,
                               long rows, int dim, int dtype, void* hip_stream) {
    const int rc = se_check(boxes, ld, inv_hi, inv_lo, rows, dim, dtype);
    if (rc != LWDETR_OK) return rc;
    if (!grad_out || !grad_boxes || !aligned(grad_out, esize(dtype)) || !aligned(grad_boxes, esize(dtype))) return LWDETR_ERR_BAD_ARG;
    if (rows == 0) return LWDETR_OK;
    SeParams p = {};
    p.boxes = boxes; p.ld = ld; p.inv_hi = inv_hi; p.inv_lo = inv_lo; p.gout = grad_out; p.gboxes = grad_boxes; p.rows = rows; p.dim = dim;
    hipStream_t st = (hipStream_t)hip_stream;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    switch (dtype) {
        case DT_F32: hipLaunchKernelGGL(sine_bwd_kernel<float>, grid, block, 0, st, p); break;
        case DT_F16: hipLaunchKernelGGL(sine_bwd_kernel<f16>, grid, block, 0, st, p); break;
        default: hipLaunchKernelGGL(sine_bwd_kernel<bf16>, grid, block, 0, st, p); break;
    }
    return tg_path_done(TG_SINE_BWD, dtype, lwdetr_check_launch());
}

int lwdetr_train_glue_path_counts(long* out, int n) {
    for (int i = 0; out && i < n && i < TGP_COUNT; ++i) out[i] = g_tg_path[i].load(std::memory_order_relaxed);
    return TGP_COUNT;
}
const char* lwdetr_train_glue_path_name(int i) { return i >= 0 && i < TGP_COUNT ? kTgPathNames[i] : nullptr; }

}  // extern "C"
