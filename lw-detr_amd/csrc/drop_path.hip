// Stochastic depth on a residual of the ViT under training (reference models/backbone/vit.py:216-220 with timm's DropPath):
//   out[r, c] = x[r, c] + (gamma[c] * y[r, c]) * scale[r / rows_per_group]
// scale holds one f32 per group of rows (a window of the ViT): 0 for a dropped group, 1 / keep for a kept one. f32 arithmetic in exactly that
// order, one rounding to the output type; the object is built without contraction, so in f32 the result is torch's x + (gamma * y) * t to the
// bit. x / out / grad_out share one type (dx), y / grad_y another (dy): f32 + 16-bit is what autocast hands over (an f32 residual stream, a
// 16-bit Linear output, an f32 gamma).
//
// Forward: memory-bound, one pass. A thread owns V consecutive channels of one row: V = 16 bytes of the narrower type (4 f32, 8 16-bit; an f32
// x beside a 16-bit y is two 16-byte accesses) when C, every leading dimension and every pointer allow whole 16-byte chunks, one element
// otherwise. A group whose scale is 0 copies x and does not read y.
// Backward: grad_x is grad_out itself and is not written. grad_y = (grad_out * scale) * gamma; grad_gamma[c] = sum_r (grad_out * scale) * y.
// A workgroup owns DP_TILE consecutive rows; a thread owns V channels and walks the tile's rows in ascending order (with fewer than 256
// channel chunks, 256 / chunks row lanes share the tile, interleaved, and are added in lane order through LDS). The workgroup writes one
// partial per channel; dp_finish_kernel adds the partials in one fixed order (16 interleaved slices of the workgroups, each ascending, then the
// slices in order: one thread walking all partials of a channel is a chain of dependent L2 round trips, measured at 90 us for 400 workgroups).
// No atomic: two calls give the same bits.
#include "common.h"

#include <atomic>

namespace {

constexpr int DP_THREADS = 256, DP_TILE = 16, DP_MAX_C = 2048, DP_PAIRS = 5;
constexpr int DPP_COUNT = 2 * DP_PAIRS;
const char* const kDpPathNames[DPP_COUNT] = {"dp_fwd_f32_f32", "dp_fwd_f16_f16", "dp_fwd_bf16_bf16", "dp_fwd_f32_f16", "dp_fwd_f32_bf16",
                                             "dp_bwd_f32_f32", "dp_bwd_f16_f16", "dp_bwd_bf16_bf16", "dp_bwd_f32_f16", "dp_bwd_f32_bf16"};
std::atomic<long> g_dp_path[DPP_COUNT];

int dp_path_done(int path, int rc) {
    if (rc == LWDETR_OK) g_dp_path[path].fetch_add(1, std::memory_order_relaxed);
    return rc;
}

struct DpParams {
    const void* a;        // forward: x; backward: grad_out
    const void* y;
    const float* gamma;
    const float* scale;
    void* b;              // forward: out; backward: grad_y (may be null)
    float* part;
    long lda, ldy, ldb, rows, rpg, total;
    int C, small;         // small: rows * chunks fits 31 bits, so the index arithmetic is 32-bit
};

// V consecutive elements as f32: 16-byte accesses for V > 1 (the caller has checked the alignment), one element for V == 1
template <typename T, int V> __device__ __forceinline__ void ld(const T* p, float (&o)[V]) {
    if constexpr (V == 1) {
        o[0] = to_f32(*p);
    } else if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int i = 0; i < V / 4; ++i) {
            const f32x4 t = ((const f32x4*)p)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[4 * i + j] = t[j];
        }
    } else {
        static_assert(V == 8, "16-bit types move 8 elements per access");
        const typename Vec<T>::v8 t = *(const typename Vec<T>::v8*)p;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = to_f32<T>(t[j]);
    }
}

template <typename T, int V> __device__ __forceinline__ void st(T* p, const float (&v)[V]) {
    if constexpr (V == 1) {
        *p = from_f32<T>(v[0]);
    } else if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int i = 0; i < V / 4; ++i) {
            f32x4 t;
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = v[4 * i + j];
            ((f32x4*)p)[i] = t;
        }
    } else {
        static_assert(V == 8, "16-bit types move 8 elements per access");
        typename Vec<T>::v8 t;
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = from_f32<T>(v[j]);
        *(typename Vec<T>::v8*)p = t;
    }
}

__device__ __forceinline__ long dp_group(const DpParams& p, long r) {
    return p.small ? (long)((unsigned)r / (unsigned)p.rpg) : r / p.rpg;
}

template <typename TX, typename TY, int V, bool GAMMA> __global__ __launch_bounds__(DP_THREADS) void dp_fwd_kernel(DpParams p) {
    const long i = (long)blockIdx.x * DP_THREADS + threadIdx.x;
    if (i >= p.total) return;
    const int ncol = p.C / V;
    long r;
    int c;
    if (p.small) {
        const unsigned q = (unsigned)i / (unsigned)ncol;
        r = q;
        c = (int)((unsigned)i - q * (unsigned)ncol) * V;
    } else {
        r = i / ncol;
        c = (int)(i - r * ncol) * V;
    }
    const float s = p.scale[dp_group(p, r)];
    float o[V];
    ld<TX, V>((const TX*)p.a + r * p.lda + c, o);
    if (s != 0.f) {
        float yv[V];
        ld<TY, V>((const TY*)p.y + r * p.ldy + c, yv);
        if (GAMMA) {
            float gv[V];
            ld<float, V>(p.gamma + c, gv);
#pragma unroll
            for (int j = 0; j < V; ++j) yv[j] = gv[j] * yv[j];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = o[j] + yv[j] * s;
    }
    st<TX, V>((TX*)p.b + r * p.ldb + c, o);
}

// GG: grad_gamma is wanted (then GAMMA, and y is read)
template <typename TX, typename TY, int V, bool GAMMA, bool GG> __global__ __launch_bounds__(DP_THREADS) void dp_bwd_kernel(DpParams p) {
    __shared__ float red[GG ? DP_THREADS * 8 : 1];
    const int tid = threadIdx.x, C = p.C, ncol = C / V;
    const int nrl = ncol >= DP_THREADS ? 1 : DP_THREADS / ncol;      // row lanes; nrl * ncol <= 256, so nrl * C <= 256 * V floats of `red`
    const int rl = tid / ncol, c0 = tid - rl * ncol;
    const bool active = rl < nrl;
    const long row0 = (long)blockIdx.x * DP_TILE, row1 = row0 + DP_TILE < p.rows ? row0 + DP_TILE : p.rows;
    if (active) {
        for (int cc = c0; cc < ncol; cc += DP_THREADS) {              // more than one trip only when nrl == 1
            const int c = cc * V;
            float acc[V], gv[V];
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = 0.f, gv[j] = 1.f;
            if (GAMMA) ld<float, V>(p.gamma + c, gv);
            for (long r = row0 + rl; r < row1; r += nrl) {
                const float s = p.scale[dp_group(p, r)];
                float gy[V];
                if (s != 0.f) {
                    ld<TX, V>((const TX*)p.a + r * p.lda + c, gy);
#pragma unroll
                    for (int j = 0; j < V; ++j) gy[j] = gy[j] * s;
                    if (GG) {
                        float yv[V];
                        ld<TY, V>((const TY*)p.y + r * p.ldy + c, yv);
#pragma unroll
                        for (int j = 0; j < V; ++j) acc[j] = acc[j] + gy[j] * yv[j];
                    }
                    if (GAMMA) {
#pragma unroll
                        for (int j = 0; j < V; ++j) gy[j] = gy[j] * gv[j];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < V; ++j) gy[j] = 0.f;
                }
                if (p.b) st<TY, V>((TY*)p.b + r * p.ldb + c, gy);
            }
            if (GG) {
                float* dst = nrl == 1 ? p.part + (long)blockIdx.x * C + c : red + rl * C + c;
#pragma unroll
                for (int j = 0; j < V; ++j) dst[j] = acc[j];
            }
        }
    }
    if (GG && nrl > 1) {                                              // block-uniform
        __syncthreads();
        if (rl == 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int c = c0 * V + j;
                float a = red[c];
                for (int q = 1; q < nrl; ++q) a = a + red[q * C + c];
                p.part[(long)blockIdx.x * C + c] = a;
            }
        }
    }
}

// grad_gamma[c]: the workgroups' partials in a fixed order. A workgroup owns DP_FIN_COLS channels; slice s of DP_FIN_SLICES adds the partials of
// workgroups s, s + 16, ... in ascending order (four loads in flight), then the slices are added in ascending order
constexpr int DP_FIN_COLS = 16, DP_FIN_SLICES = 16;
__global__ __launch_bounds__(DP_FIN_COLS * DP_FIN_SLICES) void dp_finish_kernel(const float* part, float* gg, long nwg, int C) {
    __shared__ float red[DP_FIN_SLICES][DP_FIN_COLS + 1];
    const int cl = threadIdx.x % DP_FIN_COLS, s = threadIdx.x / DP_FIN_COLS, c = blockIdx.x * DP_FIN_COLS + cl;
    float a = 0.f;
    if (c < C) {
        const float* col = part + c;
        long g = s;
        for (; g + 3 * DP_FIN_SLICES < nwg; g += 4 * DP_FIN_SLICES) {
            const float v0 = col[g * C], v1 = col[(g + DP_FIN_SLICES) * C], v2 = col[(g + 2 * DP_FIN_SLICES) * C], v3 = col[(g + 3 * DP_FIN_SLICES) * C];
            a = (((a + v0) + v1) + v2) + v3;
        }
        for (; g < nwg; g += DP_FIN_SLICES) a = a + col[g * C];
    }
    red[s][cl] = a;
    __syncthreads();
    if (s == 0 && c < C) {
        float t = red[0][cl];
        for (int q = 1; q < DP_FIN_SLICES; ++q) t = t + red[q][cl];
        gg[c] = t;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ host
size_t esize(int dtype) { return dtype == DT_F32 ? 4 : 2; }
bool aligned(const void* p, size_t a) { return (uintptr_t)p % a == 0; }
long dp_tiles(long rows) { return (rows + DP_TILE - 1) / DP_TILE; }

int pair_of(int dx, int dy) {
    if (dx == dy) return dx == DT_F32 ? 0 : (dx == DT_F16 ? 1 : (dx == DT_BF16 ? 2 : -1));
    if (dx == DT_F32) return dy == DT_F16 ? 3 : (dy == DT_BF16 ? 4 : -1);
    return -1;
}

// what both launch entries answer before they launch; `wide` receives whether the 16-byte form serves
int dp_check(int backward, const void* a, long lda, const void* y, long ldy, const float* gamma, const float* scale, const void* b, long ldb,
             const float* grad_gamma, const float* ws, long ws_floats, long rows, int C, long rpg, int dx, int dy, int* wide) {
    if (pair_of(dx, dy) < 0 || C > DP_MAX_C) return LWDETR_ERR_UNSUPPORTED;
    if (C < 1 || rows < 0 || rpg < 1 || rows % rpg != 0) return LWDETR_ERR_BAD_ARG;
    const size_t ea = esize(dx), ey = esize(dy), eb = backward ? ey : ea;
    const bool need_y = backward ? grad_gamma != nullptr : true;
    if (!a || !scale || (need_y && !y) || lda < C || (y && ldy < C) || (b && ldb < C)) return LWDETR_ERR_BAD_ARG;
    if (!backward && !b) return LWDETR_ERR_BAD_ARG;
    if (backward && ((!b && !grad_gamma) || (grad_gamma && (!gamma || !ws)))) return LWDETR_ERR_BAD_ARG;
    if (!aligned(a, ea) || !aligned(y, ey) || !aligned(b, eb) || !aligned(gamma, 4) || !aligned(scale, 4) || !aligned(grad_gamma, 4) ||
        !aligned(ws, 4))
        return LWDETR_ERR_BAD_ARG;
    if (grad_gamma && ws_floats < dp_tiles(rows) * C) return LWDETR_ERR_BAD_ARG;
    const int V = 16 / (int)(ea < ey ? ea : ey);
    const bool w = C % V == 0 && lda % V == 0 && (!y || ldy % V == 0) && (!b || ldb % V == 0) && aligned(a, 16) && aligned(y, 16) &&
                   aligned(b, 16) && aligned(gamma, 16);
    const long ncol = w ? C / V : C;
    const long blocks = backward ? dp_tiles(rows) : (rows * ncol + DP_THREADS - 1) / DP_THREADS;
    if (rows > 0x7fffffffffffL / C || blocks > 0x7fffffffL) return LWDETR_ERR_BAD_ARG;
    if (wide) *wide = w;
    return LWDETR_OK;
}

template <typename TX, typename TY, int V> void launch_fwd(const DpParams& p, hipStream_t st) {
    const dim3 grid((unsigned)((p.total + DP_THREADS - 1) / DP_THREADS)), block(DP_THREADS);
    if (p.gamma) hipLaunchKernelGGL((dp_fwd_kernel<TX, TY, V, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((dp_fwd_kernel<TX, TY, V, false>), grid, block, 0, st, p);
}

template <typename TX, typename TY, int V> void launch_bwd(const DpParams& p, hipStream_t st) {
    const dim3 grid((unsigned)dp_tiles(p.rows)), block(DP_THREADS);
    if (p.part) hipLaunchKernelGGL((dp_bwd_kernel<TX, TY, V, true, true>), grid, block, 0, st, p);
    else if (p.gamma) hipLaunchKernelGGL((dp_bwd_kernel<TX, TY, V, true, false>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((dp_bwd_kernel<TX, TY, V, false, false>), grid, block, 0, st, p);
}

template <typename TX, typename TY> void launch(const DpParams& p, int backward, int wide, hipStream_t st) {
    constexpr int V = 16 / (int)(sizeof(TX) < sizeof(TY) ? sizeof(TX) : sizeof(TY));
    if (backward) wide ? launch_bwd<TX, TY, V>(p, st) : launch_bwd<TX, TY, 1>(p, st);
    else wide ? launch_fwd<TX, TY, V>(p, st) : launch_fwd<TX, TY, 1>(p, st);
}

void launch_pair(const DpParams& p, int pair, int backward, int wide, hipStream_t st) {
    switch (pair) {
        case 0: launch<float, float>(p, backward, wide, st); break;
        case 1: launch<f16, f16>(p, backward, wide, st); break;
        case 2: launch<bf16, bf16>(p, backward, wide, st); break;
        case 3: launch<float, f16>(p, backward, wide, st); break;
        default: launch<float, bf16>(p, backward, wide, st); break;
    }
}

DpParams dp_params(const void* a, long lda, const void* y, long ldy, const float* gamma, const float* scale, void* b, long ldb, long rows, int C,
                   long rpg, int dx, int dy, int wide) {
    DpParams p = {};
    p.a = a; p.y = y; p.gamma = gamma; p.scale = scale; p.b = b; p.lda = lda; p.ldy = ldy; p.ldb = ldb; p.rows = rows; p.rpg = rpg; p.C = C;
    const int V = wide ? 16 / (int)(esize(dx) < esize(dy) ? esize(dx) : esize(dy)) : 1;
    p.total = rows * (C / V);
    p.small = p.total <= 0x7fffffffL;
    return p;
}

}  // namespace

extern "C" {

int lwdetr_drop_path_check(int backward, const void* a, long lda, const void* y, long ldy, const float* gamma, const float* scale, const void* b,
                           long ldb, const float* grad_gamma, const float* ws, long ws_floats, long rows, int C, long rows_per_group, int dx, int dy) {
    return dp_check(backward != 0, a, lda, y, ldy, gamma, scale, b, ldb, grad_gamma, ws, ws_floats, rows, C, rows_per_group, dx, dy, nullptr);
}

int lwdetr_drop_path_forward(const void* x, long ldx, const void* y, long ldy, const float* gamma, const float* scale, void* out, long ldo,
                             long rows, int C, long rows_per_group, int dx, int dy, void* hip_stream) {
    int wide = 0;
    const int rc = dp_check(0, x, ldx, y, ldy, gamma, scale, out, ldo, nullptr, nullptr, 0, rows, C, rows_per_group, dx, dy, &wide);
    if (rc != LWDETR_OK || rows == 0) return rc;
    const DpParams p = dp_params(x, ldx, y, ldy, gamma, scale, out, ldo, rows, C, rows_per_group, dx, dy, wide);
    const int pair = pair_of(dx, dy);
    launch_pair(p, pair, 0, wide, (hipStream_t)hip_stream);
    return dp_path_done(pair, lwdetr_check_launch());
}

long lwdetr_drop_path_workspace_floats(long rows, int C) {
    if (rows < 1 || C < 1) return 0;
    return dp_tiles(rows) * C;
}

int lwdetr_drop_path_backward(const void* grad_out, long ldg, const void* y, long ldy, const float* gamma, const float* scale, void* grad_y,
                              long ldgy, float* grad_gamma, float* ws, long ws_floats, long rows, int C, long rows_per_group, int dx, int dy,
                              void* hip_stream) {
    int wide = 0;
    const int rc = dp_check(1, grad_out, ldg, y, ldy, gamma, scale, grad_y, ldgy, grad_gamma, ws, ws_floats, rows, C, rows_per_group, dx, dy, &wide);
    if (rc != LWDETR_OK || rows == 0) return rc;
    DpParams p = dp_params(grad_out, ldg, y, ldy, gamma, scale, grad_y, ldgy, rows, C, rows_per_group, dx, dy, wide);
    p.part = grad_gamma ? ws : nullptr;
    const int pair = pair_of(dx, dy);
    hipStream_t st = (hipStream_t)hip_stream;
    launch_pair(p, pair, 1, wide, st);
    if (grad_gamma) {
        const int rc2 = lwdetr_check_launch();
        if (rc2 != LWDETR_OK) return rc2;
        hipLaunchKernelGGL(dp_finish_kernel, dim3((unsigned)((C + DP_FIN_COLS - 1) / DP_FIN_COLS)), dim3(DP_FIN_COLS * DP_FIN_SLICES), 0, st,
                           (const float*)ws, grad_gamma, dp_tiles(rows), C);
    }
    return dp_path_done(DP_PAIRS + pair, lwdetr_check_launch());
}

int lwdetr_drop_path_path_counts(long* out, int n) {
    for (int i = 0; out && i < n && i < DPP_COUNT; ++i) out[i] = g_dp_path[i].load(std::memory_order_relaxed);
    return DPP_COUNT;
}
const char* lwdetr_drop_path_path_name(int i) { return i >= 0 && i < DPP_COUNT ? kDpPathNames[i] : nullptr; }

}  // extern "C"
