// Few-token ViT block kernel at C = 384 (ViT-small backbone: medium, large), 16-bit, fragment-major weights: lwdetr_vit_block_few with C == 384.
//   x1 = x + gamma1 * (att Wp^T + bp);  x <- x1 + gamma2 * fc2(GELU(fc1(LN(x1))));  optional tap copy, row statistics, chained norm1 + QKV of the next block
// in one launch, ONE 16-token tile per workgroup of 8 waves (100 workgroups for a 640 x 640 image).
//
// The C = 192 kernel (mlp_small_kernel, mlp.hip) splits the HIDDEN dimension over the waves and sums eight partial fc2 tiles through LDS. At C = 384 a
// wave's partial output alone would be 96 accumulator registers beside 48 of normalised rows, and a hidden chunk's fragments another 192. Here the
// mapping is the other way round and the hidden activations of the tile go through LDS (16 x 1536 values, 48 KB):
//   projection : wave w produces channel tiles 3 w .. 3 w + 2 of x1 (16 channels each) -> x1s (LDS, rounded to the storage type)
//   LayerNorm  : every wave reads the whole x1 tile back as its B fragments (k-slot order of the accumulators) and normalises it in registers
//   fc1 + GELU : wave w produces hidden tiles 12 w .. 12 w + 11 (16 hidden units each), GELU on the accumulator layout -> hs (LDS, storage type)
//   fc2        : wave w owns channel tiles 3 w .. 3 w + 2 over ALL 48 hidden chunks (B fragments from hs: two 8-byte reads, the k-slot permutation
//                is baked into the chunk-major weight) - no cross-wave reduction; bias, LayerScale, residual, stores; new rows back into x1s
//   chained QKV: every wave normalises the whole tile again and computes feature tiles w, w + 8, ... of the 72.
// Every weight fragment (16 x 32, one contiguous KB) goes straight from L2 into A-operand registers, once per workgroup: 3.54 MB per workgroup, which is
// what the kernel's time is made of. Each phase streams its fragments through two register sets of 12 (48 registers each): set B is requested before
// set A multiplies, so a wave keeps 12 KB of loads in flight - the ~6 KB that cover an L2 round trip at the CU's ingress rate, twice.
// Roundings are those of mlp_kernel<T, 384, ., true, true>: x1, the normalised rows and the GELU output are rounded to T, f32 accumulation, gelu_for<T>.
// fc1 and the QKV sum their 12 k-chunks in order, fc2 its 48 hidden chunks in order in one accumulator.
// 4 barriers. LDS rows are == 4 dwords (mod 64): the 8-byte row accesses of a 32-lane group fall on 32 distinct even banks.
#include "common.h"
#include "vit_block_few384.h"

namespace {

constexpr int NW = 8, NTHR = NW * 64;
constexpr int C = 384, KC = C / 32, NT = C / 16, HID = 4 * C, NCH = HID / 32, X1_LD = C + 8, H_LD = HID + 8;
constexpr int NTW = NT / NW;            // channel tiles per wave (projection, fc2)
constexpr int HTW = HID / 16 / NW;      // hidden tiles per wave (fc1)
constexpr int CB = 4;                   // hidden chunks per fc2 batch: CB * NTW = 12 fragments
constexpr int NTQ = 3 * C / 16, NIT = NTQ / NW;
// Between the steps of a phase (request a set / multiply a set): without it hipcc sinks the 12 loads of a set down between the MFMAs of the other set, each
// just ahead of its use in the NEXT step - counted waits of vmcnt(1), one KB in flight per wave instead of twelve (seen in the fc2 loop).
#define STEP() __builtin_amdgcn_sched_barrier(0)
static_assert(NT % NW == 0 && HTW % 2 == 0 && (NCH / CB) % 2 == 0 && CB * NTW == KC && NTQ % NW == 0, "");
constexpr size_t LDS_BYTES = (size_t)16 * (X1_LD + H_LD) * 2 + (size_t)(HID + 7 * C) * sizeof(float);

template <typename T, bool QKV>
__global__ __launch_bounds__(NTHR, 1) void vit_block_few384_kernel(const VitFew384Params p) {
    typedef typename Vec<T>::v8 V8;
    typedef typename Vec<T>::v4 V4;
    static_assert(sizeof(T) == 2, "");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* x1s = (T*)smem_raw;                                        // [16][X1_LD]: x1, then the block's output rows
    T* hs = x1s + 16 * X1_LD;                                     // [16][H_LD]: GELU(fc1) of the tile
    float* b1s = (float*)(hs + 16 * H_LD);
    float* bps = b1s + HID; float* bqs = bps + 2 * C; float* b2s = bqs + 3 * C;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const long m0 = (long)blockIdx.x * 16;
    const int lfrag = l15 * 32 + g * 8;                           // this lane's 8 values inside a 16 x 32 fragment (512 elements)
    T* __restrict__ X = (T*)p.x;
    const T* __restrict__ W1 = (const T*)p.w1 + lfrag;            // fragment (row tile rt, k-chunk kc) at (rt * KC + kc) * 512
    const T* __restrict__ W2 = (const T*)p.w2p + lfrag;           // chunk-major: fragment (chunk hc, channel tile n) at (hc * NT + n) * 512
    for (int i = tid; i < HID; i += NTHR) b1s[i] = p.b1[i];
    for (int i = tid; i < C; i += NTHR) { bps[i] = p.bp[i]; bps[C + i] = p.gamma1[i]; b2s[i] = p.b2[i]; b2s[C + i] = p.gamma2[i]; }
    if (QKV) for (int i = tid; i < 3 * C; i += NTHR) bqs[i] = p.bqkv[i];
    const long mtok = m0 + l15;                                   // this lane's token row (clamped for loads)
    const bool mok = mtok < p.M;
    const long mrow = mok ? mtok : p.M - 1;
    // the 12 fragments of one row tile (all k-chunks) are 12 consecutive KB
    auto load_rt = [&](V8 (&dst)[KC], const T* w, int rt) {
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) dst[kc] = *(const V8*)(w + (long)(rt * KC + kc) * 512);
    };
    V8 fa[KC], fb[KC];                                            // the two register sets of every phase
    __syncthreads();                                              // biases visible

    // ---- projection: x1 = x + gamma1 * (att Wp^T + bp), wave -> channel tiles NTW wave .. NTW wave + NTW - 1
    {
        const T* __restrict__ ATT = (const T*)p.att;
        const T* __restrict__ WP = (const T*)p.wp + lfrag;
        const int n0 = wave * NTW;
        static_assert(NTW == 3, "the projection is written out for three tiles");
        load_rt(fa, WP, n0);
        load_rt(fb, WP, n0 + 1);
        V8 af[KC];
        V4 xr[NTW];
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) af[kc] = *(const V8*)(ATT + mrow * p.ldatt + kc * 32 + g * 8);
#pragma unroll
        for (int i = 0; i < NTW; ++i) xr[i] = *(const V4*)(X + mrow * p.ldx + (n0 + i) * 16 + g * 4);
        auto proj_tile = [&](const V8 (&f)[KC], int i) {
            const int c0 = (n0 + i) * 16 + g * 4;
            const f32x4 bb = *(const f32x4*)(bps + c0), gg = *(const f32x4*)(bps + C + c0);
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) a = Mma<T>::k32(f[kc], af[kc], a);
            *(V4*)(x1s + l15 * X1_LD + c0) = cvt4<T>(up4<T>(xr[i]) + gg * (a + bb));
        };
        STEP(); proj_tile(fa, 0);
        STEP(); load_rt(fa, WP, n0 + 2);
        STEP(); proj_tile(fb, 1);
        STEP(); load_rt(fb, W1, wave * HTW);                      // fc1's first hidden tile: in flight across the barrier and the LayerNorm
        STEP(); proj_tile(fa, 2);
    }
    __syncthreads();

    // ---- every wave: the whole x1 tile as B fragments (slot h * 4 + e <- channel 32 kc + 16 h + 4 g + e), LayerNorm
    V8 xf[KC];
    auto rows_to_frags = [&](float eps, bool write_stats) {
        float xv[KC][8];
        float sm = 0.f;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const V4 v = *(const V4*)(x1s + l15 * X1_LD + kc * 32 + h * 16 + g * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { xv[kc][h * 4 + e] = to_f32<T>(v[e]); sm += xv[kc][h * 4 + e]; }
            }
        sm += __shfl_xor(sm, 16); sm += __shfl_xor(sm, 32);
        const float mean = sm * (1.f / C);
        float v = 0.f;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc)
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float dl = xv[kc][e] - mean; v += dl * dl; }
        v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
        const float rstd = 1.f / sqrtf(v * (1.f / C) + eps);
        if (write_stats && wave == 0 && mok && g == 0) { p.stats_out[2 * mrow] = mean; p.stats_out[2 * mrow + 1] = rstd; }
#pragma unroll
        for (int kc = 0; kc < KC; ++kc)
#pragma unroll
            for (int e = 0; e < 8; ++e) xf[kc][e] = from_f32<T>((xv[kc][e] - mean) * rstd);
    };
    rows_to_frags(p.eps, false);

    const int n0 = wave * NTW;                                    // fc2: this wave's channel tiles
    auto load_w2 = [&](V8 (&dst)[KC], int hc0) {                  // CB chunks x NTW channel tiles
#pragma unroll
        for (int j = 0; j < CB; ++j)
#pragma unroll
            for (int i = 0; i < NTW; ++i) dst[j * NTW + i] = *(const V8*)(W2 + (long)((hc0 + j) * NT + n0 + i) * 512);
    };

    // ---- fc1 + GELU: hidden tiles HTW wave .. HTW wave + HTW - 1 -> hs
    {
        auto fc1_tile = [&](const V8 (&f)[KC], int ht) {
            f32x4 a = *(const f32x4*)(b1s + ht * 16 + g * 4);
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) a = Mma<T>::k32(f[kc], xf[kc], a);
            V4 hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[e] = from_f32<T>(gelu_for<T>(a[e]));
            *(V4*)(hs + l15 * H_LD + ht * 16 + g * 4) = hv;
        };
        const int ht0 = wave * HTW;
#pragma unroll 1
        for (int it = 0; it + 2 < HTW; it += 2) {                 // tile it is in set B (the projection left the first one there)
            STEP(); load_rt(fa, W1, ht0 + it + 1);
            STEP(); fc1_tile(fb, ht0 + it);
            STEP(); load_rt(fb, W1, ht0 + it + 2);
            STEP(); fc1_tile(fa, ht0 + it + 1);
            STEP();
        }
        STEP(); load_rt(fa, W1, ht0 + HTW - 1);
        STEP(); fc1_tile(fb, ht0 + HTW - 2);
        STEP(); load_w2(fb, 0);                                   // fc2's first batch: in flight across the barrier
        STEP(); fc1_tile(fa, ht0 + HTW - 1);
        STEP();
    }
    __syncthreads();

    // ---- fc2 over all hidden chunks for channel tiles NTW wave ..; epilogue
    {
        f32x4 acc2[NTW];
#pragma unroll
        for (int i = 0; i < NTW; ++i) acc2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto fc2_batch = [&](const V8 (&f)[KC], int hc0) {
#pragma unroll
            for (int j = 0; j < CB; ++j) {
                const T* hrow = hs + l15 * H_LD + (hc0 + j) * 32 + g * 4;
                const V4 lo = *(const V4*)hrow, hi = *(const V4*)(hrow + 16);
                const V8 hf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int i = 0; i < NTW; ++i) acc2[i] = Mma<T>::k32(f[j * NTW + i], hf, acc2[i]);
            }
        };
#pragma unroll 1
        for (int hc0 = 0; hc0 + 2 * CB < NCH; hc0 += 2 * CB) {    // batch hc0 is in set B (fc1 left the first one there)
            STEP(); load_w2(fa, hc0 + CB);
            STEP(); fc2_batch(fb, hc0);
            STEP(); load_w2(fb, hc0 + 2 * CB);
            STEP(); fc2_batch(fa, hc0 + CB);
            STEP();
        }
        STEP(); load_w2(fa, NCH - CB);
        STEP(); fc2_batch(fb, NCH - 2 * CB);
        STEP();
        if constexpr (QKV) load_rt(fb, (const T*)p.wqkv + lfrag, wave);      // the first feature tile: in flight across the epilogue and the barrier
        STEP(); fc2_batch(fa, NCH - CB);
        STEP();
        T* __restrict__ O2 = (T*)p.out2;
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            const int c0 = (n0 + i) * 16 + g * 4;
            const f32x4 b2 = *(const f32x4*)(b2s + c0), g2 = *(const f32x4*)(b2s + C + c0);
            T* xs = x1s + l15 * X1_LD + c0;
            const V4 o = cvt4<T>(up4<T>(*(const V4*)xs) + g2 * (acc2[i] + b2));
            *(V4*)xs = o;
            if (mok) {
                *(V4*)(X + mrow * p.ldx + c0) = o;
                if (O2) *(V4*)(O2 + mrow * p.ld2 + c0) = o;
            }
        }
    }
    if (!(p.stats_out || QKV)) return;
    __syncthreads();

    // ---- statistics of the new rows (every wave, from LDS) and the chained LayerNorm + QKV of the next block
    rows_to_frags(p.eps_next, p.stats_out != nullptr);
    if constexpr (QKV) {
        // Q, K: D[feature][token] -> (B, heads, Tp, hd); V: operands swapped, D[token][feature] -> V^T (B, heads, hd, Tp)
        const T* __restrict__ WQ = (const T*)p.wqkv + lfrag;
        T* __restrict__ Qo = (T*)p.q; T* __restrict__ Ko = (T*)p.k; T* __restrict__ Vo = (T*)p.vt;
        auto qkv_tile = [&](const V8 (&f)[KC], int nt) {
            const int sg = nt / NT, nl0 = (nt - sg * NT) * 16;    // wave-uniform
            if (sg < 2) {
                const int nl = nl0 + g * 4, hh = nl / p.hd, dd = nl - hh * p.hd;
                f32x4 acc = *(const f32x4*)(bqs + sg * C + nl);
#pragma unroll
                for (int kc = 0; kc < KC; ++kc) acc = Mma<T>::k32(f[kc], xf[kc], acc);
                const int mq = (int)m0 + l15, bq_ = mq / p.Tp;
                if (mq < p.M) {
                    T* dst = (sg == 0 ? Qo : Ko) + ((long)bq_ * p.heads * p.Tp + (mq - bq_ * p.Tp)) * p.hd + (long)hh * p.Tp * p.hd + dd;
                    *(V4*)dst = cvt4<T>(acc * (sg == 0 ? p.qscale : 1.f));
                }
            } else {
                const int nl = nl0 + l15, hh = nl / p.hd, dd = nl - hh * p.hd;
                const float bb = bqs[2 * C + nl];
                f32x4 acc = {bb, bb, bb, bb};
#pragma unroll
                for (int kc = 0; kc < KC; ++kc) acc = Mma<T>::k32(xf[kc], f[kc], acc);
                const int mv = (int)m0 + g * 4, bv_ = mv / p.Tp;
                if (mv < p.M)                                      // M, Tp multiples of 4: whole 4-token run
                    *(V4*)(Vo + (long)bv_ * p.heads * p.hd * p.Tp + (mv - bv_ * p.Tp) + ((long)hh * p.hd + dd) * p.Tp) = cvt4<T>(acc);
            }
        };
        static_assert(NIT % 2 == 1, "the loop below ends on set B");
#pragma unroll 1
        for (int it = 0; it + 1 < NIT; it += 2) {                 // feature tiles wave, wave + 8, ...; tile it is in set B (fc2 left the first one there)
            STEP(); load_rt(fa, WQ, wave + (it + 1) * NW);
            STEP(); qkv_tile(fb, wave + it * NW);
            STEP(); load_rt(fb, WQ, wave + (it + 2) * NW);
            STEP(); qkv_tile(fa, wave + (it + 1) * NW);
            STEP();
        }
        qkv_tile(fb, wave + (NIT - 1) * NW);
    }
}

template <typename T, bool QKV>
int launch_few384(const VitFew384Params& p, hipStream_t st) {
    static bool attr_done[16] = {};            // per device (a process may drive several GPUs)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return LWDETR_ERR_LAUNCH;
    if (!attr_done[dev]) {
        if (hipFuncSetAttribute((const void*)vit_block_few384_kernel<T, QKV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES) != hipSuccess)
            return LWDETR_ERR_LAUNCH;
        attr_done[dev] = true;
    }
    const long blocks = (p.M + 15) / 16;
    ProfScope ps(KID_MLP, (16.0 + 2.0 + (QKV ? 6.0 : 0.0)) * p.M * C * C, (double)p.M * C * sizeof(T) * 3 + (QKV ? 3.0 : 0.0) * p.M * C * sizeof(T), st);
    hipLaunchKernelGGL((vit_block_few384_kernel<T, QKV>), dim3((unsigned)blocks), dim3(NTHR), LDS_BYTES, st, p);
    return lwdetr_check_launch();
}

}  // namespace

int lwdetr_vit_block_few384_launch(const VitFew384Params& p, int dtype, hipStream_t st) {
    if (dtype == DT_F16) return p.wqkv ? launch_few384<f16, true>(p, st) : launch_few384<f16, false>(p, st);
    if (dtype == DT_BF16) return p.wqkv ? launch_few384<bf16, true>(p, st) : launch_few384<bf16, false>(p, st);
    return LWDETR_ERR_UNSUPPORTED;
}
