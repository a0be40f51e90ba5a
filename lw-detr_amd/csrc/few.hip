// Few-row GEMM / 3x3 convolution for the single-image latency path (round 6):  out = epilogue( A_view(M,K) x W(N,K)^T ),  M <= a few thousand rows.
//
// Replaces lwdetr_gemm's 64 x 64 DMA-ring kernel on the launches of one or two images whose contraction is long - first of all the six 3x3
// convolutions of the projector's C2f block (models/backbone/projector.py:101-132; M = 1600 pixels, N = 128, K = 9 x 128 = 1152): on 64 x 64 tiles
// that is 50 workgroups, each walking 36 dependent DMA -> barrier -> fragment -> MFMA steps - 19.3 us per launch where the matrix work is < 1 us
// (profiles/r5e_*: neither ring depth nor stage depth nor split-K moved it).
//
// Here nothing goes through LDS and nothing waits for a barrier: a workgroup owns 16 rows x 128 columns, its 8 waves one 16 x 16 output tile each, and a
// wave loads the MFMA fragments of a WHOLE third of the contraction (NB = 12-18 k-chunks of 32) straight from L2 into registers before it multiplies
// them - the contraction is three L2 round trips deep instead of 36 ring steps. What makes that load path fast is the weight layout (the lesson of
// lwdetr_vit_block_few, profiles/r6b_*): W arrives FRAGMENT-MAJOR - [N / 16][K / 32][16][32], lwdetr_amd.kernels.pack_frag16 - so a wave's weight load is
// one contiguous KB; the activation fragment (16 rows x 64 bytes) is the same for the 8 waves of the workgroup and comes out of L1 for seven of them.
// 100 workgroups at one 640 x 640 image (1600 / 16), 800 waves: every CU has work.
// Arithmetic: 16x16x32 MFMAs in k order, f32 accumulation, the epilogue's operation order is lwdetr_gemm's (bias, activation, scale * gamma, residual).
//
// float32 form (behind LWDETR_GEMM_FEW_F32=1 in the launch plan): the same kernel on f32 fragments. Lane (l15, g) still holds the 8 consecutive values
// k = 32 c + 8 g + s of its row for both operands - two 16-byte loads, a weight fragment is one contiguous 2 KB - and Mma<float>::k32 contracts them
// as eight exact-f32 16x16x4 MFMAs (slice s sums over { 32 c + 8 g' + s }: one permutation of k shared by both operands). A chunk costs 16 VGPRs, so a
// batch is FEW_F32_NB chunks (CONV: a divisor of Cin / 32, i.e. a tap of the kernel or a part of one) instead of a kernel row, and because an f32
// chunk is 8 dependent MFMAs (~300 clocks) the next batch is loaded while the current one is multiplied (two register sets). The batch sizes that
// were measured, with their register counts: profiles/r7a_few_row_gemm_f32.txt.
#include "common.h"

namespace {

__device__ __attribute__((aligned(32))) unsigned int g_few_zero[8];      // source of the fragments of out-of-image taps (8 values: 32 bytes in f32)

// a lane's 8 consecutive values of one fragment. f32: two 16-byte loads - the entry checks 16-byte alignment of A / W / lda, not 32
template <typename T> __device__ __forceinline__ typename Vec<T>::v8 few_load8(const T* p) { return *(const typename Vec<T>::v8*)p; }
template <> __device__ __forceinline__ f32x8 few_load8<float>(const float* p) {
    const f32x4 lo = *(const f32x4*)p, hi = *(const f32x4*)(p + 4);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// chunks per batch of the f32 form (tuning builds: -DFEW_F32_NB_PLAIN=.. etc. through the Makefile's TUNE) and whether two batches are in flight
#ifndef FEW_F32_NB_PLAIN
#define FEW_F32_NB_PLAIN 4
#endif
#ifndef FEW_F32_NB_KCH4
#define FEW_F32_NB_KCH4 4
#endif
#ifndef FEW_F32_NB_KCH6
#define FEW_F32_NB_KCH6 3
#endif
#ifndef FEW_F32_DB
#define FEW_F32_DB 1
#endif

// KCH = Cin / 32 of a 3x3 convolution; NB = chunks per batch: 3 KCH (the chunks of one kernel row; the 16-bit form) or a divisor of KCH (a tap or a
// part of one; the f32 form); PLAIN: KCH = 4. DB: the next batch is loaded before the current one is multiplied
template <typename T, int AMODE, int KCH, int NB, bool DB>
__global__ __launch_bounds__(512) void gemm_few_kernel(const lwdetr_gemm_desc d) {
    static_assert(AMODE != LWDETR_A_CONV3x3 || NB == 3 * KCH || KCH % NB == 0, "CONV: a batch is one kernel row or a divisor of one tap");
    typedef typename Vec<T>::v8 V8;
    typedef typename Vec<T>::v4 V4;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g = lane >> 4;
    const int n_tile = (int)blockIdx.y * (int)(blockDim.x >> 6) + wave;   // this wave's 16 output columns (blockDim = 64 x waves per workgroup)
    if (n_tile * 16 >= d.N) return;                                 // wave-uniform; no barrier anywhere below
    const long m = (long)blockIdx.x * 16 + l15;
    const bool m_ok = m < d.M;
    const long mc = m_ok ? m : d.M - 1;                             // clamped for addressing
    const T* __restrict__ A = (const T*)d.A;
    const T* __restrict__ Wf = (const T*)d.W;
    const T* zero = (const T*)g_few_zero;
    const int nchunks = d.K / 32;
    // row part of the activation address: PLAIN the row itself; CONV3x3 (raster rows, zero padding) the output pixel's image and coordinates
    int pb = 0, py = 0, px = 0;
    if (AMODE == LWDETR_A_CONV3x3) {
        const int hw = d.conv_hout * d.conv_wout;
        pb = (int)(mc / hw);
        const int r = (int)(mc - (long)pb * hw);
        py = r / d.conv_wout; px = r - py * d.conv_wout;
    }
    const T* arow = A + mc * d.lda + g * 8;                          // PLAIN
    const T* wbase = Wf + ((long)n_tile * nchunks * 16 + l15) * 32 + g * 8;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // one batch: its NB activation and weight fragments into registers (FEW_LOAD), then its MFMAs in chunk order (FEW_MMA)
#define FEW_LOAD(c0, xa, wa)                                                                                                             \
    _Pragma("unroll") for (int i = 0; i < NB; ++i) {                                                                                     \
        const int c = (c0) + i < nchunks ? (c0) + i : nchunks - 1;  /* past the end: a harmless reload, not multiplied */                \
        const T* src;                                                                                                                    \
        if (AMODE == LWDETR_A_CONV3x3) {                                                                                                 \
            int ky, kx, cc;                                         /* 9 KCH chunks in all, NB divides them: never past the end */       \
            if (NB == 3 * KCH) { ky = (c0) / NB; kx = i / KCH; cc = i % KCH; }           /* batch = kernel row ky */                      \
            else { const int tap = (c0) / KCH; ky = tap / 3; kx = tap - 3 * ky; cc = (c0) - tap * KCH + i; }  /* inside tap (ky, kx) */   \
            const int iy = py * d.conv_stride + ky - 1, ix = px * d.conv_stride + kx - 1;                                                \
            const bool ok = iy >= 0 && iy < d.a_tok.Hp && ix >= 0 && ix < d.a_tok.Wp;                                                    \
            src = ok ? A + (((long)pb * d.a_tok.Hp + iy) * d.a_tok.Wp + ix) * d.lda + d.a_col0 + cc * 32 + g * 8 : zero;                 \
        } else src = arow + c * 32;                                                                                                      \
        xa[i] = few_load8<T>(src);                                                                                                       \
        wa[i] = few_load8<T>(wbase + (long)c * 512);                                                                                     \
    }
#define FEW_MMA(c0, xa, wa)                                                                                                              \
    _Pragma("unroll") for (int i = 0; i < NB; ++i)                                                                                       \
        if ((c0) + i < nchunks) acc = Mma<T>::k32(wa[i], xa[i], acc);     /* D[n][row]: lane (row l15, g) holds columns 4 g .. 4 g + 3 */
    if (!DB) {
        for (int c0 = 0; c0 < nchunks; c0 += NB) {                  // wave-uniform trip count
            V8 xa[NB], wa[NB];
            FEW_LOAD(c0, xa, wa)
            FEW_MMA(c0, xa, wa)
        }
    } else {
        V8 xa0[NB], wa0[NB], xa1[NB], wa1[NB];                      // every branch below is wave-uniform; the chunk order of the sum is unchanged
        FEW_LOAD(0, xa0, wa0)
        for (int c0 = 0; c0 < nchunks; c0 += 2 * NB) {
            if (c0 + NB < nchunks) { FEW_LOAD(c0 + NB, xa1, wa1) }
            FEW_MMA(c0, xa0, wa0)
            if (c0 + 2 * NB < nchunks) { FEW_LOAD(c0 + 2 * NB, xa0, wa0) }
            if (c0 + NB < nchunks) { FEW_MMA(c0 + NB, xa1, wa1) }
        }
    }
#undef FEW_LOAD
#undef FEW_MMA
    // ---- epilogue: one LINEAR segment
    const lwdetr_gemm_seg& sg = d.seg[0];
    const int n = n_tile * 16 + g * 4;
    f32x4 x = acc;
    if (sg.bias) x += *(const f32x4*)(sg.bias + n);
    const int act = sg.act;
    if (act != ACT_NONE) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            x[e] = act == ACT_GELU ? gelu_for<T>(x[e]) : (act == ACT_SILU ? x[e] * __builtin_amdgcn_rcpf(1.f + __expf(-x[e])) : (x[e] > 0.f ? x[e] : 0.f));
    }
    x = x * sg.scale;
    if (sg.gamma) x = x * *(const f32x4*)(sg.gamma + n);
    if (!m_ok) return;
    if (sg.res) x += up4<T>(*(const V4*)((const T*)sg.res + m * sg.ldres + n));
    const V4 o = cvt4<T>(x);
    *(V4*)((T*)sg.out + m * sg.ldo + n) = o;
    if (sg.out2) *(V4*)((T*)sg.out2 + m * sg.ld2 + n) = o;
}

// batch sizes per dtype: 16-bit a kernel row (PLAIN: 12 chunks), one register set; f32 see FEW_F32_*
template <typename T> struct FewBatch { static constexpr int plain = 12, kch4 = 12, kch6 = 18; static constexpr bool db = false; };
template <> struct FewBatch<float> {
    static constexpr int plain = FEW_F32_NB_PLAIN, kch4 = FEW_F32_NB_KCH4, kch6 = FEW_F32_NB_KCH6;
    static constexpr bool db = FEW_F32_DB != 0;
};

template <typename T>
int few_launch(const lwdetr_gemm_desc& d, hipStream_t st) {
    // waves per workgroup = 16-column tiles that share a row tile's activation fragments through L1. The launch is a stream of weights through each
    // CU's load path (a 16-row tile pulls ALL of its columns' weights: 295 KB for the projector's 3x3 convolutions): fewer waves per workgroup spread
    // the same waves over more CUs (LWDETR_GEMM_FEW_WAVES, tuning; measured in profiles/r6c_*)
    int nwv = (int)lwdetr_knob(KNOB_GEMM_FEW_WAVES, 2);
    if (nwv != 1 && nwv != 2 && nwv != 4 && nwv != 8) nwv = 2;
    const int ntile = d.N / 16;
    const dim3 grid((unsigned)((d.M + 15) / 16), (unsigned)((ntile + nwv - 1) / nwv));
    const dim3 block((unsigned)(64 * nwv));
    const int kid = d.a_mode == LWDETR_A_CONV3x3 ? KID_GEMM_CONV : KID_GEMM;
    ProfScope ps(kid, 2.0 * d.M * d.N * d.K, ((double)d.M * d.K + (double)d.N * d.K + (double)d.M * d.N) * sizeof(T), st);
    int path = GP_FEW_PLAIN;
    if (d.a_mode == LWDETR_A_CONV3x3) {
        // 16-bit: a batch = the three taps of one kernel row (3 x Cin / 32 chunks): Cin = 128 -> 12, Cin = 192 -> 18
        typedef FewBatch<T> FB;
        if (d.conv_cin == 192) { hipLaunchKernelGGL((gemm_few_kernel<T, LWDETR_A_CONV3x3, 6, FB::kch6, FB::db>), grid, block, 0, st, d); path = GP_FEW_CONV_KCH6; }
        else { hipLaunchKernelGGL((gemm_few_kernel<T, LWDETR_A_CONV3x3, 4, FB::kch4, FB::db>), grid, block, 0, st, d); path = GP_FEW_CONV_KCH4; }
    } else hipLaunchKernelGGL((gemm_few_kernel<T, LWDETR_A_PLAIN, 4, FewBatch<T>::plain, FewBatch<T>::db>), grid, block, 0, st, d);
    return lwdetr_gemm_path_done(path, lwdetr_check_launch());
}

}  // namespace

extern "C" int lwdetr_gemm_few(const lwdetr_gemm_desc* desc, int dtype, void* hip_stream) {
    if (!desc) return LWDETR_ERR_BAD_ARG;
    const lwdetr_gemm_desc& d = *desc;
    if (d.M < 0 || d.N <= 0 || d.K <= 0 || !d.A || !d.W || d.nseg != 1 || !d.seg[0].out || d.seg[0].n_begin != 0) return LWDETR_ERR_BAD_ARG;
    if (d.M == 0) return LWDETR_OK;
    const lwdetr_gemm_seg& g = d.seg[0];
    if (g.act < LWDETR_ACT_NONE || g.act > LWDETR_ACT_SILU) return LWDETR_ERR_BAD_ARG;
    // what the kernel reads and writes in wide pieces: bias / gamma 16-byte loads, residual / second destination / out runs of 4 values (8 bytes in
    // 16-bit, 16 in f32), A / W fragments 16-byte loads (8 values of 16 bits: lda % 8; 4 + 4 values of f32: lda % 4);
    // columns [N, n_end) would never be written (lwdetr_gemm serves those descriptors)
    const size_t oal = dtype == DT_F32 ? 15 : 7;
    const int a_run = dtype == DT_F32 ? 4 : 8;
    if (g.n_end != d.N || ((size_t)g.bias & 15) != 0 || ((size_t)g.gamma & 15) != 0 || ((size_t)g.res & oal) != 0 || ((size_t)g.out2 & oal) != 0)
        return LWDETR_ERR_UNSUPPORTED;
    if ((dtype != DT_F32 && dtype != DT_F16 && dtype != DT_BF16) || d.A2 || d.M > 8192 || d.K % 32 != 0 || d.N % 16 != 0 || g.mode != LWDETR_OUT_LINEAR || g.rowmask || g.ln_stats ||
        g.res_mod > 0 || g.n_end < d.N || g.ldo % 4 != 0 || (g.res && g.ldres % 4 != 0) || (g.out2 && g.ld2 % 4 != 0) || d.lda % a_run != 0 ||
        ((size_t)d.A & 15) != 0 || ((size_t)d.W & 15) != 0 || ((size_t)g.out & oal) != 0)
        return LWDETR_ERR_UNSUPPORTED;
    if (d.a_mode == LWDETR_A_CONV3x3) {
        if (d.a_tok.winmajor || d.conv_cin % 32 != 0 || d.K != 9 * d.conv_cin || d.a_col0 % 8 != 0 || d.conv_hout <= 0 || d.conv_wout <= 0 ||
            (d.conv_stride != 1 && d.conv_stride != 2) || (d.conv_cin != 128 && d.conv_cin != 192))
            return LWDETR_ERR_UNSUPPORTED;
    } else if (d.a_mode != LWDETR_A_PLAIN) return LWDETR_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)hip_stream;
    return dtype == DT_F32 ? few_launch<float>(d, st) : (dtype == DT_F16 ? few_launch<f16>(d, st) : few_launch<bf16>(d, st));
}
