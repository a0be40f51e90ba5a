// The body of enc_chain_kernel / enc_chain_kernel_wide (chain.hip), included once per kernel between its braces: the same text, compiled with
//   ENC_CHAIN_NCT         class tiles of 32 columns: 3 (ncls <= 96) or 12 (ncls <= 384)
//   ENC_CHAIN_CLS_UNROLL  the unroll pragma of the class loop: unrolled for 3 tiles, rolled for 12 (unrolled 12 times the bf16 D = 384 form was reported to spill)
// Text inclusion and not a template parameter or a shared __device__ function: the narrow kernels must keep their symbols AND their code,
// instruction for instruction (tools/kernel_identity.py). A template parameter is part of the symbol; the body as a __forceinline__ function with
// the tile count as its parameter (tried) left none of the six narrow kernels identical, a few instructions each.
    typedef typename Vec<T>::v8 V8;
    constexpr int KS = D / 16, NTI = D / 32, PPT = D / 64;
    constexpr int KSI = PF ? K5 / 16 : KS, PPT5 = K5 / 64;
    constexpr int NSLOT = 32;
    constexpr int NCT = ENC_CHAIN_NCT;              // class tiles (ncls <= 32 NCT)
    constexpr int VEC_F = (PF ? 3 * D : 0) + 3 * D + 32 * NCT + 6 * D;
    constexpr int VEC_B = (VEC_F * 4 + 4095) / 4096 * 4096, VEC_DPW = VEC_B / 4096;
    constexpr bool TWO_CHAINS = D == 256 && !PF;    // second accumulator chain per tile where the registers allow it (hipcc spills otherwise)
    static_assert(KS % CH_RD == 0 && KSI % CH_RD == 0, "the fragment read-ahead ring must divide every tile");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const float* vec = (const float*)(smem + NSLOT * CH_PIECE_B);
    const float* b2s = vec; const float* gps = vec + D; const float* bps = vec + 2 * D;
    const float* bes = vec + (PF ? 3 * D : 0); const float* ges = bes + D; const float* bts = ges + D;
    const float* bcs = bts + D; const float* bvs = bcs + 32 * NCT;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const unsigned lane16 = lane * 16;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)smem;

    const long t0 = ((long)blockIdx.x * 4 + wave) * 32;
    const long mrow = t0 + j;
    const bool live = mrow < p.M;
    CH_TS(0);
    // memory-space row of this lane's token
    const long img = live ? mrow / p.npix : 0;
    const long mm = live ? img * p.S + p.lsi + (mrow - img * p.npix) : 0;

    // ---- input rows first (they are older than every weight DMA: nothing queues behind the ring fill), then vectors + ring
    const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, (int)p.in_bytes, 0x00020000);
    const unsigned in_off = live ? (unsigned)(mrow * p.ld_in * 2) : 0x80000000u;
    V8 xin[KSI];
#pragma unroll
    for (int t = 0; t < KSI; ++t)
        xin[t] = __builtin_bit_cast(V8, __builtin_amdgcn_raw_buffer_load_b128(r_in, in_off + (unsigned)((16 * t + 8 * h) * 2), 0, 0));
    const unsigned char rv = live ? p.rowvalid[mm] : 0, npd = live ? p.notpad[mm] : 0;

    WRing<NSLOT> ring;
    ring.src = (const char*)p.wstream; ring.lds0 = lds0; ring.np = p.np; ring.issued = 0; ring.wave = wave; ring.lane16 = lane16;
    {
        const char* vsrc = (const char*)p.vec;
#pragma unroll
        for (int i = 0; i < VEC_DPW; ++i) {
            const unsigned kb = (unsigned)(wave * VEC_DPW + i) * 1024u;
            ring.dma1k(vsrc, kb + lane16, lds0 + NSLOT * CH_PIECE_B + kb);
        }
        // only the pieces of the first tile (+ read-ahead + a few) now: the first begin_tile tops the ring up. The compiler waits for
        // the input rows with a vmcnt that does not know of the DMAs: every DMA issued before that wait would have to land first.
        ring.fill(2 * (PF ? PPT5 : PPT) + 2);            // (begin_tile_x: the first tile fetches the wait count of the second)
    }
    // an explicit vmcnt(0) the compiler can see (a real S_WAITCNT, not inline assembly): hipcc's own waits for the input rows and flags
    // are satisfied HERE, before the ring fill of the first begin_tile, and it adds none behind it
    __builtin_amdgcn_s_waitcnt(0x0F70);
    ring.seq_init(lds0 + NSLOT * CH_PIECE_B + VEC_B + (unsigned)wave * NSLOT * 4);
    CH_TS(1);
    auto frag = [&](int g) -> V8 {           // global fragment index g = 4 * piece + fragment
        return *(const V8*)(smem + (((unsigned)g & (NSLOT * 4 - 1)) << 10) + lane16);
    };
    auto bias16 = [&](const float* src) -> f32x16 {      // src[8 b + 4 h + e] -> register 4 b + e
        f32x16 r;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const f32x4 v = *(const f32x4*)(src + 8 * b + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) r[4 * b + e] = v[e];
        }
        return r;
    };
    const __amdgpu_buffer_rsrc_t r_mem = __builtin_amdgcn_make_buffer_rsrc(p.memory ? p.memory : p.om, 0, p.memory ? (int)p.mem_bytes : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_om = __builtin_amdgcn_make_buffer_rsrc(p.om, 0, (int)p.mem_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_cls = __builtin_amdgcn_make_buffer_rsrc(p.cls, 0, (int)p.cls_bytes, 0x00020000);
    const unsigned row_off = live ? (unsigned)(mm * D * 2) : 0x80000000u;           // byte offset of the row in (B * S, D) tensors
    const unsigned cls_off = live ? (unsigned)(mm * p.ld_cls * 2) : 0x80000000u;

    int pc = 0;                                  // next piece
    V8 fr[CH_RD];
#ifdef LWDETR_CH_TIMING
    unsigned long long tt_mfma = 0, tt_epi = 0;
#endif
    // 32 channels x 32 rows: nf fragments against x[0 .. nf), fragment stream position 4 * pc
    auto tile = [&](auto& x, auto nf_tag, f32x16 acc) -> f32x16 {
        constexpr int nf = decltype(nf_tag)::value;
        const int g0 = 4 * pc;
        // two independent accumulator chains (even / odd k-steps): a 32x32x16 MFMA that accumulates into the result of the one right
        // in front of it waits for that result
        f32x16 acc2 = {};
#pragma unroll
        for (int f = 0; f < nf; ++f) {
            const V8 a = fr[f % CH_RD];
            fr[f % CH_RD] = frag(g0 + f + CH_RD);
            if (TWO_CHAINS && (f & 1)) acc2 = Mma32c<T>::k16(a, x[f], acc2);
            else acc = Mma32c<T>::k16(a, x[f], acc);
            // pin the order: hipcc otherwise sinks every fragment read to just in front of its MFMA (each MFMA then waits a whole LDS
            // round trip: 114 - 139 cycles per MFMA slot measured, profiles/r4c_enc_chain_phase_timing.txt)
            __builtin_amdgcn_sched_barrier(0);
        }
        pc += nf / 4;
        if (TWO_CHAINS) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] += acc2[e];
        }
        return acc;
    };
    // rows rounded to T held as packed pairs (dword d of tile n = registers 2 d, 2 d + 1): LayerNorm with affine, stores the
    // result to `rs` rows (16-byte pieces) and leaves it as B operands in xo (k-slot order of an accumulator hand-over)
    auto layernorm_store = [&](unsigned (&xp)[NTI][8], float s, const float* gam, const float* bet, float eps,
                               const __amdgpu_buffer_rsrc_t& rs, V8 (&xo)[KS]) {
        s += __shfl_xor(s, 32);
        const float mean = s * (1.f / D);
        float v = 0.f;
#pragma unroll
        for (int n = 0; n < NTI; ++n)
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                float v0, v1; cunpack2<T>(xp[n][d], v0, v1);
                v0 -= mean; v1 -= mean;
                v = fmaf(v0, v0, v); v = fmaf(v1, v1, v);
            }
        v += __shfl_xor(v, 32);
        const float rstd = 1.f / sqrtf(v * (1.f / D) + eps);
#pragma unroll
        for (int n = 0; n < NTI; ++n) {
            unsigned w[8];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int c0 = 32 * n + 8 * b + 4 * h;
                const f32x4 g = *(const f32x4*)(gam + c0), be = *(const f32x4*)(bet + c0);
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    float v0, v1; cunpack2<T>(xp[n][2 * b + d], v0, v1);
                    w[2 * b + d] = cpack2<T>(fmaf((v0 - mean) * rstd, g[2 * d], be[2 * d]), fmaf((v1 - mean) * rstd, g[2 * d + 1], be[2 * d + 1]));
                }
            }
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
                const cu32x4 ow = crows8(w[4 * jb], w[4 * jb + 1], w[4 * jb + 2], w[4 * jb + 3]);
                __builtin_amdgcn_raw_buffer_store_b128(ow, rs, row_off + (unsigned)((32 * n + 16 * jb + 8 * h) * 2), 0, 0);
            }
            xo[2 * n] = __builtin_bit_cast(V8, cu32x4{w[0], w[1], w[2], w[3]});
            xo[2 * n + 1] = __builtin_bit_cast(V8, cu32x4{w[4], w[5], w[6], w[7]});
        }
        ring.stores(2 * NTI);
    };

    V8 xf[KS];                                   // `memory` rows as B operands
    // first tile: its pieces (and the two read ahead) have landed; the read-ahead ring starts
    ring.begin_tile_x(0, PF ? PPT5 : PPT, PF ? PPT5 : PPT);
#pragma unroll
    for (int i = 0; i < CH_RD; ++i) fr[i] = frag(i);
    CH_TS(2);
    if constexpr (PF) {
        // ---- projector: C2f.cv2 (1x1 conv, BatchNorm folded) + SiLU, LayerNorm over channels -> memory (projector.py:117-132)
        unsigned xp[NTI][8];
        float s = 0.f;
#pragma unroll
        for (int n = 0; n < NTI; ++n) {
            if (n > 0) ring.begin_tile_x(pc, PPT5, n + 1 < NTI ? PPT5 : PPT);
            const f32x16 acc = tile(xin, std::integral_constant<int, KSI>{}, bias16(b2s + 32 * n));
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const float a0 = acc[2 * d], a1 = acc[2 * d + 1];
                const unsigned w = cpack2<T>(a0 / (1.f + __expf(-a0)), a1 / (1.f + __expf(-a1)));
                xp[n][d] = w;
                float v0, v1; cunpack2<T>(w, v0, v1);
                s += v0 + v1;
            }
        }
        layernorm_store(xp, s, gps, bps, p.eps_p, r_mem, xf);
    } else {
#pragma unroll
        for (int t = 0; t < KS; ++t) xf[t] = xin[t];
    }
    CH_TS(3);
    // ---- value projections of all decoder layers (ms_deform_attn.py:110-114: masked_fill of the OUTPUT rows of padded pixels)
    {
        const int nvt = p.nl * NTI;
#pragma unroll 1
        for (int vt = 0; vt < nvt; ++vt) {
            if (PF || vt > 0) ring.begin_tile_x(pc, PPT, PPT);
#ifdef LWDETR_CH_TIMING
            const unsigned long long tv0 = __builtin_amdgcn_s_memrealtime();
#endif
            f32x16 acc = tile(xf, std::integral_constant<int, KS>{}, bias16(bvs + 32 * vt));
#ifdef LWDETR_CH_TIMING
            asm volatile("" : "+v"(acc));
            const unsigned long long tv1 = __builtin_amdgcn_s_memrealtime();
#endif
            const int li = vt / NTI, n = vt - li * NTI;
            const __amdgpu_buffer_rsrc_t r_v = __builtin_amdgcn_make_buffer_rsrc(p.values[li], 0, (int)p.mem_bytes, 0x00020000);
            if (!npd) {
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            }
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
                const cu32x4 ow = crows8(cpack2<T>(acc[8 * jb], acc[8 * jb + 1]), cpack2<T>(acc[8 * jb + 2], acc[8 * jb + 3]),
                                         cpack2<T>(acc[8 * jb + 4], acc[8 * jb + 5]), cpack2<T>(acc[8 * jb + 6], acc[8 * jb + 7]));
                __builtin_amdgcn_raw_buffer_store_b128(ow, r_v, row_off + (unsigned)((32 * n + 16 * jb + 8 * h) * 2), 0, 0);
            }
            ring.stores(2);
#ifdef LWDETR_CH_TIMING
            tt_mfma += tv1 - tv0; tt_epi += __builtin_amdgcn_s_memrealtime() - tv1;
#endif
        }
    }
    CH_TS(4);
    // ---- enc_output Linear on the rows (invalid proposals: the INPUT row is zeroed, transformer.py:113-116) + LayerNorm -> output_memory
    {
        if (!rv) {
#pragma unroll
            for (int t = 0; t < KS; ++t) xf[t] = V8{};
        }
        unsigned xp[NTI][8];
        float s = 0.f;
#pragma unroll
        for (int n = 0; n < NTI; ++n) {
            ring.begin_tile_x(pc, PPT, PPT);
            const f32x16 acc = tile(xf, std::integral_constant<int, KS>{}, bias16(bes + 32 * n));
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const unsigned w = cpack2<T>(acc[2 * d], acc[2 * d + 1]);
                xp[n][d] = w;
                float v0, v1; cunpack2<T>(w, v0, v1);
                s += v0 + v1;
            }
        }
        layernorm_store(xp, s, ges, bts, p.eps_e, r_om, xf);
    }
    CH_TS(5);
    // ---- class logits of every token and their maximum (the two-stage selection score, transformer.py:244-246)
    {
        float mx = -INFINITY;
        ENC_CHAIN_CLS_UNROLL
        for (int n = 0; n < NCT; ++n) {
            ring.begin_tile_x(pc, PPT, PPT);
            const f32x16 acc = tile(xf, std::integral_constant<int, KS>{}, bias16(bcs + 32 * n));
            unsigned w[8];
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                w[d] = cpack2<T>(acc[2 * d], acc[2 * d + 1]);
                float v0, v1; cunpack2<T>(w[d], v0, v1);
                const int c = 32 * n + 8 * (d >> 1) + 4 * h + 2 * (d & 1);
                if (c < p.ncls) mx = fmaxf(mx, v0);
                if (c + 1 < p.ncls) mx = fmaxf(mx, v1);
            }
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
                const cu32x4 ow = crows8(w[4 * jb], w[4 * jb + 1], w[4 * jb + 2], w[4 * jb + 3]);
                __builtin_amdgcn_raw_buffer_store_b128(ow, r_cls, cls_off + (unsigned)((32 * n + 16 * jb + 8 * h) * 2), 0, 0);
            }
            ring.stores(2);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        if (live && h == 0) p.cls_max[mm] = mx;
    }
    CH_TS(6);
#ifdef LWDETR_CH_TIMING
    if ((blockIdx.x == 0 || blockIdx.x == gridDim.x - 1) && lane == 0) { g_ch_timing[blockIdx.x != 0][wave][13] = ring.tt_wait; g_ch_timing[blockIdx.x != 0][wave][14] = ring.tt_bar;
        g_ch_timing[blockIdx.x != 0][wave][11] = tt_mfma; g_ch_timing[blockIdx.x != 0][wave][12] = tt_epi; }
#endif
