/* lwdetr_hip.h - C ABI of liblwdetr_hip.so (hand-written gfx950 kernels for the LW-DETR forward path).
 *
 * Conventions for every entry point:
 *   - all tensor pointers are DEVICE pointers, borrowed for the duration of the call (no ownership transfer);
 *   - outputs are caller-allocated and fully overwritten; nothing is allocated, nothing synchronises the host;
 *   - work is enqueued on `hip_stream` (a hipStream_t passed as void*, NULL = default stream); stateless and
 *     re-entrant per stream;
 *   - return value: 0 on success, negative LWDETR_ERR_* otherwise (launch failures are reported from
 *     hipGetLastError(), never just printed - the reference only printf's them, ms_deform_im2col_cuda.cuh:948-952);
 *   - dtype codes: 0 = float32, 1 = float16, 2 = bfloat16 (3 = float64, deformable-attention op only).
 *
 * Reference interfaces replaced (paths relative to /root/reference):
 *   lwdetr_msda_forward        models/ops/src/ms_deform_attn.h:19-35 (ms_deform_attn_forward, pybind
 *                              models/ops/src/vision.cpp:13-16) -> cuda/ms_deform_attn_cuda.cu:20-80 ->
 *                              cuda/ms_deform_im2col_cuda.cuh:237-299
 *   lwdetr_msda_backward       models/ops/src/ms_deform_attn.h:37-60 (ms_deform_attn_backward) ->
 *                              cuda/ms_deform_attn_cuda.cu:83-153 -> cuda/ms_deform_im2col_cuda.cuh:87-160, :846-920
 *   lwdetr_msda_fused_forward  models/ops/modules/ms_deform_attn.py:117-142 (softmax, location arithmetic, op call)
 *   lwdetr_gemm                torch.nn.functional.linear / conv2d / conv_transpose2d call sites of
 *                              models/backbone/vit.py:79-83,:123-138, timm Mlp, models/backbone/projector.py:85-132,
 *                              :177-193, models/transformer.py:28-39,:231-240, models/attention.py:507-560,
 *                              models/lwdetr.py:149-159 - with the bias / activation / LayerScale / residual /
 *                              layout epilogues fused
 *   lwdetr_attention           models/backbone/vit.py:130-137 (window and global softmax(QK^T)V) and
 *                              models/attention.py:563-606 (decoder self-attention)
 *   lwdetr_attn_train_forward/_backward  models/backbone/vit.py:130-137 under autograd (training: forward saves lse, backward recomputes p)
 *   lwdetr_mlp_fused           models/backbone/vit.py:217-218 (+ timm.models.layers.Mlp: fc1 -> GELU -> fc2)
 *   lwdetr_msda_train_forward/_backward  models/ops/modules/ms_deform_attn.py:113-142 under autograd (training: nothing saved, no float atomics)
 *   lwdetr_vit_block           models/backbone/vit.py:138, :199-218, :123-130 (projection + MLP + next block's norm1 / QKV)
 *   lwdetr_ffn_partial/_finish models/transformer.py:507-512, :397-400 (decoder FFN + norm3 + decoder.norm)
 *   lwdetr_layernorm           nn.LayerNorm call sites (vit.py:199,:217; transformer.py:231,:499,:511,:516,:398) and
 *                              the channel LayerNorm of models/backbone/projector.py:21-47
 *   lwdetr_match_cost/_assign  models/matcher.py:50-111 (HungarianMatcher.forward: cost matrix, scipy linear_sum_assignment)
 *   lwdetr_criterion_partials/_finish  models/lwdetr.py:256-380, :458-483 (SetCriterion's losses, evaluation only)
 *   lwdetr_cocoeval_match/_npig/_curves  datasets/coco_eval.py:26-78, :219-264 (pycocotools COCOeval for boxes: evaluateImg, accumulate)
 *   lwdetr_mt_sumsq/_norm_finish/_step  engine.py:76-83 (clip_grad_norm_, torch.optim.AdamW.step, util/utils.py:20-29 ModelEma.update / set)
 */
#ifndef LWDETR_HIP_H
#define LWDETR_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LWDETR_OK 0
#define LWDETR_ERR_BAD_ARG (-1)
#define LWDETR_ERR_UNSUPPORTED (-2)
#define LWDETR_ERR_LAUNCH (-3)

/* out[b,q,m*D+c] = sum_l sum_p attn[b,q,m,l,p] * bilinear(value[b, lvl l, :, m, c], (loc_x*W_l-.5, loc_y*H_l-.5)), zero pad.
 * value (B,S,M,D); shapes (L,2) int64 (H,W); level_start (L) int64; loc (B,Q,M,L,P,2) (x,y); attn (B,Q,M,L,P); out (B,Q,M*D).
 * A sample contributes iff h_im > -1 && w_im > -1 && h_im < H && w_im < W (h_im = loc_y*H - .5, w_im = loc_x*W - .5): a sample with a
 * non-finite location contributes nothing. value must be finite: the vector kernel reads a clamped in-map pixel with weight 0 for a
 * corner outside the map, so an inf / NaN in value reaches queries that do not sample it. The vector kernel (D % 8 == 0, P <= 8,
 * dtype 0 ... 2) serves a call only when value and out are aligned to 8 elements; any other call goes to the one-thread-per-element
 * kernel. */
int lwdetr_msda_forward(const void* value, const int64_t* shapes, const int64_t* level_start, const void* loc,
                        const void* attn, void* out, int B, int S, int M, int D, int L, int Q, int P, int dtype,
                        void* hip_stream);

/* Backward of the op (reference ms_deform_attn_backward, models/ops/src/ms_deform_attn.h:37-60 ->
 * cuda/ms_deform_attn_cuda.cu:83-153 -> cuda/ms_deform_im2col_cuda.cuh:87-160, :846-920): grad_out (B,Q,M*D) ->
 * grad_value (B,S,M,D) (zeroed here, then accumulated with atomics), grad_loc (B,Q,M,L,P,2), grad_attn (B,Q,M,L,P),
 * all fully written. dtype 0 (float32) or 3 (float64), as in the reference. */
int lwdetr_msda_backward(const void* value, const int64_t* shapes, const int64_t* level_start, const void* loc,
                         const void* attn, const void* grad_out, void* grad_value, void* grad_loc, void* grad_attn,
                         int B, int S, int M, int D, int L, int Q, int P, int dtype, void* hip_stream);

/* Model-path variant: oa is the (B*Q, ld_oa) output of the fused sampling_offsets|attention_weights Linear
 * (offsets at column 0: M*L*P*2 values, logits at column logit_col: M*L*P values); ref_boxes (B,Q,4) f32 (cx,cy,w,h);
 * valid_ratios (B,L,2) f32 (w,h). Computes the softmax over the L*P logits of a (row, head) and, per level l with vr = valid_ratios[b,l],
 * loc = ref_xy*vr + off / P * (ref_wh*vr) * 0.5 in-kernel (f32), then samples as lwdetr_msda_forward does (a non-finite location contributes
 * nothing; value must be finite). (L, P) in {1,2} x {2,4}, D % 8 == 0, dtype 0 ... 2. LWDETR_ERR_BAD_ARG unless 0 <= 2*M*L*P <= logit_col,
 * logit_col + M*L*P <= ld_oa, and value and out are aligned to 8 elements. */
int lwdetr_msda_fused_forward(const void* value, const int64_t* shapes, const int64_t* level_start, const void* oa,
                              long ld_oa, int logit_col, const float* ref_boxes, const float* valid_ratios, void* out,
                              int B, int S, int M, int D, int L, int Q, int P, int dtype, void* hip_stream);

/* ---- fused MFMA GEMM: out = epilogue(A_view(M,K) * W(N,K)^T), see lwdetr_gemm_desc ---------------------------- */
typedef struct {
    int winmajor;      /* 0: rows are raster (b,y,x) tokens; 1: window-major padded rows (see DESIGN.md "data layout") */
    int Hp, Wp, Twp;
} lwdetr_tok_layout;

enum { LWDETR_A_PLAIN = 0, LWDETR_A_CONV3x3 = 1, LWDETR_A_PATCH16 = 2 };
enum { LWDETR_ACT_NONE = 0, LWDETR_ACT_RELU = 1, LWDETR_ACT_GELU = 2, LWDETR_ACT_SILU = 3 };
enum { LWDETR_OUT_LINEAR = 0, LWDETR_OUT_HEADS = 1, LWDETR_OUT_HEADS_T = 2, LWDETR_OUT_TOKMAP = 3,
       LWDETR_OUT_DECONV2x2 = 4 };

typedef struct {           /* one column segment [n_begin, n_end) of the output */
    void* out;             /* destination base */
    void* out2;            /* optional second LINEAR destination (ViT feature taps), row stride ld2 */
    const void* res;       /* optional residual, same dtype as out, addressed LINEAR with ldres; row = m % res_mod if res_mod>0 */
    const float* bias;     /* optional f32, indexed by n - n_begin; 16-byte aligned and readable up to ceil8(n_end-n_begin) */
    const float* gamma;    /* optional f32 LayerScale (same padding rule): out = res + gamma * act(acc + bias) * scale */
    const uint8_t* rowmask;/* optional (M): rows with mask == 0 get acc = 0 before bias (rowmask_after = 0, the reference's
                              masked_fill of the INPUT row) or a zero OUTPUT row (rowmask_after = 1, masked_fill of the result) */
    float scale;           /* multiplies (acc + bias) */
    int act;
    int mode;              /* LWDETR_OUT_* */
    int n_begin, n_end;
    long ldo, ld2, ldres;
    int res_mod;
    int rowmask_after;
    int p0, p1, p2;        /* HEADS/HEADS_T: p0 = tokens per image Tp, p1 = head_dim, p2 = heads */
    lwdetr_tok_layout in_tok, out_tok;   /* TOKMAP / DECONV2x2: row decode / encode layouts */
    long out_batch_stride; /* TOKMAP / DECONV2x2: elements between images in out (0 = dense) */
    long out_row_offset;   /* TOKMAP / DECONV2x2: first row inside an image (level offset into `memory`) */
    /* LayerNorm folded into the GEMM (round 5; `nn.LayerNorm` in front of a Linear, models/backbone/vit.py:199, :217): with W' = W diag(g),
       b' = b + W beta packed by the host, LN(x) W^T + b = rstd_m (x_m . W'_n - mean_m colsum_n) + b'_n - the GEMM reads the RAW rows and the
       epilogue applies the row statistics: acc <- (acc - mean * ln_colsum[n]) * rstd before bias / activation. All segments of a launch or
       none; served by the 256 x 256 large-tile kernel only (16-bit, PLAIN A, K % 64 == 0, segment boundaries at multiples of 256):
       LWDETR_ERR_UNSUPPORTED for any other shape. */
    const float* ln_stats; /* optional (2, M) f32, planar: ln_stats[m] = mean, ln_stats[M + m] = rstd of A row m (lwdetr_row_stats); NULL = plain GEMM */
    const float* ln_colsum;/* with ln_stats: f32 sum over k of W[n][k] as stored (16-bit rounded), indexed by n - n_begin, padded like bias */
} lwdetr_gemm_seg;

typedef struct {
    const void* A; const void* A2;   /* A2 optional: A_view = A + A2 (same shape, PLAIN only) */
    const void* W;                   /* (N, K) row-major, same dtype as A */
    int M, N, K;
    long lda;
    int a_mode;
    /* CONV3x3: A is (B, Hin, Win, ldc) tokens in layout a_tok with Cin channels at column a_col0; stride 1|2; K = 9*Cin.
       PATCH16: A is the (B,3,H,W) image, rows are window-major tokens of a_tok; K = 768. */
    lwdetr_tok_layout a_tok;
    int conv_cin, conv_stride, a_col0, conv_hout, conv_wout;
    int img_h, img_w;
    int nseg;
    lwdetr_gemm_seg seg[3];
    /* Split-K for few-row GEMMs with a long contraction (round 5): splitk >= 2 asks for that many workgroups per 64 x 64 tile, each over a
       contiguous range of k-stages; honoured only where the launch takes the 64 x 64 DMA ring kernel (16-bit, no A2), ignored elsewhere.
       splitk_ws: 16-byte aligned workspace of tiles * splitk * 4352 floats (f32 partial tiles) followed by `tiles` ints (arrival counters),
       tiles = ceil(M / 64) * ceil(N / 64); the counters must be ZERO before the first launch (every launch leaves them zero), the workspace
       belongs to one launch at a time. Results do not depend on the arrival order (slabs are summed in slice order). */
    void* splitk_ws;
    int splitk;
} lwdetr_gemm_desc;

int lwdetr_gemm(const lwdetr_gemm_desc* desc, int dtype, void* hip_stream);
/* Few-row form (round 6; the single-image latency path): the same descriptor as lwdetr_gemm with W FRAGMENT-MAJOR - [N / 16][K / 32][16][32],
 * lwdetr_amd.kernels.pack_frag16 of the (N, K) matrix lwdetr_gemm takes. A workgroup owns 16 rows x 128 columns, a wave loads the MFMA fragments of a
 * third of the contraction straight from L2 before it multiplies them: no LDS ring, no barriers - the six 3x3 convolutions of the projector
 * (models/backbone/projector.py:101-132) at one 640 x 640 image 19.3 -> ~9 us each. Serves: f16 / bf16 / f32, M <= 8192, a_mode PLAIN or CONV3x3 (raster
 * rows, stride 1 | 2, Cin in {128, 192}, a_col0 % 8 == 0), K % 32 == 0, N % 16 == 0, ONE LINEAR segment over all N columns (bias, activation, scale,
 * gamma, residual, second destination; no row mask, periodic residual, folded LayerNorm or A2); LWDETR_ERR_UNSUPPORTED otherwise, before any launch
 * (nothing written, nothing counted); an unknown activation is LWDETR_ERR_BAD_ARG. Same arithmetic as lwdetr_gemm up to the f32 summation order of
 * the contraction.
 *   A 16 x 32 weight fragment is one contiguous KB in 16-bit and one contiguous 2 KB in f32. What the kernel accesses in wide pieces, per dtype:
 *     16-bit: A and W 16-byte aligned, lda % 8 == 0 (16-byte loads of 8 values); out / res / out2 8-byte aligned, ldo / ldres / ld2 % 4 == 0.
 *     f32   : A and W 16-byte aligned, lda % 4 == 0 (two 16-byte loads of 4 values); out / res / out2 16-byte aligned, ldo / ldres / ld2 % 4 == 0.
 *     both  : bias / gamma 16-byte aligned.
 *   The f32 form (dtype 0) contracts with the exact-f32 16x16x4 MFMA, f32 accumulation in k-chunk order, GELU in the erf form: the same arithmetic
 *   as lwdetr_gemm in f32 up to summation order. The launch plan takes it only with LWDETR_GEMM_FEW_F32=1 (lwdetr_amd.kernels.gemm_few_supported). */
int lwdetr_gemm_few(const lwdetr_gemm_desc* desc, int dtype, void* hip_stream);
/* Row statistics of x (M, C) for the LayerNorm-folded GEMM: stats[m] = mean, stats[M + m] = 1 / sqrt(var + eps) (planar - interleaved pairs made
 * hipcc broadcast the high half of a register pair into packed-f32 epilogue arithmetic, the instruction form tools/check_isa.py refuses),
 * two-pass f32 on the stored values -
 * the arithmetic of lwdetr_layernorm without its output pass (half its HBM traffic). C % 8 == 0 (16-bit) / C % 4 == 0 (f32).
 * LWDETR_ERR_BAD_ARG for ldx < C or an x that is not 16-byte aligned (the rows are read in 16-byte chunks). */
int lwdetr_row_stats(const void* x, long ldx, long M, int C, float eps, float* stats, int dtype, void* hip_stream);
/* Kernel selection override for tests / tuning (process-wide): big_mode -1 = default (environment LWDETR_GEMM_BIG, else
 * shape thresholds), 0 = never use the 256-row large-tile kernel, 2 = use it whenever the shape is legal for it,
 * 32 / 64 = as 2 with that stage depth. Results do not depend on it beyond f32 summation order. */
void lwdetr_gemm_tuning(int big_mode);
/* 1 if the library was built with -DLWDETR_EXPERIMENTS: the kernel forms that were built, validated and measured SLOWER than what the launch plan
 * uses (round 5: the 4-wave / 128-row large-tile GEMM, the LayerNorm-folded GEMM epilogue behind ln_stats, split-K behind splitk, the LDS window-tile
 * attention kernel) are only compiled then. The default library (0) answers such requests with LWDETR_ERR_UNSUPPORTED or takes the ordinary kernel. */
int lwdetr_has_experiments(void);
/* The persistent large-tile kernel (round 6, csrc/gemm_pt.hip: a workgroup walks its 256 x 256 tiles, the DMA ring runs on across tile boundaries,
 * the epilogue goes straight from the accumulators to memory) serves the 16-bit plain-A launches whose segments are whole 256-column tiles of
 * LINEAR / HEADS / HEADS_T outputs - the four Linear layers of a C = 768 ViT block (models/backbone/vit.py:123-138, :217-218). Process-wide
 * override for tests / tuning: pt_mode -1 = default (environment LWDETR_GEMM_PT, read once; else 1), 0 = never, 1 = at the sizes where the
 * 256-row tile pays, 2 = whenever the shape is legal; tuning: + 256 * w sets the start-skew window to w ticks of 10 ns. Results equal the
 * large-tile kernel's up to f32 rounding of the epilogue (bias first, one scale multiplication). */
void lwdetr_gemm_pt_tuning(int pt_mode);
/* launches of the persistent kernel by this process so far (tests assert which kernel served a shape) */
long lwdetr_gemm_pt_count(void);
/* Launch-path record of lwdetr_gemm and lwdetr_gemm_few: one process-wide host counter per kernel family, tile and variant (the 64 x 64 ring at
 * each depth, 128 x 64, 128 x 128; the large-tile kernel per column tile and stage depth; the persistent kernel; the few-row kernel's PLAIN and
 * CONV forms ...), incremented after a launch was issued and accepted - a refused request counts nothing. lwdetr_gemm_path_counts copies the
 * first min(n, count) counters to out (out may be NULL) and returns count; lwdetr_gemm_path_name(i) is the family name of counter i (NULL
 * outside [0, count)). Tests assert which kernel served a launch. */
int lwdetr_gemm_path_counts(long* out, int n);
const char* lwdetr_gemm_path_name(int i);

/* ---- fused softmax(QK^T)V, flash-style, MFMA ------------------------------------------------------------------- */
typedef struct {
    const void* Q;      /* (B, heads, Tp, hd)  pre-scaled by hd^-0.5 * log2(e) */
    const void* K;      /* (B, heads, Tp, hd) */
    const void* VT;     /* (B, heads, hd, Tp) */
    void* out;          /* (B*Tp, ldo) row-major, head h writes columns [h*hd, (h+1)*hd) */
    long ldo;
    int B, heads, hd, Tp;
    int seqs_per_img;   /* 16 (window attention) or 1 */
    int seq_tok_stride; /* tokens between consecutive sequences of one image */
    int keys_per_seq;   /* tokens (incl. pad rows) spanned by one sequence; >= 8 and a multiple of 4 */
    int sub_stride, sub_len; /* key j is real iff (j % sub_stride) < sub_len */
    int kind;           /* 0 window, 1 global, 2 decoder self-attention (profiling label only) */
    int vt_slack;       /* nonzero: at least 8 readable bytes follow the VT tensor (lets the LDS-ring kernel serve sequences
                           whose length is not a multiple of 8: it fetches V^T in whole 16-byte runs) */
} lwdetr_attn_desc;

int lwdetr_attention(const lwdetr_attn_desc* desc, int dtype, void* hip_stream);
/* Kernel selection override for tests / tuning (process-wide): lds_mode -1 = default (environment LWDETR_ATTN_LDS, else 2),
 * 0 = never use the LDS-ring kernel, 1 = sequences of >= 512 keys, 2 = also >= 192-key windows, 3 = everything >= 64 keys. */
void lwdetr_attention_tuning(int lds_mode);
/* LDS-ring kernel shape override for tests / tuning (process-wide): 0 = default (environment LWDETR_ATTN_LDS_CFG, else by head
 * dimension), otherwise 1000 (U - 1) + 100 QT + NW = 32 QT queries per wave, NW waves per workgroup, U 64-key blocks per ring step;
 * a shape that is not compiled in (or does not fit LDS at this head dimension) makes lwdetr_attention return LWDETR_ERR_UNSUPPORTED. */
void lwdetr_attention_tuning_cfg(int cfg);

/* ---- row LayerNorm: out[r,:] = (x[r,:]-mean)/sqrt(var+eps)*gamma+beta; biased variance; C % 4 == 0 ------------- */
/* rows_per_batch / out_batch_rows / out_row_offset let the projector write straight into `memory` (B,S,d): input row b * rows_per_batch + r
 * lands in output row b * out_batch_rows + out_row_offset + r (rows_per_batch <= 0: no remap).
 * Refused with LWDETR_ERR_BAD_ARG before anything is launched (lwdetr_layernorm, _chain, lwdetr_ffn_finish): ldx < C, ldo < C, ldo2 < C;
 * a remap with out_batch_rows < rows_per_batch, out_row_offset < 0 or out_row_offset + rows_per_batch > out_batch_rows (the slice
 * would run into the next batch); x, out, out2 or partial not 16-byte aligned (rows move in 16-byte chunks; ld* must be whole chunks,
 * C <= 2048 (16-bit) / 1024 (f32): LWDETR_ERR_UNSUPPORTED otherwise). */
int lwdetr_layernorm(const void* x, long ldx, const float* gamma, const float* beta, void* out, long ldo, long M,
                     int C, float eps, long rows_per_batch, long out_batch_rows, long out_row_offset, int dtype,
                     void* hip_stream);

/* out1 = LN1(x), out2 = LN2(out1) in one pass over the row; bit-identical to two lwdetr_layernorm launches (the second reading
 * out1). Decoder layer tail: norm3 followed by the shared decoder.norm (models/transformer.py:397-400, :466-517). */
int lwdetr_layernorm_chain(const void* x, long ldx, const float* gamma1, const float* beta1, float eps1, void* out1, long ldo1,
                           const float* gamma2, const float* beta2, float eps2, void* out2, long ldo2, long M, int C,
                           int dtype, void* hip_stream);

/* ---- decoder FFN in two launches, hidden activation on chip --------------------------------------------------------
 * Replaces models/transformer.py:507-512 (linear2(dropout(relu(linear1(tgt)))) + residual + norm3) and the shared
 * decoder.norm that follows (:397-400). lwdetr_ffn_partial: the grid is (token tiles) x (splits of the hidden dimension);
 * every workgroup keeps ReLU(x W1^T + b1) of its hidden slice in registers and writes the f32 partial product with W2 to
 * partial[split] (M, C) - the 300-queries-per-image row count alone cannot fill 256 CUs, the hidden split can.
 * lwdetr_ffn_finish: x + b2 + sum of the partial slabs (rounded to the 16-bit dtype, as the unfused GEMM epilogue rounds),
 * out1 = LN1(.), optionally out2 = LN2(out1). w1 (hid, C) plain row-major; w2_chunked (hid/32, C, 32) as for
 * lwdetr_mlp_fused. C in {256, 384}, hid % 64 == 0, 16-bit dtypes. lwdetr_ffn_splits returns the number of slabs the
 * launch for (M, C, hid) writes (> 0), or -error. lwdetr_ffn_finish: out1 MAY alias x (every row is read completely before it is
 * written; the engine updates the decoder stream in place); out2 must not alias x or out1. */
int lwdetr_ffn_splits(long M, int C, int hid, int dtype);
int lwdetr_ffn_partial(const void* x, long ldx, const void* w1, const float* b1, const void* w2_chunked, float* partial, long M,
                       int C, int hid, int dtype, void* hip_stream);
int lwdetr_ffn_finish(const void* x, long ldx, const float* partial, int splits, const float* b2, const float* gamma1,
                      const float* beta1, float eps1, void* out1, long ldo1, const float* gamma2, const float* beta2, float eps2,
                      void* out2, long ldo2, long M, int C, int dtype, void* hip_stream);

/* ---- fused ViT MLP: x <- x + gamma2 * fc2(GELU(fc1(LN(x)))), one launch, hidden activation stays on chip ---------
 * Replaces models/backbone/vit.py:217-218 (norm2 -> timm Mlp -> gamma_2 -> residual). Weight packing (host, once):
 *   w1_folded (4C, C) = fc1.weight * norm2.weight[None, :],  b1_folded = fc1.bias + fc1.weight @ norm2.bias (f32),
 *   w2_chunked (4C/32, C, 32) = fc2.weight.view(C, 4C/32, 32)[:, :, perm].permute(1, 0, 2): each 32-wide hidden chunk
 *   contiguous, inside a chunk perm = [4g+e+16*hi for g in 0..3 for hi in 0..1 for e in 0..3] (the kernel's MFMA k-slots).
 * x is updated in place; out2 (optional, row stride ld2) receives a copy (ViT feature taps); stats_out (optional, (M,2)
 * f32) receives mean and 1/sqrt(var+eps_next) of the updated rows for the next block's LayerNorm. C in {192, 384}.
 * Optional fused attention output projection (vit.py:138, :206-216): when att != NULL the kernel first computes
 * x <- x + gamma1 * (att @ wp^T + bp) (att (M,C) row stride ldatt, wp (C,C) = attn.proj.weight, bp / gamma1 f32 (C));
 * w1_folded must then have its columns permuted inside every 32-chunk with the same `perm` as w2_chunked.
 * Optional chained LayerNorm + QKV of the NEXT block (vit.py:199, :123-130) on the updated rows (needs att != NULL):
 * wqkv_next (3C, C) = next qkv.weight * next norm1.weight[None,:] with the same per-32-chunk column permutation,
 * bqkv_next (3C) f32 = [q_bias, 0, v_bias] + qkv.weight @ norm1.bias; writes Q (pre-scaled by qscale), K as
 * (B, heads, Tp, hd) and V^T as (B, heads, hd, Tp) exactly like lwdetr_gemm's HEADS / HEADS_T epilogues (LN eps = eps_next).
 * With the chained QKV, M and Tp must be multiples of 4 (a run of 4 tokens of V^T never crosses an image); M need NOT be a multiple of Tp. Row m goes to
 * image m / Tp, position m % Tp, so with M % Tp != 0 the last image is partial: its positions M % Tp .. Tp - 1 are not written, and q_out / k_out / vt_out
 * must hold ceil(M / Tp) whole images (ceil(M / Tp) * Tp * C elements each). The same holds for lwdetr_vit_block_few. */
int lwdetr_mlp_fused(void* x, long ldx, const void* w1_folded, const float* b1_folded, const void* w2_chunked,
                     const float* b2, const float* gamma2, void* out2, long ld2, float* stats_out, long M, int C,
                     float eps, float eps_next, const void* att, long ldatt, const void* wp, const float* bp,
                     const float* gamma1, const void* wqkv_next, const float* bqkv_next, void* q_out, void* k_out,
                     void* vt_out, float qscale, int heads, int hd, int Tp, int dtype, void* hip_stream);

/* The few-token form of lwdetr_mlp_fused with the attention projection (round 6; C in {192, 384}, M < 12800: the single-image latency path) on
 * FRAGMENT-MAJOR weights: w1_frag, wp_frag, wqkv_frag_next = the w1_folded / wp / wqkv_next of lwdetr_mlp_fused re-laid out as
 * [R / 16][C / 32][16][32] (lwdetr_amd.kernels.pack_frag16), so that each 16 x 32 MFMA fragment the kernel loads straight from L2 is one
 * contiguous KB (2 KB in float32) instead of 16 half lines. Everything else as lwdetr_mlp_fused (att required); in 16-bit at C = 192 the
 * results are bit-identical to it.
 * Accepted: C = 192 with dtype 0 / 1 / 2, C = 384 with dtype 1 / 2 only (C = 384 with dtype 0: LWDETR_ERR_UNSUPPORTED).
 * dtype 1 / 2 (f16 / bf16): ldx, ld2, ldatt multiples of 8 (LWDETR_ERR_BAD_ARG otherwise).
 * 16-bit C = 384 (vit_block_few384_kernel, a kernel of its own: 16-token workgroups at every M, hidden activations through LDS, each wave owns
 * output channel tiles over the whole hidden dimension; LWDETR_MLP_SMALL_TT / LWDETR_MLP_SMALL do not apply): the same argument rules as 16-bit
 * C = 192 - its widest access is 8 values at a multiple of 8 elements of a row, as there. Roundings as lwdetr_mlp_fused at C = 384, but NOT
 * bit-identical to it: equal to rounding only.
 * dtype 0 (float32; the same structure on exact-f32 16x16x4 MFMAs, 16-token workgroups at every M; sums in another order than lwdetr_mlp_fused's
 * f32 kernel, so equal to it only to rounding): ldx, ld2, ldatt multiples of 4, and x, att, out2, q_out, k_out, vt_out, w1_frag, wp_frag,
 * wqkv_frag_next, w2_chunked, b1_folded, b2, bp, gamma1, gamma2, bqkv_next 16-byte aligned - LWDETR_ERR_UNSUPPORTED otherwise, before any launch.
 * LWDETR_ERR_UNSUPPORTED outside (C, M) above and for any other dtype. */
int lwdetr_vit_block_few(void* x, long ldx, const void* w1_frag, const float* b1_folded, const void* w2_chunked, const float* b2,
                         const float* gamma2, void* out2, long ld2, float* stats_out, long M, int C, float eps, float eps_next,
                         const void* att, long ldatt, const void* wp_frag, const float* bp, const float* gamma1,
                         const void* wqkv_frag_next, const float* bqkv_next, void* q_out, void* k_out, void* vt_out, float qscale,
                         int heads, int hd, int Tp, int dtype, void* hip_stream);

/* ---- fused ViT block tail (round 3; 16-bit dtypes, C in {192, 384}, M % 4 == 0) --------------------------------------
 * Replaces, per ViT block, models/backbone/vit.py:138 + :206-216 (attention output projection, gamma_1, residual),
 * :217-218 (norm2 -> timm Mlp -> gamma_2 -> residual) and, with has_qkv, :199 + :123-130 of the NEXT block (norm1, QKV with
 * q_bias / v_bias; Q pre-scaled by qscale, Q / K as (B, heads, Tp, hd), V^T as (B, heads, hd, Tp) like lwdetr_gemm's HEADS /
 * HEADS_T epilogues). x (M, C) is updated in place, att (M, C) is the attention output; out2 (optional) receives a copy
 * of the new rows (feature taps), stats_out (optional, (M, 2) f32) mean and 1/sqrt(var + eps_next) of the new rows.
 * wstream / vec: lwdetr_amd.kernels.pack_vit_block (all weights of the block as one stream of 1 KB MFMA fragments in
 * consumption order; f32 vectors b1' | bp | g1 | 1/g1 | b2 | 1/g2 | g2 | bqkv'); sizes from the two helpers below.
 * hd must be a power of two; gamma_1 / gamma_2 must be non-zero (the kernel divides by them in f32). Refused with BAD_ARG: a row stride
 * below C (ldx, ldatt, ld2 with out2), a stats_out that is not 4-byte aligned, q_out / k_out / vt_out (M * C elements each) that overlap one
 * another - lwdetr_vit_qkv and lwdetr_vit_stem refuse the same (ldx, ldpos below C; overlapping outputs).
 *
 * Launch-form record of lwdetr_vit_block / lwdetr_vit_qkv / lwdetr_vit_stem: one process-wide host counter per kernel instantiation
 * (vitblock_<dtype>_c<C>_nh<NH>_wpc<WPC>_qkv<0|1>_g16_<0|1>, vit_qkv_<dtype>_c<C>, vit_stem_<dtype>_c<C>), incremented after a launch was
 * issued and accepted - a refused request counts nothing. lwdetr_vit_path_counts copies the first min(n, count) counters to out (out may be
 * NULL) and returns count; lwdetr_vit_path_name(i) names counter i (NULL outside [0, count)). Tests assert which form served a launch. */
int lwdetr_vit_path_counts(long* out, int n);
const char* lwdetr_vit_path_name(int i);

/* The same record for msda.hip: one counter per kernel instantiation that lwdetr_msda_forward / lwdetr_msda_backward / lwdetr_msda_fused_forward
 * launch - msda_vec8_{f32,f16,bf16}_p{2,4,n} (n: run-time P), msda_generic_{f32,f16,bf16,f64}, msda_fused_{f32,f16,bf16}_l{1,2}p{2,4},
 * msda_backward_{f32,f64}. */
int lwdetr_msda_path_counts(long* out, int n);
const char* lwdetr_msda_path_name(int i);

/* The same record for attention.hip: one counter per kernel instantiation that lwdetr_attention can launch, named by rule -
 * attn_wave_{f32,f16,bf16}_hd{16,32,64}_qt{2,4} and ..._qt2_short (attn_kernel: 32 / 64 queries per wave, the <= 128-key form of the 16-bit types;
 * no qt4 at hd 64, no short form in f32), attn_win_{f16,bf16}_hd{16,32} (one wave per (sequence, head)), attn_ring_{f16,bf16}_hd{HD}_q{QT}w{NW}u{U}
 * (the LDS-ring kernel: one name per tuning variant of lwdetr_attention_tuning_cfg, 1000 (U - 1) + 100 QT + NW; the variants whose ring does not fit
 * the LDS budget - U = 2 at hd 64, U = 4 - answer LWDETR_ERR_UNSUPPORTED and their counters never move), attn_wtile_{f16,bf16} in
 * LWDETR_EXPERIMENTS builds only. */
int lwdetr_attn_path_counts(long* out, int n);
const char* lwdetr_attn_path_name(int i);

/* Differentiable fused attention for training (attention_train.hip; reference models/backbone/vit.py:130-137 under autograd):
 * o[b,n,h*hd+d] = sum_k softmax_k(scale q[b,n,h,:] . k[b,k,h,:]) v[b,k,h,d], lse[b,h,n] = log sum_k exp(scale q . k) (f32, natural log), no mask.
 * q, k, v (and dq, dk, dv) are addressed base + b*sb + n*sn + h*sh + d with strides in ELEMENTS and d contiguous, so they may be the views
 * qkv[:, :, i] of one (B, N, 3, heads, hd) tensor; o (and d_o) is (B, N, heads*hd) with row stride o_ld (do_ld) >= heads*hd; lse is (B, heads, N).
 * hd in {16, 32, 64}, dtype 0 / 1 / 2, any B, heads, N >= 1. Scores, weights and every sum are f32 in all dtypes (f32 uses the exact
 * f32-input MFMA); nothing of size N x N is stored. Every element of o, lse, dq, dk, dv is written - the caller pre-zeroes nothing - with no
 * atomics: two calls on the same inputs give the same bits.
 * lwdetr_attn_train_backward takes the descriptor of the forward call (q, k, v, the o and lse it wrote), the output gradient d_o and the nine
 * gradient strides, and needs lwdetr_attn_train_workspace_bytes(...) bytes of 4-byte aligned device scratch (0 for short sequences: workspace
 * may then be NULL). It computes D = rowsum(d_o o), p = exp(s - lse), dv = p^T d_o, ds = p (d_o v^T - D), dq = scale ds k, dk = scale ds^T q.
 * LWDETR_ERR_BAD_ARG, before anything is launched: a null pointer, B / heads / N < 1, a scale that is not finite and positive, a tensor
 * base pointer that is not 16-byte aligned, a stride that is not a multiple of 16 bytes; LWDETR_ERR_UNSUPPORTED: any other hd or dtype.
 * Launch-form record as lwdetr_attn_path_counts: attn_train_fwd_<dt>_hd<HD>; backward at N <= 256 attn_train_bwd_one_<dt>_hd<HD> (one
 * launch), above it attn_train_bwd_dot_<dt> + attn_train_bwd_dkdv_<dt>_hd<HD> + attn_train_bwd_dq_<dt>_hd<HD>; <dt> in {f32, f16, bf16}. */
typedef struct {
    const void *q, *k, *v;
    long q_sb, q_sn, q_sh, k_sb, k_sn, k_sh, v_sb, v_sn, v_sh;
    void* o;
    long o_ld;
    float* lse;
    int B, heads, N, hd;
    float scale;
} lwdetr_attn_train_desc;
int lwdetr_attn_train_forward(const lwdetr_attn_train_desc* desc, int dtype, void* hip_stream);
long lwdetr_attn_train_workspace_bytes(int B, int heads, int N, int hd, int dtype);
int lwdetr_attn_train_backward(const lwdetr_attn_train_desc* desc, const void* d_o, long do_ld, void* dq, void* dk, void* dv,
                               long dq_sb, long dq_sn, long dq_sh, long dk_sb, long dk_sn, long dk_sh, long dv_sb, long dv_sn, long dv_sh,
                               void* workspace, int dtype, void* hip_stream);
int lwdetr_attn_train_path_counts(long* out, int n);
const char* lwdetr_attn_train_path_name(int i);

/* Differentiable deformable cross-attention for training (msda_train.hip; reference models/ops/modules/ms_deform_attn.py:113-142 between the
 * Linears, under autograd). With the sampling and border rules of lwdetr_msda_forward above, per (row = b*Q + q, head m), level l, point p:
 *   loc = ref_xy[row, l] + off / P * ref_wh[row, l] * 0.5,  a = softmax over the L*P logits of (row, m),
 *   out[b, q, m*D + c] = sum_{l,p} a * bilinear(value[b, level l, m, c], loc).
 * value: element (b, s, m, c) at value[(b*S + s)*value_ld + m*D + c], value_ld >= M*D in ELEMENTS (a column view of a wider Linear output);
 * offsets (B*Q, M*L*P*2) and logits (B*Q, M*L*P) with their own leading dimensions in elements; ref (B, Q, L, 4) f32 boxes (cx, cy, w, h) per
 * level, already multiplied by the valid ratios; mask NULL or (B, S) bytes: a row with a non-zero byte reads as zero and receives a zero
 * grad_value (masked_fill and its backward); shapes (L, 2) / level_start (L) int64 DEVICE arrays; level_start is arbitrary (gaps allowed; rows
 * of S that no level covers get a zero grad_value), every level must lie inside [0, S) and hold fewer than 2^30 pixels. value must be finite.
 * dtype 0 / 1 / 2 (f32 / f16 / bf16) is the type of value, offsets, logits, out, grad_out, grad_value, grad_offsets, grad_logits; all
 * arithmetic and every sum is f32 (expf and a true division in the softmax, no hardware approximation), each output element is rounded once.
 * lwdetr_msda_train_forward writes out (B, Q, M*D), contiguous, and saves nothing. lwdetr_msda_train_backward takes the same descriptor,
 * grad_out (B, Q, M*D) contiguous, and writes EVERY element of grad_value (B, S, M, D) contiguous, grad_offsets (B*Q, M*L*P*2) contiguous,
 * grad_logits (B*Q, M*L*P) contiguous and grad_ref (B, Q, L, 4) f32 - the caller pre-zeroes nothing:
 *   d off_x = g_x ref_w 0.5 / P,  d ref_x = sum_{m,p} g_x,  d ref_w = sum_{m,p} g_x off_x 0.5 / P  (y, h alike),  d logit_i = a_i (g_a,i - sum_j a_j g_a,j),
 * g_x, g_a the location / weight derivatives of lwdetr_msda_backward. It recomputes locations and weights with the forward's functions (same bits)
 * and needs lwdetr_msda_train_workspace_bytes(desc) bytes of 16-byte aligned device scratch (20 bytes per sample; 0 for a descriptor that would
 * be refused). No floating-point atomic is used: a second call of either entry on the same inputs returns the same bits, grad_value included.
 * LWDETR_ERR_BAD_ARG, before anything is launched: a null descriptor or pointer (mask excepted), a size < 1, a leading dimension below its row,
 * value / out / grad_out / workspace not 16-byte aligned, value_ld not a multiple of 16 bytes, another pointer not aligned to its element, a
 * workspace that is too small. LWDETR_ERR_UNSUPPORTED, before any runtime call: any other dtype (f64 included), D % 8 != 0, D > 64, L > 4,
 * P not in {1, 2, 4, 8}, L*P > 16, M > 256. Sizes are checked first, then the supported range, then pointers.
 * Launch-form record as lwdetr_msda_path_counts: msda_train_fwd_<dt>_<form> and msda_train_bwd_q_<dt>_<form> with <form> in {l1p2, l2p4} (the two
 * shipped (L, P) pairs, compile-time) or gen (run-time L, P), msda_train_bwd_v_<dt>_e{1,2,4} (D <= 16 / 32 / 64); a backward counts one bwd_q and one bwd_v. */
typedef struct {
    const void* value;
    long value_ld;
    const void* offsets;
    long offsets_ld;
    const void* logits;
    long logits_ld;
    const float* ref;
    const unsigned char* mask;
    const int64_t* shapes;
    const int64_t* level_start;
    int B, S, M, D, L, Q, P, dtype;
} lwdetr_msda_train_desc;
int lwdetr_msda_train_forward(const lwdetr_msda_train_desc* desc, void* out, void* hip_stream);
long lwdetr_msda_train_workspace_bytes(const lwdetr_msda_train_desc* desc);
int lwdetr_msda_train_backward(const lwdetr_msda_train_desc* desc, const void* grad_out, void* grad_value, void* grad_offsets, void* grad_logits,
                               float* grad_ref, void* workspace, long workspace_bytes, void* hip_stream);
/* The backward of ONE (row, head) on HOST arrays in f32, with the per-sample derivative and chain-rule functions the kernels are compiled from
 * (they are __host__ __device__), so that CPU tests cover the chain rule. value / grad_value point at this image's and head's first channel,
 * row s at + s*ld; mask NULL or this image's (S) bytes; shapes / level_start host arrays; offsets (L*P*2), logits (L*P), ref (L, 4), grad_out (D).
 * grad_offsets and grad_logits are written; grad_value and grad_ref (L, 4) are ADDED to (the caller sums heads and rows). Any D >= 1, L*P <= 16. */
int lwdetr_msda_train_backward_host(const float* value, long value_ld, const unsigned char* mask, const int64_t* shapes, const int64_t* level_start,
                                    int D, int L, int P, const float* offsets, const float* logits, const float* ref, const float* grad_out,
                                    float* grad_value, long grad_value_ld, float* grad_offsets, float* grad_logits, float* grad_ref);
int lwdetr_msda_train_path_counts(long* out, int n);
const char* lwdetr_msda_train_path_name(int i);

/* Two-stage query selection under training (two_stage_train.hip; reference models/transformer.py:224-264 with group_detr groups).
 * lwdetr_two_stage_scores: for every group g < G and row r < rows (r = b*S + s), in ONE launch,
 *   x = rowvalid[r] ? memory[r*ld .. + d) : 0,  y = LayerNorm(x W_eo[g]^T + b_eo[g]) * ln_w[g] + ln_b[g] (eps 1e-5),
 *   scores[g*rows + r] = max_c (y W_cls[g]^T + b_cls[g])_c        (f32; nothing else is written, y and the logits stay on chip).
 * Weights are stacked over groups and contiguous in `dtype`: w_eo (G, d, d), b_eo / ln_w / ln_b (G, d), w_cls (G, ncls, d), b_cls (G, ncls).
 * dtype 0 / 1 / 2; products are MFMAs of the input type (f32: the exact 16x16x4 form, no down-conversion), accumulators, LayerNorm and
 * logits f32; for the 16-bit types y is rounded once, as the operand of the class GEMM. A row's score depends on its values alone, not on its
 * place in a tile: equal rows (all invalid rows of a group) get equal bits. rows == 0 launches nothing.
 * lwdetr_two_stage_gather: idx (G, B, nq) int64, distinct inside a (g, b) -> x_sel (B, G, nq, d) = rowvalid ? memory[b, idx] : 0, props_sel
 *   (B, G, nq, 4) f32 = props[b, idx] (props (B, S, 4) f32), and the inverse table inv (B, S, G) int32 = q where group g selected the row, else
 *   -1 (every entry is written). An index outside [0, S) selects nothing: zeros, no table entry.
 * lwdetr_two_stage_scatter_backward: grad_memory (B, S, d) contiguous, every element written: row (b, s) = sum over the groups with
 *   inv[b, s, g] >= 0 of grad_x_sel[b, g, inv, :], added in ascending g in f32 and rounded once; invalid and unselected rows are zero.
 * No atomics: a second call returns the same bits.
 * LWDETR_ERR_UNSUPPORTED: a dtype other than 0 / 1 / 2. LWDETR_ERR_BAD_ARG, before anything is launched: scores - d not 256 / 384, ncls outside
 * [1, 384], G outside [1, 16], rows < 0, a null pointer, ld < d, memory / weights / d-vectors not 16-byte aligned or ld not a multiple of
 * 16 bytes; gather / scatter - B, S, nq < 1, nq > S, G outside [1, 16], d outside [1, 4096], a null pointer, ld < d, a pointer not aligned to
 * its element. The _check entries answer what the entry would answer before launching and touch no device.
 * Launch-form record as lwdetr_msda_path_counts: ts_scores_<dt>_d{256,384}, ts_gather_<dt>, ts_scatter_<dt>; <dt> in {f32, f16, bf16}. */
int lwdetr_two_stage_scores(const void* memory, long ld, const unsigned char* rowvalid, const void* w_eo, const void* b_eo, const void* ln_w,
                            const void* ln_b, const void* w_cls, const void* b_cls, float* scores, long rows, int d, int ncls, int G, int dtype,
                            void* hip_stream);
int lwdetr_two_stage_scores_check(const void* memory, long ld, const unsigned char* rowvalid, const void* w_eo, const void* b_eo, const void* ln_w,
                                  const void* ln_b, const void* w_cls, const void* b_cls, const float* scores, long rows, int d, int ncls, int G,
                                  int dtype);
int lwdetr_two_stage_gather(const void* memory, long ld, const unsigned char* rowvalid, const float* props, const int64_t* idx, void* x_sel,
                            float* props_sel, int* inv, int B, int S, int G, int nq, int d, int dtype, void* hip_stream);
int lwdetr_two_stage_gather_check(const void* memory, long ld, const unsigned char* rowvalid, const float* props, const int64_t* idx,
                                  const void* x_sel, const float* props_sel, const int* inv, int B, int S, int G, int nq, int d, int dtype);
int lwdetr_two_stage_scatter_backward(const void* grad_x_sel, const int* inv, const unsigned char* rowvalid, void* grad_memory, int B, int S, int G,
                                      int nq, int d, int dtype, void* hip_stream);
int lwdetr_two_stage_scatter_backward_check(const void* grad_x_sel, const int* inv, const unsigned char* rowvalid, const void* grad_memory, int B,
                                            int S, int G, int nq, int d, int dtype);
int lwdetr_two_stage_path_counts(long* out, int n);
const char* lwdetr_two_stage_path_name(int i);

/* Training-forward glue (train_glue.hip). dtype 0 / 1 / 2 I/O, f32 arithmetic, one rounding per output element, no floating-point atomic: a
 * second call returns the same bits.
 * lwdetr_ln2d_forward: the channels-first LayerNorm of a projector stage (reference models/backbone/projector.py:21-47). x (B, C, HW)
 *   contiguous; per pixel u = mean_c x, s = mean_c (x - u)^2 (two passes), y = w_c (x - u) / sqrt(s + eps) + b_c. tokens == 0: y (B, C, HW);
 *   tokens != 0: y (B, HW, C), the rows `memory` is made of. mean / rstd (B, HW) f32 are written for the backward. w, b are f32.
 * lwdetr_ln2d_backward: dy in the layout of the forward's y -> dx (B, C, HW) in `dtype`, dw / db (C) f32. Every workgroup (64 pixels of one
 *   image) writes one partial per channel into ws (lwdetr_ln2d_workspace_floats floats) and a second kernel adds them in ascending workgroup
 *   order.
 * lwdetr_sine_embed_forward: boxes (rows, 4) with row stride ld (elements) -> out (rows, 4 * dim) contiguous, blocks in the order y, x, w, h
 *   (box coordinates 1, 0, 2, 3); inside a block element j is sin (even j) or cos (odd j) of 2 pi box_c (inv_hi[j] + inv_lo[j]), where
 *   inv_hi + inv_lo is 1 / 10000^(2 floor(j / 2) / dim) split into two floats (dim entries each). The argument is reduced in revolutions, so
 *   the accuracy does not depend on |box|. lwdetr_sine_embed_backward: grad_out (rows, 4 * dim) contiguous -> grad_boxes (rows, 4) contiguous,
 *   one wave per row, a fixed-order butterfly over the columns. rows == 0 launches nothing.
 * LWDETR_ERR_UNSUPPORTED: a dtype other than 0 / 1 / 2. LWDETR_ERR_BAD_ARG, before anything is launched: B outside [1, 65535], C outside
 * [1, 1024], HW < 1, a workspace that is too small, dim odd or outside [2, 256], ld < 4, rows < 0, a null or misaligned pointer.
 * Launch-form record as lwdetr_msda_path_counts: ln2d_{fwd,bwd}_{nchw,tok}_<dt>, sine_{fwd,bwd}_<dt>; <dt> in {f32, f16, bf16}. */
int lwdetr_ln2d_forward(const void* x, const float* w, const float* b, void* y, float* mean, float* rstd, int B, int C, long HW, float eps,
                        int tokens, int dtype, void* hip_stream);
long lwdetr_ln2d_workspace_floats(int B, int C, long HW);
int lwdetr_ln2d_backward(const void* x, const float* w, const float* mean, const float* rstd, const void* dy, void* dx, float* dw, float* db,
                         float* ws, long ws_floats, int B, int C, long HW, int tokens, int dtype, void* hip_stream);
int lwdetr_sine_embed_forward(const void* boxes, long ld, const float* inv_hi, const float* inv_lo, void* out, long rows, int dim, int dtype,
                              void* hip_stream);
int lwdetr_sine_embed_backward(const void* boxes, long ld, const float* inv_hi, const float* inv_lo, const void* grad_out, void* grad_boxes,
                               long rows, int dim, int dtype, void* hip_stream);
int lwdetr_train_glue_path_counts(long* out, int n);
const char* lwdetr_train_glue_path_name(int i);

/* Stochastic depth on a ViT residual under training (drop_path.hip; reference models/backbone/vit.py:216-220 with timm's DropPath).
 * lwdetr_drop_path_forward: out[r, c] = x[r, c] + (gamma[c] * y[r, c]) * scale[r / rows_per_group] for r < rows, c < C. scale is f32 with
 *   rows / rows_per_group entries, each 0 (the group is dropped) or 1 / keep. x and out are in dtype dx, y in dtype dy, gamma f32; every tensor
 *   has its own leading dimension (elements, at least C). f32 arithmetic in exactly that order, one rounding to dx; in f32 the result is the
 *   bits of torch's x + (gamma * y) * t. gamma == NULL is the plain x + y * scale. 16-byte accesses when C, the leading dimensions and the
 *   pointers allow whole 16-byte chunks, element accesses otherwise. A group whose scale is 0 copies x and does not read y: a non-finite y in a
 *   dropped group does not propagate, where the reference's NaN * 0 would.
 * lwdetr_drop_path_backward: grad_out (dx) -> grad_y (dy) = (grad_out * scale) * gamma and grad_gamma[c] (f32) = sum_r (grad_out * scale) * y,
 *   in that order; grad_x is grad_out itself and is not written. Either of grad_y / grad_gamma may be NULL (not both); y is read only for
 *   grad_gamma, which needs gamma and ws. Every workgroup (16 rows) writes one partial per channel into ws
 *   (lwdetr_drop_path_workspace_floats(rows, C) floats) and a second kernel adds them in one fixed order (16 interleaved slices of the
 *   workgroups, each ascending, then the slices in order). No floating-point atomic:
 *   a second call returns the same bits. A dropped group writes zeros to grad_y and reads neither grad_out nor y.
 * (dx, dy) in {(0,0), (1,1), (2,2), (0,1), (0,2)}; the last two are what 16-bit autocast hands over. rows == 0 launches nothing.
 * LWDETR_ERR_UNSUPPORTED: any other dtype pair, C above 2048. LWDETR_ERR_BAD_ARG, before anything is launched: C < 1, rows < 0,
 * rows_per_group < 1, rows not a multiple of rows_per_group, a null pointer (gamma excepted, and the backward's optional ones as above), a
 * leading dimension below C, a pointer not aligned to its element, a workspace that is too small, more than 2^31 - 1 workgroups.
 * lwdetr_drop_path_check answers what the entry would answer before launching and touches no device: backward == 0 with (a, b) = (x, out),
 * backward != 0 with (a, b) = (grad_out, grad_y).
 * Launch-form record as lwdetr_msda_path_counts: dp_fwd_<dx>_<dy>, dp_bwd_<dx>_<dy>; <dx>_<dy> in {f32_f32, f16_f16, bf16_bf16, f32_f16,
 * f32_bf16}. The backward counts once, with or without its second kernel. */
int lwdetr_drop_path_forward(const void* x, long ldx, const void* y, long ldy, const float* gamma, const float* scale, void* out, long ldo,
                             long rows, int C, long rows_per_group, int dx, int dy, void* hip_stream);
long lwdetr_drop_path_workspace_floats(long rows, int C);
int lwdetr_drop_path_backward(const void* grad_out, long ldg, const void* y, long ldy, const float* gamma, const float* scale, void* grad_y,
                              long ldgy, float* grad_gamma, float* ws, long ws_floats, long rows, int C, long rows_per_group, int dx, int dy,
                              void* hip_stream);
int lwdetr_drop_path_check(int backward, const void* a, long lda, const void* y, long ldy, const float* gamma, const float* scale, const void* b,
                           long ldb, const float* grad_gamma, const float* ws, long ws_floats, long rows, int C, long rows_per_group, int dx,
                           int dy);
int lwdetr_drop_path_path_counts(long* out, int n);
const char* lwdetr_drop_path_path_name(int i);

/* The same record for mlp.hip: one counter per kernel instantiation that lwdetr_mlp_fused / lwdetr_vit_block_few / lwdetr_ffn_partial can launch -
 * mlp_{f16,bf16,f32}_c{192,384}_proj{0,1}_qkv{0,1} (mlp_kernel in ViT mode; proj0_qkv1 does not exist: refused), mlp_small_{f16,bf16}_tt{1,2}_qkv{0,1}_frag{0,1}
 * (the few-token kernel: 16- / 32-token workgroups, row-major weights through lwdetr_mlp_fused / fragment-major through lwdetr_vit_block_few),
 * mlp_small_f32_tt1_qkv{0,1}_frag1, vit_few384_{f16,bf16}_qkv{0,1} (counted where lwdetr_vit_block_few hands over to vit_block_few384_kernel),
 * ffn_{f16,bf16}_c{256,384} (mlp_kernel in FFN mode). lwdetr_ffn_splits is a query and counts nothing. */
int lwdetr_mlp_path_counts(long* out, int n);
const char* lwdetr_mlp_path_name(int i);

/* The same record for chain.hip: one counter per kernel instantiation that lwdetr_enc_chain / lwdetr_row_chain can launch, 24 in all -
 * enc_{f16,bf16}_{d256_pf1,d256_pf0,d384_pf0}_{narrow,wide} (enc_chain_kernel / enc_chain_kernel_wide: pf1 = the cv2 stage in front, k5 = 640;
 * narrow up to 96 classes, wide up to 384), row_{f16,bf16}_d256_{k512,res0_q0,res1_q0,res1_q1} (the row-per-wave mlp_chain_kernel: k_in = 2 D, or by
 * whether `res` / `qpos` pointers are GIVEN, used by a stage or not), split_{f16,bf16}_d{256,384} (the channel-split mlp_chain_split_kernel). */
int lwdetr_chain_path_counts(long* out, int n);
const char* lwdetr_chain_path_name(int i);
long lwdetr_vit_block_stream_bytes(int C, int has_qkv);
long lwdetr_vit_block_vec_floats(int C);
int lwdetr_vit_block(void* x, long ldx, const void* att, long ldatt, const void* wstream, const float* vec, void* out2,
                     long ld2, float* stats_out, long M, int C, float eps, float eps_next, int has_qkv, void* q_out,
                     void* k_out, void* vt_out, float qscale, int heads, int hd, int Tp, int dtype, void* hip_stream);

/* ---- row-local chains of Linear stages in one launch (round 4; 16-bit dtypes) ------------------------------------------
 * lwdetr_enc_chain: everything the forward does to ALL S encoder tokens between the projector's C2f block and the two-stage
 * top-k, one launch: [k5 != 0: C2f.cv2 1x1 convolution (BatchNorm folded) + SiLU + channel LayerNorm -> `memory`
 * (models/backbone/projector.py:117-132, :21-47)] -> value_proj of all `nl` decoder layers with the padding mask on the OUTPUT
 * rows (models/ops/modules/ms_deform_attn.py:110-114) -> enc_output Linear on the rows with invalid proposals zeroed +
 * enc_output_norm -> output_memory `om` (models/transformer.py:113-116, :231) -> enc_out_class_embed -> class logits `cls`
 * (row stride ld_cls >= 96, columns >= ncls are zero weight pads) and their row maximum `cls_max` (f32; :244-246).
 * in: k5 != 0: (M, ld_in) rows holding the k5 = 5 * d / 2 channels of the C2f concat of one level, image b = row / npix,
 * destination row b * S + lsi + row % npix of the (total_rows, D) tensors; k5 == 0: `memory` rows themselves (npix = S, lsi = 0).
 * wstream / vec: lwdetr_amd.kernels.pack_enc_chain (4 KB pieces of 32 output channels x 64 k-slots in MFMA lane order, consumption
 * order cv2 | values | enc_output | class, + 2 zero pieces; f32 vectors [b2 | ln_w | ln_b] | b_enc | g_enc | be_enc | b_cls[96] | b_val);
 * sizes from the helpers. D in {256, 384}; k5 in {0, 640 (D = 256)}.
 * Class count: 1 <= ncls <= 96 is the form above (3 class tiles of 32 columns). 96 < ncls <= 384 (Objects365: 366) takes the wide kernels
 * (12 class tiles): the class weight and bias of the stream / vec are zero-padded to 384 rows (b_cls[384]; pack_enc_chain does it by the
 * class count), `cls` has a row stride ld_cls >= 384 (ld_cls % 8 == 0 in both forms), columns [ncls, 384) are written as zeros and the row
 * maximum runs over columns < ncls only. lwdetr_enc_chain_class_cols(ncls) = 96 or 384 is that column count (LWDETR_ERR_BAD_ARG for
 * ncls < 1 or > 384); the _cls helpers give the sizes for a class count and equal the two older ones up to 96 classes (those keep the
 * narrow form's values). A class count / ld_cls that do not fit are LWDETR_ERR_BAD_ARG before any launch, as every other argument rule;
 * the 2 GB range of the row tensors (LWDETR_ERR_UNSUPPORTED) counts the real ld_cls.
 * Also LWDETR_ERR_BAD_ARG before any launch: an input row stride shorter than the row, ld_in < (k5 ? k5 : D); a launch whose largest memory row
 * ((M - 1) / npix) * S + lsi + (M - 1) % npix is not below total_rows (rowvalid / notpad / cls_max are indexed by that row); a null or not 16-byte
 * aligned values[i], i < nl (`values` is a HOST array; it is read once every other rule has passed).
 * lwdetr_enc_chain_check: the argument checks of lwdetr_enc_chain alone - what it would answer before launching (LWDETR_OK: it would
 * launch, or M == 0); no device call, no device pointer is dereferenced; the host array `values` is read (entries [0, nl), after every other rule
 * has passed) and the check answers for them as the entry does. Both read it guarded: a `values` address that cannot be read is
 * LWDETR_ERR_BAD_ARG from either, never a fault. */
long lwdetr_enc_chain_vec_floats(int D, int k5);
long lwdetr_enc_chain_pieces(int D, int k5, int nl);
long lwdetr_enc_chain_class_cols(int ncls);
long lwdetr_enc_chain_vec_floats_cls(int D, int k5, int ncls);
long lwdetr_enc_chain_pieces_cls(int D, int k5, int nl, int ncls);
int lwdetr_enc_chain_check(const void* in, long ld_in, int k5, void* memory, void* om, void* cls, long ld_cls, float* cls_max,
                           void* const* values, int nl, const unsigned char* rowvalid, const unsigned char* notpad,
                           const void* wstream, const float* vec, long M, int D, int npix, int S, int lsi, long total_rows,
                           int ncls, int dtype);
int lwdetr_enc_chain(const void* in, long ld_in, int k5, void* memory, void* om, void* cls, long ld_cls, float* cls_max,
                     void* const* values, int nl, const unsigned char* rowvalid, const unsigned char* notpad,
                     const void* wstream, const float* vec, long M, int D, int npix, int S, int lsi, long total_rows,
                     int ncls, float eps_p, float eps_e, int dtype, void* hip_stream);

/* lwdetr_row_chain: a run-time program of up to 6 Linear stages over rows that never mix (16-bit dtypes, D in {256, 384}); replaces
 * the decoder's small GEMM + LayerNorm launches: self_attn.out_proj + residual + norm1 (+ `tgt + query_pos` -> sampling_offsets |
 * attention_weights Linear), cross_attn.output_proj + residual + norm2 (models/transformer.py:498-506, ms_deform_attn.py:117-123,
 * :142), bbox_embed / class_embed on all decoder layers (models/lwdetr.py:149-159), enc_out_bbox_embed on the selected rows
 * (transformer.py:236-240), ref_point_head (transformer.py:28-39, :352-355).
 *   FULL stage: y = W x + b (+ `res` rows when RES) (ReLU) -> rounded -> (LayerNorm(eps) with affine -> rounded) (-> stored to `out`,
 *               row stride ldo) -> the operand of the following stages (+ `qpos` rows, rounded, when ADDQ); N = D; stage 0 may
 *               contract over k_in = 2 D input channels.
 *   SIDE stage: out[:, 0:n] = W x + b from the current operand (row stride ldo >= ceil4(n); columns up to ceil4(n) are written).
 * in (M, ld_in): k_in channels per row. wstream / vec: lwdetr_amd.kernels.pack_row_chain - 4 KB pieces (32 output channels x 64
 * k-slots in MFMA lane order), stage after stage, + 2 zero pieces; f32 vectors stage after stage: bias (D, or 32 * ceil(n / 32) for a
 * SIDE stage), then gamma (D), beta (D) when LN.
 * Row strides: ld_in >= k_in, and ld_res >= D / ld_q >= D for a `res` / `qpos` that is given (all D channels of such a row are loaded whether a stage
 * uses them or not), each a multiple of 8 with a 16-byte aligned pointer; anything else is LWDETR_ERR_BAD_ARG before any launch. These rules on
 * in / res / qpos are checked in front of the M == 0 return (LWDETR_OK, nothing launched): they refuse whatever M is. The per-stage rules
 * (out, ldo, flags) are checked after it, so with M == 0 they are not. */
enum { LWDETR_CHAIN_FULL = 0, LWDETR_CHAIN_SIDE = 1 };
enum { LWDETR_CHAIN_RES = 1, LWDETR_CHAIN_RELU = 2, LWDETR_CHAIN_LN = 4, LWDETR_CHAIN_STORE = 8, LWDETR_CHAIN_ADDQ = 16 };
typedef struct { int kind; int n; int flags; float eps; void* out; long ldo; } lwdetr_chain_stage;
typedef struct {
    const void* in; long ld_in; int k_in;
    const void* res; long ld_res;
    const void* qpos; long ld_q;
    const void* wstream; const float* vec;
    long M; int D; int nst;
    lwdetr_chain_stage st[6];
} lwdetr_chain_desc;
long lwdetr_row_chain_pieces(const lwdetr_chain_desc* desc);
long lwdetr_row_chain_vec_floats(const lwdetr_chain_desc* desc);
int lwdetr_row_chain(const lwdetr_chain_desc* desc, int dtype, void* hip_stream);

/* norm1 + QKV of a ViT block on its own (block 0, which has no block kernel in front of it; models/backbone/vit.py:199, :123-130):
 * q (pre-scaled by qscale), k as (B, heads, Tp, hd), v^T as (B, heads, hd, Tp) from the rows x (M, ldx). wstream / vec:
 * lwdetr_amd.kernels.pack_vit_qkv (3 C / 32 pieces of 32 features x C in natural k order, LayerNorm affine folded; f32 bias).
 * C in {192, 384}, 16-bit dtypes, M % Tp == 0, Tp % 8 == 0, hd a power of two >= 8. */
long lwdetr_vit_qkv_stream_bytes(int C);
long lwdetr_vit_qkv_vec_floats(int C);
int lwdetr_vit_qkv(const void* x, long ldx, const void* wstream, const float* vec, long M, int C, float eps, void* q_out,
                   void* k_out, void* vt_out, float qscale, int heads, int hd, int Tp, int dtype, void* hip_stream);

/* The ViT stem in one launch (round 4): x0 = patches Wpe^T + b + pos - the 16 x 16 / stride 16 patch embedding of the NCHW image plus
 * the absolute position embedding (models/backbone/vit.py:353-358, the PatchEmbed Conv2d) - stored to x (M, ldx) as the residual
 * stream, and norm1 + QKV of block 0 from the registers (vit.py:199, :123-130; outputs as lwdetr_vit_qkv). img: (B, 3, 16 Hp, 16 Wp) of
 * the model dtype; rows of x are the window-major tokens of layout (Hp, Wp, Twp) (pad rows: zero pixels), M = B * 16 * Twp; pos:
 * (16 Twp, ldpos) of the model dtype in the same token order. wstream / vec: lwdetr_amd.kernels.pack_vit_stem. Replaces the
 * PATCH16 lwdetr_gemm + lwdetr_vit_qkv pair; same rounding points (x0 rounded once from f32). C in {192, 384}, 16-bit dtypes. */
long lwdetr_vit_stem_stream_bytes(int C);
long lwdetr_vit_stem_vec_floats(int C);
int lwdetr_vit_stem(const void* img, int B, int img_h, int img_w, int Hp, int Wp, int Twp, const void* pos, long ldpos, void* x,
                    long ldx, const void* wstream, const float* vec, long M, int C, float eps, void* q_out, void* k_out,
                    void* vt_out, float qscale, int heads, int hd, int dtype, void* hip_stream);

/* ---- fused glue of the two-stage selection / decoder set-up (reference models/transformer.py:236-276, :42-68, :352-355;
 * models/lwdetr.py:150-155, :168-170). idx (B,nq) int64 = two-stage top-k; props (B,S,4) f32 anchor proposals. ---- */
/* om (B,S,d), enc_cls (B*S rows, row stride ldc >= ncls) -> om_sel (B,nq,d), logits_out (B,nq,ncls), props_sel (B,nq,4): pure copies of
 * row b * S + idx[b,q]. LWDETR_ERR_BAD_ARG for B, S, d, nq or ncls <= 0 and for ldc < ncls. */
int lwdetr_select_gather(const void* om, const void* enc_cls, long ldc, const float* props, const int64_t* idx,
                         void* om_sel, void* logits_out, float* props_sel, int B, int S, int d, int nq, int ncls,
                         int dtype, void* hip_stream);
/* enc_delta (B*nq,4): bbox-MLP output of the selected rows; writes enc boxes (B,nq,4), decoder reference boxes ref_out
 * (B,nq,4) f32, the (y,x,w,h) sine embedding of ref * valid_ratio[level 0] (B*nq, 2d) and the broadcast queries (B*nq, d).
 * valid_ratios (B,L,2) (x,y). LWDETR_ERR_BAD_ARG for B, nq, d or L <= 0 and for an odd d. */
int lwdetr_decoder_inputs(const void* enc_delta, const float* props_sel, const float* refpoint, const float* valid_ratios,
                          int L, const void* query_feat, const float* dim_t, void* enc_boxes_out, float* ref_out,
                          void* sine_out, void* xdec_out, int B, int nq, int d, int dtype, void* hip_stream);
/* out[r] = (delta_xy * ref_wh + ref_xy, exp(delta_wh) * ref_wh) with ref row r % ref_rows (no sigmoid: bbox_reparam). */
int lwdetr_box_reparam(const void* delta, const float* ref, long ref_rows, void* out, long R, int dtype, void* hip_stream);
/* lwdetr_box_reparam into coord_out AND logits_out (R, ncls) contiguous = logits_pad (R rows, row stride ldc)[:, :ncls]: the
 * user-visible pred_boxes / pred_logits of all decoder layers (models/lwdetr.py:150-173) in one launch. Input row
 * layer * ref_rows + k is written to output row layer * out_layer_rows + k (out_layer_rows >= ref_rows; 0 = ref_rows, i.e.
 * contiguous): a call that owns images [b0, b0 + B) of a (layers, B_total, nq, .) tensor passes the pointers of row b0 * nq and
 * out_layer_rows = B_total * nq. logits_out and logits_pad must NOT overlap (the kernel reads one and writes the other without ordering
 * between threads): logits_out == logits_pad is refused with LWDETR_ERR_BAD_ARG, as are ncls <= 0, ldc < ncls, out_layer_rows < ref_rows. */
int lwdetr_finalize_outputs(const void* delta, const float* ref, long ref_rows, void* coord_out, long R, const void* logits_pad,
                            long ldc, int ncls, void* logits_out, long out_layer_rows, int dtype, void* hip_stream);

/* ---- sorted top-k (one workgroup per image) and its two users -----------------------------------------------------
 * Order: descending value, equal values by ascending index (torch.topk leaves tie order unspecified). N < 2^20, K <= 1024.
 * lwdetr_rowmax : out[r] = max(x[r, 0:ncols]) in f32 - the class-max of the encoder logits (transformer.py:246).
 * lwdetr_topk   : x (B,N) contiguous -> idx_out (B,K) int64 (+ val_out (B,K) f32 when non-NULL); replaces
 *                 torch.topk(..., num_queries, dim=1) of the two-stage selection (transformer.py:247).
 * lwdetr_postprocess : PostProcess.forward (models/lwdetr.py:509-540): logits (B,nq,ncls) and boxes (B,nq,4 cxcywh)
 *                 contiguous in `dtype`, target_sizes (B,2) f32 rows (h,w) -> scores (B,K) f32 = sigmoid of the K largest
 *                 logits, labels (B,K) int64 = flat index % ncls, out_boxes (B,K,4) f32 xyxy in pixels. ---- */
int lwdetr_rowmax(const void* x, long ld, long rows, int ncols, float* out, int dtype, void* hip_stream);
int lwdetr_topk(const void* x, int B, int N, int K, int64_t* idx_out, float* val_out, int dtype, void* hip_stream);
int lwdetr_postprocess(const void* logits, const void* boxes, const float* target_sizes, int B, int nq, int ncls, int K,
                       float* scores, int64_t* labels, float* out_boxes, int dtype, void* hip_stream);
/* Same selection, written as the (B, K, 6) f32 record of the detection all-gather: score, label, x0, y0, x1, y1
 * (replaces the pickled per-image dicts of util/misc.py:99-139; labels < 2^24 are exact in f32). */
int lwdetr_postprocess_packed(const void* logits, const void* boxes, const float* target_sizes, int B, int nq, int ncls, int K,
                              float* packed, int dtype, void* hip_stream);

/* ---- evaluation criterion: Hungarian matcher and losses, inference only (models/matcher.py:50-111, models/lwdetr.py:256-455) ----
 * One call serves every "layer" of a criterion call (final, aux 0..n, enc; at most LWDETR_CRIT_MAX_LAYERS) through a HOST array of
 * descriptors: logits (B,nq,C) and boxes (B,nq,4 cxcywh) contiguous in `dtype`, converted to f32 on load. Targets arrive packed:
 * labels (sumT) int64 in [0, C) (out-of-range labels are clamped for the load), tboxes (sumT,4) f32 cxcywh, offsets (B+1) int32 on the
 * DEVICE = prefix sums of the per-image target counts; counts (B) int32 on the HOST are the same counts, from which the entries size
 * their launches (a kernel that finds offsets and counts in disagreement writes nothing for that image and sets status 2).
 * lwdetr_match_cost     : cost[layer][off_b + t][q] = w_bbox L1 + w_class (pos - neg) + w_giou (-GIoU) in f32, in the reference's operation
 *                         order (matcher.py:71-94, util/box_ops.py:21-25, :36-73), only an image's own targets; cost (layers, sumT, nq) f32.
 * lwdetr_match_assign   : rectangular linear assignment per (layer, image): shortest augmenting paths with f64 duals (the algorithm and the
 *                         optimum of scipy.optimize.linear_sum_assignment), one wave per problem. nq <= LWDETR_MATCH_MAX_NQ, T_b <= nq
 *                         (else LWDETR_ERR_UNSUPPORTED). Every loop's trip count is fixed by T_b and nq, so non-finite costs terminate
 *                         too. idx_q / idx_t (layers, sumT) int64: the T_b pairs of image b at [layer][off_b ...], ascending in the query
 *                         index (scipy's row order), idx_t local to the image. status (layers, B) int32: non-zero when the problem saw a
 *                         non-finite cost (1) or inconsistent offsets (2). steps (layers, B) int32 or NULL: shortest-path steps taken.
 * lwdetr_match_assign_host : the same solver instantiated for the host (the lanes of the wave emulated) on a HOST cost matrix (T, nq).
 * lwdetr_criterion_partials: per (layer, image, chunk of LWDETR_CRIT_QCHUNK queries) the f32 sums {loss_ce terms, |box - target|,
 *                         1 - GIoU, rows whose arg-max is not the last class, matched rows whose arg-max is the label}; the matched
 *                         (b, q) -> target map is rebuilt per chunk from the assignment. loss_form 0 = sigmoid focal loss
 *                         (lwdetr.py:330-339, :458-483), 1 = IA-BCE (lwdetr.py:266-290). partials: lwdetr_criterion_partials_floats() f32.
 * lwdetr_criterion_finish: adds the partials in a fixed order in f64 and writes out (layers, 5) f32 = loss_ce, class_error (layers with
 *                         descriptor.class_error != 0, else 0), loss_bbox, loss_giou, cardinality_error. No floating-point atomics. */
#define LWDETR_CRIT_MAX_LAYERS 8
#define LWDETR_MATCH_MAX_NQ 1024
#define LWDETR_CRIT_QCHUNK 32
typedef struct {
    const void* logits;
    const void* boxes;
    int class_error;
    int reserved;
} lwdetr_crit_layer;
int lwdetr_match_cost(const lwdetr_crit_layer* layers, int nlayers, int B, int nq, int C, const int64_t* labels, const float* tboxes,
                      const int32_t* offsets, const int32_t* counts, float w_class, float w_bbox, float w_giou, float alpha, float* cost,
                      int dtype, void* hip_stream);
int lwdetr_match_assign(const float* cost, const int32_t* offsets, const int32_t* counts, int nlayers, int B, int nq, int64_t* idx_q,
                        int64_t* idx_t, int32_t* status, int32_t* steps, void* hip_stream);
int lwdetr_match_assign_host(const float* cost, int nq, int T, int64_t* idx_q, int64_t* idx_t, int32_t* status, int32_t* steps);
long lwdetr_criterion_partials_floats(int nlayers, int B, int nq);
int lwdetr_criterion_partials(const lwdetr_crit_layer* layers, int nlayers, int B, int nq, int C, const int64_t* labels,
                              const float* tboxes, const int32_t* offsets, const int32_t* counts, const int64_t* idx_q,
                              const int64_t* idx_t, int loss_form, float alpha, float* partials, int dtype, void* hip_stream);
int lwdetr_criterion_finish(const float* partials, const lwdetr_crit_layer* layers, const int32_t* offsets, const int32_t* counts,
                            int nlayers, int B, int nq, int loss_form, float num_boxes, float* out, void* hip_stream);

/* ---- training criterion: grouped matching, four loss forms, gradients (models/lwdetr.py:218-506 in train() mode, matcher.py:50-111) ----
 * The conventions of the evaluation criterion above hold (layer descriptors, packed targets, device offsets beside host counts).
 * `groups` = group_detr: nq % groups == 0, nq / groups <= LWDETR_MATCH_MAX_NQ and T_b <= nq / groups, checked on the host counts before
 * any launch (LWDETR_ERR_UNSUPPORTED otherwise). The cost matrix is lwdetr_match_cost's: a pair's cost does not depend on the group.
 * lwdetr_match_assign_groups : one wave per (layer, image, group) on the column slice [g nq/G, (g+1) nq/G) of the cost; the solver, trip
 *                         counts and non-finite-cost guarantee of lwdetr_match_assign. idx_q / idx_t (layers, groups, sumT) int64: the T_b
 *                         pairs of image b and group g at [layer][g][off_b ...], query indices global (offset by g nq/G) and ascending
 *                         inside the group. status / steps (layers, B, groups) int32 (steps may be NULL).
 * lwdetr_criterion_train_partials / _finish : as lwdetr_criterion_partials / _finish with groups and loss_form 0 = sigmoid focal loss,
 *                         1 = IA-BCE, 2 = varifocal (lwdetr.py:313-328, :486-494), 3 = position-supervised (:292-311, :497-506; the
 *                         per-image normaliser is the image's largest matched IoU over all groups, taken inside the partials launch).
 *                         partials: lwdetr_criterion_partials_floats() f32. class_error is over the groups * sumT matched rows,
 *                         cardinality_error counts all nq rows against T_b. With groups = 1 and forms 0 / 1 the values are those of
 *                         lwdetr_criterion_partials / _finish.
 * lwdetr_criterion_backward : one launch for all layers. grad_out (layers, 5) f32 on the DEVICE is the gradient with respect to _finish's
 *                         `out`; `grads` mirrors `layers` (logits = d/d logits (B,nq,C), boxes = d/d boxes (B,nq,4), in `dtype`, written
 *                         through the const pointers; class_error ignored). Every element of every gradient is written exactly once;
 *                         box gradients of unmatched queries are zero. 1 / num_boxes and mean(1) * nq are applied in the kernel. The
 *                         graph differentiated is the reference's: IoU targets and IA-BCE's t are constants, the modulating weights are not.
 * lwdetr_criterion_grad_host : the same per-element and per-pair derivative functions on HOST arrays for one image: logits (nq, C) and
 *                         boxes (nq, 4) f32, labels (T), tboxes (T, 4), `npairs` pairs (idx_q, idx_t; idx_t local), grad_out (5) on the
 *                         host; writes grad_logits (nq, C) and grad_boxes (nq, 4) f32. */
#define LWDETR_LOSS_FOCAL 0
#define LWDETR_LOSS_IA_BCE 1
#define LWDETR_LOSS_VARIFOCAL 2
#define LWDETR_LOSS_POSITION_SUPERVISED 3
int lwdetr_match_assign_groups(const float* cost, const int32_t* offsets, const int32_t* counts, int nlayers, int B, int nq, int groups,
                               int64_t* idx_q, int64_t* idx_t, int32_t* status, int32_t* steps, void* hip_stream);
int lwdetr_criterion_train_partials(const lwdetr_crit_layer* layers, int nlayers, int B, int nq, int C, const int64_t* labels,
                                    const float* tboxes, const int32_t* offsets, const int32_t* counts, const int64_t* idx_q,
                                    const int64_t* idx_t, int groups, int loss_form, float alpha, float* partials, int dtype,
                                    void* hip_stream);
int lwdetr_criterion_train_finish(const float* partials, const lwdetr_crit_layer* layers, const int32_t* offsets, const int32_t* counts,
                                  int nlayers, int B, int nq, int groups, int loss_form, float num_boxes, float* out, void* hip_stream);
int lwdetr_criterion_backward(const lwdetr_crit_layer* layers, const lwdetr_crit_layer* grads, int nlayers, int B, int nq, int C,
                              const int64_t* labels, const float* tboxes, const int32_t* offsets, const int32_t* counts,
                              const int64_t* idx_q, const int64_t* idx_t, int groups, int loss_form, float alpha, float num_boxes,
                              const float* grad_out, int dtype, void* hip_stream);
int lwdetr_criterion_grad_host(const float* logits, const float* boxes, int nq, int C, const int64_t* labels, const float* tboxes, int T,
                               const int64_t* idx_q, const int64_t* idx_t, int npairs, int loss_form, float alpha, float num_boxes,
                               const float* grad_out, float* grad_logits, float* grad_boxes);

/* ---- COCO box evaluator: pycocotools' COCOeval for iouType 'bbox' (the class behind datasets/coco_eval.py:26-78, :219-264; the reference's
 * engine.py:104-105, :145-163 drives it). All geometry and curve arithmetic is f64 in COCOeval's operation order, FP contraction off.
 * The ground truth is packed once (lwdetr_coco_gt, a HOST struct of DEVICE pointers; HOST pointers for the _host form): image rows in
 * ascending image id, categories dense in ascending category id, the annotations of an image grouped by dense category with the dataset
 * order kept inside a group (COCO.getAnnIds / COCOeval._prepare). grp_off (n_images * n_cats + 1) int32 are the prefix offsets of the
 * (row, category) groups - grp_off[row * n_cats] is the image's own offset; box (n_ann, 4) f64 xywh; area (n_ann) f64 = the annotation's
 * `area` key; crowd (n_ann) uint8 = iscrowd; cat (n_ann) int32 dense category; cat_lut (lut_size) int32: category id -> dense index or -1.
 * max_group = the largest group, as the host counted it.
 * lwdetr_cocoeval_match : COCOeval.computeIoU + evaluateImg for one batch: dets (B, K, 6) f32 records (score, label, x0, y0, x1, y1),
 *     rows (B) int32 = the images' rows in the table (a row outside [0, n_images) keeps nothing). What it reproduces, trap by trap:
 *     - detection box -> xywh with w = x1 - x0, h = y1 - y0 IN f32 (convert_to_xywh runs on the f32 tensor, coco_eval.py:176-178), then
 *       everything f64; detection area = w * h in f64 (COCO.loadRes). Labels are category ids; an id outside the category list is dropped.
 *     - per (image, category): descending score, stable in the detection index (argsort(-score, kind='mergesort')), first 100 = maxDets[-1].
 *     - IoU as maskApi.c bbIou: w = min(dx+dw, gx+gw) - max(dx, gx), w <= 0 -> 0, same for h; i = w*h; u = da for a crowd gt, else
 *       da + ga - i with ga = gw*gh; i / u.
 *     - a gt is ignored when iscrowd is set or `area` is outside [lo, hi], BOTH ends inclusive (area 1024 is small and medium); the
 *       annotation's `ignore` key has no effect (_prepare overwrites it with iscrowd). gts are walked non-ignored first, stable.
 *     - greedy rule per threshold t, detections in score order: iou = min(t, 1 - 1e-10), m = -1; walk the gts; skip one already matched at
 *       t unless it is a crowd; stop at the first ignored gt once m is a non-ignored gt; skip when ious[d, g] < iou (STRICTLY less: an equal
 *       IoU moves the match to the later gt); else iou = ious[d, g], m = g. A matched detection inherits the gt's ignore flag; an unmatched
 *       one is ignored when its own area is outside the range.
 *     - iou_thrs (10) f64 on the HOST = np.linspace(.5, .95, 10), passed in, never recomputed. Area ranges are Params.areaRng.
 *     - "matched" means "has a gt". pycocotools tests the stored gt ID for truth (dtm == 0, cocoeval.py evaluateImg / accumulate), so an
 *       annotation with id 0 reads as unmatched there; that quirk is NOT reproduced.
 *     Out, per detection slot b * K + d: out_cat int32 dense category (-1: dropped - unknown label or rank >= 100), out_score f32,
 *     out_rank int32 rank inside its (image, category) list (-1: dropped), out_matched / out_ignored int64: bit (area * 10 + threshold).
 * lwdetr_cocoeval_match_host : the same per-(image, category) code instantiated for the host on HOST arrays, the lanes emulated.
 * lwdetr_cocoeval_npig : npig (n_cats, 4) int32 = non-ignored gts per (category, area range) over rows (n_rows) int32, the EVALUATED images,
 *     each listed once (accumulate's npig = count_nonzero(gtIg == 0)); zeroes npig first. Integer atomics.
 * lwdetr_cocoeval_curves : COCOeval.accumulate over the store ordered by (category, descending score, image id, in-image order) - the
 *     mergesort of accumulate over per-image lists concatenated in sorted image id order. seg_off (n_cats + 1) int64: the categories'
 *     segments. Per (category, area, maxDet in {1, 10, 100}, threshold), a detection taking part iff rank < maxDet: integer running tp / fp,
 *     rc = tp / npig, pr = tp / (fp + tp + 2.220446049250313e-16), the right-to-left running maximum of pr, and per recall threshold
 *     (rec_thrs (101) f64 on the HOST, ascending = np.linspace(0, 1, 101)) the first index with rc >= thr (searchsorted side 'left'):
 *     precision and score from that index, 0 when there is none; recall = rc[-1], 0 without detections. Groups with npig == 0 are not
 *     written: the caller pre-fills with -1. precision / scores (10, 101, n_cats, 4, 3) f64, recall (10, n_cats, 4, 3) f64.
 * Limits, LWDETR_ERR_UNSUPPORTED before any launch, never truncated: K <= LWDETR_COCOEVAL_MAX_DETS detections per image, max_group <=
 * LWDETR_COCOEVAL_MAX_GROUP annotations per (image, category), n_cats <= LWDETR_COCOEVAL_MAX_CATS. No entry synchronises with the host;
 * no floating-point atomics. */
#define LWDETR_COCOEVAL_MAX_DETS 1024
#define LWDETR_COCOEVAL_MAX_GROUP 256
#define LWDETR_COCOEVAL_MAX_CATS 1024
#define LWDETR_COCOEVAL_KEEP 100
#define LWDETR_COCOEVAL_NTHR 10
#define LWDETR_COCOEVAL_NAREA 4
#define LWDETR_COCOEVAL_NREC 101
typedef struct {
    const int32_t* grp_off;
    const double* box;
    const double* area;
    const uint8_t* crowd;
    const int32_t* cat;
    const int32_t* cat_lut;
    int n_images, n_cats, lut_size, n_ann, max_group, reserved;
} lwdetr_coco_gt;
int lwdetr_cocoeval_match(const lwdetr_coco_gt* gt, const float* dets, const int32_t* rows, int B, int K, const double* iou_thrs,
                          int32_t* out_cat, float* out_score, int32_t* out_rank, int64_t* out_matched, int64_t* out_ignored,
                          void* hip_stream);
int lwdetr_cocoeval_match_host(const lwdetr_coco_gt* gt, const float* dets, const int32_t* rows, int B, int K, const double* iou_thrs,
                               int32_t* out_cat, float* out_score, int32_t* out_rank, int64_t* out_matched, int64_t* out_ignored);
int lwdetr_cocoeval_npig(const lwdetr_coco_gt* gt, const int32_t* rows, int n_rows, int32_t* npig, void* hip_stream);
int lwdetr_cocoeval_curves(const int64_t* seg_off, const float* score, const int32_t* rank, const int64_t* matched, const int64_t* ignored,
                           const int32_t* npig, const double* rec_thrs, int n_cats, long n_store, double* precision, double* scores,
                           double* recall, void* hip_stream);

/* ---- training-step tail over many tensors: gradient clip, per-tensor AdamW, model EMA (engine.py:76-83: torch.nn.utils.clip_grad_norm_,
 * torch.optim.AdamW with one parameter group per parameter - util/get_param_dicts.py:53-70 -, util/utils.py:20-29 ModelEma) ----
 * Two tables in DEVICE memory describe the work (HOST memory for the _host forms and lwdetr_mt_check):
 *   lwdetr_mt_tensor, one record per tensor: p (the parameter / the model's buffer), g (gradient), m, v (exp_avg, exp_avg_sq), ema (the EMA
 *     copy's tensor), any of them NULL; numel; kind = LWDETR_MT_PARAM (f32: AdamW, and EMA where ema is set), LWDETR_MT_EMA_F32 (an f32 buffer,
 *     EMA only), LWDETR_MT_EMA_I64 (an int64 buffer, EMA only: p and ema are int64); skip != 0 for a parameter without a gradient this step;
 *     the f32 scalars the host computes in double and rounds once, as torch's non-capturable path does: decay_mul = 1 - lr * weight_decay
 *     (1 where weight_decay = 0), neg_step_size = -(lr / (1 - beta1^t)), bc2_sqrt = sqrt(1 - beta2^t).
 *   lwdetr_mt_chunk, one per piece of at most LWDETR_MT_CHUNK elements - the work of one wave -: tensor index, element offset, count. The
 *     chunks tile every tensor exactly once in table order (tensor ascending, offset ascending, every chunk but a tensor's last one full).
 * lwdetr_mt_check     : that rule on HOST copies of the tables, plus numel > 0, a known kind and element-aligned pointers; LWDETR_ERR_BAD_ARG
 *                       otherwise. The launch entries cannot read device tables: build the tables on the host, check them once, upload them.
 *                       Inside the kernels a chunk with a tensor index out of range or a range outside its tensor takes no part (never a
 *                       truncated or out-of-bounds access).
 * lwdetr_mt_sumsq     : partials[c] = f32 sum of g^2 over chunk c (0 for a record that is not PARAM, has skip set or no g); (nchunks) f32.
 * lwdetr_mt_norm_finish : one workgroup adds the partials in f64 in a fixed order; norm_clip (4) f32: [0] = total_norm = (f32) sqrt(sum),
 *                       [1] = clip_coef = min(1, max_norm / (total_norm + 1e-6)), the quotient in f64 from the unrounded norm, a NaN kept as
 *                       torch.clamp keeps it; [2] = the part of that f64 coefficient that f32 drops (0 when it clamps to 1); [3] = 0. The step
 *                       multiplies by [1] + [2] in one fused multiply-add: the clipped gradient is the correctly rounded product, where an
 *                       f32 coefficient alone costs an ulp that exp_avg_sq doubles. max_norm > 0.
 * lwdetr_mt_step      : one pass over the chunk table; every array it touches is read once and written once. flags:
 *     LWDETR_MT_SCALE_GRADS  g *= clip_coef in place (PARAM records with g, without skip). Alone only (LWDETR_ERR_UNSUPPORTED with others).
 *     LWDETR_MT_ADAMW        PARAM records with p, g, m, v and without skip: gc = g * clip_coef (norm_clip NULL: gc = g);
 *                            p *= decay_mul; m = lerp(m, gc, 1 - beta1); v = v * beta2 + (1 - beta2) * (gc * gc);
 *                            p += neg_step_size * (m / (sqrt(v) / bc2_sqrt + eps)). g is NOT written back.
 *     LWDETR_MT_EMA          every record with p and ema, after the AdamW update of the same element, from registers:
 *                            e = fl(fl(d e) + fl((1 - d) x)); LWDETR_MT_EMA_I64: (int64) trunc of the same on (float) e, (float) x.
 *     LWDETR_MT_EMA_SET      e = x (ModelEma.set). Not together with LWDETR_MT_EMA (LWDETR_ERR_BAD_ARG) or LWDETR_MT_ADAMW (UNSUPPORTED).
 *   hyper (a HOST struct, needed with ADAMW / EMA): the f32 roundings of the doubles 1 - beta1, beta2, 1 - beta2, eps, decay, 1. - decay.
 *   16-byte accesses where every array of a record that the launch touches is 16-byte aligned, element accesses otherwise.
 * lwdetr_mt_norm_host / lwdetr_mt_step_host : the same per-lane functions on HOST tables and arrays, lanes and reduction order emulated
 *                       (sumsq + finish in one call); they run lwdetr_mt_check first.
 * lwdetr_mt_launch_counts / _name : launches issued and accepted so far by the three device entries (mt_sumsq, mt_norm_finish, mt_step), in
 *                       the style of lwdetr_gemm_path_counts. LWDETR_ERR_BAD_ARG before any launch: null tables, counts <= 0, bad flags.
 * No entry synchronises with the host; no floating-point atomics. */
#define LWDETR_MT_CHUNK 1024
#define LWDETR_MT_PARAM 0
#define LWDETR_MT_EMA_F32 1
#define LWDETR_MT_EMA_I64 2
#define LWDETR_MT_SCALE_GRADS 1u
#define LWDETR_MT_ADAMW 2u
#define LWDETR_MT_EMA 4u
#define LWDETR_MT_EMA_SET 8u
typedef struct {
    void* p;
    void* g;
    void* m;
    void* v;
    void* ema;
    int64_t numel;
    int32_t kind;
    int32_t skip;
    float decay_mul;
    float neg_step_size;
    float bc2_sqrt;
    int32_t reserved;
} lwdetr_mt_tensor;
typedef struct {
    int32_t tensor;
    int32_t count;
    int64_t offset;
} lwdetr_mt_chunk;
typedef struct {
    float one_minus_beta1, beta2, one_minus_beta2, eps, ema_decay, ema_one_minus_decay;
} lwdetr_mt_hyper;
int lwdetr_mt_check(const lwdetr_mt_tensor* tensors, int ntensors, const lwdetr_mt_chunk* chunks, int nchunks);
int lwdetr_mt_sumsq(const lwdetr_mt_tensor* tensors, int ntensors, const lwdetr_mt_chunk* chunks, int nchunks, float* partials,
                    void* hip_stream);
int lwdetr_mt_norm_finish(const float* partials, int nchunks, double max_norm, float* norm_clip, void* hip_stream);
int lwdetr_mt_step(const lwdetr_mt_tensor* tensors, int ntensors, const lwdetr_mt_chunk* chunks, int nchunks, const lwdetr_mt_hyper* hyper,
                   unsigned flags, const float* norm_clip, void* hip_stream);
int lwdetr_mt_norm_host(const lwdetr_mt_tensor* tensors, int ntensors, const lwdetr_mt_chunk* chunks, int nchunks, double max_norm,
                        float* norm_clip);
int lwdetr_mt_step_host(const lwdetr_mt_tensor* tensors, int ntensors, const lwdetr_mt_chunk* chunks, int nchunks,
                        const lwdetr_mt_hyper* hyper, unsigned flags, const float* norm_clip);
int lwdetr_mt_launch_counts(long* out, int n);
const char* lwdetr_mt_launch_name(int i);

/* ---- input side: uint8 HWC -> Pillow-exact bilinear square resize -> ToTensor -> Normalize -> NCHW --
 * Replaces datasets/transforms.py:223-231 (SquareResize = PIL.Image.resize((S,S), BILINEAR)), :437-443 (Normalize) and
 * ToTensor (datasets/coco.py:127-130, deploy/benchmark.py:273-281). One descriptor per image (a DEVICE array):
 * src = uint8 RGB rows of `width` pixels, `row_stride` bytes apart; the *_off fields index `tables` (int32, device):
 * bounds = (first input index, tap count) per output column / row, coef = `ksize` 22-bit fixed-point taps per output
 * column / row (Pillow's precompute_coeffs + normalize_coeffs_8bpc, computed by the host); tmp_off = byte offset of this
 * image's height x S x 3 intermediate in `tmp`. lut = 3 x 256 floats, (v / 255 - mean[c]) / std[c]. out = (B,3,S,S). */
typedef struct {
    const uint8_t* src;
    int height, width;
    long row_stride;
    int xbounds_off, xcoef_off, xksize;
    int ybounds_off, ycoef_off, yksize;
    long tmp_off;
} lwdetr_resize_image;
int lwdetr_resize_normalize(const lwdetr_resize_image* images, int B, int max_height, const int32_t* tables, uint8_t* tmp,
                            const float* lut, void* out, int S, int dtype, void* hip_stream);

/* ---- training-time input transform (csrc/augment.hip): the reference's train recipes (datasets/coco.py:86-160 over
 * datasets/transforms.py) per image - RandomHorizontalFlip, then either one resize or RandomResize + RandomSizeCrop + a second
 * resize - then ToTensor + Normalize, and the zero padding + mask of nested_tensor_from_tensor_list (util/misc.py:317-339), for a
 * whole batch in at most four launches. Every resize is Pillow's ImagingResample as in lwdetr_resize_normalize (uint8 between passes
 * and between the two stages; a pass whose input and output lengths are equal is skipped). One descriptor per image:
 *   src / height / width / row_stride: uint8 RGB rows as in lwdetr_resize_image; flip != 0 reads source column width-1-x (whichever
 *     pass reads the source does it; no flipped copy exists);
 *   stage 1 = resize to (h1, w1), then the crop window (top, left, ch, cw) inside it - computed for the window only, with the taps of
 *     the full w1 / h1 axis at left + x and top + y. An image without a stage 1 carries (h1, w1) = (height, width) and the full window;
 *   stage 2 = resize of the (ch, cw) window to this image's own (oh, ow);
 *   row0 / rows: the source rows [row0, row0 + rows) that the stage-1 vertical pass reads for the window - the only rows the stage-1
 *     horizontal pass computes ((top, ch) when h1 == height);
 *     with bounds = the height -> h1 table they must be exactly row0 = bounds[top].first and row0 + rows = bounds[top + ch - 1].first +
 *     bounds[top + ch - 1].count. The entry cannot read the device tables: it checks the range against the image only, and a row0 above
 *     the first tap of row `top` would make the vertical pass read before its intermediate - the caller computes both from the table it
 *     uploads, as lwdetr_amd/augment.py does;
 *   bounds_off / coef_off / ksize [4]: the axis tables in `tables` (int32 elements, layout as lwdetr_resize_image) of width -> w1,
 *     height -> h1, cw -> ow, ch -> oh; an entry of a skipped pass is not read;
 *   scratch_off [3]: byte offsets into `scratch` of the uint8 intermediates rows x cw x 3 (after the stage-1 horizontal pass),
 *     ch x cw x 3 (after the stage-1 vertical pass) and ch x ow x 3 (after the stage-2 horizontal pass); unused ones are not touched.
 * The horizontal passes read the first and last bytes of a row span as whole aligned 32-bit words: the allocations behind `src` and
 * `scratch` start and end on 4-byte boundaries (device allocations do).
 * images_host and images_dev are the same B descriptors in host and in device memory: the host copy is checked and sizes the grids,
 * the kernels read the device copy. out = (B,3,Hc,Wc) in dtype 0 ... 2 and mask = (B,Hc,Wc) bytes (1 = padding) are written in full:
 * pixels outside an image's oh x ow are 0 with mask 1. LWDETR_ERR_BAD_ARG for a null pointer, B < 0, a non-positive size, a size above
 * 65535, row_stride < 3 * width, a zero-sized crop or one outside (h1, w1), (oh, ow) outside (Hc, Wc), source rows outside the image,
 * a table range outside [0, table_len) or a scratch range outside [0, scratch_bytes); nothing is launched then. B == 0 launches
 * nothing. */
typedef struct {
    const uint8_t* src;
    int height, width;
    long row_stride;
    int flip;
    int h1, w1;
    int top, left, ch, cw;
    int oh, ow;
    int row0, rows;
    int bounds_off[4], coef_off[4], ksize[4];
    long scratch_off[3];
} lwdetr_augment_image;
int lwdetr_augment_normalize(const lwdetr_augment_image* images_host, const lwdetr_augment_image* images_dev, int B,
                             const int32_t* tables, long table_len, uint8_t* scratch, long scratch_bytes, const float* lut,
                             void* out, uint8_t* mask, int Hc, int Wc, int dtype, void* hip_stream);

/* ---- run-time switches (tuning, A/B runs, tests). Every environment variable LWDETR_<NAME> that a launch path of this library looks at
 * (kernel choices and shapes: ATTN_LDS, ATTN_LDS_CFG, ATTN_SHORT, ATTN_WTILE, ATTN_WIN, ATTN_QT, CHAIN_SPLIT_ROWS, GEMM_BIG, GEMM_BIG_BN, GEMM_BIG_2WG,
 * CONV_PATCH, GEMM_TILE, GEMM_DMA, GEMM_KB, GEMM_NST, GEMM_PT, GEMM_PT_SKEW, MLP_SMALL_TT, FFN_SPLITS, MLP_SMALL, VB_GRID, VB_GELU16, VB_HALF, GEMM_FEW_WAVES) is read
 * ONCE per process into a table; no launch calls getenv. lwdetr_tuning_set overrides (is_set != 0) or clears (is_set == 0: back to the built-in
 * default, not to the environment) one entry by name, with or without the LWDETR_ prefix; LWDETR_ERR_BAD_ARG for an unknown name. Process-wide,
 * not synchronised with launches in flight on other threads. Results never depend on a switch beyond f32 summation order, except VB_GELU16
 * (DESIGN.md section 2). */
int lwdetr_tuning_set(const char* name, long value, int is_set);

/* ---- profiling: per-kernel HIP-event timing on the launch stream (off by default) ------------------------------ */
int lwdetr_prof_enable(int on);
int lwdetr_prof_num_kernels(void);
const char* lwdetr_prof_kernel_name(int kid);
int lwdetr_prof_collect(double* ms, double* flops, double* bytes, long long* count, int n);

#ifdef __cplusplus
}
#endif
#endif /* LWDETR_HIP_H */
