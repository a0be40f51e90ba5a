// The C = 384 form of lwdetr_vit_block_few (vit_block_few384.hip): operand block and launcher, called by the entry in mlp.hip.
// A translation unit of its own so that the kernels of mlp.o stay instruction-identical; the operand block is a struct of its own (not mlp.hip's
// MlpParams, which lives in that file's anonymous namespace and is part of the mangled name of every kernel there).
#pragma once
#include <hip/hip_runtime.h>

struct VitFew384Params {
    void* x; long ldx;                 // in/out (M, 384)
    const void* att; long ldatt;       // attention output (M, 384)
    const void* wp; const float* bp; const float* gamma1;        // fragment-major projection weight, bias, LayerScale
    const void* w1; const float* b1;   // fragment-major fc1 (norm2 folded in, k-slot order), folded bias (1536)
    const void* w2p; const float* b2; const float* gamma2;       // chunk-major fc2 (48, 384, 32), bias, LayerScale
    void* out2; long ld2;              // optional tap copy
    float* stats_out;                  // optional (M, 2): mean, rstd of the new rows (eps_next)
    const void* wqkv; const float* bqkv; void* q; void* k; void* vt; float qscale; int heads, hd, Tp;   // optional chained norm1 + QKV of the next block
    long M; float eps, eps_next;
};

// dtype: DT_F16 / DT_BF16 (common.h). Arguments are checked by the caller. Returns an LWDETR_* code.
int lwdetr_vit_block_few384_launch(const VitFew384Params& p, int dtype, hipStream_t st);
