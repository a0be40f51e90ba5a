// Stand-alone driver of the training-step tail's host entries for sanitizer runs (tools/train_tail_sanitize.py builds csrc/optim.hip and this
// file with -fsanitize=address,undefined on the host side): lwdetr_mt_check, lwdetr_mt_norm_host and lwdetr_mt_step_host over tensors that
// are each an exact-size heap block - a read or write one element past any of them is a heap overflow the sanitizer reports.
//   train_tail_host_check IN OUT
// IN : int32 header {ntensors, flags, clip, steps}, float header {max_norm, 1 - beta1, beta2, 1 - beta2, eps, decay, 1 - decay}, then per tensor
//      int32 {numel, kind, skip, misalign} and float {decay_mul, neg_step_size, bc2_sqrt}, then per tensor its arrays: kind PARAM p, g, m, v, ema
//      (numel f32 each), EMA_F32 p, ema (f32), EMA_I64 p, ema (int64). misalign != 0 places every array of the tensor one element into its block
//      (a view at element offset 1: the element-wise path).
// OUT: norm_clip (4 f32, zeros without clip), then per tensor the same arrays after `steps` calls.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "lwdetr_hip.h"

struct Block {                       // an exact-size allocation; data() is `shift` elements in
    void* base = nullptr;
    size_t elem = 4, n = 0, shift = 0;
    void alloc(size_t elem_, size_t n_, size_t shift_) {
        elem = elem_; n = n_; shift = shift_;
        if (posix_memalign(&base, 16, (n + shift) * elem)) base = nullptr;
    }
    char* data() const { return static_cast<char*>(base) + shift * elem; }
    ~Block() { free(base); }
};

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t h[4];
    float fh[7];
    if (fread(h, sizeof(int32_t), 4, f) != 4 || fread(fh, sizeof(float), 7, f) != 7) return 2;
    const int nt = h[0], clip = h[2], steps = h[3];
    const unsigned flags = (unsigned)h[1];
    if (nt < 1 || steps < 1) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<lwdetr_mt_tensor> rec(nt);
    std::vector<int> mis(nt);
    for (int i = 0; i < nt; ++i) {
        int32_t th[4];
        float tf[3];
        if (fread(th, sizeof(int32_t), 4, f) != 4 || fread(tf, sizeof(float), 3, f) != 3 || th[0] < 1) { fprintf(stderr, "bad tensor header\n"); return 2; }
        memset(&rec[i], 0, sizeof(rec[i]));
        rec[i].numel = th[0]; rec[i].kind = th[1]; rec[i].skip = th[2]; mis[i] = th[3] != 0;
        rec[i].decay_mul = tf[0]; rec[i].neg_step_size = tf[1]; rec[i].bc2_sqrt = tf[2];
    }
    std::vector<Block> blocks((size_t)nt * 5);
    for (int i = 0; i < nt; ++i) {
        const bool param = rec[i].kind == LWDETR_MT_PARAM;
        const size_t elem = rec[i].kind == LWDETR_MT_EMA_I64 ? 8 : 4, n = (size_t)rec[i].numel;
        void** slots[5] = {&rec[i].p, &rec[i].g, &rec[i].m, &rec[i].v, &rec[i].ema};
        for (int a = 0; a < 5; ++a) {
            if (!param && a != 0 && a != 4) continue;
            Block& b = blocks[(size_t)i * 5 + a];
            b.alloc(elem, n, mis[i] ? 1 : 0);
            if (!b.base || fread(b.data(), elem, n, f) != n) { fprintf(stderr, "short input\n"); return 2; }
            *slots[a] = b.data();
        }
        if (param && rec[i].skip) rec[i].g = nullptr;            // a parameter whose grad is None
    }
    fclose(f);
    std::vector<lwdetr_mt_chunk> chunks;
    for (int i = 0; i < nt; ++i)
        for (int64_t off = 0; off < rec[i].numel; off += LWDETR_MT_CHUNK) {
            const int64_t left = rec[i].numel - off;
            chunks.push_back({i, (int32_t)(left < LWDETR_MT_CHUNK ? left : LWDETR_MT_CHUNK), off});
        }
    int rc = lwdetr_mt_check(rec.data(), nt, chunks.data(), (int)chunks.size());
    if (rc != LWDETR_OK) { fprintf(stderr, "lwdetr_mt_check: %d\n", rc); return 1; }
    const lwdetr_mt_hyper hyper = {fh[1], fh[2], fh[3], fh[4], fh[5], fh[6]};
    float norm_clip[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < steps; ++s) {
        if (clip) {
            rc = lwdetr_mt_norm_host(rec.data(), nt, chunks.data(), (int)chunks.size(), (double)fh[0], norm_clip);
            if (rc != LWDETR_OK) { fprintf(stderr, "lwdetr_mt_norm_host: %d\n", rc); return 1; }
        }
        rc = lwdetr_mt_step_host(rec.data(), nt, chunks.data(), (int)chunks.size(), &hyper, flags, clip ? norm_clip : nullptr);
        if (rc != LWDETR_OK) { fprintf(stderr, "lwdetr_mt_step_host: %d\n", rc); return 1; }
    }
    // a table that does not hold together is refused, and nothing is touched
    std::vector<lwdetr_mt_chunk> bad = chunks;
    bad.back().count += 1;
    if (lwdetr_mt_step_host(rec.data(), nt, bad.data(), (int)bad.size(), &hyper, flags, clip ? norm_clip : nullptr) != LWDETR_ERR_BAD_ARG) return 1;
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(norm_clip, sizeof(float), 4, o) != 4) { perror(argv[2]); return 2; }
    for (const Block& b : blocks)
        if (b.base && fwrite(b.data(), b.elem, b.n, o) != b.n) { perror(argv[2]); return 2; }
    fclose(o);
    printf("ok tensors=%d chunks=%zu flags=%u clip=%d steps=%d\n", nt, chunks.size(), flags, clip, steps);
    return 0;
}
