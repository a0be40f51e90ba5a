// Stand-alone driver of the training criterion's host entries for sanitizer runs (tools/criterion_train_sanitize.py builds csrc/match.hip,
// csrc/match_train.hip and this file with -fsanitize=address,undefined on the host side): the grouped solve - lwdetr_match_assign_host on the
// column slice of every group - and lwdetr_criterion_grad_host on the pairs it returns, for one image.
//   criterion_train_host_check IN OUT
// IN : int32 header {nq, C, T, G, form}, float header {alpha, num_boxes, grad_out[5]}, then logits (nq, C), boxes (nq, 4) f32, labels (T)
//      int64, tboxes (T, 4) f32, cost (T, nq) f32 target-major, as raw arrays (exact sizes: a read or write one element past any of them is
//      a heap overflow the sanitizer reports)
// OUT: idx_q, idx_t (G * T) int64, status, steps (G) int32, grad_logits (nq, C), grad_boxes (nq, 4) f32
#include <cstdint>
#include <cstdio>
#include <vector>
#include "lwdetr_hip.h"

template <typename T> static bool rd(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <typename T> static bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t h[5];
    float fh[7];
    if (fread(h, sizeof(int32_t), 5, f) != 5 || fread(fh, sizeof(float), 7, f) != 7) return 2;
    const int nq = h[0], C = h[1], T = h[2], G = h[3], form = h[4];
    if (nq < 1 || C < 1 || T < 0 || G < 1 || nq % G) { fprintf(stderr, "bad header\n"); return 2; }
    const int gw = nq / G;
    std::vector<float> logits, boxes, tboxes, cost;
    std::vector<int64_t> labels;
    if (!rd(f, logits, (size_t)nq * C) || !rd(f, boxes, (size_t)nq * 4) || !rd(f, labels, T) || !rd(f, tboxes, (size_t)T * 4) ||
        !rd(f, cost, (size_t)T * nq)) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);
    std::vector<int64_t> idx_q((size_t)G * T), idx_t((size_t)G * T);
    std::vector<int32_t> status(G), steps(G);
    std::vector<float> slice((size_t)T * gw);
    for (int g = 0; g < G; ++g) {
        for (int t = 0; t < T; ++t)
            for (int j = 0; j < gw; ++j) slice[(size_t)t * gw + j] = cost[(size_t)t * nq + (size_t)g * gw + j];
        const int rc = lwdetr_match_assign_host(slice.data(), gw, T, idx_q.data() + (size_t)g * T, idx_t.data() + (size_t)g * T, &status[g], &steps[g]);
        if (rc != LWDETR_OK) { fprintf(stderr, "lwdetr_match_assign_host: %d\n", rc); return 1; }
        for (int t = 0; t < T; ++t) idx_q[(size_t)g * T + t] += (int64_t)g * gw;
    }
    std::vector<float> gl((size_t)nq * C), gb((size_t)nq * 4);
    const int rc = lwdetr_criterion_grad_host(logits.data(), boxes.data(), nq, C, labels.data(), tboxes.data(), T, idx_q.data(), idx_t.data(), G * T,
                                              form, fh[0], fh[1], fh + 2, gl.data(), gb.data());
    if (rc != LWDETR_OK) { fprintf(stderr, "lwdetr_criterion_grad_host: %d\n", rc); return 1; }
    FILE* o = fopen(argv[2], "wb");
    if (!o || !wr(o, idx_q) || !wr(o, idx_t) || !wr(o, status) || !wr(o, steps) || !wr(o, gl) || !wr(o, gb)) { perror(argv[2]); return 2; }
    fclose(o);
    printf("ok nq=%d C=%d T=%d G=%d form=%d\n", nq, C, T, G, form);
    return 0;
}
