// Stand-alone driver of lwdetr_cocoeval_match_host for sanitizer runs (tools/cocoeval_sanitize.py builds csrc/cocoeval.hip and this file
// with -fsanitize=address,undefined on the host side and runs it on the generated set of tests/cocoeval_cases.py):
//   cocoeval_host_check IN OUT
// IN : int32 header {n_images, n_cats, lut_size, n_ann, max_group, B, K}, then grp_off, box, area, cat, cat_lut, rows, dets, iou_thrs, crowd
//      as raw arrays (exact sizes: a read or write one element past any of them is a heap overflow the sanitizer reports)
// OUT: out_cat, out_score, out_rank, out_matched, out_ignored as raw arrays
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
    int32_t h[7];
    if (fread(h, sizeof(int32_t), 7, f) != 7) return 2;
    const size_t n_img = h[0], n_cat = h[1], lut = h[2], n_ann = h[3], B = h[5], K = h[6];
    std::vector<int32_t> grp_off, cat, cat_lut, rows;
    std::vector<double> box, area, thr;
    std::vector<float> dets;
    std::vector<uint8_t> crowd;
    if (!rd(f, grp_off, n_img * n_cat + 1) || !rd(f, box, n_ann * 4) || !rd(f, area, n_ann) || !rd(f, cat, n_ann) || !rd(f, cat_lut, lut) ||
        !rd(f, rows, B) || !rd(f, dets, B * K * 6) || !rd(f, thr, LWDETR_COCOEVAL_NTHR) || !rd(f, crowd, n_ann)) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);
    lwdetr_coco_gt gt = {grp_off.data(), box.data(), area.data(), crowd.data(), cat.data(), cat_lut.data(), h[0], h[1], h[2], h[3], h[4], 0};
    std::vector<int32_t> o_cat(B * K), o_rank(B * K);
    std::vector<float> o_score(B * K);
    std::vector<int64_t> o_m(B * K), o_i(B * K);
    const int rc = lwdetr_cocoeval_match_host(&gt, dets.data(), rows.data(), (int)B, (int)K, thr.data(), o_cat.data(), o_score.data(),
                                              o_rank.data(), o_m.data(), o_i.data());
    if (rc != LWDETR_OK) { fprintf(stderr, "lwdetr_cocoeval_match_host: %d\n", rc); return 1; }
    FILE* o = fopen(argv[2], "wb");
    if (!o || !wr(o, o_cat) || !wr(o, o_score) || !wr(o, o_rank) || !wr(o, o_m) || !wr(o, o_i)) { perror(argv[2]); return 2; }
    fclose(o);
    printf("ok B=%zu K=%zu\n", B, K);
    return 0;
}
