// Training-time input transform for gfx950: the reference's train recipes (datasets/coco.py:86-160 over datasets/transforms.py) for a
// whole batch - RandomHorizontalFlip, then either one resize or RandomResize + RandomSizeCrop + a second resize, then ToTensor + Normalize,
// and the zero padding + mask of nested_tensor_from_tensor_list (util/misc.py:317-339). The random draws are made on the host
// (lwdetr_amd/augment.py, in the reference's order); a descriptor carries one image's outcome.
//
// Every resize is Pillow's ImagingResample exactly as preproc.hip implements it (22-bit coefficients, accumulator seeded with 1 << 21,
// clip8(acc >> 22), horizontal pass first, uint8 between passes - and here between the two stages as well, because the reference
// materialises a PIL image after each step). Up to four passes per image, one launch per pass over all images:
//   1  stage-1 horizontal   source (flipped on the fly)              -> A = rows x cw x 3   only the crop window's columns, only the
//                                                                                           source rows the window's rows tap
//   2  stage-1 vertical     A (or the source, when pass 1 is skipped) -> B = ch x cw x 3     only the crop window's rows
//   3  stage-2 horizontal   the stage-1 window W1                     -> C = ch x ow x 3
//   4  stage-2 vertical     C (or W1, when pass 3 is skipped)         -> canvas (B,3,Hc,Wc) through the 3 x 256 table, + mask, + padding
// W1 is B, or A (pass 2 skipped: A holds exactly the window's rows), or the window of the flipped source (both skipped). A pass whose
// input and output lengths are equal is skipped, as in Pillow - its image returns at once - and whichever pass reads the source applies
// the flip by reading column width-1-x. Restricting stage 1 to the crop window is exact: an output pixel depends on its own taps only,
// and those are the taps of the full w1 / h1 axis at left + x / top + y. Pure byte / integer work, HBM-bound; x fastest in every pass.
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int ROUND = 1 << (PRECISION_BITS - 1);
enum { AX_X1 = 0, AX_Y1 = 1, AX_X2 = 2, AX_Y2 = 3, SC_A = 0, SC_B = 1, SC_C = 2 };

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// pixel (y, x) of a pass's input sits at p + y * pitch + sx * x * 3 (sx = -1: the flipped source)
struct View { const uint8_t* p; long pitch; int sx; };

__device__ __forceinline__ View source_view(const lwdetr_augment_image& im, int y0, int x0) {
    View v;
    v.p = im.src + (long)y0 * im.row_stride + (long)(im.flip ? im.width - 1 - x0 : x0) * 3;
    v.pitch = im.row_stride; v.sx = im.flip ? -1 : 1;
    return v;
}
__device__ __forceinline__ bool has_h1(const lwdetr_augment_image& im) { return im.w1 != im.width; }
__device__ __forceinline__ bool has_v1(const lwdetr_augment_image& im) { return im.h1 != im.height; }
__device__ __forceinline__ bool has_h2(const lwdetr_augment_image& im) { return im.ow != im.cw; }
__device__ __forceinline__ bool has_v2(const lwdetr_augment_image& im) { return im.oh != im.ch; }

// the stage-1 window (ch x cw), wherever the skipped passes left it
__device__ __forceinline__ View window_view(const lwdetr_augment_image& im, const uint8_t* scratch) {
    if (has_v1(im)) return View{scratch + im.scratch_off[SC_B], (long)im.cw * 3, 1};
    if (has_h1(im)) return View{scratch + im.scratch_off[SC_A], (long)im.cw * 3, 1};     // rows == ch, row0 == top
    return source_view(im, im.top, im.left);
}

// horizontal passes (STAGE 0: pass 1, STAGE 1: pass 3): a workgroup = 256 consecutive output pixels of one row, one lane per pixel. The source
// bytes those pixels tap form one contiguous span of the input row (bounds grow with x; the flipped source runs backwards through the same
// span): the workgroup brings it into LDS with aligned 32-bit loads - the words that hold the span's first and last bytes are read whole, so
// the buffers behind `src` and `scratch` start and end on 4-byte boundaries, as device allocations do -, the lanes tap LDS, and the 768 result
// bytes leave as aligned 32-bit stores. A span above H_SPAN_BYTES (a reduction by more than about ten) is tapped in memory instead.
constexpr int H_SPAN_BYTES = 8192;

template <int STAGE>
__global__ __launch_bounds__(256) void augment_h_kernel(const lwdetr_augment_image* __restrict__ imgs, const int32_t* __restrict__ tab,
                                                        uint8_t* __restrict__ scratch) {
    __shared__ uint32_t sin[H_SPAN_BYTES / 4];
    __shared__ uint32_t sout[256 * 3 / 4];
    constexpr int ax = STAGE == 0 ? AX_X1 : AX_X2;
    const lwdetr_augment_image im = imgs[blockIdx.z];
    if (STAGE == 0 ? !has_h1(im) : !has_h2(im)) return;
    const int nrows = STAGE == 0 ? im.rows : im.ch, ncols = STAGE == 0 ? im.cw : im.ow, tx0 = STAGE == 0 ? im.left : 0;
    const int y = blockIdx.y, xb = blockIdx.x * 256, tid = threadIdx.x;
    if (y >= nrows || xb >= ncols) return;                                 // the whole workgroup
    const View in = STAGE == 0 ? source_view(im, im.row0, 0) : window_view(im, scratch);
    const int nb = ncols - xb < 256 ? ncols - xb : 256;                    // pixels of this workgroup
    const int32_t* bounds = tab + im.bounds_off[ax];
    const int tlast = tx0 + xb + nb - 1;
    const int tmin = bounds[2 * (tx0 + xb)], tmax = bounds[2 * tlast] + bounds[2 * tlast + 1];       // input pixels [tmin, tmax) are tapped
    const int span = (tmax - tmin) * 3;
    const uint8_t* rowp = in.p + (long)y * in.pitch;
    const uint8_t* lo = rowp + (in.sx > 0 ? (long)tmin * 3 : -(long)(tmax - 1) * 3);                 // the span's lowest address
    const int mis = (int)((uintptr_t)lo & 3);
    const bool staged = mis + span <= H_SPAN_BYTES;
    if (staged) {
        const uint32_t* a0 = (const uint32_t*)(lo - mis);
        const int nw = (mis + span + 3) >> 2;
        for (int i = tid; i < nw; i += 256) sin[i] = a0[i];
    }
    __syncthreads();
    uint8_t* so = (uint8_t*)sout;
    if (tid < nb) {
        const int tx = tx0 + xb + tid;
        const int xmin = bounds[2 * tx], n = bounds[2 * tx + 1];
        const int32_t* k = tab + im.coef_off[ax] + (long)tx * im.ksize[ax];
        const uint8_t* px = staged ? (const uint8_t*)sin + mis + (in.sx > 0 ? xmin - tmin : tmax - 1 - xmin) * 3 : rowp + (long)in.sx * xmin * 3;
        const int step = in.sx * 3;
        int a0 = ROUND, a1 = ROUND, a2 = ROUND;
        for (int t = 0; t < n; ++t) {
            const int c = k[t];
            a0 += px[step * t] * c; a1 += px[step * t + 1] * c; a2 += px[step * t + 2] * c;
        }
        so[3 * tid] = (uint8_t)clip8(a0); so[3 * tid + 1] = (uint8_t)clip8(a1); so[3 * tid + 2] = (uint8_t)clip8(a2);
    }
    __syncthreads();
    // the workgroup's 3 * nb result bytes: whole aligned words as 32-bit stores, the ragged ends byte by byte
    uint8_t* out = scratch + im.scratch_off[STAGE == 0 ? SC_A : SC_C] + ((long)y * ncols + xb) * 3;
    const int omis = (int)((uintptr_t)out & 3), nbytes = nb * 3;
    const int b0 = 4 * tid - omis;                                         // lane tid: bytes [b0, b0 + 4) of the result (at most 193 words)
    if (b0 >= 0 && b0 + 4 <= nbytes) {
        *(uint32_t*)(out + b0) = (uint32_t)so[b0] | ((uint32_t)so[b0 + 1] << 8) | ((uint32_t)so[b0 + 2] << 16) | ((uint32_t)so[b0 + 3] << 24);
    } else {
        for (int i = 0; i < 4; ++i)
            if (b0 + i >= 0 && b0 + i < nbytes) out[b0 + i] = so[b0 + i];
    }
}

// 3 * npx consecutive bytes at lo, in memory order: three aligned 32-bit loads when `wide`, bytes otherwise
__device__ __forceinline__ void load_px(const uint8_t* lo, bool wide, int npx, int (&v)[12]) {
    if (wide) {
        const uint32_t* p4 = (const uint32_t*)lo;
        const uint32_t w0 = p4[0], w1 = p4[1], w2 = p4[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = (int)((w0 >> (8 * i)) & 255); v[4 + i] = (int)((w1 >> (8 * i)) & 255); v[8 + i] = (int)((w2 >> (8 * i)) & 255);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) v[i] = i < 3 * npx ? (int)lo[i] : 0;
    }
}

// One lane's share of a vertical pass: pixels x0 ... x0 + npx - 1 (npx <= 4) of output row `ty` of the axis table `ax`, from the rows of
// `in` (whose row 0 is input row `in_row0`). px[i][c] = result of pixel x0 + i, whatever the direction the view runs in.
__device__ __forceinline__ void vertical_px(const lwdetr_augment_image& im, const int32_t* __restrict__ tab, const View& in, int in_row0, int ax,
                                            int ty, bool resample, int x0, int npx, int (&px)[4][3]) {
    int ymin = ty, n = 1;
    const int32_t* k = nullptr;
    if (resample) {
        ymin = tab[im.bounds_off[ax] + 2 * ty]; n = tab[im.bounds_off[ax] + 2 * ty + 1];
        k = tab + im.coef_off[ax] + (long)ty * im.ksize[ax];
    }
    // lowest address of the npx pixels: pixel x0 going up, pixel x0 + npx - 1 going down
    const uint8_t* lo = in.p + (long)(ymin - in_row0) * in.pitch + (long)in.sx * (in.sx > 0 ? x0 : x0 + npx - 1) * 3;
    const bool wide = npx == 4 && (((uintptr_t)lo | (uintptr_t)in.pitch) & 3) == 0;
    int acc[12], v[12];
    if (resample) {
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = ROUND;
        for (int t = 0; t < n; ++t) {
            const int c = k[t];
            load_px(lo + (long)t * in.pitch, wide, npx, v);
#pragma unroll
            for (int i = 0; i < 12; ++i) acc[i] += v[i] * c;
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = clip8(acc[i]);
    } else {
        load_px(lo, wide, npx, acc);                  // equal lengths: the pass is skipped, the bytes are taken as they are
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = in.sx > 0 ? i : npx - 1 - i;    // memory order -> pixel order
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int s = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) s = (q == j) ? acc[3 * q + c] : s;
            px[i][c] = i < npx ? s : 0;
        }
    }
}

// pass 2: B[y][x][c], y < ch, x < cw. One lane = 4 consecutive pixels.
__global__ __launch_bounds__(256) void augment_v1_kernel(const lwdetr_augment_image* __restrict__ imgs, const int32_t* __restrict__ tab,
                                                         uint8_t* __restrict__ scratch) {
    const lwdetr_augment_image im = imgs[blockIdx.z];
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y;
    if (!has_v1(im) || x0 >= im.cw || y >= im.ch) return;
    const int npx = im.cw - x0 < 4 ? im.cw - x0 : 4;
    View in;
    int in_row0;
    if (has_h1(im)) { in = View{scratch + im.scratch_off[SC_A], (long)im.cw * 3, 1}; in_row0 = im.row0; }
    else { in = source_view(im, 0, im.left); in_row0 = 0; }
    int px[4][3];
    vertical_px(im, tab, in, in_row0, AX_Y1, im.top + y, true, x0, npx, px);
    uint8_t* o = scratch + im.scratch_off[SC_B] + ((long)y * im.cw + x0) * 3;
    if (npx == 4 && (((uintptr_t)o) & 3) == 0) {
        uint32_t w[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            uint32_t u = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) { const int e = 4 * q + b; u |= (uint32_t)px[e / 3][e % 3] << (8 * b); }
            w[q] = u;
        }
        uint32_t* o4 = (uint32_t*)o;
        o4[0] = w[0]; o4[1] = w[1]; o4[2] = w[2];
    } else {
        for (int i = 0; i < npx; ++i) { o[3 * i] = (uint8_t)px[i][0]; o[3 * i + 1] = (uint8_t)px[i][1]; o[3 * i + 2] = (uint8_t)px[i][2]; }
    }
}

// pass 4 over the whole Hc x Wc canvas: stage-2 vertical pass + ToTensor + Normalize inside the image's oh x ow, zeros outside; the mask
// from the same lanes. One lane = 4 consecutive canvas pixels (8 / 16-byte stores per plane and one 32-bit mask store when aligned).
template <typename T>
__global__ __launch_bounds__(256) void augment_v2_kernel(const lwdetr_augment_image* __restrict__ imgs, const int32_t* __restrict__ tab,
                                                         const uint8_t* __restrict__ scratch, const float* __restrict__ lut,
                                                         T* __restrict__ out, uint8_t* __restrict__ mask, int Hc, int Wc) {
    __shared__ float slut[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += blockDim.x) slut[i] = lut[i];
    __syncthreads();
    const lwdetr_augment_image im = imgs[blockIdx.z];
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y;
    if (x0 >= Wc) return;
    const int ncv = Wc - x0 < 4 ? Wc - x0 : 4;                                         // canvas pixels of this lane
    const int npx = (y < im.oh && x0 < im.ow) ? (im.ow - x0 < 4 ? im.ow - x0 : 4) : 0;   // of which inside the image
    int px[4][3] = {};
    if (npx > 0) {
        View in = has_h2(im) ? View{scratch + im.scratch_off[SC_C], (long)im.ow * 3, 1} : window_view(im, scratch);
        vertical_px(im, tab, in, 0, AX_Y2, y, has_v2(im), x0, npx, px);
    }
    const long plane = (long)Hc * Wc;
    T* o = out + (long)blockIdx.z * 3 * plane + (long)y * Wc + x0;
    typedef T V4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        T v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = from_f32<T>(i < npx ? slut[ch * 256 + px[i][ch]] : 0.f);
        T* oc = o + (long)ch * plane;
        if (ncv == 4 && (((uintptr_t)oc) & (4 * sizeof(T) - 1)) == 0) *(V4*)oc = V4{v[0], v[1], v[2], v[3]};
        else for (int i = 0; i < ncv; ++i) oc[i] = v[i];
    }
    uint8_t* m = mask + (long)blockIdx.z * plane + (long)y * Wc + x0;
    if (ncv == 4 && (((uintptr_t)m) & 3) == 0) {
        uint32_t u = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) u |= (uint32_t)(i < npx ? 0 : 1) << (8 * i);
        *(uint32_t*)m = u;
    } else {
        for (int i = 0; i < ncv; ++i) m[i] = i < npx ? 0 : 1;
    }
}

bool table_ok(const lwdetr_augment_image& d, int ax, int out_len, long table_len) {
    const long b = d.bounds_off[ax], c = d.coef_off[ax], ks = d.ksize[ax];
    return b >= 0 && c >= 0 && ks > 0 && b + 2L * out_len <= table_len && c + ks * out_len <= table_len;
}
bool scratch_ok(const lwdetr_augment_image& d, int which, long bytes, long scratch_bytes) {
    return d.scratch_off[which] >= 0 && d.scratch_off[which] + bytes <= scratch_bytes;
}

}  // namespace

extern "C" int lwdetr_augment_normalize(const lwdetr_augment_image* images_host, const lwdetr_augment_image* images_dev, int B,
                                        const int32_t* tables, long table_len, uint8_t* scratch, long scratch_bytes, const float* lut,
                                        void* out, uint8_t* mask, int Hc, int Wc, int dtype, void* hip_stream) {
    const int LIM = 65535;
    if (B < 0 || Hc < 0 || Wc < 0 || Hc > LIM || Wc > LIM || B > LIM || table_len < 0 || scratch_bytes < 0) return LWDETR_ERR_BAD_ARG;
    if (dtype != DT_F32 && dtype != DT_F16 && dtype != DT_BF16) return LWDETR_ERR_UNSUPPORTED;
    if (B == 0) return LWDETR_OK;
    if (!images_host || !images_dev || !tables || !scratch || !lut || !out || !mask || Hc == 0 || Wc == 0) return LWDETR_ERR_BAD_ARG;
    int rows1 = 0, cols1 = 0, rows2 = 0, cols2 = 0, rows3 = 0, cols3 = 0;       // grid extents of passes 1-3 (0: no image needs the pass)
    for (int b = 0; b < B; ++b) {
        const lwdetr_augment_image& d = images_host[b];
        if (!d.src || d.height <= 0 || d.width <= 0 || d.height > LIM || d.width > LIM || d.row_stride < 3L * d.width) return LWDETR_ERR_BAD_ARG;
        if (d.h1 <= 0 || d.w1 <= 0 || d.h1 > LIM || d.w1 > LIM || d.oh <= 0 || d.ow <= 0 || d.oh > Hc || d.ow > Wc) return LWDETR_ERR_BAD_ARG;
        if (d.ch <= 0 || d.cw <= 0 || d.top < 0 || d.left < 0 || d.top > d.h1 - d.ch || d.left > d.w1 - d.cw) return LWDETR_ERR_BAD_ARG;
        const bool h1 = d.w1 != d.width, v1 = d.h1 != d.height, h2 = d.ow != d.cw, v2 = d.oh != d.ch;
        if (h1) {
            // the rows pass 1 computes: what pass 2 taps, or exactly the window's rows when there is no pass 2
            if (d.row0 < 0 || d.rows <= 0 || d.row0 > d.height - d.rows || (!v1 && (d.row0 != d.top || d.rows != d.ch))) return LWDETR_ERR_BAD_ARG;
            if (!table_ok(d, AX_X1, d.w1, table_len) || !scratch_ok(d, SC_A, 3L * d.rows * d.cw, scratch_bytes)) return LWDETR_ERR_BAD_ARG;
            rows1 = d.rows > rows1 ? d.rows : rows1; cols1 = d.cw > cols1 ? d.cw : cols1;
        }
        if (v1) {
            if (!table_ok(d, AX_Y1, d.h1, table_len) || !scratch_ok(d, SC_B, 3L * d.ch * d.cw, scratch_bytes)) return LWDETR_ERR_BAD_ARG;
            rows2 = d.ch > rows2 ? d.ch : rows2; cols2 = d.cw > cols2 ? d.cw : cols2;
        }
        if (h2) {
            if (!table_ok(d, AX_X2, d.ow, table_len) || !scratch_ok(d, SC_C, 3L * d.ch * d.ow, scratch_bytes)) return LWDETR_ERR_BAD_ARG;
            rows3 = d.ch > rows3 ? d.ch : rows3; cols3 = d.ow > cols3 ? d.ow : cols3;
        }
        if (v2 && !table_ok(d, AX_Y2, d.oh, table_len)) return LWDETR_ERR_BAD_ARG;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    ProfScope ps(KID_ELTWISE, 0.0, 0.0, st);
    const unsigned nb = (unsigned)B;
    if (cols1 > 0)
        hipLaunchKernelGGL((augment_h_kernel<0>), dim3((unsigned)((cols1 + 255) / 256), (unsigned)rows1, nb), dim3(256), 0, st, images_dev, tables, scratch);
    if (cols2 > 0)
        hipLaunchKernelGGL(augment_v1_kernel, dim3((unsigned)((cols2 + 1023) / 1024), (unsigned)rows2, nb), dim3(256), 0, st, images_dev, tables, scratch);
    if (cols3 > 0)
        hipLaunchKernelGGL((augment_h_kernel<1>), dim3((unsigned)((cols3 + 255) / 256), (unsigned)rows3, nb), dim3(256), 0, st, images_dev, tables, scratch);
    const dim3 g4((unsigned)((Wc + 1023) / 1024), (unsigned)Hc, nb);
    switch (dtype) {
        case DT_F32: hipLaunchKernelGGL((augment_v2_kernel<float>), g4, dim3(256), 0, st, images_dev, tables, scratch, lut, (float*)out, mask, Hc, Wc); break;
        case DT_F16: hipLaunchKernelGGL((augment_v2_kernel<f16>), g4, dim3(256), 0, st, images_dev, tables, scratch, lut, (f16*)out, mask, Hc, Wc); break;
        default: hipLaunchKernelGGL((augment_v2_kernel<bf16>), g4, dim3(256), 0, st, images_dev, tables, scratch, lut, (bf16*)out, mask, Hc, Wc); break;
    }
    return lwdetr_check_launch();
}
