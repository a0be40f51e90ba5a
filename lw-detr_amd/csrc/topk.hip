// Sorted top-k selection for gfx950, one workgroup per image (512 threads up to N = 4096, 1024 above), and the two places LW-DETR uses it:
//   * two-stage query selection: class-max of the encoder logits (rowmax kernel) -> top-nq rows in descending order
//     (reference models/transformer.py:246-248, torch.topk(enc_outputs_class.max(-1)[0], num_queries, dim=1))
//   * PostProcess: top-num_select of sigmoid(logits) over nq x classes, labels = idx % C, boxes = idx // C gathered,
//     cxcywh -> xyxy, scaled by the target size (reference models/lwdetr.py:509-540, util/box_ops.py:21-25)
// Order = a composite per element,
//     comp = (key - kmin) << nb | (2^nb - 1 - index),   key = order_preserving_u32(value), nb = bits of N - 1,
// which is unique, so the selected SET and its ORDER are fully deterministic: descending value, equal values by ascending index
// (torch.topk leaves the order of ties unspecified). kmin / kmax, the image's smallest and largest key, are reduced in the load pass.
//   1. load pass: 16-byte loads, keys to the LDS cache, kmin / kmax.
//   2. one histogram pass over the first digit = the top 11 bits of kmax - kmin, i.e. bits that vary (detection logits sit in three
//      or four binades: the top 11 bits of the raw key put a third of them into ONE bin, whose LDS counter then serialised 10^4 adds).
//      All waves scan it (each thread owns 2048 / threads consecutive bins and zeroes them as it reads them, a wave suffix scan, one
//      partial per wave) and leave, per bin, the number of elements in higher bins (sfx): the winners' bucket offsets.
//   3. one pass that compares every key with the threshold bin's smallest key and queues the few at or above it per wave; each wave
//      then drops its queue's elements of bins above the threshold bin into their buckets of sel[] and the threshold bin's elements
//      into a candidate list (at most TK_CAND); the candidates are ranked among themselves and the best of them fill the last bucket.
//      A threshold bin with more elements than that (heavy ties) goes on with 11-bit digits of the composite over all elements.
//   4. rank of a winner = its bucket's offset + the winners of the same bucket above it: a handful of compares, where ranking the k
//      winners against each other took k * k and more time than everything else together.
#include "common.h"
#include <type_traits>

// Phase timing for tuning (a private build with -DLWDETR_TK_TIMING, TUNE= of the Makefile; never in the product library): s_memrealtime
// stamps (10 ns ticks) of wave 0 of workgroup 0 at the phase boundaries of the last selection launch.
#ifdef LWDETR_TK_TIMING
__device__ unsigned long long g_tk_timing[16];
#define TK_TS(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_tk_timing[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
extern "C" int lwdetr_debug_tk_timing(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tk_timing), sizeof(g_tk_timing)) == hipSuccess ? 0 : 1;
}
#else
#define TK_TS(i) do {} while (0)
#endif

namespace {

constexpr int TK_MAXK = 1024;
constexpr int TK_IDX_BITS = 20;                             // N < 2^20: the interface's limit, at most 32 + 20 composite bits
constexpr unsigned TK_IDX_MASK = (1u << TK_IDX_BITS) - 1;
constexpr int TK_BINS = 2048;
constexpr int TK_DIGIT = 11;
constexpr int TK_QUEUE = 128;                                // K + TK_CAND elements at most over all waves; a full queue places at once
constexpr int TK_CAND = 512;                                 // candidates ranked by all-pairs compares: TK_CAND^2 / threads per thread at most
constexpr int TK_SMALL_THREADS = 512, TK_LARGE_THREADS = 1024;
constexpr int TK_SMALL_N = 4096;                             // up to here the 512-thread form (N = 1600, K = 300: 9.6 us with 256 threads, 8.2 with 512)

__device__ __forceinline__ unsigned fkey(float f) {          // monotone float -> u32 (ascending)
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

template <typename T> struct TkVec { typedef typename Vec<T>::v8 type; };       // 16 bytes of T
template <> struct TkVec<float> { typedef f32x4 type; };

struct alignas(32) TopkShared {
    unsigned hist[TK_BINS];                 // digit counts of the running pass; zero between passes; the buckets' fill counts at the end
    unsigned sfx[TK_BINS];                  // first digit d -> number of elements with a larger first digit
    unsigned long long sel[TK_MAXK];        // the winners, grouped by first digit (descending)
    unsigned long long cand[TK_CAND];
    unsigned long long queue[16][TK_QUEUE]; // per wave: what its scan found at or above the threshold bin, placed after the scan
    unsigned wtot[16], wmin[16], wmax[16];  // one partial per wave
    unsigned bstar, above, cnt, nsel;
};

// how the composites of one image are built and where its winners lie in sh.sel (uniform over the workgroup)
struct TkCode {
    unsigned kmin, idxmask, bstar1;
    int nb, sh1;                            // first digit of a composite = c >> sh1
    __device__ __forceinline__ unsigned long long comp(unsigned key, int i) const {
        return ((unsigned long long)(key - kmin) << nb) | (unsigned long long)(idxmask - (unsigned)i);
    }
    __device__ __forceinline__ int index(unsigned long long c) const { return (int)(idxmask - ((unsigned)c & idxmask)); }
    __device__ __forceinline__ float value(unsigned long long c) const { return fkey_inv((unsigned)(c >> nb) + kmin); }
};

// elements in front of the first 16-byte boundary of x (an image's base is only element-aligned)
template <typename T>
__device__ __forceinline__ int tk_head(const T* x, int N) {
    const int head = (int)(((16u - (unsigned)((uintptr_t)x & 15)) & 15u) / sizeof(T));
    return head < N ? head : N;
}
// The key of element i lives in word tk_pad(head) + i of the cache: the 16-byte vectors of the load pass then start on 16-byte boundaries of LDS too.
__device__ __forceinline__ int tk_pad(int head) { return (4 - (head & 3)) & 3; }

template <int NE> using TkN = std::integral_constant<int, NE>;
// adapts a per-element f(key, i) to the iterators below, which hand over runs of NE consecutive elements: f(TkN<NE>, keys, first index)
template <typename F>
struct TkEach {
    F f;
    template <int NE> __device__ __forceinline__ void operator()(TkN<NE>, const unsigned* k, int i0) const {
#pragma unroll
        for (int e = 0; e < NE; ++e) f(k[e], i0 + e);
    }
};
template <typename F> __device__ __forceinline__ TkEach<F> tk_each(F f) { return TkEach<F>{f}; }

// f(TkN<NE>, keys, i0) over every element of x[0, N): 16-byte loads over the 16-byte aligned body, four per thread issued before the first is
// used, scalar loads for the head in front of it and the tail behind it
template <typename T, int THREADS, typename F>
__device__ __forceinline__ void tk_for_global(const T* __restrict__ x, int N, F f) {
    typedef typename TkVec<T>::type VT;
    constexpr int EPV = 16 / (int)sizeof(T);
    const int tid = threadIdx.x;
    const int head = tk_head(x, N);
    const int nvec = (N - head) / EPV;
    const int tail = head + nvec * EPV;
    const bool has_h = tid < head, has_t = tail + tid < N;
    T hv = T(0), tv = T(0);
    if (has_h) hv = x[tid];
    if (has_t) tv = x[tail + tid];
    const VT* __restrict__ xv = (const VT*)(x + head);
    for (int v0 = tid; v0 < nvec; v0 += 4 * THREADS) {
        VT r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (v0 + u * THREADS < nvec) r[u] = xv[v0 + u * THREADS];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (v0 + u * THREADS < nvec) {
                unsigned k[EPV];
#pragma unroll
                for (int e = 0; e < EPV; ++e) k[e] = fkey(to_f32<T>(r[u][e]));
                f(TkN<EPV>(), k, head + (v0 + u * THREADS) * EPV);
            }
    }
    if (has_h) { const unsigned k = fkey(to_f32<T>(hv)); f(TkN<1>(), &k, tid); }
    if (has_t) { const unsigned k = fkey(to_f32<T>(tv)); f(TkN<1>(), &k, tail + tid); }
}

// the same over the key cache in LDS: one 16-byte read per four elements, the up to three words on either side of the whole quads one by one
template <int THREADS, typename F>
__device__ __forceinline__ void tk_for_cached(const unsigned* __restrict__ keys, int pad, int N, F f) {
    const uint4* __restrict__ k4 = (const uint4*)keys;
    const int end = pad + N;                               // the keys are words [pad, end)
    const int qa = (pad + 3) >> 2, qb = end >> 2;           // whole quads [qa, qb)
    for (int q = qa + (int)threadIdx.x; q < qb; q += THREADS) {
        const uint4 v = k4[q];
        const unsigned k[4] = {v.x, v.y, v.z, v.w};
        f(TkN<4>(), k, q * 4 - pad);
    }
    if (threadIdx.x < 8) {
        const int t = threadIdx.x;
        const int w = t < 4 ? pad + t : 4 * (qb > qa ? qb : qa) + (t - 4);
        if (w < end && (t >= 4 || w < 4 * qa)) { const unsigned k = keys[w]; f(TkN<1>(), &k, w - pad); }
    }
}

template <typename T, bool CACHE, int THREADS, typename F>
__device__ __forceinline__ void tk_for_keys(const T* __restrict__ x, const unsigned* __restrict__ keys, int pad, int N, F f) {
    if (CACHE) tk_for_cached<THREADS>(keys, pad, N, f);
    else tk_for_global<T, THREADS>(x, N, f);
}

// The load pass: kmin / kmax of this thread's elements and, CACHE, their keys into LDS (16-byte stores for the vectors).
template <typename T, bool CACHE, int THREADS>
__device__ __forceinline__ void tk_load(const T* __restrict__ x, int N, unsigned* __restrict__ keys, int pad, unsigned& kmin, unsigned& kmax) {
    typedef typename TkVec<T>::type VT;
    constexpr int EPV = 16 / (int)sizeof(T);
    const int tid = threadIdx.x;
    const int head = tk_head(x, N);
    const int nvec = (N - head) / EPV;
    const int tail = head + nvec * EPV;
    const bool has_h = tid < head, has_t = tail + tid < N;
    T hv = T(0), tv = T(0);
    if (has_h) hv = x[tid];
    if (has_t) tv = x[tail + tid];
    const VT* __restrict__ xv = (const VT*)(x + head);
    for (int v0 = tid; v0 < nvec; v0 += 4 * THREADS) {
        VT r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (v0 + u * THREADS < nvec) r[u] = xv[v0 + u * THREADS];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (v0 + u * THREADS < nvec) {
                unsigned k[EPV];
#pragma unroll
                for (int e = 0; e < EPV; ++e) {
                    k[e] = fkey(to_f32<T>(r[u][e]));
                    kmin = k[e] < kmin ? k[e] : kmin;
                    kmax = k[e] > kmax ? k[e] : kmax;
                }
                if (CACHE) {                                // word pad + head + EPV * v: a multiple of four
                    uint4* dst = (uint4*)(keys + pad + head + (v0 + u * THREADS) * EPV);
#pragma unroll
                    for (int e = 0; e < EPV; e += 4) dst[e >> 2] = make_uint4(k[e], k[e + 1], k[e + 2], k[e + 3]);
                }
            }
    }
    if (has_h) {
        const unsigned k = fkey(to_f32<T>(hv));
        if (CACHE) keys[pad + tid] = k;
        kmin = k < kmin ? k : kmin; kmax = k > kmax ? k : kmax;
    }
    if (has_t) {
        const unsigned k = fkey(to_f32<T>(tv));
        if (CACHE) keys[pad + tail + tid] = k;
        kmin = k < kmin ? k : kmin; kmax = k > kmax ? k : kmax;
    }
}

// Scan of sh.hist from the highest bin down, by all threads, after the barrier that ends the pass: the bin that holds the rem-th element,
// the number of elements above it and its own count. Thread t owns bins [t * PER, (t + 1) * PER) and leaves them zeroed.
// SFX: sh.sfx[bin] = number of elements in higher bins, for every bin. Ends with a barrier.
template <int THREADS, bool SFX>
__device__ __forceinline__ void tk_scan(TopkShared& sh, unsigned rem, unsigned& bstar, unsigned& above, unsigned& cnt) {
    constexpr int PER = TK_BINS / THREADS, NW = THREADS / 64;
    typedef unsigned BinV __attribute__((ext_vector_type(PER)));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    BinV* hv = (BinV*)sh.hist;
    const BinV cv = hv[tid];
    hv[tid] = BinV(0);
    unsigned own = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) own += cv[j];
    unsigned s = own;                               // inclusive suffix sum over the lanes of the wave (lane 63 = highest bins)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_down(s, o);
        if (lane + o < 64) s += t;
    }
    if (lane == 0) sh.wtot[wave] = s;
    __syncthreads();
    unsigned excl = s - own;                        // elements in higher bins: of this wave, then of the waves above
    for (int w = wave + 1; w < NW; ++w) excl += sh.wtot[w];
    if (SFX) {
        BinV sv;
        unsigned acc = excl;
#pragma unroll
        for (int j = PER - 1; j >= 0; --j) { sv[j] = acc; acc += cv[j]; }
        ((BinV*)sh.sfx)[tid] = sv;
    }
    if (excl < rem && rem <= excl + own) {          // exactly one thread: its bins hold the rem-th element
        unsigned acc = excl;
        bool found = false;
#pragma unroll
        for (int j = PER - 1; j >= 0; --j) {
            if (!found && acc + cv[j] >= rem) { sh.bstar = (unsigned)(tid * PER + j); sh.above = acc; sh.cnt = cv[j]; found = true; }
            acc += cv[j];
        }
    }
    __syncthreads();
    bstar = sh.bstar; above = sh.above; cnt = sh.cnt;
}

// Leaves the k winners' composites in sh.sel[0..k), grouped by first digit (descending), and sh.sfx. All threads call it.
// CACHE: the 32-bit keys of the image are written to LDS (`keys`, dynamic shared memory) by the load pass and read from there by the
// later ones - one dependent L2 round trip per element instead of three or more.
template <typename T, bool CACHE, int THREADS>
__device__ TkCode topk_select(const T* __restrict__ x, int N, int K, TopkShared& sh, unsigned* __restrict__ keys) {
    const int tid = threadIdx.x, lane = tid & 63;
    TK_TS(0);
    // ---- load pass
    const int pad = tk_pad(tk_head(x, N));
    unsigned kmin = 0xFFFFFFFFu, kmax = 0;
    if (tid == 0) sh.nsel = 0;
    for (int i = tid; i < TK_BINS; i += THREADS) sh.hist[i] = 0;
    tk_load<T, CACHE, THREADS>(x, N, keys, pad, kmin, kmax);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned a = __shfl_xor(kmin, o), b = __shfl_xor(kmax, o);
        kmin = a < kmin ? a : kmin;
        kmax = b > kmax ? b : kmax;
    }
    if (lane == 0) { sh.wmin[tid >> 6] = kmin; sh.wmax[tid >> 6] = kmax; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < THREADS / 64; w += 4) {
        const uint4 a = *(const uint4*)&sh.wmin[w], b = *(const uint4*)&sh.wmax[w];
        kmin = min(min(kmin, min(a.x, a.y)), min(a.z, a.w));
        kmax = max(max(kmax, max(b.x, b.y)), max(b.z, b.w));
    }
    TK_TS(1);
    TkCode code;
    code.kmin = kmin;
    const unsigned range = kmax - kmin;
    code.nb = N > 1 ? 32 - __builtin_clz((unsigned)(N - 1)) : 0;
    code.idxmask = (1u << code.nb) - 1u;
    const int kb = range ? 32 - __builtin_clz(range) : 0;            // key - kmin < 2^kb
    // ---- first digit: the top bits of key - kmin
    const int bits1 = kb > TK_DIGIT ? TK_DIGIT : kb;
    const int ksh = kb - bits1;                                      // <= 21
    code.sh1 = ksh + code.nb;
    tk_for_keys<T, CACHE, THREADS>(x, keys, pad, N, tk_each([&](unsigned k, int i) { atomicAdd(&sh.hist[(k - kmin) >> ksh], 1u); }));
    __syncthreads();
    unsigned bstar, above, cnt;
    tk_scan<THREADS, true>(sh, (unsigned)K, bstar, above, cnt);
    code.bstar1 = bstar;
    unsigned rem = (unsigned)K - above;                 // how many of the threshold bin's cnt elements are taken
    TK_TS(2);
    if (cnt == rem || cnt <= (unsigned)TK_CAND) {
        // ---- higher bins into their buckets; the threshold bin too if it is taken whole, else into the candidate list
        const bool whole = cnt == rem;
        const unsigned kthr = kmin + (bstar << ksh);    // smallest key of the threshold bin (bstar << ksh <= kmax - kmin): one compare per element
        auto place = [&](unsigned long long c) {
            const unsigned d = (unsigned)(c >> code.sh1);
            if (d > bstar || whole) {
                const unsigned p = sh.sfx[d] + atomicAdd(&sh.hist[d], 1u);
                if (p < (unsigned)TK_MAXK) sh.sel[p] = c;
            } else {
                const unsigned p = atomicAdd(&sh.nsel, 1u);
                if (p < (unsigned)TK_CAND) sh.cand[p] = c;
            }
        };
        // One element in eighty is placed, but more than half of a wave's steps hold one, and a placement is three dependent LDS round trips. So the
        // scan only queues: the lanes that hold one write it behind the wave's count (ballot, no round trip) into the wave's own queue, which the
        // wave places afterwards, 64 at a time. wq_n is the same in all lanes still in the loop, and lane 0 of a wave leaves an iterator's vector
        // loop last; the scalar runs at the edges (NE = 1) come under other lane masks and are placed at once, as is what a full queue cannot take.
        unsigned long long* wq = sh.queue[tid >> 6];
        unsigned wq_n = 0;
        tk_for_keys<T, CACHE, THREADS>(x, keys, pad, N, [&](auto ne, const unsigned* k, int i0) {
            constexpr int NE = decltype(ne)::value;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const bool hit = k[e] >= kthr;
                if (NE == 1) {
                    if (hit) place(code.comp(k[e], i0 + e));
                } else {
                    const unsigned long long m = __ballot(hit);
                    if (m) {
                        const unsigned pos = wq_n + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
                        if (hit) {
                            const unsigned long long c = code.comp(k[e], i0 + e);
                            if (pos < (unsigned)TK_QUEUE) wq[pos] = c;
                            else place(c);
                        }
                        wq_n += (unsigned)__popcll(m);
                    }
                }
            }
        });
        wq_n = (unsigned)__builtin_amdgcn_readfirstlane((int)wq_n);
        wq_n = wq_n < (unsigned)TK_QUEUE ? wq_n : (unsigned)TK_QUEUE;
        __threadfence_block();
        for (unsigned j = lane; j < wq_n; j += 64) place(wq[j]);
        __syncthreads();
        TK_TS(3);
        if (!whole) {                                   // the rem largest candidates, in order, are the last bucket
            for (unsigned i = tid; i < cnt; i += THREADS) {
                const unsigned long long mine = sh.cand[i];
                unsigned r = 0;
                for (unsigned j = 0; j < cnt; ++j) r += sh.cand[j] > mine ? 1u : 0u;
                if (r < rem) sh.sel[above + r] = mine;
            }
            __syncthreads();
        }
        TK_TS(4);
        return code;
    }
    // ---- a large tie around the threshold: 11-bit digits of the composite below the first one, over all elements
    int top = code.sh1;                                 // bits not yet decided
    unsigned long long prefix = bstar;                  // digits decided so far (the high bits of the threshold composite)
    while (top > 0) {
        const int bits = top > TK_DIGIT ? TK_DIGIT : top;
        const int shift = top - bits;
        const unsigned dmask = (1u << bits) - 1u;
        tk_for_keys<T, CACHE, THREADS>(x, keys, pad, N, tk_each([&](unsigned k, int i) {
            const unsigned long long c = code.comp(k, i);
            if ((c >> top) == prefix) atomicAdd(&sh.hist[(unsigned)(c >> shift) & dmask], 1u);
        }));
        __syncthreads();
        tk_scan<THREADS, false>(sh, rem, bstar, above, cnt);
        rem -= above;
        prefix = (prefix << bits) | bstar;
        top = shift;
        if (cnt == rem) break;                          // the whole bin is taken: threshold found
    }
    const unsigned long long thr = prefix << top;
    tk_for_keys<T, CACHE, THREADS>(x, keys, pad, N, tk_each([&](unsigned k, int i) {
        const unsigned long long c = code.comp(k, i);
        if (c >= thr) {
            const unsigned d = (unsigned)(c >> code.sh1);
            const unsigned p = sh.sfx[d] + atomicAdd(&sh.hist[d], 1u);
            if (p < (unsigned)TK_MAXK) sh.sel[p] = c;
        }
    }));
    __syncthreads();
    TK_TS(8);
    return code;
}

// Descending rank of winner c: the offset of its bucket plus the winners of that bucket above it.
__device__ __forceinline__ unsigned tk_rank(const TopkShared& sh, const TkCode& code, int K, unsigned long long c) {
    const unsigned d = (unsigned)(c >> code.sh1);
    const unsigned lo = sh.sfx[d];
    const unsigned below = sh.sfx[d ? d - 1 : 0];
    const unsigned hi = d == code.bstar1 ? (unsigned)K : below;      // the threshold bin's bucket is the last one
    unsigned r = lo;
    for (unsigned j = lo; j < hi; ++j) r += sh.sel[j] > c ? 1u : 0u;
    return r;
}

template <typename T, bool CACHE, int THREADS>
__global__ __launch_bounds__(THREADS) void topk_kernel(const T* __restrict__ x, int N, int K, int64_t* __restrict__ idx_out,
                                                       float* __restrict__ val_out) {
    __shared__ TopkShared sh;
    extern __shared__ __attribute__((aligned(16))) unsigned tk_keys[];
    const int b = blockIdx.x;
    const TkCode code = topk_select<T, CACHE, THREADS>(x + (long)b * N, N, K, sh, tk_keys);
    for (int e = threadIdx.x; e < K; e += THREADS) {
        const unsigned long long c = sh.sel[e];
        const unsigned r = tk_rank(sh, code, K, c);
        idx_out[(long)b * K + r] = (int64_t)code.index(c);
        if (val_out) val_out[(long)b * K + r] = code.value(c);
    }
    TK_TS(10);
}

// PostProcess: sigmoid is monotone, so the top-k runs on the logits and only the k winners go through sigmoid.
template <typename T, bool CACHE, int THREADS>
__global__ __launch_bounds__(THREADS) void postprocess_kernel(const T* __restrict__ logits, const T* __restrict__ boxes,
                                                              const float* __restrict__ sizes, int nq, int ncls, int K,
                                                              float* __restrict__ scores, int64_t* __restrict__ labels,
                                                              float* __restrict__ out_boxes, float* __restrict__ packed) {
    __shared__ TopkShared sh;
    extern __shared__ __attribute__((aligned(16))) unsigned tk_keys[];
    const int b = blockIdx.x;
    const int N = nq * ncls;
    const TkCode code = topk_select<T, CACHE, THREADS>(logits + (long)b * N, N, K, sh, tk_keys);
    const float ih = sizes[b * 2], iw = sizes[b * 2 + 1];                   // target_sizes rows are (h, w)
    for (int e = threadIdx.x; e < K; e += THREADS) {
        const unsigned long long c = sh.sel[e];
        const int i = code.index(c);
        const int q = i / ncls;
        const T* bx = boxes + ((long)b * nq + q) * 4;                       // fetched while the winner is ranked
        const T b0 = bx[0], b1 = bx[1], b2 = bx[2], b3 = bx[3];
        const long o = (long)b * K + tk_rank(sh, code, K, c);
        const float v = code.value(c);
        const float score = to_f32<T>(from_f32<T>(1.f / (1.f + expf(-v))));   // sigmoid evaluated in f32, stored at T's precision
        const float cx = to_f32<T>(b0), cy = to_f32<T>(b1);
        const float w = fmaxf(to_f32<T>(b2), 0.f), h = fmaxf(to_f32<T>(b3), 0.f);
        // corners are formed at T's precision (the reference computes them on the model-dtype tensor) and scaled in f32
        const float x0 = to_f32<T>(from_f32<T>(cx - 0.5f * w)) * iw, y0 = to_f32<T>(from_f32<T>(cy - 0.5f * h)) * ih;
        const float x1 = to_f32<T>(from_f32<T>(cx + 0.5f * w)) * iw, y1 = to_f32<T>(from_f32<T>(cy + 0.5f * h)) * ih;
        if (packed) {       // (B, K, 6) f32 rows: score, label, x0, y0, x1, y1 - the record the detection all-gather ships
            float* pr = packed + o * 6;
            pr[0] = score; pr[1] = (float)(i - q * ncls); pr[2] = x0; pr[3] = y0; pr[4] = x1; pr[5] = y1;
        } else {
            scores[o] = score;
            labels[o] = (int64_t)(i - q * ncls);
            out_boxes[o * 4 + 0] = x0; out_boxes[o * 4 + 1] = y0; out_boxes[o * 4 + 2] = x1; out_boxes[o * 4 + 3] = y1;
        }
    }
    TK_TS(10);
}

// Row maximum over the first `ncols` entries of each row: 16 lanes per row, 4-element vector loads (ld % 4 == 0).
template <typename T>
__global__ __launch_bounds__(256) void rowmax_kernel(const T* __restrict__ x, long ld, long rows, int ncols, float* __restrict__ out) {
    constexpr int EPC = 4;
    typedef T VC __attribute__((ext_vector_type(EPC)));
    const int lane16 = threadIdx.x & 15;
    const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    float m = -INFINITY;
    if (row < rows) {
        const T* xr = x + row * ld;
        const int full = ncols / EPC;
        for (int c = lane16; c < full; c += 16) {
            const VC t = *(const VC*)(xr + c * EPC);
#pragma unroll
            for (int e = 0; e < EPC; ++e) m = fmaxf(m, to_f32<T>(t[e]));
        }
        for (int c = full * EPC + lane16; c < ncols; c += 16) m = fmaxf(m, to_f32<T>(xr[c]));
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (row < rows && lane16 == 0) out[row] = m;
}

}  // namespace

// key cache: whatever is left of the 160 KB beside TopkShared; larger inputs (e.g. 300 x 366 Objects365 logits) re-read global
constexpr size_t TK_CACHE_BYTES = 160 * 1024 - sizeof(TopkShared) - 256;
static size_t tk_cache_alloc(size_t n) { return ((n + 3) * 4 + 15) & ~(size_t)15; }    // up to 3 words of padding in front; read 16 bytes at a time
static bool tk_allow_lds(const void* fn) {
    // once per kernel instantiation (keyed by its address); hipFuncSetAttribute is not a stream operation
    static const void* done[16]; static int ndone = 0;
    for (int i = 0; i < ndone; ++i) if (done[i] == fn) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tk_cache_alloc(TK_CACHE_BYTES / 4)) != hipSuccess) return false;
    if (ndone < 16) done[ndone++] = fn;
    return true;
}

#define LWDETR_DISPATCH_T(dtype, CALL)                 \
    switch (dtype) {                                   \
        case DT_F32: { typedef float TT; CALL; break; } \
        case DT_F16: { typedef f16 TT; CALL; break; }   \
        case DT_BF16: { typedef bf16 TT; CALL; break; } \
        default: return LWDETR_ERR_UNSUPPORTED;        \
    }

extern "C" int lwdetr_rowmax(const void* x, long ld, long rows, int ncols, float* out, int dtype, void* hip_stream) {
    if (!x || !out || rows < 0 || ncols <= 0 || ld < ncols) return LWDETR_ERR_BAD_ARG;
    if (rows == 0) return LWDETR_OK;
    if (ld % 4 || ((uintptr_t)x & 15)) return LWDETR_ERR_BAD_ARG;                // vector-aligned row starts
    hipStream_t st = (hipStream_t)hip_stream;
    ProfScope ps(KID_ELTWISE, 0.0, (double)rows * ncols * (dtype == DT_F32 ? 4 : 2), st);
    LWDETR_DISPATCH_T(dtype, hipLaunchKernelGGL((rowmax_kernel<TT>), dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st,
                                                (const TT*)x, ld, rows, ncols, out));
    return lwdetr_check_launch();
}

extern "C" int lwdetr_topk(const void* x, int B, int N, int K, int64_t* idx_out, float* val_out, int dtype, void* hip_stream) {
    if (!x || !idx_out || B < 0 || K <= 0 || K > N || K > TK_MAXK || N > (int)TK_IDX_MASK) return LWDETR_ERR_BAD_ARG;
    if (B == 0) return LWDETR_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    ProfScope ps(KID_ELTWISE, 0.0, (double)B * N * (dtype == DT_F32 ? 4 : 2), st);
    const bool cache = (size_t)N * 4 <= TK_CACHE_BYTES;
    const bool small = N <= TK_SMALL_N;
#define TK_LAUNCH(CACHE, THREADS)                                                                                                 \
    do {                                                                                                                           \
        if (CACHE && !tk_allow_lds((const void*)topk_kernel<TT, CACHE, THREADS>)) return LWDETR_ERR_LAUNCH;                        \
        hipLaunchKernelGGL((topk_kernel<TT, CACHE, THREADS>), dim3(B), dim3(THREADS), CACHE ? tk_cache_alloc((size_t)N) : 0, st, \
                           (const TT*)x, N, K, idx_out, val_out);                                                                 \
    } while (0)
    LWDETR_DISPATCH_T(dtype, {
        if (small) TK_LAUNCH(true, TK_SMALL_THREADS);               // N <= TK_SMALL_N always fits the cache
        else if (cache) TK_LAUNCH(true, TK_LARGE_THREADS);
        else TK_LAUNCH(false, TK_LARGE_THREADS);
    });
#undef TK_LAUNCH
    return lwdetr_check_launch();
}

static int postprocess_impl(const void* logits, const void* boxes, const float* target_sizes, int B, int nq, int ncls, int K,
                                  float* scores, int64_t* labels, float* out_boxes, float* packed, int dtype, void* hip_stream) {
    if (!logits || !boxes || !target_sizes || B < 0 || nq <= 0 || ncls <= 0 || K <= 0 ||
        K > TK_MAXK || (long)nq * ncls > (long)TK_IDX_MASK || K > nq * ncls)
        return LWDETR_ERR_BAD_ARG;
    if (B == 0) return LWDETR_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    ProfScope ps(KID_ELTWISE, 0.0, (double)B * nq * ncls * (dtype == DT_F32 ? 4 : 2), st);
    const size_t n = (size_t)nq * ncls;
    const bool cache = n * 4 <= TK_CACHE_BYTES;
    const bool small = n <= (size_t)TK_SMALL_N;
#define TK_LAUNCH(CACHE, THREADS)                                                                                                  \
    do {                                                                                                                            \
        if (CACHE && !tk_allow_lds((const void*)postprocess_kernel<TT, CACHE, THREADS>)) return LWDETR_ERR_LAUNCH;                  \
        hipLaunchKernelGGL((postprocess_kernel<TT, CACHE, THREADS>), dim3(B), dim3(THREADS), CACHE ? tk_cache_alloc(n) : 0, st,    \
                           (const TT*)logits, (const TT*)boxes, target_sizes, nq, ncls, K, scores, labels, out_boxes, packed);     \
    } while (0)
    LWDETR_DISPATCH_T(dtype, {
        if (small) TK_LAUNCH(true, TK_SMALL_THREADS);
        else if (cache) TK_LAUNCH(true, TK_LARGE_THREADS);
        else TK_LAUNCH(false, TK_LARGE_THREADS);
    });
#undef TK_LAUNCH
    return lwdetr_check_launch();
}

extern "C" int lwdetr_postprocess(const void* logits, const void* boxes, const float* target_sizes, int B, int nq, int ncls, int K,
                                  float* scores, int64_t* labels, float* out_boxes, int dtype, void* hip_stream) {
    if (!scores || !labels || !out_boxes) return LWDETR_ERR_BAD_ARG;
    return postprocess_impl(logits, boxes, target_sizes, B, nq, ncls, K, scores, labels, out_boxes, nullptr, dtype, hip_stream);
}

extern "C" int lwdetr_postprocess_packed(const void* logits, const void* boxes, const float* target_sizes, int B, int nq, int ncls,
                                         int K, float* packed, int dtype, void* hip_stream) {
    if (!packed) return LWDETR_ERR_BAD_ARG;
    return postprocess_impl(logits, boxes, target_sizes, B, nq, ncls, K, nullptr, nullptr, nullptr, packed, dtype, hip_stream);
}
