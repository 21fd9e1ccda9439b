// What the stages of the CLIP grounding chain share, one definition each: the frame order of the score kernels, the rank key of a score, the bitonic
// sort of (key, index) pairs, the two duration sums (block_mask_sum, and span_mask_sum for the span kernels) with the duration rule, the span rules
// (SPAN_NOT_FINITE and span_slice: a span's frame window; span_encode: a frame window's (centre, width); sim_usable / sim_quantise: a usable similarity as an integer;
// contrast_f64: the contrast of exact integer sums), the two window rules (stage 2's shifted windows, stage 1's clipped ones), the sampled frames of a
// window and the small helpers around them.  Included by the chain's translation units only (sample.hip for rv_topk_cosine / rv_topk_pool,
// similarity.hip, rank.hip, propose.hip, prefilter.hip, prefilter_ext.hip, gather.hip, and the chain library's prefilter_chain.hip, spans_chain.hip,
// valid_chain.hip, refine_chain.hip, anchors_chain.hip): two stages that have to agree bit for bit call the same code.
#pragma once
#include "kernels.h"

namespace {

constexpr int TOPK_FRAMES_MAX = 64;   // the most frames a top-k score adds up: k of rv_span_scores(_multi), rv_topk_pool and rv_window_select

__device__ __forceinline__ float qnan() { return __int_as_float(0x7fc00000); }
__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }
__device__ __forceinline__ int top_bit(uint64_t w) { return 63 - __clzll((long long)w); }   // w != 0
__device__ __forceinline__ bool span_solid(float s, float e) { return fabsf(s) < INFINITY && fabsf(e) < INFINITY && e > s; }   // not void

template <typename T>
__device__ __forceinline__ float ld(const T* p);
template <>
__device__ __forceinline__ float ld<float>(const float* p) { return *p; }
template <>
__device__ __forceinline__ float ld<op16_t>(const op16_t* p) { return op16_to_f32(*p); }

// VEC features from p as f32: one element, or one 16-byte load (VEC = 16 B / sizeof(T), p 16-byte aligned)
template <typename T, int VEC>
__device__ __forceinline__ void load_features(const T* p, float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = ld<T>(p);
    } else if constexpr (sizeof(T) == 2) {
        const op16x8 r = *(const op16x8*)p;
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = op16_to_f32((op16_t)r[e]);
    } else {
        const f32x4 r = *(const f32x4*)p;
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = r[e];
    }
}

// ---- frame order ----
// The order of the score kernels (torch.topk's): NaN before every number, then the larger value, then the smaller frame index.  A strict total
// order over (value, index) pairs with distinct indices, so "the first entry strictly after the previous pick" walks the frames in rank order
// without marking the picked ones: no round can return a frame twice or, while rounds <= frames, none at all.
struct ArgMax {
    float v;
    int i;
};
__device__ __forceinline__ bool rank_before(ArgMax a, ArgMax b) {  // a ranks strictly before b
    const bool an = a.v != a.v, bn = b.v != b.v;
    if (an != bn) return an;
    return (an || a.v == b.v) ? a.i < b.i : a.v > b.v;
}
__device__ __forceinline__ ArgMax rank_none() { return ArgMax{-INFINITY, 0x7fffffff}; }   // after every frame's entry
__device__ __forceinline__ ArgMax rank_start() { return ArgMax{qnan(), -1}; }             // before every frame's entry
__device__ __forceinline__ ArgMax rank_next(ArgMax best, ArgMax prev, ArgMax c) {  // the earlier of best and c among the entries after prev
    return (rank_before(prev, c) && rank_before(c, best)) ? c : best;
}
__device__ __forceinline__ ArgMax wave_rank_first(ArgMax a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ArgMax b{__shfl_xor(a.v, o, 64), __shfl_xor(a.i, o, 64)};
        a = rank_before(b, a) ? b : a;
    }
    return a;
}

// ---- score key ----
// Rank key of a score: an unsigned number that is SMALLER for what ranks earlier.  Numbers in descending order (-0 counts as +0, so the index decides
// between them), every NaN behind -inf with the largest key.  Ties go to the smaller index: the pair (key, index) is compared, and a padding entry
// carries the NaN key with an index past the row's entries, so it lands behind all of them.
__device__ __forceinline__ uint32_t rank_key(float x) {
    if (x != x) return 0xffffffffu;
    uint32_t b = (uint32_t)__float_as_int(x);
    if (b == 0x80000000u) b = 0u;
    const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // ascending with the value
    return ~asc;                                                         // (-inf: 0xff800000, below the NaN key)
}

// ---- sort ----
// Bitonic sort of keys[0, P) in LDS, ascending, by the TPB threads of the block (all call; P a power of two; the caller's stores to keys lie behind a
// barrier, and one ends every step here)
template <int TPB>
__device__ __forceinline__ void bitonic_sort_u64(uint64_t* keys, int P) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += TPB) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;      // the pair (i, i + j), bit j of i clear
                const uint64_t a = keys[i], b = keys[l];
                if ((a > b) == ((i & k) == 0)) {
                    keys[i] = b;
                    keys[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

// ---- duration ----
// The sum of a mask row, the same bits in every thread of the block (all call; red: TPB / 64 floats of LDS): per-thread partials over the frames
// tid, tid + TPB, .., the wave's sum, then the waves' sums from left to right, every add rounded on its own.  One barrier, behind the stores to red.
template <int TPB>
__device__ __forceinline__ float block_mask_sum(const float* __restrict__ m, int L, float* red) {
    float part = 0.f;
    for (int i = threadIdx.x; i < L; i += TPB) part = __fadd_rn(part, m[i]);
    part = wave_sum(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    float dur = red[0];
#pragma unroll
    for (int w = 1; w < TPB / 64; ++w) dur = __fadd_rn(dur, red[w]);
    return dur;
}
// D = min(L, floor(dur)) frames; none for a sum that is not finite or below 1
__device__ __forceinline__ int duration_frames(float dur, int L) {
    if (!(fabsf(dur) < INFINITY && dur >= 1.f)) return 0;
    return dur >= (float)L ? L : (int)floorf(dur);
}

// ---- spans ----
// The span kernels' sum of the mask row of row `row` - row / rpm of `mask`, L floats a row; the address is made inside the adding threads' branch, where
// the kernels had it - (span_scores_kernel, span_refine_kernel, span_anchors_kernel), the same bits in every thread of the block: the
// raw f32 sum over the frames tid, tid + 256, .. of the block's first 256 threads, the wave's sum, then the four wave partials added pairwise,
// (r0 + r1) + (r2 + r3).  NOT block_mask_sum(): other bits on a mask that is not 0 / 1.  All TPB threads of the block call (TPB >= 256; a larger
// block's other threads only wait); red: 4 floats of LDS.  One barrier, behind the stores to red and in front of its loads: part of the contract -
// no thread may leave the kernel before the call, and what the caller stored to LDS before it is visible behind it.
template <int TPB, typename Row>
__device__ __forceinline__ float span_mask_sum(const float* __restrict__ mask, Row row, int rpm, int L, float* red) {
    const int tid = threadIdx.x;
    if (TPB == 256 || tid < 256) {
        const float* m = mask + (int64_t)(row / rpm) * L;      // (inside the branch: the threads that only wait do not divide)
        float s = 0.f;
        for (int l = tid; l < L; l += 256) s += m[l];
        s = wave_sum(s);
        if ((tid & 63) == 0) red[tid >> 6] = s;
    }
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// f32 -> int32 as torch's .to(torch.int32) gives it for the values the reference meets; outside int32's range (undefined there) the value saturates
__device__ __forceinline__ int sat_i32(float v) {
    return v >= 2147483648.f ? 0x7fffffff : (v <= -2147483648.f ? (int)0x80000000 : (int)v);
}
// The frame window [lo, hi) of a span in a row of L frames, the reference's rule.  The caller scales the span's ends x1 and x2 (fractions of the duration;
// c - 0.5 w and c + 0.5 w, or start and end: its form) to frames, p = __fmul_rn(x, dur), and tests them ITSELF, SPAN_NOT_FINITE(p1, p2) -> a void span, the
// window (-1, -1): the test and its branch stay in the kernel's text because a helper that returns it makes the compiler lay the kernel out otherwise
// (the block of the void span in front of the body; profiles/grounding_rules_isa.txt).  span_slice then gives, for finite p1 and p2,
// start = max(0, int(floor(p1))), end = int(ceil(p2)) and Python's range(L)[start:end] over the ARRAY length L: lo = min(start, L),
// hi = end < 0 ? max(end + L, 0) : min(end, L).
#define SPAN_NOT_FINITE(p1, p2) (!(fabsf(p1) < INFINITY) || !(fabsf(p2) < INFINITY))      /* NaN or +-inf */
__device__ __forceinline__ void span_slice(float p1, float p2, int L, int& lo, int& hi) {
    int start = sat_i32(floorf(p1));
    start = start < 0 ? 0 : start;
    const int end = sat_i32(ceilf(p2));
    lo = start < L ? start : L;
    if (end < 0) { hi = end + L; hi = hi < 0 ? 0 : hi; }
    else hi = end < L ? end : L;
}
// The (centre, width) of the frame window [lo, hi) as the span generators hand it on: c = ((lo + hi) * 0.5) / dur, w = ((hi - lo) - 0.5) / dur, every
// operation rounded to f32 on its own.  span_slice() of it scaled by the same dur gives [lo, hi) back.
__device__ __forceinline__ void span_encode(int lo, int hi, float dur, float& c, float& w) {
    const float flo = (float)lo, fhi = (float)hi;
    c = __fdiv_rn(__fmul_rn(__fadd_rn(flo, fhi), 0.5f), dur);
    w = __fdiv_rn(__fsub_rn(__fsub_rn(fhi, flo), 0.5f), dur);
}
// A similarity that is not a number is never usable; a usable one counts as the integer round(clamp(v, -1, 1) * 2^24): an exact product, ties to even,
// +-inf clamps to +-1.  Sums of these are exact, so no result depends on the order of a scan or a reduction.  (When the similarity is loaded - behind
// the validity entry or next to it - is the caller's.)
__device__ __forceinline__ bool sim_usable(float v) { return v == v; }
__device__ __forceinline__ long long sim_quantise(float v) {
    return (long long)__float2int_rn(__fmul_rn(fminf(fmaxf(v, -1.f), 1.f), 16777216.f));
}
// J = Sin / Cin - Sout / Cout in float64 from exact integer sums and counts (two divisions and a subtraction, each rounded on its own).  Whether the
// pair is admissible is the caller's test, and so is what stands in for a count of 0.
__device__ __forceinline__ double contrast_f64(long long Sin, int Cin, long long Sout, int Cout) {
    return __dsub_rn(__ddiv_rn((double)Sin, (double)Cin), __ddiv_rn((double)Sout, (double)Cout));
}

// ---- windows ----
// frames [lo, hi) of window i of a row of D frames: stage2.cut_windows' rule in integers, the start clamped at 0 (rv_window_select scores these
// windows, rv_window_gather samples them: an index means the same window in both)
__device__ __forceinline__ void ws_bounds(int i, int win, int stride, int D, int& lo, int& hi) {
    int64_t s = (int64_t)i * win / stride;
    int64_t e = s + win < (int64_t)D - 1 ? s + win : (int64_t)D - 1;
    if (e - s < win) s = e - win;
    lo = s > 0 ? (int)s : 0;
    hi = (int)e + 1;
}
// W_r = max(0, ceil(D / hop) - 1) windows, hop = win / stride
__device__ __forceinline__ int ws_count(int win, int stride, int D) {
    const int hop = win / stride;
    const int W = (D + hop - 1) / hop - 1;
    return W < 0 ? 0 : W;
}
// frames [lo, hi) of window i of stage1.cut_windows' rule (half-overlapping windows, the last ones clipped at D - 1 and NOT shifted back): there are
// ws_count(win, 2, D) of them, s = (i * win) / 2 (for an odd win not i * (win / 2)), e = min(s + win, D - 1).  -> false for a void window (s > e:
// an odd win only, first at D = 15 for win = 5, where the host's linspace runs past the array); s == e is a window of one frame.
__device__ __forceinline__ bool ws_bounds_clipped(int i, int win, int D, int& lo, int& hi) {
    const int64_t s = (int64_t)i * win / 2;
    const int64_t e = s + win < (int64_t)D - 1 ? s + win : (int64_t)D - 1;
    lo = (int)s;
    hi = (int)e + 1;
    return s <= e;
}

// ---- sampled frames ----
// np.linspace(s, e, F, dtype=int32)[j]: step = (e - s) / (F - 1), y = j * step (or (j * (e - s)) / (F - 1) when the step is 0), y += s, the last one is e,
// floor - numpy's float64 operations in numpy's order, the multiply and the add rounded each on its own (no contraction inside this body).  The result
// lies in [s, e] (j * step <= (F - 2) / (F - 1) * (e - s) * (1 + 2^-52)^2 < e - s); the clamp states that for the loads that follow and changes no
// value.  rv_window_gather* samples a window's frames with it and rvc_window_select_frames scores those samples: entry j means the same frame in both.
__device__ __forceinline__ int gw_linspace(int s, int e, int F, int j) {
#pragma clang fp contract(off)
    if (F == 1) return s;
    if (j == F - 1) return e;
    const double delta = (double)(e - s), div = (double)(F - 1);
    const double step = __ddiv_rn(delta, div);
    double y = step == 0.0 ? __ddiv_rn(__dmul_rn((double)j, delta), div) : __dmul_rn((double)j, step);
    y = __dadd_rn(y, (double)s);
    const int idx = (int)floor(y);
    return idx < s ? s : idx > e ? e : idx;
}

}  // namespace
