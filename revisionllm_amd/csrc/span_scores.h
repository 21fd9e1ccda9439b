// The span-score kernel of the CLIP grounding chain, one source for rv_span_scores / rv_span_scores_multi (similarity.hip: the default instances) and
// rvc_span_scores_masked / rvc_span_scores_masked_rows (spans_chain.hip: MASKED = true, a per-frame validity row and / or the non-finite similarities skipped).  The window rule
// is SPAN_NOT_FINITE / span_slice() of grounding.h, the duration span_mask_sum(): the entries agree on a window bit for bit because they run this code.
#pragma once
#include "grounding.h"

namespace {

// What the masked instances take beyond the default ones' arguments (nothing, for those: their argument list is the parent's)
template <bool MASKED>
struct SpanMasking {};
template <>
struct SpanMasking<true> {
    const float* valid;      // f32 [rows / rpv, L] or null: every frame inside the window counts
    int32_t* n_usable;       // i32 [rows, N] or null
    int skip_nan;            // 1: a frame whose similarity is NaN is hidden as well
    int rpv;                 // "rows per validity row": rpm for rvc_span_scores_masked (one per mask row), 1 for a validity row per row of sims
};

// One wave per span (4 spans per block, all of row blockIdx.y).  A row is a video (rpm = 1, rv_span_scores) or one of a video's rpm queries
// (rv_span_scores_multi): similarities, spans and outputs are indexed by the row, the mask - and hence the duration - by row / rpm ("rows per mask").
// The block adds the row's mask row up first (span_mask_sum: the duration; 0 / 1 masks: exact in any
// order up to 2^24 frames; every block of a video repeats that sum - N / 4 reads of an L2-resident row of 4 L bytes - which is the price of keeping the
// matching call at two launches with no pass of its own for B numbers), then each wave turns its (centre, width) into the reference's slice of the similarity row (span_slice):
//   x1 = c - 0.5 w, x2 = c + 0.5 w, p = x * duration (every operation rounded to f32 on its own: no contraction), start = max(0, int(floor(p1))),
//   end = int(ceil(p2)), and Python's range(L)[start:end] over the ARRAY length L: lo = min(start, L), hi = end < 0 ? max(end + L, 0) : min(end, L).
// Every read of sims lies in [b L + lo, b L + hi).  MODE 0: the sum of the min(k, hi - lo) first entries in rank order (NaN, larger value, smaller
// index: k wave-wide rank rounds over a lane-strided window, no LDS); MODE 1: sum_t softmax_t(s / tau) s_t in two lane-strided passes - the maximum, then both sums - (a NaN in
// the window is carried next to the running maximum, which fmaxf would drop).  An empty window scores 0; a non-finite p1 / p2 gives NaN and the
// window (-1, -1).
// MASKED: frame t of the window is USABLE when its validity entry (row b / rpv, read only where sims is read) is not 0 and, under skip_nan, its
// similarity is a number; a hidden frame's similarity enters no comparison and no sum (it is skipped, not multiplied by 0).  With n usable frames the
// rank rounds are min(k, n) and walk the usable frames only, the softmax runs over them only, a window with hi > lo and n = 0 scores NaN, and
// n_usable takes n (0 for an empty or void span).
template <int MODE, bool MASKED = false>
__global__ __launch_bounds__(256) void span_scores_kernel(const float* __restrict__ sims, const float* __restrict__ spans, const float* __restrict__ mask,
                                                          int rpm, int L, int N, int k, float tau, float* __restrict__ scores,
                                                          int32_t* __restrict__ windows, const SpanMasking<MASKED> mk) {
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float duration = span_mask_sum<256>(mask, b, rpm, L, red);
    const int n = blockIdx.x * 4 + wave;
    if (n >= N) return;
    const int64_t sp = (int64_t)b * N + n;
    const float c = spans[sp * 2], w = spans[sp * 2 + 1];
    const float hw = __fmul_rn(0.5f, w);
    const float p1 = __fmul_rn(__fsub_rn(c, hw), duration), p2 = __fmul_rn(__fadd_rn(c, hw), duration);
    if (SPAN_NOT_FINITE(p1, p2)) {
        if (lane == 0) {
            scores[sp] = qnan();
            if (windows) windows[sp * 2] = windows[sp * 2 + 1] = -1;
            if constexpr (MASKED) {
                if (mk.n_usable) mk.n_usable[sp] = 0;
            }
        }
        return;
    }
    int lo, hi;
    span_slice(p1, p2, L, lo, hi);
    if (lane == 0 && windows) {
        windows[sp * 2] = lo;
        windows[sp * 2 + 1] = hi;
    }
    const float* s = sims + (int64_t)b * L;
    float acc = 0.f;
    if constexpr (!MASKED) {
        if (hi > lo) {
            if constexpr (MODE == 0) {
                ArgMax prev = rank_start();
                const int rounds = k < hi - lo ? k : hi - lo;
                for (int r = 0; r < rounds; ++r) {
                    ArgMax best = rank_none();
                    for (int t = lo + lane; t < hi; t += 64) best = rank_next(best, prev, ArgMax{s[t], t});
                    best = wave_rank_first(best);
                    acc += best.v;
                    prev = best;
                }
            } else {
                float mx = -INFINITY;
                bool nan = false;
                for (int t = lo + lane; t < hi; t += 64) {
                    const float x = s[t] / tau;
                    nan |= x != x;
                    mx = fmaxf(mx, x);
                }
                mx = wave_max(mx);
                if (__ballot(nan) != 0ull) mx = qnan();
                float z = 0.f, zs = 0.f;
                for (int t = lo + lane; t < hi; t += 64) {
                    const float v = s[t];
                    const float e = expf(v / tau - mx);
                    z += e;
                    zs += e * v;
                }
                acc = wave_sum(zs) / wave_sum(z);
            }
        }
    } else {
        const float* vr = mk.valid ? mk.valid + (int64_t)(b / mk.rpv) * L : nullptr;
        const bool skip = mk.skip_nan != 0;
        // (t in [lo, hi): the validity entry first, the similarity only behind a usable one; v: the similarity of a usable frame)
        auto usable = [&](int t, float& v) {
            if (vr && !(vr[t] != 0.f)) return false;
            v = s[t];
            return !(skip && v != v);
        };
        int nu = 0;
        if (hi > lo) {
            for (int t = lo + lane; t < hi; t += 64) {
                float v;
                nu += usable(t, v) ? 1 : 0;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nu += __shfl_xor(nu, o, 64);
            if (nu == 0) {
                acc = qnan();
            } else if constexpr (MODE == 0) {
                ArgMax prev = rank_start();
                const int rounds = k < nu ? k : nu;
                for (int r = 0; r < rounds; ++r) {
                    ArgMax best = rank_none();
                    for (int t = lo + lane; t < hi; t += 64) {
                        float v;
                        if (usable(t, v)) best = rank_next(best, prev, ArgMax{v, t});
                    }
                    best = wave_rank_first(best);
                    acc += best.v;
                    prev = best;
                }
            } else {
                float mx = -INFINITY;
                bool nan = false;
                for (int t = lo + lane; t < hi; t += 64) {
                    float v;
                    if (usable(t, v)) {
                        const float x = v / tau;
                        nan |= x != x;
                        mx = fmaxf(mx, x);
                    }
                }
                mx = wave_max(mx);
                if (__ballot(nan) != 0ull) mx = qnan();
                float z = 0.f, zs = 0.f;
                for (int t = lo + lane; t < hi; t += 64) {
                    float v;
                    if (usable(t, v)) {
                        const float e = expf(v / tau - mx);
                        z += e;
                        zs += e * v;
                    }
                }
                acc = wave_sum(zs) / wave_sum(z);
            }
        }
        if (lane == 0 && mk.n_usable) mk.n_usable[sp] = nu;
    }
    if (lane == 0) scores[sp] = acc;
}

}  // namespace
