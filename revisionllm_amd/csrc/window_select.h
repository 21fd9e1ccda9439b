// The coarse window selection, one definition for both window rules: per row the duration from the mask, every window of the rule scored by the sum of
// its top-k sims, rank order, greedy selection with a minimum separation, top up in rank order, the first `keep` handed back ascending - one launch.
//   RULE = RV_WINDOWS_SHIFTED   stage2.cut_windows' windows (grounding.h ws_bounds): prefilter.hip, behind rv_window_select (include/revision_hip.h)
//   RULE = RV_WINDOWS_CLIPPED   stage1.cut_windows' windows (ws_bounds_clipped), the void ones left out: prefilter_ext.hip, behind
//                               rvx_window_select_clipped of the companion library (include/revision_hip_ext.h)
//   either RULE, with a frame set and a validity row: prefilter_chain.hip, behind rvc_window_select_frames of the chain library
//                               (include/revision_hip_chain.h); see FRAMES and MASKED in front of the kernel
// A window's score is accumulated add by add in rank order, as span_scores_kernel (similarity.hip) does it, and everything after the scores is integer
// work, so a row's result does not depend on R, on the row's place or on any tiling.
#pragma once
#include "grounding.h"

namespace {

constexpr int WS_TPB = 1024;         // 16 waves: the windows of a row are scored 16 at a time
constexpr int WS_WAVES = WS_TPB / 64;
constexpr int WS_REG = 16;           // a window of up to 64 * 16 frames is loaded once and ranked from registers
constexpr int WS_MAX_W = 2048;       // = SR_MAX of rv_span_rank
constexpr int WS_MAX_L = 1 << 20;    // = rv_span_propose's limit
constexpr int WS_PER = WS_MAX_W / WS_TPB;   // consecutive entries of a thread in the two prefix sums

struct WindowArgs {
    const float* sims;
    const float* mask;
    const float* gt;
    int32_t* select;
    int32_t* n_select;
    int32_t* n_windows;
    float* win_scores;
    int32_t* bounds;
    int32_t* order;
    int32_t* hit_rank;
    int L, rpm, win, stride, k, keep, min_sep, Wcap;
    const float* valid;          // (the frame-set instances only: prefilter_chain.hip)
    int32_t* n_candidates;
    int F;
};

constexpr int WS_FRAMES_ALL = 0;       // = RV_FRAMES_ALL of include/revision_hip_chain.h: a window's score reads its frames [lo, hi)
constexpr int WS_FRAMES_SAMPLED = 1;   // = RV_FRAMES_SAMPLED: it reads the F entries gw_linspace(lo, hi - 1, F, j) that rv_window_gather* hands on

// The frame order (grounding.h) as one unsigned number per frame, for a window held in registers: (frame key << 32 | frame index), SMALLER for what ranks earlier.
// A NaN has the key 0, a number its rank_key (from 0x007fffff for +inf to 0xff800000 for -inf; -0 as +0, so the index decides between them as
// rank_before()'s a.v == b.v does); 0xffffffff marks a slot behind the window's end.
__device__ __forceinline__ uint32_t ws_frame_key(float x) { return x != x ? 0u : rank_key(x); }
// the number behind a frame key != 0 (-0 comes back as +0: added to a sum that started at +0 it gives the same bits)
__device__ __forceinline__ float ws_key_value(uint32_t key) {
    const uint32_t asc = ~key;
    return __uint_as_float((asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc);
}
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t b = (uint64_t)__shfl_xor((unsigned long long)a, o, 64);
        a = b < a ? b : a;
    }
    return a;
}

__device__ __forceinline__ int wave_sum_i32(int a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    return a;
}
// the frame behind entry j of a window's frame set
template <int FRAMES>
__device__ __forceinline__ int ws_frame_at(int lo, int hi, int F, int j) {
    if constexpr (FRAMES == WS_FRAMES_SAMPLED) return gw_linspace(lo, hi - 1, F, j);
    else return lo + j;
}

// how many of the counts c of the threads before this one (all threads call; wsum: WS_WAVES ints)
__device__ __forceinline__ int ws_before(int c, int* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    return base + inc - c;
}

// The windows of a row of D frames under RULE: how many there are, and frames [lo, hi) of window i.  The clipped rule counts the windows that are not
// void: window i is void when (i * win) / 2 > D - 1, that is when i * win >= 2 D, so the non-void ones are the indices up to (2 D - 1) / win and the
// void ones a suffix of ws_count's range (an odd win only: an even one gives i * (win / 2) <= D - 1 for every i below ceil(D / (win / 2)) - 1).
template <int RULE>
__device__ __forceinline__ int ws_rule_count(int win, int stride, int D) {
    if constexpr (RULE == RV_WINDOWS_CLIPPED) {
        const int64_t W0 = ws_count(win, 2, D);
        const int64_t solid = D >= 1 ? (2 * (int64_t)D - 1) / win + 1 : 0;
        return (int)(solid < W0 ? solid : W0);
    } else {
        return ws_count(win, stride, D);
    }
}
template <int RULE>
__device__ __forceinline__ void ws_rule_bounds(int i, int win, int stride, int D, int& lo, int& hi) {
    if constexpr (RULE == RV_WINDOWS_CLIPPED) ws_bounds_clipped(i, win, D, lo, hi);      // (i < ws_rule_count: never void)
    else ws_bounds(i, win, stride, D, lo, hi);
}

// One workgroup per row.  (1) duration: block sum of the mask row; (2) the waves take windows in turn and score each with k wave-wide rank rounds over
// the lane-strided window - loaded once and kept as frame keys in registers when it has at most 64 * WS_REG frames, so that its loads are in flight
// together and a round is two 64-bit compares per frame and a wave-wide minimum; read again from the row in every round when it is longer (the same
// order, the same picks) - and the (key, index) pair goes to LDS; (3) bitonic sort of the pairs: ascending = rank order; (4) pass 1 walks the rank order with one live flag per WINDOW INDEX: every thread
// reads the pivot's flag (one broadcast read); a dead pivot costs nothing more, a live one is taken,
// the threads clear the flags of its neighbours (at most 2 min_sep - 2 of them; never its own, so that a slower thread still reads it as live) and one
// barrier follows.  The walk stops once `limit` windows are taken: n_select of them, or all W when order / hit_rank want the whole sequence (a greedy
// prefix does not depend on what follows it); (5) pass 2 puts the windows not taken behind them in rank order, places by a block prefix sum; (6) the
// first n_select entries are flagged by index and a second prefix sum hands them back ascending.
//
// FRAMES and MASKED (rvc_window_select_frames; the defaults are the kernel of rv_window_select and rvx_window_select_clipped, whose code they leave as it
// was): a window is scored on the entries of its frame set - every frame, or the F sampled ones, a frame that is sampled twice counting twice - that
// `valid` does not hide, in the frame order with ties to the smaller POSITION j in the set (under WS_FRAMES_ALL the frame index: the same order).  A
// sampled set has at most 64 * WS_REG entries and is always ranked from registers.  A window without a usable entry is no candidate: it gets the
// key 0xffffffff with bit 31 of the index half set, which sorts it behind every candidate (a NaN-scored one has that key with the bit clear) and with
// the padding, and everything behind the sort runs over the C candidates at the front.  COUNT: n_candidates is written.
template <int RULE, int FRAMES = WS_FRAMES_ALL, bool MASKED = false, bool COUNT = false>
__global__ __launch_bounds__(WS_TPB) void window_select_kernel(const WindowArgs a) {
    constexpr bool PLAIN = FRAMES == WS_FRAMES_ALL && !MASKED;
    __shared__ uint64_t keys[WS_MAX_W];      // key << 32 | index, ascending = rank order
    __shared__ uint16_t seq[WS_MAX_W];       // the selection sequence
    __shared__ uint8_t live[WS_MAX_W];       // by window index: pass 1's flags, then "among the first n_select"
    __shared__ uint8_t taken[WS_MAX_W];      // by window index
    __shared__ float red[WS_WAVES];
    __shared__ int wsum[WS_WAVES];
    __shared__ int first;
    __shared__ int ncand;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    const int L = a.L, win = a.win, stride = a.stride, Wcap = a.Wcap, keep = a.keep, min_sep = a.min_sep;
    const float* __restrict__ s = a.sims + r * L;
    const float* __restrict__ m = a.mask + (r / a.rpm) * L;

    if (tid == 0) first = 0x7fffffff;           // (in front of the sum: its barrier covers this store)
    if constexpr (MASKED)
        if (tid == 0) ncand = 0;
    const int D = duration_frames(block_mask_sum<WS_TPB>(m, L, red), L);
    const int W = ws_rule_count<RULE>(win, stride, D);   // (W <= Wcap: D <= L)
    int P = 1;
    while (P < W) P <<= 1;
    const bool to_bounds = a.bounds && r % a.rpm == 0;
    int32_t* __restrict__ bnd = to_bounds ? a.bounds + (r / a.rpm) * Wcap * 2 : nullptr;

    for (int i = wave; i < W; i += WS_WAVES) {
        int lo, hi;
        ws_rule_bounds<RULE>(i, win, stride, D, lo, hi);
        float acc = 0.f;
        bool cand = true;
        if constexpr (PLAIN) {
            const int rounds = a.k < hi - lo ? a.k : hi - lo;
            if (hi - lo <= 64 * WS_REG) {
                uint32_t kk[WS_REG];
#pragma unroll
                for (int j = 0; j < WS_REG; ++j) {
                    const int t = lo + lane + 64 * j;
                    kk[j] = t < hi ? ws_frame_key(s[t]) : 0xffffffffu;
                }
                uint64_t from = 0ull;                                       // the smallest (key, index) a round may still pick
                for (int q = 0; q < rounds; ++q) {
                    uint64_t best = ~0ull;
#pragma unroll
                    for (int j = 0; j < WS_REG; ++j) {
                        const uint64_t c = (uint64_t)kk[j] << 32 | (uint32_t)(lo + lane + 64 * j);
                        if (c >= from && c < best) best = c;
                    }
                    best = wave_min_u64(best);                              // (rounds <= hi - lo: a frame of the window, never an empty slot)
                    const uint32_t key = (uint32_t)(best >> 32);
                    acc = __fadd_rn(acc, key ? ws_key_value(key) : s[(uint32_t)best]);      // a NaN frame: its own bits from the row
                    from = best + 1ull;
                }
            } else {
                ArgMax prev = rank_start();
                for (int q = 0; q < rounds; ++q) {
                    ArgMax best = rank_none();
                    for (int t = lo + lane; t < hi; t += 64) best = rank_next(best, prev, ArgMax{s[t], t});
                    best = wave_rank_first(best);
                    acc = __fadd_rn(acc, best.v);
                    prev = best;
                }
            }
        } else {
            const float* __restrict__ vld = MASKED ? a.valid + (r / a.rpm) * L : nullptr;
            const int N = FRAMES == WS_FRAMES_SAMPLED ? a.F : hi - lo;      // entries of the frame set
            int n = N;                                                      // the usable ones
            if (FRAMES == WS_FRAMES_SAMPLED || N <= 64 * WS_REG) {
                uint32_t kk[WS_REG];
                int mine = 0;
#pragma unroll
                for (int j = 0; j < WS_REG; ++j) {
                    const int p = lane + 64 * j;
                    uint32_t key = 0xffffffffu;
                    if (p < N) {
                        const int t = ws_frame_at<FRAMES>(lo, hi, a.F, p);      // in [lo, hi): a frame of the row
                        bool use = true;
                        if constexpr (MASKED) use = vld[t] != 0.f;
                        if (use) {
                            key = ws_frame_key(s[t]);
                            ++mine;
                        }
                    }
                    kk[j] = key;
                }
                if constexpr (MASKED) n = wave_sum_i32(mine);
                const int rounds = a.k < n ? a.k : n;
                uint64_t from = 0ull;
                for (int q = 0; q < rounds; ++q) {
                    uint64_t best = ~0ull;
#pragma unroll
                    for (int j = 0; j < WS_REG; ++j) {
                        const uint64_t c = (uint64_t)kk[j] << 32 | (uint32_t)(lane + 64 * j);
                        if (c >= from && c < best) best = c;
                    }
                    best = wave_min_u64(best);                              // (rounds <= n: a usable entry, never an empty slot)
                    const uint32_t key = (uint32_t)(best >> 32);
                    acc = __fadd_rn(acc, key ? ws_key_value(key) : s[ws_frame_at<FRAMES>(lo, hi, a.F, (int)(uint32_t)best)]);
                    from = best + 1ull;
                }
            } else if constexpr (MASKED) {                                  // (every frame of a long window, some hidden)
                int mine = 0;
                for (int t = lo + lane; t < hi; t += 64) mine += vld[t] != 0.f ? 1 : 0;
                n = wave_sum_i32(mine);
                const int rounds = a.k < n ? a.k : n;
                ArgMax prev = rank_start();
                for (int q = 0; q < rounds; ++q) {
                    ArgMax best = rank_none();
                    for (int t = lo + lane; t < hi; t += 64)
                        if (vld[t] != 0.f) best = rank_next(best, prev, ArgMax{s[t], t});
                    best = wave_rank_first(best);
                    acc = __fadd_rn(acc, best.v);
                    prev = best;
                }
            }
            cand = n > 0;
        }
        if (lane == 0) {
            if constexpr (MASKED) {
                keys[i] = cand ? (uint64_t)rank_key(acc) << 32 | (uint32_t)i : (uint64_t)0xffffffffu << 32 | 0x80000000u | (uint32_t)i;
                if (a.win_scores) a.win_scores[r * Wcap + i] = cand ? acc : qnan();
                if (cand) atomicAdd(&ncand, 1);                              // (LDS; a count does not depend on the order of arrival)
            } else {
                keys[i] = (uint64_t)rank_key(acc) << 32 | (uint32_t)i;
                if (a.win_scores) a.win_scores[r * Wcap + i] = acc;
            }
            if (to_bounds) {
                bnd[2 * i] = lo;
                bnd[2 * i + 1] = hi;
            }
        }
    }
    for (int i = W + tid; i < Wcap; i += WS_TPB) {
        if (a.win_scores) a.win_scores[r * Wcap + i] = qnan();
        if (to_bounds) bnd[2 * i] = bnd[2 * i + 1] = -1;
        if (a.order) a.order[r * Wcap + i] = -1;
    }
    for (int i = tid; i < P; i += WS_TPB) {
        if (i >= W) keys[i] = (uint64_t)0xffffffffu << 32 | (MASKED ? 0x80000000u : 0u) | (uint32_t)i;
        live[i] = 1;
        taken[i] = 0;
    }
    __syncthreads();
    int C = W;                                // the candidates: the first C entries of the rank order
    if constexpr (MASKED) C = ncand;
    bitonic_sort_u64<WS_TPB>(keys, P);

    const int n_sel = keep < C ? keep : C;
    const int limit = (a.order || a.hit_rank) ? C : n_sel;
    if (min_sep == 1) {                      // nothing dies: the sequence is the rank order
        for (int p = tid; p < limit; p += WS_TPB) seq[p] = (uint16_t)(uint32_t)keys[p];
    } else {
        int nt = 0;
        for (int p = 0; p < C && nt < limit; ++p) {
            const int i = (int)(uint32_t)keys[p];
            if (!live[i]) continue;          // (the same value in every thread: the last write to it lies behind a barrier)
            if (tid == 0) {
                seq[nt] = (uint16_t)i;
                taken[i] = 1;
            }
            ++nt;
            if (nt < limit) {
                const int j1 = i + min_sep - 1 < W - 1 ? i + min_sep - 1 : W - 1;
                for (int j = (i - min_sep + 1 > 0 ? i - min_sep + 1 : 0) + tid; j <= j1; j += WS_TPB)
                    if (j != i) live[j] = 0;
            }
            __syncthreads();
        }
        __syncthreads();
        if (nt < limit) {                    // pass 1 ran dry: the rest in rank order
            int c = 0;
            for (int e = 0; e < WS_PER; ++e) {
                const int p = tid * WS_PER + e;
                c += (p < C && !taken[(uint32_t)keys[p]]) ? 1 : 0;
            }
            int pos = nt + ws_before(c, wsum);
            for (int e = 0; e < WS_PER; ++e) {
                const int p = tid * WS_PER + e;
                if (p < C) {
                    const int i = (int)(uint32_t)keys[p];
                    if (!taken[i]) {
                        if (pos < limit) seq[pos] = (uint16_t)i;
                        ++pos;
                    }
                }
            }
        }
    }
    __syncthreads();

    for (int i = tid; i < W; i += WS_TPB) live[i] = 0;
    if (a.order) {
        for (int p = tid; p < C; p += WS_TPB) a.order[r * Wcap + p] = seq[p];
        if constexpr (MASKED)
            for (int p = C + tid; p < W; p += WS_TPB) a.order[r * Wcap + p] = -1;
    }
    if (a.hit_rank) {
        const float gs = a.gt[r * 2], ge = a.gt[r * 2 + 1];
        if (span_solid(gs, ge)) {
            int mine = 0x7fffffff;
            for (int p = tid; p < C; p += WS_TPB) {                    // ascending p: the first one found is this thread's smallest
                int lo, hi;
                ws_rule_bounds<RULE>(seq[p], win, stride, D, lo, hi);
                if ((float)lo < ge && (float)hi > gs) {
                    mine = p;
                    break;
                }
            }
            if (mine != 0x7fffffff) atomicMin(&first, mine);           // (LDS; the minimum does not depend on the order of arrival)
        }
    }
    __syncthreads();
    for (int p = tid; p < n_sel; p += WS_TPB) live[seq[p]] = 1;
    __syncthreads();
    {
        int c = 0;
        for (int e = 0; e < WS_PER; ++e) {
            const int i = tid * WS_PER + e;
            c += (i < W && live[i]) ? 1 : 0;
        }
        int pos = ws_before(c, wsum);
        for (int e = 0; e < WS_PER; ++e) {
            const int i = tid * WS_PER + e;
            if (i < W && live[i]) a.select[r * keep + pos++] = i;
        }
    }
    for (int p = n_sel + tid; p < keep; p += WS_TPB) a.select[r * keep + p] = -1;
    if (tid == 0) {
        a.n_select[r] = n_sel;
        a.n_windows[r] = W;
        if constexpr (COUNT) a.n_candidates[r] = C;
        if (a.hit_rank) a.hit_rank[r] = first == 0x7fffffff ? -1 : first;
    }
}

}  // namespace

