// The span-proposal kernel of the CLIP grounding chain, one source for rv_span_propose (propose.hip: the default instance) and rvc_span_propose_masked[_rows]
// (spans_chain.hip: MASKED = true, a per-frame validity row and / or the non-finite similarities skipped), with the smoothing and the refusals the two
// entries share.  The definition stands in include/revision_hip.h, what MASKED changes in include/revision_hip_chain.h.  Every f32 operation is rounded
// on its own (__fadd_rn, __fsub_rn, __fmul_rn, __fdiv_rn), so a row's result does not depend on R, on the row's place or on the tiling.
#pragma once
#include <type_traits>

#include "grounding.h"

namespace {

constexpr int SP_TPB = 256;          // 4 waves; a tile is 256 frames, one per thread
constexpr int SP_LEVELS = 8;
constexpr int SP_HALO = 32;          // smooth <= 65
constexpr int SP_MAX_N = 2048;       // = SR_MAX of rv_span_rank
constexpr int SP_MAX_L = 1 << 20;    // the span encoding gives back (lo, hi) up to here

struct ProposeArgs {
    const float* sims;
    const float* mask;
    float* spans;
    int32_t* n_spans;
    int32_t* n_found;
    int32_t* windows;
    float* smoothed;
    int L, rpm, T, relative, h, gap, min_len, max_len, N;
    float levels[SP_LEVELS];
};
// the masked instance's argument block: the default one's (unchanged, so the default instance's argument loads are the parent's) and the validity behind it
struct ProposeMaskedArgs : ProposeArgs {
    const float* valid;      // f32 [R / rpv, L] or null
    int skip_nan;            // 1: a frame whose similarity is NaN is hidden as well
    int rpv;                 // "rows per validity row": rpm for rvc_span_propose_masked (one per mask row), 1 for a validity row per row of sims
};
template <bool MASKED>
using ProposeArgsOf = std::conditional_t<MASKED, ProposeMaskedArgs, ProposeArgs>;

// s'[t0 + tid] of the row whose first D frames are s (NaN for a frame at or past D).  The tile and a halo of h frames on each side are staged in LDS;
// no frame outside [0, D) is read.  The adds run in ascending order and one division follows.  The caller puts a barrier between two calls.
// MASKED: a frame is USABLE when its validity entry (vr, read only where s is read; null: every frame) is not 0 and, under skip, its similarity is a
// number; `ok` holds that beside the staged row (a hidden frame is staged as 0 and its similarity is not read unless skip has to look at it).  s' of a
// usable frame is the sum of the usable frames of its box in ascending order from the first usable one, divided by their count; s' of a hidden frame
// is NaN.
template <bool MASKED>
__device__ __forceinline__ float sp_smooth(const float* __restrict__ s, float* stage, int t0, int D, int h, const float* __restrict__ vr = nullptr,
                                           bool skip = false, unsigned char* ok = nullptr) {
    const int tid = threadIdx.x;
    for (int i = tid; i < SP_TPB + 2 * h; i += SP_TPB) {
        const int g = t0 - h + i;
        if constexpr (MASKED) {
            float v = 0.f;
            bool u = g >= 0 && g < D;
            if (u && vr) u = vr[g] != 0.f;
            if (u) {
                v = s[g];
                if (skip && v != v) {
                    u = false;
                    v = 0.f;
                }
            }
            stage[i] = v;
            ok[i] = u ? 1 : 0;
        } else {
            stage[i] = (g >= 0 && g < D) ? s[g] : 0.f;
        }
    }
    __syncthreads();
    const int t = t0 + tid;
    float v = qnan();
    if constexpr (MASKED) {
        if (t < D && ok[h + tid]) {
            const int a = max(0, t - h), b = min(D - 1, t + h);
            const float* w = stage + (h - t0);                  // w[j] = s[j] for the frames staged
            const unsigned char* u = ok + (h - t0);
            float sum = 0.f;
            int cnt = 0;
            for (int j = a; j <= b; ++j) {
                if (u[j]) {
                    sum = cnt ? __fadd_rn(sum, w[j]) : w[j];
                    ++cnt;
                }
            }
            v = __fdiv_rn(sum, (float)cnt);                     // (cnt >= 1: frame t itself)
        }
    } else if (t < D) {
        const int a = max(0, t - h), b = min(D - 1, t + h);
        const float* w = stage + (h - t0);                      // w[j] = s[j] for the frames staged
        float sum = w[a];
        for (int j = a + 1; j <= b; ++j) sum = __fadd_rn(sum, w[j]);
        v = __fdiv_rn(sum, (float)(b - a + 1));
    }
    return v;
}

// One workgroup per row.  Three walks over the row's tiles: (1) s' -> mx / mn (and the `smoothed` output), (2) detection that counts the surviving runs
// of every level, (3) the same detection, now storing each run at its place (levels T-1 .. 0, ascending lo inside a level).  The row stays in L2.
// Detection: per level and wave one ballot word of the "above" bits; the words of three consecutive tiles sit in a ring in LDS, and tile k-1 is examined
// once tile k's words are there, so the gap + 1 <= 64 frames before and after a frame are one 64-bit word each whatever wave or tile edge lies between.
// A frame starts a run when no above bit lies in the gap + 1 frames before it and ends one when none lies in the gap + 1 frames after it.  The thread on
// a run's end finds its lo: the last start at or before it in its wave's start word, else in the earlier waves' words (LDS), else the open run's lo the
// block carries across tiles.  It knows (lo, hi) of every level that ends there, so the length filter and the level l + 1 duplicate test are its own.
// Places: the block carries each level's count; inside a tile the emit words of the earlier waves (LDS) and the lower lanes give the rest.
// MASKED changes the smoothing alone (sp_smooth): a hidden frame's s' is NaN, so it drops out of the range and is never above like any other NaN.
template <bool MASKED = false>
__global__ __launch_bounds__(SP_TPB) void span_propose_kernel(const ProposeArgsOf<MASKED> a) {
    __shared__ float stage[SP_TPB + 2 * SP_HALO];
    __shared__ uint64_t bits[SP_LEVELS][12];                    // ring of 3 tiles x 4 wave words
    __shared__ uint64_t starts[SP_LEVELS][4], emits[SP_LEVELS][4];
    __shared__ float red[3][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    const int L = a.L, T = a.T, h = a.h, N = a.N;
    const float* __restrict__ s = a.sims + r * L;
    const float* __restrict__ m = a.mask + (r / a.rpm) * L;
    unsigned char* ok = nullptr;
    if constexpr (MASKED) {
        __shared__ unsigned char usable[SP_TPB + 2 * SP_HALO];
        ok = usable;
    }
    auto smooth_tile = [&](int t0, int D) {
        if constexpr (MASKED) {
            return sp_smooth<true>(s, stage, t0, D, h, a.valid ? a.valid + (int64_t)((int)blockIdx.x / a.rpv) * L : nullptr, a.skip_nan != 0, ok);
        } else {
            return sp_smooth<false>(s, stage, t0, D, h);
        }
    };

    const float dur = block_mask_sum<SP_TPB>(m, L, red[0]);
    const int D = duration_frames(dur, L);
    const int ntiles = (D + SP_TPB - 1) / SP_TPB;

    // (1) s', its largest and smallest number (a NaN is skipped)
    float mx = -INFINITY, mn = INFINITY;
    for (int k = 0; k < ntiles; ++k) {
        const float v = smooth_tile(k * SP_TPB, D);
        const int t = k * SP_TPB + tid;
        if (t < D) {
            if (a.smoothed) a.smoothed[r * L + t] = v;
            if (v == v) {
                mx = fmaxf(mx, v);
                mn = fminf(mn, v);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        mn = fminf(mn, __shfl_xor(mn, o, 64));
    }
    if (lane == 0) {
        red[1][wave] = mx;
        red[2][wave] = mn;
    }
    __syncthreads();
    mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    mn = fminf(fminf(red[2][0], red[2][1]), fminf(red[2][2], red[2][3]));
    float theta[SP_LEVELS];
#pragma unroll
    for (int l = 0; l < SP_LEVELS; ++l) {
        const float lv = a.levels[l < T ? l : 0];
        theta[l] = a.relative ? __fadd_rn(mn, __fmul_rn(lv, __fsub_rn(mx, mn))) : lv;
    }

    const int g1 = a.gap + 1;
    int base[SP_LEVELS], cnt[SP_LEVELS], open_lo[SP_LEVELS];
#pragma unroll
    for (int l = 0; l < SP_LEVELS; ++l) base[l] = 0;
    int found = 0;
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int l = 0; l < SP_LEVELS; ++l) cnt[l] = open_lo[l] = 0;
        if (tid < SP_LEVELS * 12) (&bits[0][0])[tid] = 0ull;
        __syncthreads();
        for (int k = 0; k <= ntiles; ++k) {
            const int slot = (k % 3) * 4;
            if (k < ntiles) {                                   // tile k's above words
                const float v = smooth_tile(k * SP_TPB, D);
#pragma unroll
                for (int l = 0; l < SP_LEVELS; ++l) {
                    if (l < T) {
                        const uint64_t wd = __ballot(v > theta[l]);     // (a NaN, and with it a frame past D, is never above)
                        if (lane == 0) bits[l][slot + wave] = wd;
                    }
                }
            } else if (tid < SP_LEVELS * 4) {                   // behind the row's end: nothing above
                bits[tid >> 2][slot + (tid & 3)] = 0ull;
            }
            __syncthreads();
            if (k == 0) continue;
            // tile k-1: its words, the last word of tile k-2 before them, the first word of tile k behind them
            const int t0 = (k - 1) * SP_TPB, t = t0 + tid;
            const int cur_i = ((k - 1) % 3) * 4 + wave;
            const int prev_i = wave > 0 ? cur_i - 1 : ((k + 1) % 3) * 4 + 3;
            const int next_i = wave < 3 ? cur_i + 1 : slot;
            uint32_t ends = 0u;
            int lo[SP_LEVELS], place[SP_LEVELS];
#pragma unroll
            for (int l = 0; l < SP_LEVELS; ++l) {
                lo[l] = -1;
                if (l < T) {
                    const uint64_t cur = bits[l][cur_i], prv = bits[l][prev_i], nxt = bits[l][next_i];
                    const bool above = (cur >> lane) & 1ull;
                    const uint64_t back = lane > 0 ? (cur << (64 - lane)) | (prv >> lane) : prv;              // bit i: frame t - 64 + i
                    const uint64_t fwd = lane < 63 ? (cur >> (lane + 1)) | (nxt << (63 - lane)) : nxt;        // bit i: frame t + 1 + i
                    const bool st = above && (back >> (64 - g1)) == 0ull;
                    const bool en = above && (fwd & low_bits(g1)) == 0ull;
                    const uint64_t sw = __ballot(st);
                    if (lane == 0) starts[l][wave] = sw;
                    const uint64_t mine = sw & low_bits(lane + 1);
                    if (mine) lo[l] = t0 + wave * 64 + top_bit(mine);
                    if (en) ends |= 1u << l;
                }
            }
            __syncthreads();
            uint32_t emit = 0u;
#pragma unroll
            for (int l = SP_LEVELS - 1; l >= 0; --l) {
                if (l < T) {
                    bool e = false;
                    if ((ends >> l) & 1u) {
                        for (int w = wave - 1; w >= 0 && lo[l] < 0; --w) {
                            const uint64_t sw = starts[l][w];
                            if (sw) lo[l] = t0 + w * 64 + top_bit(sw);
                        }
                        if (lo[l] < 0) lo[l] = open_lo[l];
                        const int len = t + 1 - lo[l];
                        e = len >= a.min_len && (a.max_len == 0 || len <= a.max_len);
                        const int up =l + 1 < SP_LEVELS ? l + 1 : l;
                        if (l < T - 1 && ((ends >> up) & 1u) && lo[up] == lo[l]) e = false;      // level l + 1 has a run with this (lo, hi)
                    }
                    const uint64_t ew = __ballot(e);
                    if (lane == 0) emits[l][wave] = ew;
                    place[l] = __popcll(ew & low_bits(lane));
                    if (e) emit |= 1u << l;
                }
            }
            __syncthreads();
#pragma unroll
            for (int l = 0; l < SP_LEVELS; ++l) {
                if (l < T) {
                    int before = 0, all = 0, last = -1;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const int c = __popcll(emits[l][w]);
                        if (w < wave) before += c;
                        all += c;
                        const uint64_t sw = starts[l][w];
                        if (sw) last = t0 + w * 64 + top_bit(sw);
                    }
                    if (pass == 1 && ((emit >> l) & 1u)) {
                        const int pos = base[l] + cnt[l] + before + place[l];
                        if (pos < N) {
                            const int64_t o = (r * N + pos) * 2;
                            span_encode(lo[l], t + 1, dur, a.spans[o], a.spans[o + 1]);
                            if (a.windows) {
                                a.windows[o] = lo[l];
                                a.windows[o + 1] = t + 1;
                            }
                        }
                    }
                    cnt[l] += all;
                    if (last >= 0) open_lo[l] = last;
                }
            }
        }
        if (pass == 0) {
#pragma unroll
            for (int l = SP_LEVELS - 1; l >= 0; --l) {
                if (l < T) {
                    base[l] = found;
                    found += cnt[l];
                }
            }
            if (found == 0) break;
        }
    }
    const int kept = found < N ? found : N;
    for (int i = kept + tid; i < N; i += SP_TPB) {
        const int64_t o = (r * N + i) * 2;
        a.spans[o] = a.spans[o + 1] = qnan();
        if (a.windows) a.windows[o] = a.windows[o + 1] = -1;
    }
    if (tid == 0) {
        a.n_spans[r] = kept;
        if (a.n_found) a.n_found[r] = found;
    }
}

// the refusals rv_span_propose and rvc_span_propose_masked share, under the entry's own name; -> RV_OK and the argument block, its levels copied
static int propose_args(const char* who, const float* sims, const float* mask, int32_t R, int32_t rpm, int32_t L, const float* levels, int32_t T,
                        int32_t relative, int32_t smooth, int32_t gap, int32_t min_len, int32_t max_len, int32_t N, float* spans, int32_t* n_spans,
                        int32_t* n_found, int32_t* windows, float* smoothed, ProposeArgs& a) {
    RV_CHECK_ARG(sims && mask && levels && spans && n_spans, "%s: bad arguments (a null sims, mask, levels, spans or n_spans)", who);
    RV_CHECK_ARG(R >= 1 && rpm >= 1 && R % rpm == 0, "%s: R=%d rows with rpm=%d rows per mask row (R >= 1, rpm >= 1, R a multiple of rpm)", who, R, rpm);
    RV_CHECK_ARG(L >= 1 && L <= SP_MAX_L, "%s: L=%d must be in [1, %d]", who, L, SP_MAX_L);
    RV_CHECK_ARG(T >= 1 && T <= SP_LEVELS, "%s: T=%d levels (1 to %d)", who, T, SP_LEVELS);
    RV_CHECK_ARG(relative == 0 || relative == 1, "%s: relative=%d must be 0 or 1", who, relative);
    for (int l = 0; l < T; ++l) {
        RV_CHECK_ARG(fabsf(levels[l]) < INFINITY, "%s: level %d is not finite", who, l);
        RV_CHECK_ARG(l == 0 || levels[l] > levels[l - 1], "%s: levels must be strictly ascending (level %d)", who, l);
        RV_CHECK_ARG(!relative || (levels[l] >= 0.f && levels[l] < 1.f), "%s: relative level %d outside [0, 1)", who, l);
    }
    RV_CHECK_ARG(smooth >= 1 && smooth <= 2 * SP_HALO + 1 && (smooth & 1), "%s: smooth=%d must be odd and in [1, %d]", who, smooth, 2 * SP_HALO + 1);
    RV_CHECK_ARG(gap >= 0 && gap <= 63, "%s: gap=%d must be in [0, 63]", who, gap);
    RV_CHECK_ARG(min_len >= 1, "%s: min_len=%d must be >= 1", who, min_len);
    RV_CHECK_ARG(max_len >= 0 && (max_len == 0 || max_len >= min_len), "%s: max_len=%d must be 0 (no limit) or >= min_len=%d", who, max_len, min_len);
    RV_CHECK_ARG(N >= 1 && N <= SP_MAX_N, "%s: N=%d spans per row (1 to %d)", who, N, SP_MAX_N);
    a = ProposeArgs{sims, mask, spans, n_spans, n_found, windows, smoothed, L, rpm, T, relative, smooth / 2, gap, min_len, max_len, N, {}};
    for (int l = 0; l < T; ++l) a.levels[l] = levels[l];
    return RV_OK;
}

}  // namespace
