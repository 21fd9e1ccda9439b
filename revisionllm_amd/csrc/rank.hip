// The stage behind the scores (no counterpart in the reference, whose eval/metrics.py ranks on the host from JSON logs):
//   rv_span_rank   per row of scored proposals: rank order, greedy temporal NMS, top-M, IoU against a ground-truth span and first hits - one launch
// The definition stands in include/revision_hip.h.  The order is that of grounding.h's rank_key: descending score, ties to the smaller index, NaN last.
#include "grounding.h"

namespace {

// (start, end) of a proposal: form 1 is (centre, width) under span_cxw_to_xx's rule, each operation rounded on its own
__device__ __forceinline__ void span_bounds(const float* __restrict__ p, int form, float& s, float& e) {
    const float a = p[0], b = p[1];
    if (form == 1) {
        const float hw = __fmul_rn(0.5f, b);
        s = __fsub_rn(a, hw);
        e = __fadd_rn(a, hw);
    } else {
        s = a;
        e = b;
    }
}
// inter and union of two SOLID spans (a void one never gets here)
__device__ __forceinline__ void span_overlap(float sa, float ea, float sb, float eb, float& inter, float& uni) {
    const float d = __fsub_rn(fminf(ea, eb), fmaxf(sa, sb));
    inter = d > 0.f ? d : 0.f;
    uni = __fsub_rn(__fadd_rn(__fsub_rn(ea, sa), __fsub_rn(eb, sb)), inter);
}
__device__ __forceinline__ float span_iou(float sa, float ea, float sb, float eb) {
    float inter, uni;
    span_overlap(sa, ea, sb, eb, inter, uni);
    return uni > 0.f ? __fdiv_rn(inter, uni) : 0.f;
}

// N <= 64: a wave per row, four rows per block, no LDS and no barrier.  Lane i loads proposal i; its rank is the number of lanes whose (key, index) is
// smaller (64 broadcasts), a forward cross-lane permute sends index and bounds to lane `rank`, and from there lane p is the p-th proposal in rank order.
// NMS: the undecided proposals are a 64-bit mask; its lowest set bit is the next kept pivot, whose bounds are broadcast, every lane tests itself against
// them and the ballot of the suppressed leaves the mask.  A void pivot is kept and suppresses nothing.
__global__ __launch_bounds__(256) void span_rank_wave_kernel(const float* __restrict__ scores, const float* __restrict__ spans, int form, int64_t R, int N,
                                                             int top, float nms, const float* __restrict__ gt, const float* __restrict__ hit, int T,
                                                             int32_t* __restrict__ order, int32_t* __restrict__ keep, int32_t* __restrict__ n_keep,
                                                             float* __restrict__ keep_iou, int32_t* __restrict__ first_hit) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    uint32_t key = 0xffffffffu;
    float s = 0.f, e = 0.f;
    if (lane < N) {
        key = rank_key(scores[r * N + lane]);
        span_bounds(spans + (r * N + lane) * 2, form, s, e);
    }
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)key, j);
        rank += (kj < key || (kj == key && j < lane)) ? 1 : 0;
    }
    const int si = __builtin_amdgcn_ds_permute(rank << 2, lane);                                   // lane p: the index of the p-th in rank order
    const float ss = __int_as_float(__builtin_amdgcn_ds_permute(rank << 2, __float_as_int(s)));
    const float se = __int_as_float(__builtin_amdgcn_ds_permute(rank << 2, __float_as_int(e)));
    const bool solid = lane < N && span_solid(ss, se);
    if (order && lane < N) order[r * N + lane] = si;

    uint64_t kept;
    int nk;
    if (nms >= 1.f) {                                   // inter <= union: nothing is ever suppressed
        kept = low_bits(top);
        nk = top;
    } else {
        uint64_t live = low_bits(N);
        kept = 0ull;
        nk = 0;
        while (live != 0ull && nk < top) {
            const int p = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)live) - 1);
            kept |= 1ull << p;
            live &= live - 1ull;
            ++nk;
            const float ps = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ss), p));
            const float pe = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(se), p));
            if (nk < top && span_solid(ps, pe)) {      // (the pivot that fills the list suppresses nobody who could still be kept)
                bool dies = false;
                if (solid) {
                    float inter, uni;
                    span_overlap(ps, pe, ss, se, inter, uni);
                    dies = inter > __fmul_rn(nms, uni);
                }
                live &= ~__ballot(dies);               // (lanes at or before p are out of the mask already)
            }
        }
    }
    const bool mine = (kept >> lane) & 1ull;
    const int pos = __popcll(kept & low_bits(lane));   // place of this lane's proposal among the kept
    const int64_t kb = r * top;
    if (mine) keep[kb + pos] = si;
    if (lane >= nk && lane < top) keep[kb + lane] = -1;
    if (lane == 0) n_keep[r] = nk;
    if (!gt) return;
    const float gs = gt[r * 2], ge = gt[r * 2 + 1];
    const float iou = mine && solid && span_solid(gs, ge) ? span_iou(ss, se, gs, ge) : 0.f;
    if (keep_iou) {
        if (mine) keep_iou[kb + pos] = iou;
        if (lane >= nk && lane < top) keep_iou[kb + lane] = 0.f;
    }
    if (first_hit) {
        int fh = -1;
        for (int t = 0; t < T; ++t) {
            const uint64_t m = __ballot(mine && iou > hit[t]);
            const int v = m ? __popcll(kept & low_bits(__ffsll((unsigned long long)m) - 1)) : -1;
            if (lane == t) fh = v;
        }
        if (lane < T) first_hit[r * T + lane] = fh;
    }
}

// 65 <= N <= 2048: a block per row.  (key, index) pairs (8 B) and bounds (8 B) of up to 2048 entries in static LDS, the live flags (1 B) and the kept
// list (2 B) beside them: 38 KB.  Bitonic sort of P = N rounded up to a power of two; a padding entry has the NaN key and an index >= N.
// NMS walks the sorted order: every thread reads the pivot's flag (one broadcast read); a dead pivot costs nothing more, a live one is kept and, unless
// void, the threads clear the flags of the later proposals it suppresses, then one barrier - at most `top` barriers.  The flag reads of one round and the
// flag writes of the next cannot meet: a thread writes only behind the barrier that ends the round in which the others read.
constexpr int SR_MAX = 2048;
__global__ __launch_bounds__(256) void span_rank_block_kernel(const float* __restrict__ scores, const float* __restrict__ spans, int form, int N, int P,
                                                              int top, float nms, const float* __restrict__ gt, const float* __restrict__ hit, int T,
                                                              int32_t* __restrict__ order, int32_t* __restrict__ keep, int32_t* __restrict__ n_keep,
                                                              float* __restrict__ keep_iou, int32_t* __restrict__ first_hit) {
    __shared__ uint64_t keys[SR_MAX];        // key << 32 | index, ascending = rank order
    __shared__ float bs[SR_MAX], be[SR_MAX]; // bounds by ORIGINAL index
    __shared__ uint16_t kept[SR_MAX];        // original indices of the kept, in rank order
    __shared__ uint8_t live[SR_MAX];         // by sorted position
    __shared__ int fh[16];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const float* sc = scores + r * N;
    const float* sp = spans + r * N * 2;
    for (int i = tid; i < P; i += 256) {
        uint32_t key = 0xffffffffu;
        if (i < N) {
            key = rank_key(sc[i]);
            float s, e;
            span_bounds(sp + 2 * i, form, s, e);
            bs[i] = s;
            be[i] = e;
        }
        keys[i] = (uint64_t)key << 32 | (uint32_t)i;
        live[i] = 1;
    }
    if (tid < 16) fh[tid] = 0x7fffffff;
    __syncthreads();
    bitonic_sort_u64<256>(keys, P);
    if (order)
        for (int p = tid; p < N; p += 256) order[r * N + p] = (int32_t)(uint32_t)keys[p];

    int nk = 0;
    if (nms >= 1.f) {                                   // inter <= union: nothing is ever suppressed
        for (int p = tid; p < top; p += 256) kept[p] = (uint16_t)(uint32_t)keys[p];
        nk = top;
    } else {
        for (int p = 0; p < N && nk < top; ++p) {
            if (!live[p]) continue;                     // (the same value in every thread: the last write to it lies behind a barrier)
            const int ip = (int)(uint32_t)keys[p];
            if (tid == 0) kept[nk] = (uint16_t)ip;
            ++nk;
            const float ps = bs[ip], pe = be[ip];
            if (!span_solid(ps, pe) || nk == top) continue;
            for (int q = p + 1 + tid; q < N; q += 256) {
                if (!live[q]) continue;
                const int iq = (int)(uint32_t)keys[q];
                const float qs = bs[iq], qe = be[iq];
                if (!span_solid(qs, qe)) continue;
                float inter, uni;
                span_overlap(ps, pe, qs, qe, inter, uni);
                if (inter > __fmul_rn(nms, uni)) live[q] = 0;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    const int64_t kb = r * top;
    float gs = 0.f, ge = 0.f;
    bool gsolid = false;
    if (gt) {
        gs = gt[r * 2];
        ge = gt[r * 2 + 1];
        gsolid = span_solid(gs, ge);
    }
    for (int q = tid; q < top; q += 256) {
        const bool in = q < nk;
        const int i = in ? (int)kept[q] : -1;
        keep[kb + q] = i;
        if (!gt) continue;
        float iou = 0.f;
        if (in && gsolid && span_solid(bs[i], be[i])) iou = span_iou(bs[i], be[i], gs, ge);
        if (keep_iou) keep_iou[kb + q] = iou;
        if (first_hit)
            for (int t = 0; t < T; ++t)
                if (iou > hit[t]) atomicMin(&fh[t], q);   // (LDS; the minimum does not depend on the order of arrival)
    }
    if (tid == 0) n_keep[r] = nk;
    if (gt && first_hit) {
        __syncthreads();
        if (tid < T) first_hit[r * T + tid] = fh[tid] == 0x7fffffff ? -1 : fh[tid];
    }
}

}  // namespace

extern "C" int rv_span_rank(const float* scores, const float* spans, int32_t form, int32_t R, int32_t N, int32_t top, float nms_iou, const float* gt,
                            const float* hit_iou, int32_t T, int32_t* order, int32_t* keep, int32_t* n_keep, float* keep_iou, int32_t* first_hit,
                            void* stream) {
    RV_CHECK_ARG(scores && spans && keep && n_keep && R > 0 && N > 0, "rv_span_rank: bad arguments");
    RV_CHECK_ARG(N <= SR_MAX, "rv_span_rank: N=%d proposals per row (at most %d)", N, SR_MAX);
    RV_CHECK_ARG(top >= 1 && top <= N, "rv_span_rank: top=%d must be in [1, N=%d]", top, N);
    RV_CHECK_ARG(form == 0 || form == 1, "rv_span_rank: form=%d must be 0 (start, end) or 1 (centre, width)", form);
    RV_CHECK_ARG(nms_iou >= 0.f && nms_iou < INFINITY, "rv_span_rank: nms_iou must be finite and >= 0");
    RV_CHECK_ARG(T >= 0 && T <= 16, "rv_span_rank: T=%d thresholds (at most 16)", T);
    RV_CHECK_ARG(gt || (!hit_iou && T == 0 && !keep_iou && !first_hit), "rv_span_rank: hit_iou, T > 0, keep_iou and first_hit need gt");
    RV_CHECK_ARG(T == 0 || hit_iou, "rv_span_rank: T=%d thresholds without hit_iou", T);
    RV_CHECK_ARG(!gt || T > 0 || keep_iou, "rv_span_rank: gt with neither thresholds nor keep_iou");
    hipStream_t st = as_stream(stream);
    if (N <= 64) {
        hipLaunchKernelGGL(span_rank_wave_kernel, dim3((unsigned)cdiv(R, 4)), dim3(256), 0, st, scores, spans, form, (int64_t)R, N, top, nms_iou, gt, hit_iou,
                           T, order, keep, n_keep, keep_iou, first_hit);
    } else {
        int P = 128;
        while (P < N) P <<= 1;
        hipLaunchKernelGGL(span_rank_block_kernel, dim3((unsigned)R), dim3(256), 0, st, scores, spans, form, N, P, top, nms_iou, gt, hit_iou, T, order, keep,
                           n_keep, keep_iou, first_hit);
    }
    RV_CHECK_LAUNCH("rv_span_rank");
    return RV_OK;
}
