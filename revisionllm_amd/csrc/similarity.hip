// Proposal-query matching with several texts per video (forward_clip_matching, eval/similarity.py:24-69, for Q queries on the same features):
//   rv_frame_cosine_multi   the cosine rows of Q texts against every frame of their video, the features read once for all of them
// (rv_span_scores_multi, the span kernel of rv_span_scores with one mask row per Q rows, lives next to that kernel in sample.hip.)
// and the stage behind the scores (no counterpart in the reference, whose eval/metrics.py ranks on the host from JSON logs):
//   rv_span_rank            per row of scored proposals: rank order, greedy temporal NMS, top-M, IoU against a ground-truth span and first hits
//
// With Q texts the rows are a small matrix product [Q x d] . [d x L] per video, which goes to the f32-input MFMA (v_mfma_f32_16x16x4_f32): per output
// element that instruction is a k-ordered fmaf chain with no wider accumulation, so "all arithmetic f32" (the single-text kernel's contract) holds, a
// 16-bit feature converted to f32 in a register is exact, and both builds and f32 features share this one code path and one error bound.
#include "kernels.h"

namespace {

constexpr int CM_TPB = 256;      // 4 waves
constexpr int CM_FT = 2;         // 16-frame MFMA tiles of a wave: a text fragment is loaded once for both
constexpr int CM_FRAMES = 4 * 16 * CM_FT;   // frames of one block (128)
constexpr int CM_TILES = 8;      // 16-query tiles whose accumulators a wave holds in one pass over its frames (128 queries, 2 x 32 registers)
constexpr int CM_AHEAD = 4;      // k-steps whose feature loads a wave issues together

// unit[r] = text[r] / |text[r]| for the B Q text rows, one wave per row (a zero text: 0 / 0 = NaN in every column, which makes that query's row NaN
// and no other).  A launch of its own into the caller's workspace: in the main kernel every block would repeat the Q d divisions.
__global__ __launch_bounds__(256) void text_unit_kernel(const float* __restrict__ text, int64_t rows, int d, float* __restrict__ unit) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* t = text + r * d;
    float ss = 0.f;
    for (int c = lane; c < d; c += 64) ss += t[c] * t[c];
    const float norm = sqrtf(wave_sum(ss));
    float* u = unit + r * d;
    for (int c = lane; c < d; c += 64) u[c] = t[c] / norm;
}

template <typename T, int VEC>
__device__ __forceinline__ void load_features(const T* p, float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        if constexpr (sizeof(T) == 2) v[0] = op16_to_f32(*p);
        else v[0] = *p;
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

template <int VEC>
__device__ __forceinline__ void load_text(const float* p, float (&v)[VEC]) {
    if constexpr (VEC == 1) v[0] = *p;
    else {
#pragma unroll
        for (int h = 0; h < VEC / 4; ++h) {
            const f32x4 r = *(const f32x4*)(p + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * h + e] = r[e];
        }
    }
}

// One pass of a wave over its 32 frames (CM_FT = 2 tiles of 16) for the NT 16-query tiles from q0 on.  The MFMA takes the texts as A (lane: row = lane & 15,
// k = lane >> 4) and the features as B (k = lane >> 4, column = lane & 15) - the two maps are the same, so a lane holds the same k of "its" text row and of
// "its" frame of each tile - and leaves D[query (lane >> 4) * 4 + r][frame lane & 15] in register r: for each query, 16 lanes store 16 consecutive frames.
// A text fragment is loaded once and multiplies both frame tiles.
// k order: step s gives lane group g = lane >> 4 the VEC elements from k = (4 s + g) VEC on, and MFMA e of the step multiplies element e of every
// lane, i.e. k = (4 s + g) VEC + e for g = 0..3.  Both operands use that one permutation of k, which depends on d and the element type alone, so an
// output element's fmaf chain is the same whatever Q, the query's slot and the other texts are.  Past d both operands are 0 (never loaded: 0 . NaN is NaN).
// Steps run in groups of CM_AHEAD whose feature loads are issued together (no condition in a whole group: they lie inside d), then one by one.
// |f|^2: each lane squares what it loaded for the dot product; the four lanes of a frame add up at the end (two shuffles, the same bits in all four).
template <typename T, int VEC, int NT>
__device__ __forceinline__ void cosine_pass(const T* const (&f)[CM_FT], const float* __restrict__ unit_b, int q0, int Q, int l, int L, int d,
                                            float* __restrict__ out_b) {
    const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const float* tp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int q = q0 + t * 16 + col;
        tp[t] = unit_b + (int64_t)(q < Q ? q : Q - 1) * d;          // (past the last query: that query again, never a row outside the texts)
    }
    f32x4 acc[CM_FT][NT];
    float sq[CM_FT];
#pragma unroll
    for (int j = 0; j < CM_FT; ++j) {
        sq[j] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // one k-step: the features fv of both tiles (already loaded), every text tile's fragment at k (inside: load it, else zeros)
    auto step = [&](const float (&fv)[CM_FT][VEC], int k, bool inside) {
#pragma unroll
        for (int j = 0; j < CM_FT; ++j)
#pragma unroll
            for (int e = 0; e < VEC; ++e) sq[j] += fv[j][e] * fv[j][e];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float tv[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) tv[e] = 0.f;
            if (inside) load_text<VEC>(tp[t] + k, tv);
#pragma unroll
            for (int e = 0; e < VEC; ++e)
#pragma unroll
                for (int j = 0; j < CM_FT; ++j) acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(tv[e], fv[j][e], acc[j][t], 0, 0, 0);
        }
    };
    const int steps = (d + 4 * VEC - 1) / (4 * VEC);
    int s = 0;
    for (; (s + CM_AHEAD) * 4 * VEC <= d; s += CM_AHEAD) {
        float fv[CM_AHEAD][CM_FT][VEC];
#pragma unroll
        for (int u = 0; u < CM_AHEAD; ++u)
#pragma unroll
            for (int j = 0; j < CM_FT; ++j) load_features<T, VEC>(f[j] + (4 * (s + u) + g) * VEC, fv[u][j]);
#pragma unroll
        for (int u = 0; u < CM_AHEAD; ++u) step(fv[u], (4 * (s + u) + g) * VEC, true);
    }
    for (; s < steps; ++s) {
        const int k = (4 * s + g) * VEC;
        float fv[CM_FT][VEC];
#pragma unroll
        for (int j = 0; j < CM_FT; ++j) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) fv[j][e] = 0.f;
            if (k < d) load_features<T, VEC>(f[j] + k, fv[j]);       // (d is a multiple of VEC: a lane's vector lies inside the row or is not read)
        }
        step(fv, k, k < d);
    }
#pragma unroll
    for (int j = 0; j < CM_FT; ++j) {
        float q2 = sq[j];
        q2 += __shfl_xor(q2, 16, 64);
        q2 += __shfl_xor(q2, 32, 64);
        const float fnorm = sqrtf(q2);                                // a zero frame: 0 / 0 = NaN in its column for every query
        const int lj = l + 16 * j;
        if (lj >= L) continue;                                        // rows past L and columns past Q of a tile are never stored
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = q0 + t * 16 + g * 4 + r;
                if (q < Q) out_b[(int64_t)q * L + lj] = acc[j][t][r] / fnorm;
            }
        }
    }
}

// out[b, q, l] = <f_bl, t_bq> / (|f_bl| |t_bq|) in the single-text kernel's order of operations: the texts are normalised first (unit = t / |t|,
// text_unit_kernel), the dot product <f, unit> follows, and the division by |f| comes last.  A block owns 128 frames of video blockIdx.y, a wave 32 of
// them, and produces every query's column for them: up to CM_TILES 16-query tiles per pass, so the features come from global memory once per call up to
// 128 queries (once per 128 queries beyond: the later passes find the wave's 32 rows in the caches).  The unit texts are read from global memory as
// well (Q d floats per video, resident in L2; the four waves of a block walk them in step).  No LDS, no barrier.
// VECTOR: 16-byte feature loads (d a multiple of 16 B / sizeof(T), 16-byte aligned rows); else one element per lane and step, for every d and alignment.
template <typename T, bool VECTOR>
__global__ __launch_bounds__(CM_TPB) void frame_cosine_multi_kernel(const T* __restrict__ video, const float* __restrict__ unit, int Q, int L, int d,
                                                                    float* __restrict__ out) {
    constexpr int VEC = VECTOR ? 16 / (int)sizeof(T) : 1;
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l0 = blockIdx.x * CM_FRAMES + wave * (16 * CM_FT);
    if (l0 >= L) return;
    const int l = l0 + (lane & 15);
    const T* f[CM_FT];
#pragma unroll
    for (int j = 0; j < CM_FT; ++j) {
        const int lj = l + 16 * j;
        f[j] = video + ((int64_t)b * L + (lj < L ? lj : L - 1)) * d;   // (past the last frame: that frame again, never a row outside the video)
    }
    const float* unit_b = unit + (int64_t)b * Q * d;
    float* out_b = out + (int64_t)b * Q * L;
    for (int q0 = 0; q0 < Q; q0 += 16 * CM_TILES) {
        const int tiles = (Q - q0 + 15) / 16;                           // (the choice of NT changes which tiles share a pass, not any element's chain)
        if (tiles > 4) cosine_pass<T, VEC, 8>(f, unit_b, q0, Q, l, L, d, out_b);
        else if (tiles > 2) cosine_pass<T, VEC, 4>(f, unit_b, q0, Q, l, L, d, out_b);
        else if (tiles > 1) cosine_pass<T, VEC, 2>(f, unit_b, q0, Q, l, L, d, out_b);
        else cosine_pass<T, VEC, 1>(f, unit_b, q0, Q, l, L, d, out_b);
    }
}


// ---- rv_span_rank: sort, greedy temporal NMS, top-M and hits against a ground-truth span, one launch ----
// Rank key of a score: an unsigned number that is SMALLER for what ranks earlier.  Numbers in descending order (-0 counts as +0, so the index decides
// between them), every NaN behind -inf with the largest key.  Ties go to the smaller index: the pair (key, index) is compared, and a padding entry
// carries the NaN key with an index >= N, so it lands behind every proposal.
__device__ __forceinline__ uint32_t rank_key(float x) {
    if (x != x) return 0xffffffffu;
    uint32_t b = (uint32_t)__float_as_int(x);
    if (b == 0x80000000u) b = 0u;
    const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // ascending with the value
    return ~asc;                                                         // (-inf: 0xff800000, below the NaN key)
}
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
__device__ __forceinline__ bool span_solid(float s, float e) { return fabsf(s) < INFINITY && fabsf(e) < INFINITY && e > s; }   // not void
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
__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

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
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += 256) {
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

extern "C" int rv_frame_cosine_multi(const void* video, int dtype, const float* text, int32_t B, int32_t Q, int32_t L, int32_t d, float* text_unit,
                                     float* out, void* stream) {
    RV_CHECK_ARG(video && text && text_unit && out && B > 0 && Q > 0 && L > 0 && d > 0, "rv_frame_cosine_multi: bad arguments");
    RV_CHECK_ARG(dtype == RV_OP16 || dtype == RV_F32, "rv_frame_cosine_multi: dtype must be f32 or %s", RV_OP16_NAME);
    RV_CHECK_ARG((int64_t)B * Q <= 65535, "rv_frame_cosine_multi: at most 65535 (video, query) rows per launch (B=%d, Q=%d)", B, Q);
    const int vec = dtype == RV_OP16 ? 8 : 4;
    const bool vector = d % vec == 0 && ((uintptr_t)video & 15u) == 0 && ((uintptr_t)text_unit & 15u) == 0;
    const dim3 grid((unsigned)cdiv(L, CM_FRAMES), B);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(text_unit_kernel, dim3((unsigned)cdiv((int64_t)B * Q, 4)), dim3(256), 0, st, text, (int64_t)B * Q, d, text_unit);
    if (dtype == RV_OP16) {
        if (vector) hipLaunchKernelGGL((frame_cosine_multi_kernel<op16_t, true>), grid, dim3(CM_TPB), 0, st, (const op16_t*)video, text_unit, Q, L, d, out);
        else hipLaunchKernelGGL((frame_cosine_multi_kernel<op16_t, false>), grid, dim3(CM_TPB), 0, st, (const op16_t*)video, text_unit, Q, L, d, out);
    } else {
        if (vector) hipLaunchKernelGGL((frame_cosine_multi_kernel<float, true>), grid, dim3(CM_TPB), 0, st, (const float*)video, text_unit, Q, L, d, out);
        else hipLaunchKernelGGL((frame_cosine_multi_kernel<float, false>), grid, dim3(CM_TPB), 0, st, (const float*)video, text_unit, Q, L, d, out);
    }
    RV_CHECK_LAUNCH("rv_frame_cosine_multi");
    return RV_OK;
}

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
