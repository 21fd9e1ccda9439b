// Proposal-query matching with several texts per video (forward_clip_matching, eval/similarity.py:24-69, for Q queries on the same features):
//   rv_frame_cosine_multi   the cosine rows of Q texts against every frame of their video, the features read once for all of them
// (rv_span_scores_multi, the span kernel of rv_span_scores with one mask row per Q rows, lives next to that kernel in sample.hip.)
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
