// Proposal-query matching (forward_clip_matching / _get_predicted_proposal_feat, eval/similarity.py:24-69) without a host round trip, for one text
// per video and for Q texts on the same features, and the two poolings beside it:
//   rv_frame_cosine         per-frame cosine row of a whole video against its text CLS
//   rv_frame_cosine_multi   the cosine rows of Q texts against every frame of their video, the features read once for all of them
//   rv_span_scores          (centre, width) proposals -> windows -> top-k / softmax score
//   rv_span_scores_multi    the same kernel over [B,Q] rows of similarities and proposals that share their video's mask row
//   rv_attn_pool            _attention_pooling (eval/similarity.py:96-113)
// (rv_topk_pool, the other pooling, stands with rv_topk_cosine in sample.hip.)  The stages behind the scores are rank.hip, propose.hip, prefilter.hip.
#include "span_scores.h"

namespace {

// ---- one text per video ----
// The reference scores a proposal by slicing its window out of the video, normalising every frame of the slice, pooling the top-k frames by
// <frame / |frame|, text / |text|> and taking the pooled row's dot product with the text: the SUM of the top-k cosines of the window.  So the features
// are read once into a cosine row (frame_cosine_kernel) and every span works on that row (span_scores_kernel).

constexpr int FC_TPB = 256;        // 4 waves
constexpr int FC_FRAMES = 32;      // frames of one block (8 per wave): the text row is normalised once per 32 frames
constexpr int FC_FLIGHT = 4;       // frames a wave of the 16-byte-load path reads at a time
constexpr int FC_DMAX = 8192;      // the staged text row: 32 KB of LDS

// out[b, l] = <f_l, t_b> / (|f_l| |t_b|): the text row goes to LDS as t / |t| (a zero text: 0 / 0 = NaN in every column), a wave takes a frame, the dot
// product and the sum of squares come from the same loads, and the division by |f_l| is the reference's (a zero frame: 0 / 0 = NaN).
// VECTOR: 16-byte loads (d a multiple of 16 B / sizeof(T), 16-byte aligned rows), FC_FLIGHT frames of a wave in flight; else one element per lane and step.
template <typename T, bool VECTOR>
__global__ __launch_bounds__(FC_TPB) void frame_cosine_kernel(const T* __restrict__ video, const float* __restrict__ text, int L, int d,
                                                              float* __restrict__ out) {
    constexpr int VEC = 16 / (int)sizeof(T);
    // [d] t / |t|.  One symbol with the other kernels' smem: an aligned(16) here took effect or not with its neighbours in the file, so none is claimed
    // (with it: two 16-byte LDS reads per chunk and 91 VGPRs instead of 110 in the 16-bit instance - not timed yet)
    extern __shared__ float smem[];
    __shared__ float red[FC_TPB / 64];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* t = text + (int64_t)b * d;
    float ss = 0.f;
    for (int c = tid; c < d; c += FC_TPB) {
        const float v = t[c];
        smem[c] = v;
        ss += v * v;
    }
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    const float tnorm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    for (int c = tid; c < d; c += FC_TPB) smem[c] = smem[c] / tnorm;    // (each thread rewrites the elements it wrote)
    __syncthreads();
    const int l0 = blockIdx.x * FC_FRAMES + wave * (FC_FRAMES / 4);
    const int l1 = l0 + FC_FRAMES / 4 < L ? l0 + FC_FRAMES / 4 : L;
    const T* f = video + (int64_t)b * L * d;
    float* o = out + (int64_t)b * L;
    if constexpr (VECTOR) {
        const int chunks = d / VEC;
        for (int l = l0; l < l1; l += FC_FLIGHT) {
            const T* fr[FC_FLIGHT];
            float dot[FC_FLIGHT], sq[FC_FLIGHT];
#pragma unroll
            for (int j = 0; j < FC_FLIGHT; ++j) {
                fr[j] = f + (int64_t)(l + j < l1 ? l + j : l1 - 1) * d;     // (past the wave's last frame: that frame again, never a row outside the video)
                dot[j] = sq[j] = 0.f;
            }
            for (int cc = lane; cc < chunks; cc += 64) {
                float v[FC_FLIGHT][VEC];
#pragma unroll
                for (int j = 0; j < FC_FLIGHT; ++j) load_features<T, VEC>(fr[j] + cc * VEC, v[j]);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float tn = smem[cc * VEC + e];
#pragma unroll
                    for (int j = 0; j < FC_FLIGHT; ++j) {
                        dot[j] += v[j][e] * tn;
                        sq[j] += v[j][e] * v[j][e];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < FC_FLIGHT; ++j) {
                const float dj = wave_sum(dot[j]), qj = wave_sum(sq[j]);
                if (lane == 0 && l + j < l1) o[l + j] = dj / sqrtf(qj);
            }
        }
    } else {
        for (int l = l0; l < l1; ++l) {
            const T* fa = f + (int64_t)l * d;
            float da = 0.f, qa = 0.f;
            for (int c = lane; c < d; c += 64) {
                const float v = ld<T>(fa + c);
                da += v * smem[c];
                qa += v * v;
            }
            da = wave_sum(da);
            qa = wave_sum(qa);
            if (lane == 0) o[l] = da / sqrtf(qa);
        }
    }
}

// (span_scores_kernel and the window rule: span_scores.h, one source with the chain library's masked instances)

// _attention_pooling (similarity.py:96-113) for one (video, text) pair per block, laid out as topk_pool_kernel: x[t] = <f_t, q> / tau to LDS (one wave per
// frame), the softmax over the frames with the maximum subtracted (a NaN x is carried into the maximum: the whole row is NaN then, as torch.softmax's
// is), then out[c] = sum_t p[t] f[t][c] with the threads over the columns, frames in ascending order.
template <typename T>
__global__ __launch_bounds__(256) void attn_pool_kernel(const T* __restrict__ video, const float* __restrict__ text, int Tn, int d, int Nt, float tau,
                                                        float* __restrict__ out) {
    extern __shared__ float smem[];
    float* qs = smem;          // [d]
    float* xs = smem + d;      // [Tn] x, then p
    __shared__ float red[64];
    const int v = blockIdx.x, tx = blockIdx.y;
    const T* f = video + (int64_t)v * Tn * d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = tid; c < d; c += 256) qs[c] = text[(int64_t)tx * d + c];
    __syncthreads();
    for (int t = wave; t < Tn; t += 4) {
        float s = 0.f;
        for (int c = lane; c < d; c += 64) s += ld<T>(f + (int64_t)t * d + c) * qs[c];
        s = wave_sum(s);
        if (lane == 0) xs[t] = s / tau;
    }
    __syncthreads();
    float mx = -INFINITY;
    bool nan = false;
    for (int t = tid; t < Tn; t += 256) {
        const float x = xs[t];
        nan |= x != x;
        mx = fmaxf(mx, x);
    }
    mx = wave_max(mx);
    if (__ballot(nan) != 0ull) mx = qnan();
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (red[0] != red[0] || red[1] != red[1] || red[2] != red[2] || red[3] != red[3]) mx = qnan();
    float z = 0.f;
    for (int t = tid; t < Tn; t += 256) {
        const float e = expf(xs[t] - mx);
        xs[t] = e;                                  // (each thread rewrites the elements it read)
        z += e;
    }
    z = wave_sum(z);
    if (lane == 0) red[4 + wave] = z;
    __syncthreads();
    z = (red[4] + red[5]) + (red[6] + red[7]);
    for (int t = tid; t < Tn; t += 256) xs[t] = xs[t] / z;
    __syncthreads();
    float* o = out + ((int64_t)v * Nt + tx) * d;
    for (int c = tid; c < d; c += 256) {
        float a = 0.f;
        for (int t = 0; t < Tn; ++t) a += xs[t] * ld<T>(f + (int64_t)t * d + c);
        o[c] = a;
    }
}

// ---- several texts per video ----
// With Q texts the rows are a small matrix product [Q x d] . [d x L] per video, which goes to the f32-input MFMA (v_mfma_f32_16x16x4_f32): per output
// element that instruction is a k-ordered fmaf chain with no wider accumulation, so "all arithmetic f32" (the single-text kernel's contract) holds, a
// 16-bit feature converted to f32 in a register is exact, and both builds and f32 features share this one code path and one error bound.
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

extern "C" int rv_frame_cosine(const void* video, int dtype, const float* text, int32_t B, int32_t L, int32_t d, float* out, void* stream) {
    RV_CHECK_ARG(video && text && out && B > 0 && L > 0 && d > 0, "rv_frame_cosine: bad arguments");
    RV_CHECK_ARG(dtype == RV_OP16 || dtype == RV_F32, "rv_frame_cosine: dtype must be f32 or %s", RV_OP16_NAME);
    RV_CHECK_ARG(d <= FC_DMAX, "rv_frame_cosine: d=%d exceeds the %d columns of the staged text row", d, FC_DMAX);
    RV_CHECK_ARG(B <= 65535, "rv_frame_cosine: at most 65535 videos per launch");
    const int vec = dtype == RV_OP16 ? 8 : 4;
    const bool vector = d % vec == 0 && ((uintptr_t)video & 15u) == 0;
    const dim3 grid((unsigned)cdiv(L, FC_FRAMES), B);
    const size_t sm = (size_t)d * sizeof(float);
    hipStream_t st = as_stream(stream);
    if (dtype == RV_OP16) {
        if (vector) hipLaunchKernelGGL((frame_cosine_kernel<op16_t, true>), grid, dim3(FC_TPB), sm, st, (const op16_t*)video, text, L, d, out);
        else hipLaunchKernelGGL((frame_cosine_kernel<op16_t, false>), grid, dim3(FC_TPB), sm, st, (const op16_t*)video, text, L, d, out);
    } else {
        if (vector) hipLaunchKernelGGL((frame_cosine_kernel<float, true>), grid, dim3(FC_TPB), sm, st, (const float*)video, text, L, d, out);
        else hipLaunchKernelGGL((frame_cosine_kernel<float, false>), grid, dim3(FC_TPB), sm, st, (const float*)video, text, L, d, out);
    }
    RV_CHECK_LAUNCH("rv_frame_cosine");
    return RV_OK;
}

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

// the part rv_span_scores and rv_span_scores_multi share, behind each entry's own refusals: rows = rows of sims, rpm of them per mask row
static int launch_span_scores(const char* who, const float* sims, const float* spans, const float* mask, int rows, int rpm, int L, int N, int mode, int k,
                              float temperature, float* scores, int32_t* windows, void* stream) {
    const dim3 grid((unsigned)cdiv(N, 4), (unsigned)rows);
    if (mode == 0) {
        RV_CHECK_ARG(k >= 1 && k <= TOPK_FRAMES_MAX, "%s: k=%d must be in [1, %d]", who, k, TOPK_FRAMES_MAX);
        hipLaunchKernelGGL(span_scores_kernel<0>, grid, dim3(256), 0, as_stream(stream), sims, spans, mask, rpm, L, N, k, 1.0f, scores, windows, SpanMasking<false>{});
    } else {
        RV_CHECK_ARG(temperature != 0.f && fabsf(temperature) < INFINITY, "%s: temperature must be finite and not 0", who);
        hipLaunchKernelGGL(span_scores_kernel<1>, grid, dim3(256), 0, as_stream(stream), sims, spans, mask, rpm, L, N, k, temperature, scores, windows, SpanMasking<false>{});
    }
    RV_CHECK_LAUNCH(who);
    return RV_OK;
}

extern "C" int rv_span_scores(const float* sims, const float* spans, const float* mask, int32_t B, int32_t L, int32_t N, int32_t mode, int32_t k,
                              float temperature, float* scores, int32_t* windows, void* stream) {
    RV_CHECK_ARG(sims && spans && mask && scores && B > 0 && L > 0 && N > 0, "rv_span_scores: bad arguments");
    RV_CHECK_ARG(mode == 0 || mode == 1, "rv_span_scores: mode=%d must be 0 (top-k) or 1 (attention)", mode);
    RV_CHECK_ARG(B <= 65535, "rv_span_scores: at most 65535 videos per launch");
    return launch_span_scores("rv_span_scores", sims, spans, mask, B, 1, L, N, mode, k, temperature, scores, windows, stream);
}

extern "C" int rv_span_scores_multi(const float* sims, const float* spans, const float* mask, int32_t B, int32_t Q, int32_t L, int32_t N, int32_t mode,
                                    int32_t k, float temperature, float* scores, int32_t* windows, void* stream) {
    RV_CHECK_ARG(sims && spans && mask && scores && B > 0 && Q > 0 && L > 0 && N > 0, "rv_span_scores_multi: bad arguments");
    RV_CHECK_ARG(mode == 0 || mode == 1, "rv_span_scores_multi: mode=%d must be 0 (top-k) or 1 (attention)", mode);
    RV_CHECK_ARG((int64_t)B * Q <= 65535, "rv_span_scores_multi: at most 65535 (video, query) rows per launch (B=%d, Q=%d)", B, Q);
    return launch_span_scores("rv_span_scores_multi", sims, spans, mask, B * Q, Q, L, N, mode, k, temperature, scores, windows, stream);
}

extern "C" int rv_attn_pool(const void* video, int dtype, const float* text, int32_t Nv, int32_t T, int32_t d, int32_t Nt, float temperature,
                            float* out, void* stream) {
    RV_CHECK_ARG(video && text && out && Nv > 0 && T > 0 && d > 0 && Nt > 0, "rv_attn_pool: bad arguments");
    RV_CHECK_ARG(dtype == RV_OP16 || dtype == RV_F32, "rv_attn_pool: dtype must be f32 or %s", RV_OP16_NAME);
    RV_CHECK_ARG(temperature != 0.f && fabsf(temperature) < INFINITY, "rv_attn_pool: temperature must be finite and not 0");
    RV_CHECK_ARG(Nt <= 65535, "rv_attn_pool: at most 65535 texts per launch");
    const size_t sm = (size_t)(d + T) * sizeof(float);
    RV_CHECK_ARG(sm + 64 * sizeof(float) <= 64 * 1024, "rv_attn_pool: d + T too large for LDS (dynamic %zu B + 256 B static)", sm);
    if (dtype == RV_OP16)
        hipLaunchKernelGGL(attn_pool_kernel<op16_t>, dim3(Nv, Nt), dim3(256), sm, as_stream(stream), (const op16_t*)video, text, T, d, Nt, temperature, out);
    else
        hipLaunchKernelGGL(attn_pool_kernel<float>, dim3(Nv, Nt), dim3(256), sm, as_stream(stream), (const float*)video, text, T, d, Nt, temperature, out);
    RV_CHECK_LAUNCH("rv_attn_pool");
    return RV_OK;
}
