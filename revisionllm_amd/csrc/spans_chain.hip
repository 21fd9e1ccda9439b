// The chain library's span entries (librevision_hip_chain.so, include/revision_hip_chain.h): the fine half of the grounding chain with a say in which
// frames count, as rvc_window_select_frames gave the coarse half one.
//   rvc_span_scores_masked         rv_span_scores / rv_span_scores_multi over the frames a per-frame validity row does not hide and / or over the
//                                  similarities that are numbers; the usable count of every window on request - one launch
//   rvc_span_propose_masked        rv_span_propose with the smoothing, the range and the runs taken over those frames - one launch
//   rvc_span_scores_masked_rows,   the same two with a say in how many rows share a validity row (rpv, "rows per validity row", beside rpm, "rows per
//   rvc_span_propose_masked_rows   mask row"): rpv = 1 gives every query of a video its own validity row - what rvc_windows_valid makes of a per-query
//                                  window selection - while the video's mask row, hence the duration, stays shared.  The first two are rpv = rpm.
// The kernels are span_scores.h's and span_propose.h's, instantiated here with MASKED = true; they read f32 rows only, so one library serves both
// operand flavours.  The error string is error.hip's, linked in with its rv_* names local (csrc/exports_chain.map).
#include "span_propose.h"
#include "span_scores.h"

#include "../../include/revision_hip_chain.h"

namespace {

// both score entries under the entry's own name (`rows_form`: rpv is the caller's and is checked; else it is rpm)
int scores_masked(const char* who, bool rows_form, const float* sims, const float* spans, const float* mask, const float* valid, int32_t rpv, int32_t rows,
                  int32_t rpm, int32_t L, int32_t N, int32_t mode, int32_t k, float temperature, int32_t skip_nan, float* scores, int32_t* windows,
                  int32_t* n_usable, void* stream) {
    RV_CHECK_ARG(sims && spans && mask && scores && rows > 0 && L > 0 && N > 0,
                 "%s: bad arguments (a null sims, spans, mask or scores, or rows, L or N below 1)", who);
    RV_CHECK_ARG(rpm >= 1 && rows % rpm == 0, "%s: rows=%d with rpm=%d rows per mask row (rpm >= 1, rows a multiple of rpm)", who, rows, rpm);
    if (rows_form)
        RV_CHECK_ARG(rpv >= 1 && rows % rpv == 0, "%s: rows=%d with rpv=%d rows per validity row (rpv >= 1, rows a multiple of rpv)", who, rows, rpv);
    RV_CHECK_ARG(rows <= 65535, "%s: at most 65535 rows per launch (rows=%d)", who, rows);
    RV_CHECK_ARG(mode == 0 || mode == 1, "%s: mode=%d must be 0 (top-k) or 1 (attention)", who, mode);
    RV_CHECK_ARG(skip_nan == 0 || skip_nan == 1, "%s: skip_nan=%d must be 0 or 1", who, skip_nan);
    const dim3 grid((unsigned)cdiv(N, 4), (unsigned)rows);
    const SpanMasking<true> mk{valid, n_usable, skip_nan, rpv};
    if (mode == 0) {
        RV_CHECK_ARG(k >= 1 && k <= TOPK_FRAMES_MAX, "%s: k=%d must be in [1, %d]", who, k, TOPK_FRAMES_MAX);
        hipLaunchKernelGGL((span_scores_kernel<0, true>), grid, dim3(256), 0, as_stream(stream), sims, spans, mask, rpm, L, N, k, 1.0f, scores, windows, mk);
    } else {
        RV_CHECK_ARG(temperature != 0.f && fabsf(temperature) < INFINITY, "%s: temperature must be finite and not 0", who);
        hipLaunchKernelGGL((span_scores_kernel<1, true>), grid, dim3(256), 0, as_stream(stream), sims, spans, mask, rpm, L, N, k, temperature, scores, windows,
                           mk);
    }
    RV_CHECK_LAUNCH(who);
    return RV_OK;
}

// both proposal entries, likewise
int propose_masked(const char* who, bool rows_form, const float* sims, const float* mask, const float* valid, int32_t rpv, int32_t R, int32_t rpm, int32_t L,
                   const float* levels, int32_t T, int32_t relative, int32_t smooth, int32_t gap, int32_t min_len, int32_t max_len, int32_t N,
                   int32_t skip_nan, float* spans, int32_t* n_spans, int32_t* n_found, int32_t* windows, float* smoothed, void* stream) {
    ProposeMaskedArgs a;
    if (const int rc = propose_args(who, sims, mask, R, rpm, L, levels, T, relative, smooth, gap, min_len, max_len, N, spans, n_spans, n_found, windows,
                                    smoothed, a))
        return rc;
    RV_CHECK_ARG(skip_nan == 0 || skip_nan == 1, "%s: skip_nan=%d must be 0 or 1", who, skip_nan);
    if (rows_form) RV_CHECK_ARG(rpv >= 1 && R % rpv == 0, "%s: R=%d rows with rpv=%d rows per validity row (rpv >= 1, R a multiple of rpv)", who, R, rpv);
    a.valid = valid;
    a.skip_nan = skip_nan;
    a.rpv = rpv;
    hipLaunchKernelGGL(span_propose_kernel<true>, dim3((unsigned)R), dim3(SP_TPB), 0, as_stream(stream), a);
    RV_CHECK_LAUNCH(who);
    return RV_OK;
}

}  // namespace

extern "C" int rvc_span_scores_masked(const float* sims, const float* spans, const float* mask, const float* valid, int32_t rows, int32_t rpm, int32_t L,
                                      int32_t N, int32_t mode, int32_t k, float temperature, int32_t skip_nan, float* scores, int32_t* windows,
                                      int32_t* n_usable, void* stream) {
    return scores_masked("rvc_span_scores_masked", false, sims, spans, mask, valid, rpm, rows, rpm, L, N, mode, k, temperature, skip_nan, scores, windows,
                         n_usable, stream);
}

extern "C" int rvc_span_scores_masked_rows(const float* sims, const float* spans, const float* mask, const float* valid, int32_t rpv, int32_t rows,
                                           int32_t rpm, int32_t L, int32_t N, int32_t mode, int32_t k, float temperature, int32_t skip_nan, float* scores,
                                           int32_t* windows, int32_t* n_usable, void* stream) {
    return scores_masked("rvc_span_scores_masked_rows", true, sims, spans, mask, valid, rpv, rows, rpm, L, N, mode, k, temperature, skip_nan, scores, windows,
                         n_usable, stream);
}

extern "C" int rvc_span_propose_masked(const float* sims, const float* mask, const float* valid, int32_t R, int32_t rpm, int32_t L, const float* levels,
                                       int32_t T, int32_t relative, int32_t smooth, int32_t gap, int32_t min_len, int32_t max_len, int32_t N,
                                       int32_t skip_nan, float* spans, int32_t* n_spans, int32_t* n_found, int32_t* windows, float* smoothed, void* stream) {
    return propose_masked("rvc_span_propose_masked", false, sims, mask, valid, rpm, R, rpm, L, levels, T, relative, smooth, gap, min_len, max_len, N, skip_nan,
                          spans, n_spans, n_found, windows, smoothed, stream);
}

extern "C" int rvc_span_propose_masked_rows(const float* sims, const float* mask, const float* valid, int32_t rpv, int32_t R, int32_t rpm, int32_t L,
                                            const float* levels, int32_t T, int32_t relative, int32_t smooth, int32_t gap, int32_t min_len, int32_t max_len,
                                            int32_t N, int32_t skip_nan, float* spans, int32_t* n_spans, int32_t* n_found, int32_t* windows, float* smoothed,
                                            void* stream) {
    return propose_masked("rvc_span_propose_masked_rows", true, sims, mask, valid, rpv, R, rpm, L, levels, T, relative, smooth, gap, min_len, max_len, N,
                          skip_nan, spans, n_spans, n_found, windows, smoothed, stream);
}
