// Span proposals from a similarity row (no counterpart in the reference; temporal grouping of a thresholded row at several levels, in the manner of TAG /
// watershed proposals):
//   rv_span_propose   per row: duration from the mask, box smoothing, T thresholds, runs with gaps of at most `gap` frames closed, length filter, duplicates
//                     across levels dropped, (centre, width) spans in the form rv_span_scores / rv_span_rank read - one launch
// The definition stands in include/revision_hip.h.  Every f32 operation is rounded on its own (__fadd_rn, __fsub_rn, __fmul_rn, __fdiv_rn), so a row's
// result does not depend on R, on the row's place or on the tiling.
// The kernel, its smoothing and the refusals are span_propose.h's (one source with the chain library's masked instance); this is the default instance.
#include "span_propose.h"

extern "C" int rv_span_propose(const float* sims, const float* mask, int32_t R, int32_t rpm, int32_t L, const float* levels, int32_t T, int32_t relative,
                               int32_t smooth, int32_t gap, int32_t min_len, int32_t max_len, int32_t N, float* spans, int32_t* n_spans, int32_t* n_found,
                               int32_t* windows, float* smoothed, void* stream) {
    ProposeArgs a;
    if (const int rc = propose_args("rv_span_propose", sims, mask, R, rpm, L, levels, T, relative, smooth, gap, min_len, max_len, N, spans, n_spans, n_found,
                                    windows, smoothed, a))
        return rc;
    hipLaunchKernelGGL(span_propose_kernel<false>, dim3((unsigned)R), dim3(SP_TPB), 0, as_stream(stream), a);
    RV_CHECK_LAUNCH("rv_span_propose");
    return RV_OK;
}
