// Coarse window selection for the stage-2 recursion (the stage the reference evaluates in eval/evaluate_pre_filtered_window.py and feeds from a
// stage-1 LLM log, e2e2.py:278-294; here the choice comes from the per-frame cosine row):
//   rv_window_select   per row: duration from the mask, every window of stage2.cut_windows' geometry scored by the sum of its top-k sims, rank order,
//                      greedy selection with a minimum separation, top up in rank order, the first `keep` handed back ascending - one launch
// The definition stands in include/revision_hip.h; the kernel is window_select.h's, instantiated here for the shifted windows.
#include "window_select.h"

extern "C" int rv_window_select(const float* sims, const float* mask, int32_t R, int32_t rpm, int32_t L, int32_t win, int32_t stride, int32_t k,
                                int32_t keep, int32_t min_sep, int32_t Wcap, const float* gt, int32_t* select, int32_t* n_select, int32_t* n_windows,
                                float* win_scores, int32_t* bounds, int32_t* order, int32_t* hit_rank, void* stream) {
    RV_CHECK_ARG(sims && mask && select && n_select && n_windows,
                 "rv_window_select: bad arguments (a null sims, mask, select, n_select or n_windows)");
    RV_CHECK_ARG(R >= 1 && rpm >= 1 && R % rpm == 0, "rv_window_select: R=%d rows with rpm=%d rows per mask row (R >= 1, rpm >= 1, R a multiple of rpm)", R,
                 rpm);
    RV_CHECK_ARG(L >= 1 && L <= WS_MAX_L, "rv_window_select: L=%d must be in [1, %d]", L, WS_MAX_L);
    RV_CHECK_ARG(stride >= 1 && win >= stride && win <= L, "rv_window_select: win=%d frames with stride=%d (stride >= 1, stride <= win <= L=%d)", win, stride,
                 L);
    RV_CHECK_ARG(k >= 1 && k <= TOPK_FRAMES_MAX, "rv_window_select: k=%d must be in [1, 64]", k);
    const int64_t hop = win / stride;
    const int64_t cap = cdiv(L, hop) - 1 > 1 ? cdiv(L, hop) - 1 : 1;
    RV_CHECK_ARG(cap <= WS_MAX_W, "rv_window_select: L=%d, win=%d, stride=%d give up to %lld windows (at most %d)", L, win, stride, (long long)cap, WS_MAX_W);
    RV_CHECK_ARG(Wcap == cap, "rv_window_select: Wcap=%d must be max(1, ceil(L / (win / stride)) - 1) = %lld", Wcap, (long long)cap);
    RV_CHECK_ARG(keep >= 1 && keep <= Wcap, "rv_window_select: keep=%d must be in [1, Wcap=%d]", keep, Wcap);
    RV_CHECK_ARG(min_sep >= 1 && min_sep <= Wcap, "rv_window_select: min_sep=%d must be in [1, Wcap=%d]", min_sep, Wcap);
    RV_CHECK_ARG(gt || !hit_rank, "rv_window_select: hit_rank needs gt");
    const WindowArgs a{sims, mask, gt, select, n_select, n_windows, win_scores, bounds, order, hit_rank, L, rpm, win, stride, k, keep, min_sep, Wcap};
    hipLaunchKernelGGL(window_select_kernel<RV_WINDOWS_SHIFTED>, dim3((unsigned)R), dim3(WS_TPB), 0, as_stream(stream), a);
    RV_CHECK_LAUNCH("rv_window_select");
    return RV_OK;
}
