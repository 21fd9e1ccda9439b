// The companion library (librevision_hip_ext.so, include/revision_hip_ext.h): entries that came after the main library's symbol set was closed.
//   rvx_window_select_clipped   the coarse window selection of prefilter.hip on the stage-1 driver's windows: per row the duration from the mask, every
//                               non-void window of stage1.cut_windows' geometry scored by the sum of its top-k sims, rank order, greedy selection with a
//                               minimum separation, top up in rank order, the first `keep` handed back ascending - one launch
// The kernel is window_select.h's, instantiated here for the clipped windows; it reads f32 rows only, so one library serves both operand flavours.  The
// error string is error.hip's, linked in with its rv_* names local (csrc/exports_ext.map).
#include "window_select.h"

#include "../../include/revision_hip_ext.h"

extern "C" int rvx_abi_version(void) { return RVX_ABI_VERSION; }
extern "C" int rvx_last_error(char* buf, size_t n) { return rv_last_error(buf, n); }

extern "C" int rvx_window_select_clipped(const float* sims, const float* mask, int32_t R, int32_t rpm, int32_t L, int32_t win, int32_t k, int32_t keep,
                                         int32_t min_sep, int32_t Wcap, const float* gt, int32_t* select, int32_t* n_select, int32_t* n_windows,
                                         float* win_scores, int32_t* bounds, int32_t* order, int32_t* hit_rank, void* stream) {
    RV_CHECK_ARG(sims && mask && select && n_select && n_windows,
                 "rvx_window_select_clipped: bad arguments (a null sims, mask, select, n_select or n_windows)");
    RV_CHECK_ARG(R >= 1 && rpm >= 1 && R % rpm == 0,
                 "rvx_window_select_clipped: R=%d rows with rpm=%d rows per mask row (R >= 1, rpm >= 1, R a multiple of rpm)", R, rpm);
    RV_CHECK_ARG(L >= 1 && L <= WS_MAX_L, "rvx_window_select_clipped: L=%d must be in [1, %d]", L, WS_MAX_L);
    RV_CHECK_ARG(win >= 2 && win <= L, "rvx_window_select_clipped: win=%d frames (2 <= win <= L=%d)", win, L);
    RV_CHECK_ARG(k >= 1 && k <= TOPK_FRAMES_MAX, "rvx_window_select_clipped: k=%d must be in [1, 64]", k);
    const int64_t hop = win / 2;
    const int64_t cap = cdiv(L, hop) - 1 > 1 ? cdiv(L, hop) - 1 : 1;
    RV_CHECK_ARG(cap <= WS_MAX_W, "rvx_window_select_clipped: L=%d, win=%d give up to %lld windows (at most %d)", L, win, (long long)cap, WS_MAX_W);
    RV_CHECK_ARG(Wcap == cap, "rvx_window_select_clipped: Wcap=%d must be max(1, ceil(L / (win / 2)) - 1) = %lld", Wcap, (long long)cap);
    RV_CHECK_ARG(keep >= 1 && keep <= Wcap, "rvx_window_select_clipped: keep=%d must be in [1, Wcap=%d]", keep, Wcap);
    RV_CHECK_ARG(min_sep >= 1 && min_sep <= Wcap, "rvx_window_select_clipped: min_sep=%d must be in [1, Wcap=%d]", min_sep, Wcap);
    RV_CHECK_ARG(gt || !hit_rank, "rvx_window_select_clipped: hit_rank needs gt");
    const WindowArgs a{sims, mask, gt, select, n_select, n_windows, win_scores, bounds, order, hit_rank, L, rpm, win, 2, k, keep, min_sep, Wcap};
    hipLaunchKernelGGL(window_select_kernel<RV_WINDOWS_CLIPPED>, dim3((unsigned)R), dim3(WS_TPB), 0, as_stream(stream), a);
    RV_CHECK_LAUNCH("rvx_window_select_clipped");
    return RV_OK;
}
