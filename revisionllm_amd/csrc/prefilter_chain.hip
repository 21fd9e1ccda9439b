// The chain library (librevision_hip_chain.so, include/revision_hip_chain.h): entries of the CLIP grounding chain that came after the main library's
// and the companion library's symbol sets were closed.  This one stays open: the next chain entry goes in here.
//   rvc_window_select_frames   the coarse window selection of prefilter.hip / prefilter_ext.hip under either window rule, with a window scored on a
//                              chosen frame set - every frame, or the F frames rv_window_gather* samples of it - and on the frames a per-frame
//                              validity row does not hide; a window without a usable frame is no candidate - one launch
// The kernel is window_select.h's, instantiated here over the rule, the frame set and the validity; it reads f32 rows only, so one library serves both
// operand flavours.  The error string is error.hip's, linked in with its rv_* names local (csrc/exports_chain.map).
#include "window_select.h"

#include "../../include/revision_hip_chain.h"

static_assert(WS_FRAMES_ALL == RV_FRAMES_ALL && WS_FRAMES_SAMPLED == RV_FRAMES_SAMPLED, "window_select.h and revision_hip_chain.h name the frame sets alike");
static_assert(RVC_MAX_SAMPLED == 64 * WS_REG, "a sampled frame set is ranked from registers");

extern "C" int rvc_abi_version(void) { return RVC_ABI_VERSION; }
extern "C" int rvc_last_error(char* buf, size_t n) { return rv_last_error(buf, n); }

namespace {

template <int RULE, int FRAMES>
void wsf_launch(const WindowArgs& a, int R, hipStream_t st) {
    if (a.valid) hipLaunchKernelGGL((window_select_kernel<RULE, FRAMES, true, true>), dim3((unsigned)R), dim3(WS_TPB), 0, st, a);
    else hipLaunchKernelGGL((window_select_kernel<RULE, FRAMES, false, true>), dim3((unsigned)R), dim3(WS_TPB), 0, st, a);
}

template <int RULE>
void wsf_dispatch(const WindowArgs& a, int frames, int R, hipStream_t st) {
    if (frames == RV_FRAMES_SAMPLED) wsf_launch<RULE, WS_FRAMES_SAMPLED>(a, R, st);
    else wsf_launch<RULE, WS_FRAMES_ALL>(a, R, st);
}

}  // namespace

extern "C" int rvc_window_select_frames(const float* sims, const float* mask, const float* valid, int32_t R, int32_t rpm, int32_t L, int32_t rule,
                                        int32_t win, int32_t stride, int32_t frames, int32_t F, int32_t k, int32_t keep, int32_t min_sep, int32_t Wcap,
                                        const float* gt, int32_t* select, int32_t* n_select, int32_t* n_windows, int32_t* n_candidates, float* win_scores,
                                        int32_t* bounds, int32_t* order, int32_t* hit_rank, void* stream) {
    RV_CHECK_ARG(sims && mask && select && n_select && n_windows && n_candidates,
                 "rvc_window_select_frames: bad arguments (a null sims, mask, select, n_select, n_windows or n_candidates)");
    RV_CHECK_ARG(rule == RV_WINDOWS_SHIFTED || rule == RV_WINDOWS_CLIPPED, "rvc_window_select_frames: rule=%d (0: shifted windows, 1: clipped windows)", rule);
    RV_CHECK_ARG(frames == RV_FRAMES_ALL || frames == RV_FRAMES_SAMPLED, "rvc_window_select_frames: frames=%d (0: every frame, 1: the sampled frames)",
                 frames);
    RV_CHECK_ARG(R >= 1 && rpm >= 1 && R % rpm == 0,
                 "rvc_window_select_frames: R=%d rows with rpm=%d rows per mask row (R >= 1, rpm >= 1, R a multiple of rpm)", R, rpm);
    RV_CHECK_ARG(L >= 1 && L <= WS_MAX_L, "rvc_window_select_frames: L=%d must be in [1, %d]", L, WS_MAX_L);
    RV_CHECK_ARG(rule != RV_WINDOWS_CLIPPED || stride == 2,
                 "rvc_window_select_frames: stride=%d with the clipped rule (its windows overlap by half: stride 2)", stride);
    RV_CHECK_ARG(stride >= 1 && win >= stride && win <= L,
                 "rvc_window_select_frames: win=%d frames with stride=%d (stride >= 1, stride <= win <= L=%d)", win, stride, L);
    RV_CHECK_ARG(frames != RV_FRAMES_SAMPLED || (F >= 1 && F <= RVC_MAX_SAMPLED),
                 "rvc_window_select_frames: F=%d sampled frames per window must be in [1, %d]", F, RVC_MAX_SAMPLED);
    RV_CHECK_ARG(frames != RV_FRAMES_ALL || F == 0, "rvc_window_select_frames: F=%d with every frame of a window (F = 0)", F);
    RV_CHECK_ARG(k >= 1 && k <= TOPK_FRAMES_MAX, "rvc_window_select_frames: k=%d must be in [1, 64]", k);
    const int64_t hop = win / stride;
    const int64_t cap = cdiv(L, hop) - 1 > 1 ? cdiv(L, hop) - 1 : 1;
    RV_CHECK_ARG(cap <= WS_MAX_W, "rvc_window_select_frames: L=%d, win=%d, stride=%d give up to %lld windows (at most %d)", L, win, stride, (long long)cap,
                 WS_MAX_W);
    RV_CHECK_ARG(Wcap == cap, "rvc_window_select_frames: Wcap=%d must be max(1, ceil(L / (win / stride)) - 1) = %lld", Wcap, (long long)cap);
    RV_CHECK_ARG(keep >= 1 && keep <= Wcap, "rvc_window_select_frames: keep=%d must be in [1, Wcap=%d]", keep, Wcap);
    RV_CHECK_ARG(min_sep >= 1 && min_sep <= Wcap, "rvc_window_select_frames: min_sep=%d must be in [1, Wcap=%d]", min_sep, Wcap);
    RV_CHECK_ARG(gt || !hit_rank, "rvc_window_select_frames: hit_rank needs gt");
    const WindowArgs a{sims, mask, gt, select, n_select, n_windows, win_scores, bounds, order, hit_rank, L, rpm, win, stride, k, keep, min_sep, Wcap,
                       valid, n_candidates, F};
    if (rule == RV_WINDOWS_CLIPPED) wsf_dispatch<RV_WINDOWS_CLIPPED>(a, frames, R, as_stream(stream));
    else wsf_dispatch<RV_WINDOWS_SHIFTED>(a, frames, R, as_stream(stream));
    RV_CHECK_LAUNCH("rvc_window_select_frames");
    return RV_OK;
}
