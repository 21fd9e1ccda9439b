/*
 * revision_hip_chain.h - C ABI of librevision_hip_chain.so, the third library beside librevision_hip*.so (include/revision_hip.h) and
 * librevision_hip_ext.so (include/revision_hip_ext.h).
 *
 * The symbol sets of those two are closed; entries of the CLIP grounding chain added since live here, every exported name starting with rvc_.  This
 * library is OPEN: a later chain entry is added to it (its tests hold header, binding table and exported symbols to each other, not to a fixed list).
 * The conventions are revision_hip.h's: plain C, caller-owned DEVICE pointers, all work enqueued on the caller's hipStream_t (passed as void*),
 * nothing synchronises, nothing is allocated, 0 on success and a negative rv_status (the same values: RV_ERR_ARG = -1, RV_ERR_HIP = -3) on error,
 * with rvc_last_error() giving the message of the last failure on the calling thread.  The entries work on f32 rows only, so there is ONE build of
 * this library for both operand flavours of the main one, and it can be loaded with either or with both.
 */
#ifndef REVISION_HIP_CHAIN_H
#define REVISION_HIP_CHAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVC_ABI_VERSION 1

/* the window rules, as revision_hip.h names them for rv_window_gather_rule */
#ifndef RV_WINDOWS_SHIFTED
#define RV_WINDOWS_SHIFTED 0
#define RV_WINDOWS_CLIPPED 1
#endif
/* the frame sets of rvc_window_select_frames */
#define RV_FRAMES_ALL 0
#define RV_FRAMES_SAMPLED 1
#define RVC_MAX_SAMPLED 1024 /* the most sampled frames per window */

/* Everything below is exported; nothing else is (the library is built with -fvisibility=hidden and csrc/exports_chain.map). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int rvc_abi_version(void);
int rvc_last_error(char* buf, size_t n);

/* ---- coarse window selection on a chosen frame set: rv_window_select (revision_hip.h) and rvx_window_select_clipped (revision_hip_ext.h) in one
 * entry, with a say in WHICH frames of a window count towards its score.  The LLM is handed num_frames sampled frames of a window
 * (rv_window_gather*), not all of them, and some frames of a movie are no evidence at all (a zeroed feature row gives a NaN cosine; credits; a region
 * outside the chapters searched).  One kernel source with those two (csrc/window_select.h), further instances ----
 * sims f32 [R,L], mask f32 [R / rpm, L] (rpm = "rows per mask"; R a multiple of rpm), valid f32 [R / rpm, L] or NULL, gt f32 [R,2] (start, end) in
 * frames, or NULL ->
 *   select       i32 [R,keep]          the chosen windows' indices ASCENDING (what rv_window_gather[_rule] takes as `select`), then -1
 *   n_select     i32 [R]               min(keep, n_candidates)
 *   n_windows    i32 [R]               W_r, the row's windows by its geometry (rule 1: the non-void ones), candidates or not
 *   n_candidates i32 [R]               C_r, the windows with at least one usable entry in their frame set
 *   win_scores   f32 [R,Wcap]          (optional) the score of every window; NaN (0x7fc00000) for a window that is no candidate and in the padding
 *   bounds       i32 [R / rpm,Wcap,2]  (optional) (lo, hi) of every one of the W_r windows, candidate or not, (-1, -1) in the padding; written by
 *                                      the first row of each mask row
 *   order        i32 [R,Wcap]          (optional) the selection sequence seq over the C_r candidates, -1 behind them
 *   hit_rank     i32 [R]               (optional, needs gt) the smallest place p with window seq[p] covering the ground truth, or -1
 * Duration, window count and bounds: rv_window_select's for rule = RV_WINDOWS_SHIFTED (stride as there), rvx_window_select_clipped's for rule =
 * RV_WINDOWS_CLIPPED (stride must be 2; the void suffix is left out as there).  `valid` does not change the duration: the mask alone gives D, and
 * only frames [0, D) are read, of sims and of valid.
 * Frame set of a window [lo, hi), a sequence of entries (position j -> frame t_j):
 *   frames = RV_FRAMES_ALL (0), F = 0:   t_j = lo + j, j = 0 .. hi - lo - 1.
 *   frames = RV_FRAMES_SAMPLED (1), F:   t_j = np.linspace(lo, hi - 1, F, dtype=int32)[j], j = 0 .. F - 1 - exactly the frames rv_window_gather[_rule]
 *                                        with this F copies out of the window (one definition of the index rule serves both: numpy's float64
 *                                        operations in numpy's order).  With F above hi - lo a frame occurs more than once and counts as often as it
 *                                        occurs.  1 <= F <= 1024: a sampled set is ranked from registers.
 * Validity: entry j is USABLE when valid is NULL or valid[t_j] != 0 (the f32 comparison: -0 hides a frame, a NaN in valid does not - it compares
 * unequal to 0).  A hidden frame's sim is never looked at: NaN or infinities under it leave no trace.
 * Score: with n usable entries, the sum of the first min(k, n) of them in the frame order - NaN first, then the larger value, then the smaller
 * POSITION j (under RV_FRAMES_ALL that is the smaller frame index) - accumulated from +0 in that order, each add rounded: rv_span_scores' bits for
 * the same multiset of values.  With valid = NULL and RV_FRAMES_ALL every output equals rv_window_select's / rvx_window_select_clipped's bit for bit.
 * Candidates: a window with n = 0 is no candidate.  It is never taken, kills no neighbour, appears in neither select nor order and cannot give
 * hit_rank; its win_scores slot holds 0x7fc00000 and its bounds slot its geometry.  Unlike the clipped rule's void windows the non-candidates lie
 * AMONG the candidates: min_sep still counts window indices, so two candidates on either side of a non-candidate are 2 apart.
 * Rank order, selection sequence (pass 1 with min_sep, pass 2 the top-up), select and hit_rank: rv_window_select's, over the C_r candidates (a
 * candidate whose score is NaN ranks behind every number and in front of no non-candidate, which has no rank).  n_select = min(keep, C_r).
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: a null sims / mask / select / n_select / n_windows / n_candidates; rule outside
 * {0, 1}; frames outside {0, 1}; R < 1; rpm < 1; R not a multiple of rpm; L < 1 or L > 1048576; rule 1 with stride != 2; stride < 1; win < stride;
 * win > L; RV_FRAMES_SAMPLED with F < 1 or F > 1024; RV_FRAMES_ALL with F != 0; k outside [1, 64]; Wcap != max(1, ceil(L / (win / stride)) - 1) or
 * Wcap > 2048; keep outside [1, Wcap]; min_sep outside [1, Wcap]; hit_rank without gt.
 * One 1024-thread workgroup per row, rows on the grid's x dimension with 64-bit offsets; 24 KB of LDS whatever L; vector stores only, no global
 * atomics, no scratch. */
int rvc_window_select_frames(const float* sims, const float* mask, const float* valid, int32_t R, int32_t rpm, int32_t L, int32_t rule, int32_t win,
                             int32_t stride, int32_t frames, int32_t F, int32_t k, int32_t keep, int32_t min_sep, int32_t Wcap, const float* gt,
                             int32_t* select, int32_t* n_select, int32_t* n_windows, int32_t* n_candidates, float* win_scores, int32_t* bounds,
                             int32_t* order, int32_t* hit_rank, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif

#endif /* REVISION_HIP_CHAIN_H */
