/*
 * revision_hip_ext.h - C ABI of librevision_hip_ext.so, the companion of librevision_hip*.so (include/revision_hip.h).
 *
 * The main library's symbol set is closed at RV_ABI_VERSION 5; entries added since live here, every exported name starting with rvx_.  The
 * conventions are revision_hip.h's: plain C, caller-owned DEVICE pointers, all work enqueued on the caller's hipStream_t (passed as void*), nothing
 * synchronises, nothing is allocated, 0 on success and a negative rv_status (the same values: RV_ERR_ARG = -1, RV_ERR_HIP = -3) on error, with
 * rvx_last_error() giving the message of the last failure on the calling thread.  The entries work on f32 rows only, so there is ONE build of this
 * library for both operand flavours of the main one, and it can be loaded with either or with both.
 */
#ifndef REVISION_HIP_EXT_H
#define REVISION_HIP_EXT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVX_ABI_VERSION 1

/* Everything below is exported; nothing else is (the library is built with -fvisibility=hidden and csrc/exports_ext.map). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int rvx_abi_version(void);
int rvx_last_error(char* buf, size_t n);

/* ---- coarse window selection for the stage-1 driver: which of stage1.cut_windows' half-overlapping windows a query should see, chosen from its
 * per-frame cosine row (the geometry the reference evaluates in eval/evaluate_pre_filtered_window.py: windows sliding by half their length; scoring
 * the windows by their top-k cosines is this project's own definition).  It is rv_window_select's selection (revision_hip.h) under the clipped window
 * rule of rv_window_gather_rule (RV_WINDOWS_CLIPPED): one kernel source, two instances ----
 * sims f32 [R,L] (a row = one video, or one (video, query): rv_frame_cosine[_multi]'s rows), mask f32 [R / rpm, L] (rpm = "rows per mask", as in
 * rv_span_propose; R a multiple of rpm), gt f32 [R,2] (start, end) in frames, or NULL ->
 *   select     i32 [R,keep]          the chosen windows' indices ASCENDING (what rv_window_gather_rule takes as `select`), then -1
 *   n_select   i32 [R]               min(keep, W_r)
 *   n_windows  i32 [R]               W_r, the row's non-void windows
 *   win_scores f32 [R,Wcap]          (optional) the score of every window, NaN (0x7fc00000) in the padding
 *   bounds     i32 [R / rpm,Wcap,2]  (optional) (lo, hi) of every window, (-1, -1) in the padding; written by the first row of each mask row
 *   order      i32 [R,Wcap]          (optional) the selection sequence seq, -1 in the padding
 *   hit_rank   i32 [R]               (optional, needs gt) the smallest place p with window seq[p] covering the ground truth, or -1
 * Duration (rv_span_propose's rule): dur = the f32 sum of the row's mask row, D = min(L, max(0, int(floor(dur)))), D = 0 for a non-finite dur.  Only
 * frames [0, D) exist for the row; no frame of sims at or past D is read.  The result is defined for masks whose sum is exact in any order (0 / 1
 * masks); for other masks it is build-defined (the order of the sum is the kernel's).
 * Windows (stage1.cut_windows' rule in integers, 64-bit intermediate products): hop = win / 2 (integer division), W0 = max(0, ceil(D / hop) - 1);
 * for i in [0, W0): s = (i * win) / 2 - for an odd win NOT i * hop -, e = min(s + win, D - 1); the window is frames [lo, hi) = [s, e + 1).  There is
 * no back-shift: a window that is not clipped has win + 1 frames, the last ones are shorter, down to ONE frame when s == e.  A window with s > e is
 * VOID (an odd win only; first at D = 6 for win = 3 and at D = 15 for win = 5; the host's np.linspace indexes past the array there).  s grows with i,
 * so the void windows are a suffix of [0, W0): window i is void exactly when i * win >= 2 D.  Void windows are no candidates: W_r = the number of
 * non-void windows = min(W0, (2 D - 1) / win + 1) for D >= 1, n_windows reports it, a void index never appears in select or order, and its
 * win_scores and bounds slots are padding.  An index means the same window here and in rv_window_gather_rule (which stores zeros for a void one).
 * Score of a window: the sum of its min(k, hi - lo) largest sims in rv_span_scores' mode-0 order - NaN first, then the larger value, then the
 * smaller index - accumulated from 0 in that order, each add rounded: a NaN frame gives a NaN window, and the score equals rv_span_scores' on a span
 * whose window is [lo, hi) bit for bit.  A window of up to 1024 frames (win <= 1023) is loaded once and ranked from registers, a longer one is read
 * again in every round: the same order, the same picks.
 * Rank order (rv_span_rank's): descending score, ties (-0 against +0 included) to the smaller index, NaN after every number, NaNs among themselves
 * by index.
 * Selection sequence seq, a permutation of the W_r windows.  Pass 1 walks the rank order: a window still alive is taken, and every window j with
 * |i - j| < min_sep dies; a dead window is skipped and kills nothing; min_sep = 1 kills nothing.  Pass 2 appends the windows not yet taken in rank
 * order.  n_select = min(keep, W_r); select = the first n_select entries of seq sorted ascending.  (The first entries of pass 1 do not depend on how
 * far the walk goes, so select needs no more of seq than n_select entries.)
 * Ground truth: a window covers it when float(lo) < ge && float(hi) > gs (both strict); a gt that is not finite or has ge <= gs is void and gives
 * hit_rank = -1.  With min_sep = 1 the place is the score rank.
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: a null sims / mask / select / n_select / n_windows; R < 1; rpm < 1; R not a
 * multiple of rpm; L < 1 or L > 1048576; win < 2; win > L; k outside [1, 64]; Wcap != max(1, ceil(L / hop) - 1) or Wcap > 2048; keep outside
 * [1, Wcap]; min_sep outside [1, Wcap]; hit_rank without gt.
 * One 1024-thread workgroup per row, rows on the grid's x dimension with 64-bit offsets (no limit of 65535 on R); 24 KB of LDS whatever L; vector
 * stores only, no global atomics, no scratch. */
int rvx_window_select_clipped(const float* sims, const float* mask, int32_t R, int32_t rpm, int32_t L, int32_t win, int32_t k, int32_t keep,
                              int32_t min_sep, int32_t Wcap, const float* gt, int32_t* select, int32_t* n_select, int32_t* n_windows,
                              float* win_scores, int32_t* bounds, int32_t* order, int32_t* hit_rank, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif

#endif /* REVISION_HIP_EXT_H */
