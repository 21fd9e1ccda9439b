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

/* ---- span scores over the usable frames: rv_span_scores / rv_span_scores_multi (revision_hip.h) with a say in WHICH frames of a window count.  One
 * kernel source with those two (csrc/span_scores.h), further instances ----
 * sims f32 [rows,L], spans f32 [rows,N,2] as (centre, width), mask f32 [rows / rpm, L] (rpm = "rows per mask": 1 is rv_span_scores' layout, Q is
 * rv_span_scores_multi's with rows = B Q), valid f32 [rows / rpm, L] or NULL ->
 *   scores    f32 [rows,N]
 *   windows   i32 [rows,N,2]   (optional) (lo, hi) of every span; (-1, -1) for a non-finite one
 *   n_usable  i32 [rows,N]     (optional) n, the usable frames of the window; 0 for an empty or a non-finite span
 * Duration, window rule and `windows`: rv_span_scores', operation for operation - the raw f32 sum of the mask row, x = c -+ 0.5 w and p = x * duration
 * with each operation rounded on its own, start = max(0, int(floor(p1))), end = int(ceil(p2)), Python's range(L)[start:end] over the ARRAY length L
 * with a negative end included; a non-finite p gives the score NaN and the window (-1, -1).  `valid` never changes the duration.
 * USABLE: frame t of row r is usable when valid == NULL || valid[(r / rpm) * L + t] != 0 (the f32 comparison: -0 hides a frame, a NaN in valid does
 * not - it compares unequal to 0) and, with skip_nan = 1, sims[r * L + t] == sims[r * L + t] as well (its similarity is a number).  A hidden frame's
 * similarity never enters any arithmetic: NaN and infinities under it leave no trace.  valid is read only where sims is read: inside [lo, hi).
 * mode 0 (top-k): with n usable frames in [lo, hi), the sum of the first min(k, n) of them in the frame order - NaN first, then the larger value, then
 * the smaller index - accumulated from +0 in that order, each add rounded.  mode 1 (attention): sum_t softmax_t(s / temperature) s_t over the usable
 * frames only; a hidden frame contributes neither to the maximum nor to either sum (it is skipped, not multiplied by 0).  An empty window (hi <= lo)
 * scores 0; a window with hi > lo and n = 0 scores NaN (0x7fc00000).
 * Identity: with valid = NULL and skip_nan = 0 every output equals rv_span_scores' (rpm = 1) / rv_span_scores_multi's (rpm = Q) bit for bit, in
 * both modes.
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: a null sims / spans / mask / scores; rows, L or N below 1; rpm < 1; rows not a
 * multiple of rpm; rows > 65535; mode outside {0, 1}; skip_nan outside {0, 1}; mode 0 with k outside [1, 64]; mode 1 with a temperature that is 0 or
 * not finite.
 * One wave per span, four spans per 256-thread workgroup, the row on the grid's y dimension; 16 B of LDS; vector stores only, no global atomics, no
 * scratch. */
int rvc_span_scores_masked(const float* sims, const float* spans, const float* mask, const float* valid, int32_t rows, int32_t rpm, int32_t L, int32_t N,
                           int32_t mode, int32_t k, float temperature, int32_t skip_nan, float* scores, int32_t* windows, int32_t* n_usable,
                           void* stream);

/* ---- span proposals from the usable frames: rv_span_propose (revision_hip.h) under the same validity.  One kernel source with it
 * (csrc/span_propose.h), a further instance ----
 * The arguments and outputs of rv_span_propose, with valid f32 [R / rpm, L] or NULL behind mask and skip_nan behind N.  USABLE is defined as above,
 * for the frames [0, D) of the duration, which the mask alone gives.  The rule is rv_span_propose's with three changes, and nothing else moves:
 *   (a) smoothing: for a usable t, s'[t] is the sum of the usable frames of [t - h, t + h] n [0, D), h = smooth / 2, taken in ascending order starting
 *       from the first usable one, each add rounded, divided by their count as f32; for a hidden t, s'[t] is NaN (0x7fc00000).
 *   (b) range: the row's largest and smallest s' are taken over the non-NaN s' as before, so the hidden frames drop out by (a).
 *   (c) detection: a hidden frame is never above; it breaks a run unless `gap` closes it; a run's length hi - lo counts the hidden frames inside it.
 * A row with no usable frame gives 0 spans and n_found 0.  `smoothed` holds NaN at the hidden frames.  Unchanged: the span encoding, the order
 * (highest level first, ascending lo), the duplicate rule, the padding, the counts.
 * Identities: valid = NULL with skip_nan = 0 is rv_span_propose bit for bit.  valid of ones is valid = NULL.  At smooth = 1 the call equals
 * rv_span_propose on sims with NaN (0x7fc00000) written over the hidden frames, in every output.  At smooth = 1 skip_nan alone changes nothing (a NaN
 * similarity is its own s' there; its bits in `smoothed` become 0x7fc00000 whatever NaN it was).
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: everything rv_span_propose refuses (a null sims / mask / levels / spans / n_spans
 * among it) and skip_nan outside {0, 1}.
 * One 256-thread workgroup per row, three walks over the row's 256-frame tiles; 2928 B of LDS whatever L (the parent's 2608 and one byte per staged
 * frame); vector stores only, no global atomics, no scratch. */
int rvc_span_propose_masked(const float* sims, const float* mask, const float* valid, int32_t R, int32_t rpm, int32_t L, const float* levels, int32_t T,
                            int32_t relative, int32_t smooth, int32_t gap, int32_t min_len, int32_t max_len, int32_t N, int32_t skip_nan, float* spans,
                            int32_t* n_spans, int32_t* n_found, int32_t* windows, float* smoothed, void* stream);

/* ---- a window selection becomes a validity row: the joint between the coarse half (rvc_window_select_frames) and the fine half (the masked span
 * entries).  "Search each query only inside the windows chosen for it" is this launch in front of the two _rows entries below ----
 * select i32 [R,keep] (rvc_window_select_frames' `select` as it lies, -1 padding included, or window indices from anywhere: the LLM's answers, a
 * retrieval log), mask f32 [R / rpm, L] (rpm = "rows per mask"; R a multiple of rpm), valid_in f32 [R / rpm, L] or NULL ->
 *   valid     f32 [R,L]   1.0f at the frames the row's named windows cover, +0.0f elsewhere; EVERY element of [r, 0 .. L) is written, so the caller may
 *                         pass uninitialised memory
 *   n_valid   i32 [R]     (optional) the ones of the row
 * Duration: D from the mask row (r / rpm) by the code of rvc_window_select_frames (the block sum of csrc/grounding.h at that kernel's width and
 * duration_frames): bit for bit that entry's duration.
 * Windows: the window count W_r and the frames [lo, hi) of window i are rvc_window_select_frames' for the same rule / win / stride (ws_count,
 * ws_bounds, ws_bounds_clipped); the clipped rule's void windows are no windows, so W_r counts the others as n_windows does there.
 * Frame set of a window: rvc_window_select_frames' - frames = RV_FRAMES_ALL (0), F = 0: every frame of [lo, hi); frames = RV_FRAMES_SAMPLED (1):
 * np.linspace(lo, hi - 1, F, dtype=int32)[j] for j < F, the frames rv_window_gather[_rule] hands on.  An index means the same frames in the selection,
 * in the gather and here.
 * Ignored entries: an entry of select outside [0, W_r) names nothing and is ignored, as rv_window_gather ignores it: the -1 padding, anything negative,
 * anything >= W_r, a void window.  Order and duplicates do not matter.
 * valid[r, t] = 1.0f when all three hold: t < D; t is in the frame set of at least one named window of row r; valid_in is NULL or
 * valid_in[(r / rpm) * L + t] != 0 (the f32 comparison of the entries above: -0 hides a frame, a NaN in valid_in does not).  Otherwise +0.0f; the
 * frames at or behind D are 0.  valid_in is read only at frames a named window covers.
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: a null select / mask / valid; rule outside {0, 1}; frames outside {0, 1}; R < 1;
 * rpm < 1; R not a multiple of rpm; L < 1 or L > 1048576; rule 1 with stride != 2; stride < 1; win < stride; win > L; RV_FRAMES_SAMPLED with F < 1 or
 * F > 1024; RV_FRAMES_ALL with F != 0; keep outside [1, 2048].
 * One 1024-thread workgroup per row, rows on the grid's x dimension with 64-bit offsets: the duration, a zero fill of the row (16-byte stores between
 * its 16-byte boundaries), behind a barrier the named windows' frames stored as 0 / 1 (overlapping windows store the same value to a frame, so the
 * order does not show), behind another barrier the count.  128 B of LDS whatever L; vector stores only, no atomics, no scratch. */
int rvc_windows_valid(const int32_t* select, const float* mask, const float* valid_in, int32_t R, int32_t rpm, int32_t L, int32_t rule, int32_t win,
                      int32_t stride, int32_t frames, int32_t F, int32_t keep, float* valid, int32_t* n_valid, void* stream);

/* ---- the two masked span entries with a validity row per ROW: rvc_span_scores_masked and rvc_span_propose_masked with one more argument, rpv ("rows
 * per validity row"), directly behind valid ----
 * valid is f32 [rows / rpv, L] (or NULL), and frame t of row r is usable by valid[(r / rpv) * L + t]; everything else is the definition of the entry
 * without _rows word for word.  The mask row, hence the duration, stays row (r / rpm).  rpv = 1 with rpm = Q on a [B,Q,L] layout gives every query
 * its own validity row - rvc_windows_valid's output for a per-query selection - under its video's one duration.
 * Identities: with rpv = rpm every output equals the entry without _rows bit for bit.  With rpv = 1 on a [B,Q,L] layout every (b, q) equals that
 * entry on the row alone (rpm = 1, its video's mask row, its own validity row) bit for bit.
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: everything the entry without _rows refuses, under the same conditions, and rpv < 1
 * or rows not a multiple of rpv.
 * The kernels, the launch geometry and the resources are those entries': one more scalar argument. */
int rvc_span_scores_masked_rows(const float* sims, const float* spans, const float* mask, const float* valid, int32_t rpv, int32_t rows, int32_t rpm,
                                int32_t L, int32_t N, int32_t mode, int32_t k, float temperature, int32_t skip_nan, float* scores, int32_t* windows,
                                int32_t* n_usable, void* stream);
int rvc_span_propose_masked_rows(const float* sims, const float* mask, const float* valid, int32_t rpv, int32_t R, int32_t rpm, int32_t L,
                                 const float* levels, int32_t T, int32_t relative, int32_t smooth, int32_t gap, int32_t min_len, int32_t max_len, int32_t N,
                                 int32_t skip_nan, float* spans, int32_t* n_spans, int32_t* n_found, int32_t* windows, float* smoothed, void* stream);

/* ---- boundary refinement: the stage behind the ranking.  A proposal's bounds are where a SMOOTHED row crosses a threshold, an LLM answer's or a
 * retrieval log's are whatever they are; this entry moves every span to the neighbouring start / end pair with the largest contrast between the
 * frames inside and the frames just outside, under the chain's validity rows, and hands the spans back in the encoding rv_span_scores and rv_span_rank
 * read ----
 * sims f32 [rows,L] (COSINE rows: values are clamped to [-1, 1]), spans f32 [rows,N,2], form (1: (centre, width), 0: (start, end); fractions of the
 * duration, as rv_span_rank's forms), mask f32 [rows / rpm, L] (rpm = "rows per mask"), valid f32 [rows / rpv, L] or NULL (rpv = "rows per validity
 * row": rpm for a row per mask row, 1 for a row per row of sims) ->
 *   out_spans  f32 [rows,N,2]   ALWAYS (centre, width), rv_span_propose's encoding of the chosen window; two quiet NaNs (0x7fc00000) for a void span
 *   windows    i32 [rows,N,2]   (optional) the chosen (a, b); (-1, -1) for a void span
 *   contrast   f32 [rows,N]     (optional) (float)J of the choice; NaN when no candidate is admissible and for a void span
 *   contrast0  f32 [rows,N]     (optional) (float)J of the original pair; NaN when it is not admissible and for a void span
 * Duration and window: dur is the mask row's raw f32 sum as rv_span_scores takes it, D = min(L, floor(dur)) frames (none for a sum that is not finite
 * or below 1: rvc_window_select_frames' duration_frames).  form 1: x1 = c - 0.5 w, x2 = c + 0.5 w; form 0: x1 = start, x2 = end.  From there the
 * window [lo, hi) is rv_span_scores' rule, operation for operation: p = x * dur, each operation rounded on its own, start = max(0, int(floor(p1))),
 * end = int(ceil(p2)), saturating, Python's range(L)[start:end] over the ARRAY length L with a negative end included.  Then lo0 = min(lo, D),
 * hi0 = min(hi, D).  A VOID span names nothing: a non-finite p1 / p2, or hi0 <= lo0.
 * USABLE: frame t < D is usable when valid == NULL || valid[(r / rpv) * L + t] != 0 (the f32 comparison of the entries above: -0 hides a frame, a
 * NaN in valid does not) and its similarity is a number.  A usable frame's value is the integer q[t] = rint(clamp(s[t], -1, 1) * 16777216.f) (2^24
 * steps to the unit; the product is exact in f32, the rounding is ties-to-even; +-inf clamps to +-1).  For an interval, S(x, y) is the int64 sum of q
 * over the usable frames of [x, y) and C(x, y) their count: exact integers, so NO RESULT DEPENDS ON THE ORDER OF ANY SUM.  A hidden frame's similarity
 * enters nothing; valid is read only where sims is read.
 * Candidates: a in [max(0, lo0 - radius), min(lo0 + radius, D - 1)], b in [max(1, hi0 - radius), min(hi0 + radius, D)], b - a >= min_len - except
 * that the original pair (lo0, hi0) is always a candidate.  A candidate is ADMISSIBLE when Cin = C(a, b) > 0 and
 * Cout = C(max(0, a - margin), a) + C(b, min(D, b + margin)) > 0.  Its contrast, in float64 with each of the three operations rounded on its own, is
 *   J(a, b) = (double)Sin / (double)Cin - (double)Sout / (double)Cout,   Sin = S(a, b), Sout = S(max(0, a - margin), a) + S(b, min(D, b + margin))
 * (|S| <= 2^44: the conversions are exact and J is one well-defined double).
 * Choice: the admissible candidate with the largest J; then the smallest |a - lo0| + |b - hi0|; then the smaller a; then the smaller b.  With no
 * admissible candidate the original pair is kept and contrast is NaN.
 * Output: windows = (a, b); out_spans: c = ((a + b) * 0.5) / dur, w = ((b - a) - 0.5) / dur in f32, each operation rounded - so rv_span_scores
 * recovers exactly [a, b) from out_spans for L <= 2^20 under a 0 / 1 mask.
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: a null sims / spans / mask / out_spans; form outside {0, 1}; rows or N below 1; L
 * outside [1, 1048576]; rpm or rpv below 1, or rows not a multiple of either; rows > 65535; radius outside [1, 64]; margin outside [1, 128];
 * min_len < 1.
 * One wave per span, four spans per 256-thread workgroup, the row on the grid's y dimension.  Every read of sims and valid lies in front of D, inside
 * the zones [lo0 - radius - margin, lo0 + radius) and [hi0 - radius, hi0 + radius + margin) or inside the span.  24688 B of LDS whatever L (514
 * prefix pairs per wave); vector stores only, no atomics, no scratch. */
int rvc_span_refine(const float* sims, const float* spans, int32_t form, const float* mask, const float* valid, int32_t rpv, int32_t rows, int32_t rpm,
                    int32_t L, int32_t N, int32_t radius, int32_t margin, int32_t min_len, float* out_spans, int32_t* windows, float* contrast,
                    float* contrast0, void* stream);

/* ---- multi-scale sliding-window proposals: the chain's SECOND generator of candidate moments, beside rv_span_propose.  That one thresholds the row at
 * fractions of its range, so one outlier frame (a title card, a shot that matches the query text literally) compresses every level and a long, modest
 * plateau is never proposed.  This one slides windows ("anchors") of up to eight lengths along the row, scores each from its own frames and their
 * surroundings alone, and hands back each scale's local peaks in the encoding rv_span_scores, rv_span_rank and rvc_span_refine read ----
 * sims f32 [rows,L] (COSINE rows: values are clamped to [-1, 1]), mask f32 [rows / rpm, L] (rpm = "rows per mask"), valid f32 [rows / rpv, L] or NULL
 * (rpv = "rows per validity row": rpm for a row per mask row, 1 for a row per row of sims), scales: a HOST table of S int32 triples
 * (len, stride, margin) in frames, 1 <= S <= 8 ->
 *   out_spans  f32 [rows,max_spans,2]   (centre, width), rv_span_propose's encoding of the kept peaks' windows; two quiet NaNs (0x7fc00000) in the padding
 *   scores     f32 [rows,max_spans]     (float)J of every kept peak; NaN (0x7fc00000) in the padding
 *   n_spans    i32 [rows]               min(n_found, max_spans)
 *   n_found    i32 [rows]               the peaks of the row, kept or not
 *   windows    i32 [rows,max_spans,2]   (optional) (a, b) of every kept peak; (-1, -1) in the padding
 *   scale      i32 [rows,max_spans]     (optional) the scale index of every kept peak; -1 in the padding
 * Duration, usable frames, quantisation and sums are rvc_span_refine's: dur is the mask row's raw f32 sum as rv_span_scores takes it,
 * D = min(L, floor(dur)) frames (none for a sum that is not finite or below 1).  USABLE: frame t < D is usable when valid == NULL ||
 * valid[(r / rpv) * L + t] != 0 (the f32 comparison of the entries above: -0 hides a frame, a NaN in valid does not) and its similarity is a number.
 * A usable frame's value is the integer q[t] = rint(clamp(s[t], -1, 1) * 16777216.f) (2^24 steps to the unit; the product is exact in f32, the
 * rounding is ties-to-even; +-inf clamps to +-1).  S(x, y) is the int64 sum of q over the usable frames of [x, y) and C(x, y) their count: exact
 * integers, so NO RESULT DEPENDS ON THE ORDER OF ANY SUM.  A hidden frame's similarity enters nothing; nothing at or behind D is read, of sims or
 * of valid.
 * Anchors: scale s has the anchors [a_i, a_i + len_s) with a_i = i * stride_s for every i >= 0 with a_i + len_s <= D and, if D >= len_s and
 * (D - len_s) % stride_s != 0, ONE MORE, the last index, flush with the end: a = D - len_s.  A scale with len_s > D has no anchors.
 * Score, by mode, with b = a + len_s, Sin = S(a, b), Cin = C(a, b):
 *   RVC_ANCHORS_MEAN (0):      J = (double)Sin / (double)Cin.
 *   RVC_ANCHORS_CONTRAST (1):  J = (double)Sin / (double)Cin - (double)Sout / (double)Cout, Sout = S(max(0, a - margin_s), a) + S(b, min(D, b + margin_s))
 *                              and Cout likewise: rvc_span_refine's J, operation for operation, in float64 with each of the three operations rounded
 *                              on its own.  An anchor touching 0 or D has one-sided context.
 * An anchor is ADMISSIBLE when Cin >= min_usable and, in contrast mode, Cout > 0.
 * Peaks (local suppression within a scale): order a scale's anchors by (J descending as float64 VALUES, index ascending).  An admissible anchor i is
 * a PEAK when no admissible j != i of the same scale with |j - i| <= peak precedes it in that order.  peak = 0 makes every admissible anchor a peak.
 * A FLAT STRETCH THEREFORE YIELDS ONLY ITS FIRST ANCHOR (and, where the stretch is longer than peak anchors, NOT one anchor every peak + 1: each later
 * anchor is preceded by its left neighbour).  Scales do not suppress each other: rv_span_rank's NMS does that.
 * Capacity: n_found is the number of peaks of the row.  If n_found > max_spans, the kept set is the first max_spans peaks in the order (J descending,
 * scale index ascending, anchor index ascending): truncation is by score, not by position.
 * Output order: the kept peaks in (scale index, anchor index) order.  out_spans: c = ((a + b) * 0.5) / dur, w = ((b - a) - 0.5) / dur in f32, each
 * operation rounded - so rv_span_scores recovers exactly [a, b) from out_spans for L <= 2^20 under a 0 / 1 mask.
 * Workspace: rvc_span_anchors_workspace(L, scales, S, rows) bytes of device memory, 16-byte aligned, contents arbitrary before and after: per row
 * L + 1 prefix pairs (S, C) and two 64-bit keys for each anchor a row of D = L frames has.  That function refuses (returns RV_ERR_ARG) what the entry
 * refuses of L, scales, S and rows, but for the margins.
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: a null sims / mask / out_spans / scores / n_spans / n_found / scales; mode outside
 * {0, 1}; S outside [1, 8]; L outside [1, 1048576]; rows < 1; a scale with len < 1 or stride outside [1, len], or with margin < 1 in contrast mode;
 * rpm or rpv below 1, or rows not a multiple of either; peak outside [0, 64]; min_usable < 1; max_spans outside [1, 2048] (rv_span_rank's N); a null
 * or misaligned workspace, or workspace_bytes below rvc_span_anchors_workspace().
 * One 1024-thread workgroup per row, rows on the grid's x dimension with 64-bit offsets (no 65535 limit): one walk over the row for the prefix pairs,
 * one pass over the anchors for their scores, one for the peak test, then an ordered compaction; only a row with n_found > max_spans pays eight more
 * passes over its anchors for the cut.  1664 B of LDS whatever L; vector stores only, no global atomics (integer LDS atomics count the cut's
 * histogram), no scratch. */
#define RVC_ANCHORS_MEAN 0
#define RVC_ANCHORS_CONTRAST 1
int64_t rvc_span_anchors_workspace(int32_t L, const int32_t* scales, int32_t S, int32_t rows);
int rvc_span_anchors(const float* sims, const float* mask, const float* valid, int32_t rpv, int32_t rows, int32_t rpm, int32_t L, const int32_t* scales,
                     int32_t S, int32_t mode, int32_t peak, int32_t min_usable, int32_t max_spans, float* out_spans, float* scores, int32_t* n_spans,
                     int32_t* n_found, int32_t* windows, int32_t* scale, void* workspace, int64_t workspace_bytes, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif

#endif /* REVISION_HIP_CHAIN_H */
