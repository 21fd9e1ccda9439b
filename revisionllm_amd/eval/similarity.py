"""The reference's ``revisionllm/eval/similarity.py`` under its module name: ``span_cxw_to_xx`` (:5-21), ``forward_clip_matching`` (:24-41),
``_get_predicted_proposal_feat`` (:44-69), ``_topk_pooling`` (:71-94, imported by the drivers at eval_nlq_retrieval_e2e2.py:22 / eval_nlq_negative.py:21 and
called at e2e2.py:384, negative.py:313) and ``_attention_pooling`` (:96-113), with the reference's positional signatures.  The arithmetic is the HIP
kernels behind ``rv_topk_pool``, ``rv_frame_cosine`` + ``rv_span_scores`` and ``rv_attn_pool``; there is no CPU path (host tensors are staged to the
device and the result comes back on the caller's device, in the float dtype of the video features like the reference's result).  Only
``span_cxw_to_xx`` is plain torch on whatever device its input lives.

Proposal-query matching: the reference walks the proposals in a Python double loop (slice, per-frame norm, topk, gather, einsum per proposal, after two
device -> host copies of the window bounds).  A proposal's score is the sum of the top-k cosines of its window, so here the features are read once into a
per-frame cosine row and one more launch scores every span on that row; durations and windows never leave the device.  Keywords after ``is_groundtruth``
are this build's: ``k`` (the reference's 3), ``pooling`` ("topk", or "attention" = the alternative commented out at similarity.py:63 with ``temperature``),
``return_windows``.  Not taken: the reference's bf16 arithmetic (16-bit features are read as stored, all arithmetic is f32), per-frame
masking (as in the reference the mask only gives each video's duration).  Per-frame masking is taken under new names only:
``forward_clip_matching_masked``, ``propose_spans_masked`` and ``ground_queries_masked`` accept the ``valid`` rows of ``select_windows_frames`` and /
or skip the NaN cosines of zeroed feature rows (``skip_nan``) - ``rvc_span_scores_masked`` and ``rvc_span_propose_masked`` of the chain library behind
the unchanged cosine kernels, the same number of launches, no synchronisation.

Several texts per video (this build's addition, no counterpart in the reference): ``forward_clip_matching_multi`` scores Q queries, each with its own
proposals, against one pass over their video's features (``rv_frame_cosine_multi`` on the f32-input MFMA + ``rv_span_scores_multi``).

Ranking (this build's addition; the reference ranks on the host from JSON logs, metric_retrieval_forward.py:35-56): ``rank_proposals`` takes the score
rows of either matching call with their proposals and returns, per row, the best proposals in order with near-duplicates removed and - given a ground
truth - their IoUs and first hits (``rv_span_rank``, one launch); ``eval.metrics.grounding_metrics_ranked`` reduces those to mIoU / R{r}@{m}.

Proposals (this build's addition; the reference's proposals come from the LLM): ``propose_spans`` turns the per-frame cosine rows themselves into
candidate spans - the row smoothed, thresholded at several levels, stretches above a threshold with short gaps closed (``rv_span_propose``, one
launch) - in the (centre, width) form every call above takes.  ``ground_queries`` chains the four device stages - cosine rows, proposals, span scores,
ranking - into a grounder that needs no proposals from outside and never synchronises: ``Grounding(spans, scores, n_keep, proposals, rank)``.

Window selection (the reference evaluates this stage in evaluate_pre_filtered_window.py and feeds it from a stage-1 LLM log, e2e2.py:278-294):
``select_windows`` turns the cosine rows into the sorted window list ``run_query(grounding_windows=)`` takes - every window of ``cut_windows``'
geometry scored by its top-k cosines, the best ``keep`` spread at least ``min_sep`` apart (``rv_window_select``, one launch) - and, given a ground
truth, the place of the first window that overlaps it (``eval.metrics.window_recall``).

Coarse to fine (this build's addition): ``ground_queries_in_windows`` joins the two halves per query - the cosine rows once, the windows chosen on
them (or given: the LLM's answers, a retrieval log), ``windows_valid`` turning each query's windows into its own validity row
(``rvc_windows_valid``), and the proposal, score and rank stages run under those rows (``rvc_span_propose_masked_rows``,
``rvc_span_scores_masked_rows``) - in a fixed number of launches whatever Q, with no synchronisation."""
import collections
import math

import torch

from .. import ops

_FLOATS = (torch.float16, torch.bfloat16, torch.float32)


def span_cxw_to_xx(cxw_spans):
    """(..., 2) rows of (centre, width) -> (..., 2) rows of (start, end) = (centre - width / 2, centre + width / 2), in the input's type and on its device."""
    centre, width = cxw_spans.unbind(dim=-1)
    half = 0.5 * width                       # exact: the two bounds carry one rounding each, as the reference's do
    return torch.stack((centre - half, centre + half), dim=-1)


def _device_of(t, who):
    if t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        from ..hip import HipLibraryError
        raise HipLibraryError(f"{who} runs on the HIP device path only (no GPU visible)")
    return torch.device("cuda", torch.cuda.current_device())


def _features_up(video, dev):
    """The features on the device in a type the kernels read (16-bit floats and f32 as they are, anything else as f32)."""
    video = video if video.is_cuda else ops.h2d(video, dev)
    return video if video.dtype in _FLOATS else video.float()


def _topk_pooling(text_embeds, video_embeds, k):
    """text_embeds [num_texts, d], video_embeds [num_vids, num_frames, d] -> [num_vids, num_texts, d]: for every (video, text)
    the SUM of the k frames with the largest ``<frame, text>``."""
    if text_embeds.dim() != 2 or video_embeds.dim() != 3 or text_embeds.shape[1] != video_embeds.shape[2]:
        raise ValueError(f"_topk_pooling: text {tuple(text_embeds.shape)} / video {tuple(video_embeds.shape)}")
    home, dt = video_embeds.device, video_embeds.dtype
    if not video_embeds.is_cuda:
        if not torch.cuda.is_available():
            from ..hip import HipLibraryError
            raise HipLibraryError("_topk_pooling runs on the HIP device path only (no GPU visible)")
        dev = torch.device("cuda", torch.cuda.current_device())
        video_embeds = ops.h2d(video_embeds, dev)
    if video_embeds.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        video_embeds = video_embeds.float()
    text = text_embeds.to(video_embeds.device).float()
    return ops.topk_pool(text, video_embeds, k).to(device=home, dtype=dt)


def _attention_pooling(text_embeds, video_embeds, temperature):
    """text_embeds [num_texts, d], video_embeds [num_vids, num_frames, d] -> [num_vids, num_texts, d]: for every (video, text)
    ``sum_t softmax_t(<frame_t, text> / temperature) frame_t`` (similarity.py:96-113)."""
    if text_embeds.dim() != 2 or video_embeds.dim() != 3 or text_embeds.shape[1] != video_embeds.shape[2]:
        raise ValueError(f"_attention_pooling: text {tuple(text_embeds.shape)} / video {tuple(video_embeds.shape)}")
    temperature = float(temperature)
    if temperature == 0.0 or not math.isfinite(temperature):
        raise ValueError(f"_attention_pooling: temperature={temperature} must be finite and not 0")
    home, dt = video_embeds.device, video_embeds.dtype
    dev = _device_of(video_embeds, "_attention_pooling")
    video = _features_up(video_embeds, dev)
    text = ops.h2d(text_embeds, dev).float()
    return ops.attn_pool(text, video, temperature).to(device=home, dtype=dt if dt.is_floating_point else torch.float32)


def _match_checks(who, text, video, mask, proposal, k, pooling, temperature, multi):
    """The refusals of the matching calls, raised before any device is looked for."""
    if proposal is None:
        raise TypeError(f"{who}: proposal is None (the reference fails there too: it has no default proposals)")
    for name, t in (("text", text), ("video", video), ("mask", mask), ("proposal", proposal)):
        if not torch.is_tensor(t):
            raise ValueError(f"{who}: {name} must be a tensor (got {type(t).__name__})")
    if multi:
        if video.dim() != 3 or text.dim() != 3 or text.shape[0] != video.shape[0] or text.shape[2] != video.shape[2]:
            raise ValueError(f"{who}: text {tuple(text.shape)} / video {tuple(video.shape)} (expected [B, Q, d] and [B, L, d])")
        if text.shape[1] == 0:
            raise ValueError(f"{who}: no text in {tuple(text.shape)}")
    elif video.dim() != 3 or text.dim() != 2 or text.shape != (video.shape[0], video.shape[2]):
        raise ValueError(f"{who}: text {tuple(text.shape)} / video {tuple(video.shape)} (expected [B, d] and [B, L, d])")
    if mask.shape != video.shape[:2]:
        raise ValueError(f"{who}: mask {tuple(mask.shape)} for video {tuple(video.shape)} (expected [B, L])")
    if multi:
        if proposal.dim() != 4 or proposal.shape[:2] != text.shape[:2] or proposal.shape[3] != 2:
            raise ValueError(f"{who}: proposal {tuple(proposal.shape)} (expected [B={text.shape[0]}, Q={text.shape[1]}, N, 2] rows of (centre, width))")
    elif proposal.dim() != 3 or proposal.shape[0] != video.shape[0] or proposal.shape[2] != 2:
        raise ValueError(f"{who}: proposal {tuple(proposal.shape)} (expected [B={video.shape[0]}, N, 2] rows of (centre, width))")
    if min(video.shape) == 0:
        raise ValueError(f"{who}: empty video {tuple(video.shape)}")
    for name, t in (("text", text), ("video", video), ("proposal", proposal)):
        if not t.dtype.is_floating_point:
            raise ValueError(f"{who}: {name} must be a floating-point tensor (got {t.dtype})")
    if mask.dtype.is_complex:
        raise ValueError(f"{who}: mask must be bool, integer or floating point (got {mask.dtype})")
    if pooling not in ops.SPAN_POOLINGS:
        raise ValueError(f"{who}: pooling={pooling!r} (expected one of {sorted(ops.SPAN_POOLINGS)})")
    if pooling == "topk" and not (isinstance(k, int) and 1 <= k <= 64):
        raise ValueError(f"{who}: k={k!r} must be an integer in [1, 64]")
    if pooling == "attention" and (float(temperature) == 0.0 or not math.isfinite(float(temperature))):
        raise ValueError(f"{who}: temperature={temperature} must be finite and not 0")


def _match(who, text, video, mask, proposal, k, pooling, temperature, return_windows, multi=False):
    _match_checks(who, text, video, mask, proposal, k, pooling, temperature, multi)
    home, dt = video.device, video.dtype
    dev = _device_of(video, who)
    video = _features_up(video, dev)
    cosine, scores = (ops.frame_cosine_multi, ops.span_scores_multi) if multi else (ops.frame_cosine, ops.span_scores)
    sims = cosine(ops.h2d(text, dev).float(), video)
    out = scores(sims, ops.h2d(proposal, dev).float(), ops.h2d(mask, dev).float(), k=k, pooling=pooling, temperature=temperature,
                 return_windows=return_windows)
    if return_windows:
        return out[0].to(device=home, dtype=dt), out[1].to(device=home)
    return out.to(device=home, dtype=dt)


def forward_clip_matching(src_cls_txt, src_vid_appear, src_vid_appear_mask, proposal=None, is_groundtruth=False, *, k=3, pooling="topk",
                          temperature=0.01, return_windows=False):
    """src_cls_txt [B, d], src_vid_appear [B, L, d], src_vid_appear_mask [B, L] (0 on padding: its row sum is the video's duration), proposal [B, N, 2]
    rows of (centre, width) as fractions of the duration -> the proposal-query similarity matrix [B, N] (similarity.py:24-41): the sum of the
    min(k, len) largest cosines between the text CLS and the frames of ``range(L)[floor(x1 * duration) : ceil(x2 * duration)]``; an empty window scores 0.
    Two launches (plus one small cast kernel for each of: a mask or proposals that are not f32, a 16-bit result), no device -> host copy and no synchronisation
    when the inputs live on the device.  ``return_windows``: also the i32 [B, N, 2] windows
    (lo, hi) the scores were taken over.  ``is_groundtruth`` is accepted and unused, as in the reference."""
    return _match("forward_clip_matching", src_cls_txt, src_vid_appear, src_vid_appear_mask, proposal, k, pooling, temperature, return_windows)


def forward_clip_matching_multi(src_cls_txt, src_vid_appear, src_vid_appear_mask, proposal=None, is_groundtruth=False, *, k=3, pooling="topk",
                                temperature=0.01, return_windows=False):
    """``forward_clip_matching`` for Q queries per video: src_cls_txt [B, Q, d], src_vid_appear [B, L, d], src_vid_appear_mask [B, L], proposal
    [B, Q, N, 2] (each query's own (centre, width) rows) -> [B, Q, N], with ``return_windows`` also the i32 [B, Q, N, 2] windows.  ``out[:, q]`` is
    ``forward_clip_matching(src_cls_txt[:, q], src_vid_appear, src_vid_appear_mask, proposal[:, q])`` within the cosine bound (the windows exactly),
    but the features are read once for all Q texts: three launches (text norms, cosine rows on the f32-input MFMA, spans), no synchronisation, and the
    video is not copied.  A query's scores do not depend on Q, on its slot or on the other texts, bit for bit; Q = 1 takes the same kernels (callers
    with one text per video keep ``forward_clip_matching``).  Dtype and device handling, keywords and refusals are ``forward_clip_matching``'s."""
    return _match("forward_clip_matching_multi", src_cls_txt, src_vid_appear, src_vid_appear_mask, proposal, k, pooling, temperature, return_windows,
                  multi=True)


def rank_proposals(scores, proposal, *, top=None, nms_iou=1.0, gt=None, hit_iou=ops.HIT_IOU, return_order=False):
    """scores [B, N] or [B, Q, N] (``forward_clip_matching`` / ``_multi``'s result), proposal [..., N, 2] rows of (centre, width) as those calls take them,
    gt [..., 2] rows of (start, end) or None -> ``ops.SpanRank(keep, n_keep, keep_iou, first_hit, order)``: per row the indices of the proposals that
    survive greedy NMS (``inter > nms_iou * union`` against an earlier kept one; 1.0 = none) in descending score order, at most ``top`` (None: all), padded
    with -1; how many; with ``gt`` their IoUs with it and, per threshold of ``hit_iou``, the first kept place whose IoU exceeds it (-1: none); with
    ``return_order`` the full rank order.  Ties go to the smaller index and a NaN score ranks last.  One launch, no synchronisation and no device -> host
    copy when the inputs live on the device; host tensors are staged and the results come back on the device ``scores`` lives on.  16-bit scores are
    read as f32 (exact)."""
    who = "rank_proposals"
    for name, t in (("scores", scores), ("proposal", proposal)) + ((("gt", gt),) if gt is not None else ()):
        if not torch.is_tensor(t):
            raise ValueError(f"{who}: {name} must be a tensor (got {type(t).__name__})")
        if not t.dtype.is_floating_point:
            raise ValueError(f"{who}: {name} must be a floating-point tensor (got {t.dtype})")
    if scores.dim() not in (2, 3) or proposal.shape != scores.shape + (2,):
        raise ValueError(f"{who}: scores {tuple(scores.shape)} / proposal {tuple(proposal.shape)} (expected [B, N] or [B, Q, N] and [..., N, 2] rows of "
                         f"(centre, width))")
    if gt is not None and gt.shape != scores.shape[:-1] + (2,):
        raise ValueError(f"{who}: gt {tuple(gt.shape)} for scores {tuple(scores.shape)} (expected [..., 2] rows of (start, end))")
    if scores.shape[-1] > ops.SPAN_RANK_MAX:
        raise ValueError(f"{who}: N={scores.shape[-1]} proposals per row (at most {ops.SPAN_RANK_MAX})")
    ops.span_rank_keywords(who, top, nms_iou, hit_iou)
    home = scores.device
    dev = _device_of(scores, who)
    out = ops.span_rank(ops.h2d(scores, dev).float(), ops.h2d(proposal, dev).float(), top=top, nms_iou=nms_iou, form="cxw",
                        gt=None if gt is None else ops.h2d(gt, dev).float(), hit_iou=hit_iou, return_order=return_order)
    return ops.SpanRank(*(None if t is None else t.to(home) for t in out))


def propose_spans(sims, mask, *, levels=ops.SPAN_PROPOSE_LEVELS, relative=True, smooth=1, gap=0, min_len=1, max_len=None, max_spans=256,
                  return_windows=False, return_smoothed=False):
    """``ops.span_propose`` with the device handling of the matching calls: sims [R, L] or [B, Q, L] (the cosine rows; 16-bit rows are read as f32, which
    is exact), mask [R, L] / [B, L] of any bool, integer or float dtype -> ``ops.SpanProposals(spans, n_spans, n_found, windows, smoothed)``: per row
    up to ``max_spans`` candidate spans as (centre, width) fractions of the duration (NaN in the padding), how many, how many there were before
    ``max_spans`` cut the list, and on request their (lo, hi) frame windows and the smoothed row.  One launch, no synchronisation and no device -> host
    copy when the inputs live on the device; host tensors are staged and the results come back on the device ``sims`` lives on."""
    who = "propose_spans"
    ops.span_propose_keywords(who, levels, relative, smooth, gap, min_len, max_len, max_spans)
    ops.span_propose_shapes(who, sims, mask)
    home = sims.device
    dev = _device_of(sims, who)
    out = ops.span_propose(ops.h2d(sims, dev).float(), ops.h2d(mask, dev), levels=levels, relative=relative, smooth=smooth, gap=gap, min_len=min_len,
                           max_len=max_len, max_spans=max_spans, return_windows=return_windows, return_smoothed=return_smoothed)
    return ops.SpanProposals(*(None if t is None else t.to(home) for t in out))


Grounding = collections.namedtuple("Grounding", "spans scores n_keep proposals rank")


def ground_queries(text, video, mask, *, top=10, nms_iou=0.5, k=3, pooling="topk", temperature=0.01, gt=None, hit_iou=ops.HIT_IOU, **propose_keywords):
    """Ground queries in their videos with the matching stage alone: text [B, d] or [B, Q, d], video [B, L, d], mask [B, L], gt [..., 2] rows of
    (start, end) or None -> ``Grounding(spans, scores, n_keep, proposals, rank)``.  Four device stages: the cosine rows (``ops.frame_cosine[_multi]``),
    candidate spans from those rows (``ops.span_propose`` with ``propose_keywords``: levels, relative, smooth, gap, min_len, max_len, max_spans,
    return_windows, return_smoothed), their scores (``ops.span_scores[_multi]`` with ``k``, ``pooling``, ``temperature``) and the ranking
    (``ops.span_rank`` with ``top``, ``nms_iou``, ``gt``, ``hit_iou``).  ``spans`` f32 [..., top, 2] are the kept proposals as (centre, width) in rank
    order and ``scores`` f32 [..., top] their scores, both gathered by ``rank.keep`` with NaN in the padding; ``n_keep`` i32 [...] counts the kept
    places that hold a proposal (``rank.n_keep`` also counts padding spans, which rank last); ``proposals`` and ``rank`` are the ``SpanProposals`` and
    ``SpanRank`` they came from.  ``top`` above ``max_spans`` is ``max_spans``.  No synchronisation and no device -> host copy when the inputs live on
    the device; host tensors are staged and every result comes back on the device ``video`` lives on."""
    return _ground("ground_queries", text, video, mask, None, False, top, nms_iou, k, pooling, temperature, gt, hit_iou, propose_keywords)


def _ground(who, text, video, mask, valid, skip_nan, top, nms_iou, k, pooling, temperature, gt, hit_iou, propose_keywords, masked=False, windows=None, refine=None,
            anchors=None):
    """``ground_queries``, ``ground_queries_masked`` (``masked``: the proposal and the score stage are the chain library's, under ``valid`` and
    ``skip_nan``), ``ground_queries_refined`` (``refine``: a callable ``(sims, mask, valid, kept spans) -> (ops.RefinedSpans, scores)`` that runs behind
    the gather of the kept spans, on the device; the result is ``(Grounding, RefinedSpans, scores)``) and ``ground_queries_in_windows`` (the rows form - ``windows``: a callable ``(sims, mask, valid, gt) -> (selection or None,
    ops.WindowsValid)`` that runs behind the cosine rows; the proposal and the score stage then run under ITS validity rows, one per row of sims, and
    the result is ``(Grounding, selection, WindowsValid)``) and ``ground_queries_anchored`` (``anchors``: a callable ``(sims, mask, valid) ->
    ops.SpanAnchors`` that is the proposal AND the score stage; its caller has checked ``valid``): one body."""
    for name, t in (("text", text), ("video", video), ("mask", mask)) + ((("gt", gt),) if gt is not None else ()):
        if not torch.is_tensor(t):
            raise ValueError(f"{who}: {name} must be a tensor (got {type(t).__name__})")
    multi = text.dim() == 3
    if video.dim() != 3 or text.dim() not in (2, 3) or text.shape[0] != video.shape[0] or text.shape[-1] != video.shape[2] or min(text.shape) == 0:
        raise ValueError(f"{who}: text {tuple(text.shape)} / video {tuple(video.shape)} (expected [B, d] or [B, Q, d] and [B, L, d])")
    if mask.shape != video.shape[:2]:
        raise ValueError(f"{who}: mask {tuple(mask.shape)} for video {tuple(video.shape)} (expected [B, L])")
    if min(video.shape) == 0:
        raise ValueError(f"{who}: empty video {tuple(video.shape)}")
    for name, t in (("text", text), ("video", video)) + ((("gt", gt),) if gt is not None else ()):
        if not t.dtype.is_floating_point:
            raise ValueError(f"{who}: {name} must be a floating-point tensor (got {t.dtype})")
    if mask.dtype.is_complex:
        raise ValueError(f"{who}: mask must be bool, integer or floating point (got {mask.dtype})")
    if gt is not None and gt.shape != text.shape[:-1] + (2,):
        raise ValueError(f"{who}: gt {tuple(gt.shape)} for text {tuple(text.shape)} (expected [..., 2] rows of (start, end))")
    if video.shape[1] > ops.SPAN_PROPOSE_MAX_FRAMES:
        raise ValueError(f"{who}: L={video.shape[1]} frames (at most {ops.SPAN_PROPOSE_MAX_FRAMES})")
    if pooling not in ops.SPAN_POOLINGS:
        raise ValueError(f"{who}: pooling={pooling!r} (expected one of {sorted(ops.SPAN_POOLINGS)})")
    if pooling == "topk" and not (isinstance(k, int) and 1 <= k <= 64):
        raise ValueError(f"{who}: k={k!r} must be an integer in [1, 64]")
    if pooling == "attention" and (float(temperature) == 0.0 or not math.isfinite(float(temperature))):
        raise ValueError(f"{who}: temperature={temperature} must be finite and not 0")
    ops.span_rank_keywords(who, top, nms_iou, hit_iou)
    unknown = set(propose_keywords) - {"levels", "relative", "smooth", "gap", "min_len", "max_len", "max_spans", "return_windows", "return_smoothed"}
    if unknown:
        raise TypeError(f"{who}: unexpected keyword(s) {sorted(unknown)}")
    ops.span_propose_keywords(who, **{n: v for n, v in propose_keywords.items() if not n.startswith("return_")})
    if masked:
        ops.window_select_valid(who, valid, mask)
        ops.skip_nan_flag(who, skip_nan)
    if anchors is not None:
        ops.span_anchors_checks(who, torch.empty(text.shape[:-1] + (video.shape[1],), device="meta"), mask, valid)
    home = video.device
    dev = _device_of(video, who)
    video = _features_up(video, dev)
    mask = ops.h2d(mask, dev).float()
    cosine, score = (ops.frame_cosine_multi, ops.span_scores_multi) if multi else (ops.frame_cosine, ops.span_scores)
    sims = cosine(ops.h2d(text, dev).float(), video)
    gt = None if gt is None else ops.h2d(gt, dev).float()
    if windows is not None:
        selection, rows_valid = windows(sims, mask, None if valid is None else ops.h2d(valid, dev), gt)
        proposals = ops.span_propose_masked_rows(sims, mask, valid=rows_valid.valid, skip_nan=skip_nan, **propose_keywords)
        scores = ops.span_scores_masked_rows(sims, proposals.spans, mask, valid=rows_valid.valid, skip_nan=skip_nan, k=k, pooling=pooling,
                                             temperature=temperature).scores
    elif anchors is not None:
        valid = None if valid is None else ops.h2d(valid, dev)
        proposals = anchors(sims, mask, valid)
        scores = proposals.scores
    elif masked:
        valid = None if valid is None else ops.h2d(valid, dev)
        proposals = ops.span_propose_masked(sims, mask, valid=valid, skip_nan=skip_nan, **propose_keywords)
        scores = ops.span_scores_masked(sims, proposals.spans, mask, valid=valid, skip_nan=skip_nan, k=k, pooling=pooling, temperature=temperature).scores
    else:
        proposals = ops.span_propose(sims, mask, **propose_keywords)
        scores = score(sims, proposals.spans, mask, k=k, pooling=pooling, temperature=temperature)
    rank = ops.span_rank(scores, proposals.spans, top=top, nms_iou=nms_iou, form="cxw", gt=gt, hit_iou=hit_iou)
    held = (rank.keep >= 0) & (rank.keep < proposals.n_spans.unsqueeze(-1))                 # kept places that hold a proposal: a prefix (NaN ranks last)
    at = rank.keep.clamp(min=0).long()
    nan = torch.full((), float("nan"), dtype=torch.float32, device=dev)
    spans = torch.where(held.unsqueeze(-1), torch.gather(proposals.spans, -2, at.unsqueeze(-1).expand(at.shape + (2,))), nan)
    kept_scores = torch.where(held, torch.gather(scores, -1, at), nan)
    back = lambda tup: type(tup)(*(None if t is None else t.to(home) for t in tup))                 # noqa: E731
    grounding = Grounding(spans.to(home), kept_scores.to(home), held.sum(-1, dtype=torch.int32).to(home), back(proposals), back(rank))
    if windows is not None:
        return grounding, None if selection is None else back(selection), back(rows_valid)
    if refine is not None:
        refined, refined_scores = refine(sims, mask, valid, spans)
        return grounding, back(refined), refined_scores.to(home)
    return grounding


def forward_clip_matching_masked(src_cls_txt, src_vid_appear, src_vid_appear_mask, proposal, *, valid=None, skip_nan=False, k=3, pooling="topk",
                                 temperature=0.01, return_windows=False, return_usable=False):
    """``forward_clip_matching`` (src_cls_txt [B, d], proposal [B, N, 2]) / ``forward_clip_matching_multi`` (src_cls_txt [B, Q, d], proposal
    [B, Q, N, 2]) over the frames that count -> ``ops.MaskedSpanScores(scores, windows, n_usable)``: the scores [B, N] / [B, Q, N] in the float dtype
    of the video features, with ``return_windows`` the i32 windows and with ``return_usable`` the i32 count of usable frames of every window (None
    unless asked for).  ``valid`` [B, L] (bool, uint8 or float; None: every frame) hides the frames where it is 0 and ``skip_nan`` the frames whose
    cosine is NaN (a zeroed feature row); the duration and the windows stay the mask's.  A non-empty window without a usable frame scores NaN.  The
    cosine rows come from the unchanged ``ops.frame_cosine[_multi]``, the scores from ``ops.span_scores_masked``: the launches, the device handling,
    the refusals and the absence of any synchronisation are the unmasked calls'."""
    who = "forward_clip_matching_masked"
    multi = torch.is_tensor(src_cls_txt) and src_cls_txt.dim() == 3
    if pooling == "topk" and isinstance(k, bool):
        raise ValueError(f"{who}: k={k!r} must be an integer in [1, 64]")
    if pooling == "attention" and (isinstance(temperature, bool) or not isinstance(temperature, (int, float))):
        raise ValueError(f"{who}: temperature={temperature!r} must be a number")
    _match_checks(who, src_cls_txt, src_vid_appear, src_vid_appear_mask, proposal, k, pooling, temperature, multi)
    ops.window_select_valid(who, valid, src_vid_appear_mask)
    ops.skip_nan_flag(who, skip_nan)
    home, dt = src_vid_appear.device, src_vid_appear.dtype
    dev = _device_of(src_vid_appear, who)
    video = _features_up(src_vid_appear, dev)
    sims = (ops.frame_cosine_multi if multi else ops.frame_cosine)(ops.h2d(src_cls_txt, dev).float(), video)
    out = ops.span_scores_masked(sims, ops.h2d(proposal, dev).float(), ops.h2d(src_vid_appear_mask, dev).float(),
                                 valid=None if valid is None else ops.h2d(valid, dev), skip_nan=skip_nan, k=k, pooling=pooling, temperature=temperature,
                                 return_windows=return_windows, return_usable=return_usable)
    return ops.MaskedSpanScores(out.scores.to(device=home, dtype=dt), *(None if t is None else t.to(home) for t in out[1:]))


def propose_spans_masked(sims, mask, *, valid=None, skip_nan=False, levels=ops.SPAN_PROPOSE_LEVELS, relative=True, smooth=1, gap=0, min_len=1,
                         max_len=None, max_spans=256, return_windows=False, return_smoothed=False):
    """``propose_spans`` from the frames that count (``ops.span_propose_masked``): the same sims, mask, keywords, device handling and
    ``ops.SpanProposals``, with ``valid`` [mask's shape] hiding the frames where it is 0 and ``skip_nan`` the frames whose cosine is NaN.  One launch,
    no synchronisation and no device -> host copy when the inputs live on the device."""
    who = "propose_spans_masked"
    ops.span_propose_keywords(who, levels, relative, smooth, gap, min_len, max_len, max_spans)
    ops.span_propose_shapes(who, sims, mask)
    ops.window_select_valid(who, valid, mask)
    ops.skip_nan_flag(who, skip_nan)
    home = sims.device
    dev = _device_of(sims, who)
    out = ops.span_propose_masked(ops.h2d(sims, dev).float(), ops.h2d(mask, dev), valid=None if valid is None else ops.h2d(valid, dev), skip_nan=skip_nan,
                                  levels=levels, relative=relative, smooth=smooth, gap=gap, min_len=min_len, max_len=max_len, max_spans=max_spans,
                                  return_windows=return_windows, return_smoothed=return_smoothed)
    return ops.SpanProposals(*(None if t is None else t.to(home) for t in out))


def ground_queries_masked(text, video, mask, *, valid=None, skip_nan=False, top=10, nms_iou=0.5, k=3, pooling="topk", temperature=0.01, gt=None,
                          hit_iou=ops.HIT_IOU, **propose_keywords):
    """``ground_queries`` over the frames that count: the same inputs, keywords and ``Grounding``, with ``valid`` [B, L] (bool, uint8 or float; None:
    every frame) hiding the frames where it is 0 and ``skip_nan`` the frames whose cosine is NaN - black frames, padding inside a movie, decoder
    drop-outs, whose zeroed feature rows would otherwise turn every proposal around them into a NaN score that ranks last.  The four stages are
    ``ops.frame_cosine[_multi]`` (unchanged), ``ops.span_propose_masked``, ``ops.span_scores_masked`` and ``ops.span_rank`` (unchanged: a NaN score
    already ranks last): as many launches as ``ground_queries``, no synchronisation and no device -> host copy when the inputs live on the device."""
    return _ground("ground_queries_masked", text, video, mask, valid, skip_nan, top, nms_iou, k, pooling, temperature, gt, hit_iou, propose_keywords,
                   masked=True)


def refine_spans(sims, spans, mask, *, form="cxw", radius, margin, min_len=1, valid=None, return_windows=False, return_contrast=False):
    """``ops.span_refine`` with the device handling of ``propose_spans_masked``: sims [R, L] or [B, Q, L] (the cosine rows; 16-bit rows are read as
    f32, which is exact), spans [..., N, 2] as (centre, width) (``form="cxw"``) or (start, end) (``"xx"``) - kept proposals, an LLM's answers, a
    retrieval log - mask [R, L] / [B, L], ``valid`` of the mask's shape or of ``sims``' shape -> ``ops.RefinedSpans(spans, windows, contrast,
    contrast0)``: every span moved to the neighbouring (start, end) pair with the largest contrast between the usable frames inside and those within
    ``margin`` frames outside, ALWAYS as (centre, width).  One launch, no synchronisation and no device -> host copy when the inputs live on the
    device; host tensors are staged and the results come back on the device ``sims`` lives on."""
    who = "refine_spans"
    ops.span_refine_keywords(who, radius, margin, min_len, form, return_windows, return_contrast)
    ops.span_refine_checks(who, sims.float() if torch.is_tensor(sims) and sims.dtype in _FLOATS else sims, spans, mask, valid)
    home = sims.device
    dev = _device_of(sims, who)
    out = ops.span_refine(ops.h2d(sims, dev).float(), ops.h2d(spans, dev), ops.h2d(mask, dev), form=form, radius=radius, margin=margin, min_len=min_len,
                          valid=None if valid is None else ops.h2d(valid, dev), return_windows=return_windows, return_contrast=return_contrast)
    return ops.RefinedSpans(*(None if t is None else t.to(home) for t in out))


RefinedGrounding = collections.namedtuple("RefinedGrounding", "grounding refined scores")


def _refine_kept(radius, margin, min_len, form, skip_nan, k, pooling, temperature):
    """The stage behind the gather of the kept spans, for ``_ground(refine=)``: ``(sims, mask, valid, kept spans) -> (ops.RefinedSpans, scores)`` -
    ``ops.span_refine`` with windows and contrasts, then ``ops.span_scores_masked``' scores of the refined spans (``ops.span_scores_masked_rows``
    under a validity row per row of sims)."""
    def refine(sims, m, v, kept):
        out = ops.span_refine(sims, kept, m, form="cxw", radius=radius, margin=margin, min_len=min_len, valid=v, return_windows=True, return_contrast=True)
        score = ops.span_scores_masked_rows if v is not None and v.shape == sims.shape and v.shape != m.shape else ops.span_scores_masked
        scores = score(sims, out.spans, m, valid=v, skip_nan=skip_nan, k=k, pooling=pooling, temperature=temperature).scores
        return (out._replace(spans=span_cxw_to_xx(out.spans)) if form == "xx" else out), scores
    return refine


def ground_queries_refined(text, video, mask, *, radius, margin, min_len=1, form="cxw", valid=None, skip_nan=False, top=10, nms_iou=0.5, k=3,
                           pooling="topk", temperature=0.01, gt=None, hit_iou=ops.HIT_IOU, **propose_keywords):
    """``ground_queries_masked`` with the kept spans' bounds refined behind the ranking: the same inputs and keywords ->
    ``RefinedGrounding(grounding, refined, scores)``.  ``grounding`` is what ``ground_queries_masked`` returns for the same keywords (``min_len``
    among its proposal keywords), untouched.  ``refined`` is ``ops.span_refine`` on its kept ``[..., top, 2]`` spans under the same ``valid``, with
    ``radius``, ``margin`` and ``min_len``, windows and contrasts included: ``ops.RefinedSpans(spans, windows, contrast, contrast0)`` in rank order, a
    padding place NaN / (-1, -1).  ``skip_nan`` is implied in this stage - a NaN cosine is never usable there - and applies to the proposal and score
    stages as given.  ``scores`` f32 [..., top] are ``ops.span_scores_masked``' scores of the refined spans (``valid``, ``skip_nan``, ``k``,
    ``pooling``, ``temperature``); the order stays the ranking's.  ``form`` is the form ``refined.spans`` comes back in: "cxw" as the kernel writes it,
    "xx" converted with ``span_cxw_to_xx`` (the scores are taken on the (centre, width) spans either way).  There is NO second NMS: two kept spans
    may refine onto each other, or onto the same window.  The launches are ``ground_queries_masked``' and two more (three with ``form="xx"``), a fixed
    number whatever Q; no synchronisation and no device -> host copy when the inputs live on the device."""
    who = "ground_queries_refined"
    ops.span_refine_keywords(who, radius, margin, min_len, form)
    if "min_len" in propose_keywords:                                  # (cannot happen through the signature; stated for a caller's **dict)
        raise TypeError(f"{who}: min_len given twice")

    grounding, refined, scores = _ground(who, text, video, mask, valid, skip_nan, top, nms_iou, k, pooling, temperature, gt, hit_iou,
                                         dict(propose_keywords, min_len=min_len), masked=True,
                                         refine=_refine_kept(radius, margin, min_len, form, skip_nan, k, pooling, temperature))
    return RefinedGrounding(grounding, refined, scores)


def propose_anchors(sims, mask, *, scales, score="contrast", peak=2, min_usable=1, valid=None, max_spans=256, return_windows=False, return_scale=False):
    """``ops.span_anchors`` with the device handling of ``propose_spans``: sims [R, L] or [B, Q, L] (the cosine rows; 16-bit rows are read as f32,
    which is exact), mask [R, L] / [B, L], ``valid`` of the mask's shape or of ``sims``' shape -> ``ops.SpanAnchors(spans, scores, n_spans, n_found,
    windows, scale)``: per row the local peaks of sliding windows at every one of ``scales``, scored by their frames' mean cosine or its contrast
    with the frames just outside - candidates that do not depend on the row's range of values, which ``propose_spans``' relative levels do.  One
    launch, no synchronisation and no device -> host copy when the inputs live on the device; host tensors are staged and the results come back on
    the device ``sims`` lives on."""
    who = "propose_anchors"
    ops.span_anchors_keywords(who, scales, score, peak, min_usable, max_spans, return_windows, return_scale)
    ops.span_anchors_checks(who, sims, mask, valid)
    home = sims.device
    dev = _device_of(sims, who)
    out = ops.span_anchors(ops.h2d(sims, dev).float(), ops.h2d(mask, dev), scales=scales, score=score, peak=peak, min_usable=min_usable,
                           valid=None if valid is None else ops.h2d(valid, dev), max_spans=max_spans, return_windows=return_windows,
                           return_scale=return_scale)
    return ops.SpanAnchors(*(None if t is None else t.to(home) for t in out))


def ground_queries_anchored(text, video, mask, *, scales, score="contrast", peak=2, min_usable=1, valid=None, max_spans=256, top=10, nms_iou=0.5,
                            gt=None, hit_iou=ops.HIT_IOU, radius=None, margin=None, min_len=1):
    """``ground_queries`` with the sliding-window generator in place of the threshold one - the zero-shot CLIP baseline of the MAD benchmark: text
    [B, d] or [B, Q, d], video [B, L, d], mask [B, L], gt [..., 2] rows of (start, end) or None -> ``Grounding(spans, scores, n_keep, proposals,
    rank)`` with ``proposals`` the ``ops.SpanAnchors`` (windows and scale indices included).  Three device stages: the cosine rows
    (``ops.frame_cosine[_multi]``), ``ops.span_anchors`` on them (``scales``, ``score``, ``peak``, ``min_usable``, ``valid``, ``max_spans``) - the
    proposal and the score stage in one: a window's score IS what ranks it - and ``ops.span_rank`` (``top``, ``nms_iou``, ``gt``, ``hit_iou``),
    whose NMS is what suppresses across scales.  ``valid`` has the mask's shape (a row per video) or ``text``'s leading shape and L (a row per
    query).  With ``radius`` and ``margin`` (both or neither) the kept spans' bounds are refined behind the ranking by the stage of
    ``ground_queries_refined`` (``ops.span_refine`` with ``radius``, ``margin``, ``min_len``, then ``ops.span_scores_masked``' top-3 scores of the
    refined spans with NaN cosines skipped) and the result is ``RefinedGrounding(grounding, refined, scores)``.  A fixed number of launches whatever
    Q; no synchronisation and no device -> host copy when the inputs live on the device; host tensors are staged and every result comes back on the
    device ``video`` lives on."""
    who = "ground_queries_anchored"
    ops.span_anchors_keywords(who, scales, score, peak, min_usable, max_spans)
    if (radius is None) != (margin is None):
        raise ValueError(f"{who}: radius={radius!r} and margin={margin!r} must be given together (refine the kept spans) or not at all")
    refine = None
    if radius is not None:
        ops.span_refine_keywords(who, radius, margin, min_len)
        refine = _refine_kept(radius, margin, min_len, "cxw", True, 3, "topk", 0.01)
    elif not (isinstance(min_len, int) and not isinstance(min_len, bool) and min_len >= 1):
        raise ValueError(f"{who}: min_len={min_len!r} must be a positive integer")

    def anchors(sims, m, v):
        return ops.span_anchors(sims, m, scales=scales, score=score, peak=peak, min_usable=min_usable, valid=v, max_spans=max_spans, return_windows=True,
                                return_scale=True)
    out = _ground(who, text, video, mask, valid, False, top, nms_iou, 3, "topk", 0.01, gt, hit_iou, {}, refine=refine, anchors=anchors)
    return RefinedGrounding(*out) if refine is not None else out


def windows_valid(select, mask, *, rule, win, stride=None, frames="all", num_frames=None, valid=None, return_count=False):
    """``ops.windows_valid`` with the device handling of ``propose_spans_masked``: select i32 [R, keep] or [B, Q, keep] (``select_windows_frames``'
    ``select``, or window indices from anywhere), mask [R, L] / [B, L], the keywords of that function -> ``ops.WindowsValid(valid, n_valid)``: f32
    [..., L] rows that are 1 at the frames the named windows cover - the ``valid`` of ``ops.span_scores_masked_rows`` /
    ``ops.span_propose_masked_rows``.  One launch, no synchronisation and no device -> host copy when the inputs live on the device; host tensors are
    staged and the results come back on the device ``select`` lives on."""
    who = "windows_valid"
    ops.windows_valid_checks(who, select, mask, rule, win, stride, frames, num_frames, valid, return_count)
    home = select.device
    dev = _device_of(select, who)
    out = ops.windows_valid(ops.h2d(select, dev), ops.h2d(mask, dev), rule=rule, win=win, stride=stride, frames=frames, num_frames=num_frames,
                            valid=None if valid is None else ops.h2d(valid, dev), return_count=return_count)
    return ops.WindowsValid(*(None if t is None else t.to(home) for t in out))


WindowedGrounding = collections.namedtuple("WindowedGrounding", "grounding selection valid n_valid")


def ground_queries_in_windows(text, video, mask, *, rule, win, stride=None, select=None, keep=None, frames="all", num_frames=None, select_k=3, min_sep=1,
                              valid=None, skip_nan=False, top=10, nms_iou=0.5, k=3, pooling="topk", temperature=0.01, gt=None, hit_iou=ops.HIT_IOU,
                              **propose_keywords):
    """Coarse to fine: ground every query only inside the windows chosen for it.  text [B, d] or [B, Q, d], video [B, L, d], mask [B, L], the inputs
    and keywords of ``ground_queries_masked`` -> ``WindowedGrounding(grounding, selection, valid, n_valid)``: the ``Grounding``, the
    ``ops.FrameWindowSelection`` the windows came from (None when ``select`` was given), the f32 [..., L] validity rows the fine half ran under and
    their i32 [...] counts of usable frames.  Exactly one of ``select`` and ``keep`` is given: ``select`` i32 [..., n] names each query's windows
    (the LLM's answers, a retrieval log; -1 and indices outside the row's windows name nothing); ``keep`` chooses them here with
    ``ops.window_select_frames`` (``rule``, ``win``, ``stride``, ``frames``, ``num_frames``, ``valid``, ``k=select_k``, ``min_sep``; ``gt`` - (start, end)
    as fractions of the duration, as the ranking takes it - times the mask's row sum as its frames).  The cosine rows are computed once and feed both
    halves: ``ops.frame_cosine[_multi]``, (``ops.window_select_frames``,) ``ops.windows_valid`` under the caller's ``valid``,
    ``ops.span_propose_masked_rows``, ``ops.span_scores_masked_rows``, ``ops.span_rank`` and the gather of the kept spans - a fixed number of launches
    whatever Q, no synchronisation and no device -> host copy when the inputs live on the device."""
    who = "ground_queries_in_windows"
    if (select is None) == (keep is None):
        raise ValueError(f"{who}: exactly one of select (the windows to search) and keep (how many to choose here) must be given")
    kw = ops.window_select_frames_keywords(who, rule, win, stride, 1 if keep is None else keep, frames, num_frames, select_k, min_sep)
    stride = kw[2]
    if select is not None:
        if not torch.is_tensor(select) or not torch.is_tensor(text) or select.dtype != torch.int32 or select.dim() != text.dim() \
                or select.shape[:-1] != text.shape[:-1] or not 1 <= select.shape[-1] <= ops.WINDOWS_VALID_MAX_KEEP:
            raise ValueError(f"{who}: select must be an int32 tensor [..., n] over text's leading shape with 1 <= n <= {ops.WINDOWS_VALID_MAX_KEEP} "
                             f"(got {tuple(select.shape) if torch.is_tensor(select) else type(select).__name__})")
    if torch.is_tensor(video) and video.dim() == 3 and video.shape[1] >= 1:
        if keep is not None:
            ops.window_select_capacity(who, video.shape[1], kw[1], stride, kw[7])
        elif kw[1] > video.shape[1]:
            raise ValueError(f"{who}: win={kw[1]} frames for rows of L={video.shape[1]}")

    def windows(sims, m, v, gt_dev):
        selection = None
        if keep is not None:
            gt_frames = None if gt_dev is None else gt_dev * m.sum(-1).view((-1,) + (1,) * (gt_dev.dim() - 1))
            selection = ops.window_select_frames(sims, m, rule=rule, win=win, stride=stride, keep=keep, frames=frames, num_frames=num_frames, valid=v,
                                                 k=select_k, min_sep=min_sep, gt=gt_frames)
        chosen = selection.select if selection is not None else ops.h2d(select, sims.device)
        return selection, ops.windows_valid(chosen, m, rule=rule, win=win, stride=stride, frames=frames, num_frames=num_frames, valid=v, return_count=True)
    grounding, selection, rows_valid = _ground(who, text, video, mask, valid, skip_nan, top, nms_iou, k, pooling, temperature, gt, hit_iou, propose_keywords,
                                               masked=True, windows=windows)
    return WindowedGrounding(grounding, selection, rows_valid.valid, rows_valid.n_valid)


def select_windows(text, video, mask, *, win, stride, keep, k=3, min_sep=1, gt=None, return_scores=False, return_bounds=False, return_order=False):
    """Choose the stage-2 recursion's windows from the CLIP features alone: text [B, d] or [B, Q, d], video [B, L, d], mask [B, L], gt [..., 2] rows of
    (start, end) in frames or None -> ``ops.WindowSelection(select, n_select, n_windows, scores, bounds, order, hit_rank)``.  Two device stages: the
    cosine rows (``ops.frame_cosine[_multi]``) and ``ops.window_select`` on them with the same keywords (``rv_window_select``: the windows of
    ``stage2.cut_windows`` for ``clip_length = win``, each scored by its ``k`` largest cosines, taken in rank order at least ``min_sep`` indices apart,
    topped up in rank order, the first ``keep`` handed back ascending - the form of ``run_query(grounding_windows=)``).  ``hit_rank`` feeds
    ``eval.metrics.window_recall``.  No synchronisation and no device -> host copy when the inputs live on the device; host tensors are staged and
    every result comes back on the device ``video`` lives on."""
    return _select_windows("select_windows", lambda sims, m, **kw: ops.window_select(sims, m, stride=stride, **kw), text, video, mask, win, stride, keep, k,
                           min_sep, gt, return_scores, return_bounds, return_order)


def select_windows_clipped(text, video, mask, *, win, keep, k=3, min_sep=1, gt=None, return_scores=False, return_bounds=False, return_order=False):
    """``select_windows`` for the stage-1 driver's windows: the same inputs, checks and ``ops.WindowSelection``, with ``ops.window_select_clipped``
    (``rvx_window_select_clipped``) behind the cosine rows - the half-overlapping windows of ``stage1.cut_windows`` for ``clip_length = win``, the void
    ones left out; ``select`` is what ``ops.window_gather_clipped(select=)`` takes.  No synchronisation and no device -> host copy when the inputs
    live on the device."""
    return _select_windows("select_windows_clipped", ops.window_select_clipped, text, video, mask, win, 2, keep, k, min_sep, gt, return_scores, return_bounds,
                           return_order)


def select_windows_frames(text, video, mask, *, rule, win, stride=None, keep, frames="all", num_frames=None, valid=None, k=3, min_sep=1, gt=None,
                          return_scores=False, return_bounds=False, return_order=False):
    """``select_windows`` (``rule="shifted"``) / ``select_windows_clipped`` (``rule="clipped"``) with ``ops.window_select_frames`` behind the cosine
    rows: the same inputs and checks, the keywords of that function - a window is scored on ``frames="all"`` of its frames or on the ``num_frames``
    ``"sampled"`` ones the gather hands to the LLM, and on the frames ``valid`` [B, L] does not hide - and its ``ops.FrameWindowSelection`` (the
    fields of ``ops.WindowSelection`` and ``n_candidates``).  No synchronisation and no device -> host copy when the inputs live on the device."""
    who = "select_windows_frames"
    ops.window_select_frames_keywords(who, rule, win, stride, keep, frames, num_frames, k, min_sep)
    ops.window_select_valid(who, valid, mask)
    stride = 2 if rule == "clipped" else stride

    def call(sims, m, **kw):
        v = None if valid is None else ops.h2d(valid, sims.device)
        return ops.window_select_frames(sims, m, rule=rule, stride=stride, frames=frames, num_frames=num_frames, valid=v, **kw)
    return _select_windows(who, call, text, video, mask, win, stride, keep, k, min_sep, gt, return_scores, return_bounds, return_order,
                           result=ops.FrameWindowSelection)


def _select_windows(who, call, text, video, mask, win, stride, keep, k, min_sep, gt, return_scores, return_bounds, return_order, result=None):
    """``select_windows`` (``call``: ``ops.window_select`` at its stride), ``select_windows_clipped`` (``ops.window_select_clipped``, stride 2) and
    ``select_windows_frames`` (``ops.window_select_frames``, ``result`` its namedtuple): one body."""
    for name, t in (("text", text), ("video", video), ("mask", mask)):
        if not torch.is_tensor(t):
            raise ValueError(f"{who}: {name} must be a tensor (got {type(t).__name__})")
    multi = text.dim() == 3
    if video.dim() != 3 or text.dim() not in (2, 3) or text.shape[0] != video.shape[0] or text.shape[-1] != video.shape[2] or min(text.shape) == 0:
        raise ValueError(f"{who}: text {tuple(text.shape)} / video {tuple(video.shape)} (expected [B, d] or [B, Q, d] and [B, L, d])")
    if mask.shape != video.shape[:2]:
        raise ValueError(f"{who}: mask {tuple(mask.shape)} for video {tuple(video.shape)} (expected [B, L])")
    if min(video.shape) == 0:
        raise ValueError(f"{who}: empty video {tuple(video.shape)}")
    for name, t in (("text", text), ("video", video)):
        if not t.dtype.is_floating_point:
            raise ValueError(f"{who}: {name} must be a floating-point tensor (got {t.dtype})")
    if mask.dtype.is_complex:
        raise ValueError(f"{who}: mask must be bool, integer or floating point (got {mask.dtype})")
    if video.shape[1] > ops.SPAN_PROPOSE_MAX_FRAMES:
        raise ValueError(f"{who}: L={video.shape[1]} frames (at most {ops.SPAN_PROPOSE_MAX_FRAMES})")
    kw = ops.window_select_keywords(who, win, stride, keep, k, min_sep)
    ops.window_select_capacity(who, video.shape[1], kw[0], kw[1], kw[4])
    ops.window_select_gt(who, gt, tuple(text.shape[:-1]))
    home = video.device
    dev = _device_of(video, who)
    sims = (ops.frame_cosine_multi if multi else ops.frame_cosine)(ops.h2d(text, dev).float(), _features_up(video, dev))
    out = call(sims, ops.h2d(mask, dev), win=win, keep=keep, k=k, min_sep=min_sep, gt=None if gt is None else ops.h2d(gt, dev).float(),
               return_scores=return_scores, return_bounds=return_bounds, return_order=return_order)
    return (result or ops.WindowSelection)(*(None if t is None else t.to(home) for t in out))


def _get_predicted_proposal_feat(src_vid_appear, src_vid_appear_mask, pred_proposal, text_cls_features):
    """similarity.py:44-69 with the reference's argument order.  ``text_cls_features`` are the unit-norm rows ``forward_clip_matching`` hands over
    there; the cosine kernel normalises them (again), so rows of another length give the same scores as their unit-norm versions."""
    return _match("_get_predicted_proposal_feat", text_cls_features, src_vid_appear, src_vid_appear_mask, pred_proposal, 3, "topk", 0.01, False)
