"""The CLIP grounding chain's wrappers (cosine rows, span scores, ranking, span proposals, window selection, window gather under both window rules, the proposals' cosine scores, the two
poolings) with their checkers, constants and namedtuples; ``ops`` re-exports every public name.  Every function takes / returns torch DEVICE tensors and enqueues on torch's current stream."""
import collections
import collections.abc
import math
import numbers
import struct
import types

import torch

from . import hip


def _score_lib(t):
    return hip.lib(None if t.dtype == torch.float32 else t)


def topk_pool(text_embeds, video_embeds, k, return_index=False):
    """``_topk_pooling`` (similarity.py:71-94) on the device: text [Nt,d], video [Nv,T,d] (bf16 or f32) -> f32 [Nv,Nt,d], the SUM
    of each video's k frames most similar to each text."""
    Nv, T, d = video_embeds.shape
    Nt = text_embeds.shape[0]
    out = torch.empty(Nv, Nt, d, dtype=torch.float32, device=video_embeds.device)
    idx = torch.empty(Nv, Nt, k, dtype=torch.int32, device=video_embeds.device) if return_index else None
    hip.check(_score_lib(video_embeds).rv_topk_pool(hip.ptr(video_embeds.contiguous()), hip.dtype_code(video_embeds), hip.ptr(text_embeds.float().contiguous()), Nv, T, d,
                                                    Nt, int(k), hip.ptr(out), hip.ptr(idx), hip.stream()), "rv_topk_pool")
    return (out, idx) if return_index else out


def frame_cosine(text, video):
    """The per-frame cosine row of ``forward_clip_matching`` (similarity.py:36, :61-64): text f32 [B,d], video [B,L,d] (16-bit operands or f32) -> f32 [B,L],
    ``<f_l, t_b> / (|f_l| |t_b|)``; a zero frame or a zero text gives NaN as the reference's divisions do."""
    if video.dim() != 3 or text.dim() != 2 or text.shape != (video.shape[0], video.shape[2]):
        raise ValueError(f"frame_cosine: text {tuple(text.shape)} / video {tuple(video.shape)}")
    B, L, d = video.shape
    out = torch.empty(B, L, dtype=torch.float32, device=video.device)
    hip.check(_score_lib(video).rv_frame_cosine(hip.ptr(video.contiguous()), hip.dtype_code(video), hip.ptr(text.float().contiguous()), B, L, d, hip.ptr(out), hip.stream()),
              "rv_frame_cosine")
    return out


SPAN_POOLINGS = {"topk": 0, "attention": 1}


def _span_scores(who, sims, spans, mask, k, pooling, temperature, return_windows):
    """``span_scores`` (rows [B]) and ``span_scores_multi`` (rows [B,Q], one mask row per video): one body, the entry point named by ``who``."""
    nd = 3 if who == "span_scores_multi" else 2
    if pooling not in SPAN_POOLINGS:
        raise ValueError(f"{who}: pooling={pooling!r} (expected one of {sorted(SPAN_POOLINGS)})")
    if (sims.dim() != nd or spans.dim() != nd + 1 or spans.shape[:-2] != sims.shape[:-1] or spans.shape[-1] != 2
            or mask.shape != (sims.shape[0], sims.shape[-1])):
        raise ValueError(f"{who}: sims {tuple(sims.shape)} / spans {tuple(spans.shape)} / mask {tuple(mask.shape)}")
    if sims.dtype != torch.float32:
        raise ValueError(f"{who}: sims must be float32 (got {sims.dtype})")
    lead, L, N = tuple(sims.shape[:-1]), sims.shape[-1], spans.shape[-2]
    scores = torch.empty(lead + (N,), dtype=torch.float32, device=sims.device)
    win = torch.empty(lead + (N, 2), dtype=torch.int32, device=sims.device) if return_windows else None
    if N > 0:
        hip.check(getattr(hip.lib(), "rv_" + who)(hip.ptr(sims.contiguous()), hip.ptr(spans.float().contiguous()), hip.ptr(mask.float().contiguous()), *lead, L, N,
                                                  SPAN_POOLINGS[pooling], int(k), float(temperature), hip.ptr(scores), hip.ptr(win), hip.stream()),
                  "rv_" + who)
    return (scores, win) if return_windows else scores


def span_scores(sims, spans, mask, k=3, pooling="topk", temperature=0.01, return_windows=False):
    """sims f32 [B,L], spans [B,N,2] as (centre, width), mask [B,L] -> scores f32 [B,N] (and the windows i32 [B,N,2] as (lo, hi) of ``range(L)[start:end]``):
    the reference's window rule (similarity.py:52-60) and, per window, the sum of its min(k, len) largest sims (``pooling="topk"``) or
    ``sum softmax(s / temperature) s`` (``"attention"``).  Nothing comes back to the host."""
    return _span_scores("span_scores", sims, spans, mask, k, pooling, temperature, return_windows)


def frame_cosine_multi(text, video):
    """``frame_cosine`` for Q texts per video: text f32 [B,Q,d], video [B,L,d] (16-bit operands or f32, passed as it is when contiguous) -> f32 [B,Q,L],
    ``<f_bl, t_bq> / (|f_bl| |t_bq|)`` with the features read once for all Q texts (``rv_frame_cosine_multi``: f32-input MFMA).  A query's row does not
    depend on Q, on its slot or on the other texts.  A zero text gives a NaN row, a zero frame a NaN column.  No synchronisation."""
    if video.dim() != 3 or text.dim() != 3 or text.shape[0] != video.shape[0] or text.shape[2] != video.shape[2]:
        raise ValueError(f"frame_cosine_multi: text {tuple(text.shape)} / video {tuple(video.shape)} (expected [B, Q, d] and [B, L, d])")
    B, L, d = video.shape
    Q = text.shape[1]
    text = text.float().contiguous()
    unit = torch.empty_like(text)                       # the kernel's workspace: text / |text|
    out = torch.empty(B, Q, L, dtype=torch.float32, device=video.device)
    hip.check(_score_lib(video).rv_frame_cosine_multi(hip.ptr(video.contiguous()), hip.dtype_code(video), hip.ptr(text), B, Q, L, d, hip.ptr(unit), hip.ptr(out),
                                                      hip.stream()), "rv_frame_cosine_multi")
    return out


def span_scores_multi(sims, spans, mask, k=3, pooling="topk", temperature=0.01, return_windows=False):
    """``span_scores`` for Q queries per video: sims f32 [B,Q,L], spans [B,Q,N,2] (each query's own (centre, width) proposals), mask [B,L] (one duration
    per video) -> scores f32 [B,Q,N] (and the windows i32 [B,Q,N,2]).  The kernel of ``span_scores``: each (b, q) row equals ``span_scores`` on that
    row bit for bit.  No synchronisation."""
    return _span_scores("span_scores_multi", sims, spans, mask, k, pooling, temperature, return_windows)


SPAN_FORMS = {"xx": 0, "cxw": 1}
SPAN_RANK_MAX = 2048
HIT_IOU = (0.1, 0.3, 0.5, 0.7, 0.9)
SpanRank = collections.namedtuple("SpanRank", "keep n_keep keep_iou first_hit order")
_hit_tables = collections.OrderedDict()
_HIT_TABLES_MAX = 16


def _hit_table(hit_iou, device):
    """The thresholds as an f32 device vector, uploaded once per (values, device, stream) and kept for the last 16 such keys: a ranking call then queues no
    copy.  The stream is part of the key because the upload is ordered on the stream that was current when it was queued: a call on another stream gets a
    table of its own, uploaded on that stream, instead of reading this one without ordering."""
    key = (hit_iou, str(device), torch.cuda.current_stream(device).cuda_stream)
    table = _hit_tables.get(key)
    if table is None:
        from .ops import h2d                   # (ops imports this module: at call time both are complete)
        table = _hit_tables[key] = h2d(torch.tensor(hit_iou, dtype=torch.float32), device)
        while len(_hit_tables) > _HIT_TABLES_MAX:
            _hit_tables.popitem(last=False)        # (the allocator keeps a freed block ordered behind the work queued on its stream)
    else:
        _hit_tables.move_to_end(key)
    return table


def span_rank_keywords(who, top, nms_iou, hit_iou):
    """The keyword refusals of ``span_rank`` (raised before any device is looked for) -> (nms_iou as float, hit_iou as a tuple of floats)."""
    if top is not None and not (isinstance(top, numbers.Integral) and not isinstance(top, bool) and top >= 1):
        raise ValueError(f"{who}: top={top!r} must be a positive integer or None")
    try:
        nms_iou, hit_iou = float(nms_iou), tuple(float(h) for h in hit_iou)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: nms_iou={nms_iou!r} must be a number and hit_iou={hit_iou!r} a sequence of numbers") from None
    if not (math.isfinite(nms_iou) and nms_iou >= 0.0):
        raise ValueError(f"{who}: nms_iou={nms_iou} must be finite and >= 0")
    if len(hit_iou) > 16:
        raise ValueError(f"{who}: {len(hit_iou)} thresholds in hit_iou (at most 16)")
    return nms_iou, hit_iou


def span_rank(scores, spans, top=None, nms_iou=1.0, form="cxw", gt=None, hit_iou=HIT_IOU, return_order=False):
    """Rank scored proposals on the device (``rv_span_rank``): scores [R,N] or [B,Q,N], spans [...,N,2] as (centre, width) (``form="cxw"``) or (start, end)
    (``"xx"``), gt [...,2] as (start, end) or None -> SpanRank(keep i32 [...,top], n_keep i32 [...], keep_iou f32 [...,top], first_hit i32 [...,T], order
    i32 [...,N]); parts not asked for are None (keep_iou and first_hit need ``gt``, order ``return_order``).  Descending score, ties to the smaller index,
    NaN last; greedy NMS at ``inter > nms_iou * union`` (1.0: none); ``keep`` is padded with -1, ``keep_iou`` with 0; ``first_hit[..., t]`` is the first
    kept place whose IoU with gt exceeds ``hit_iou[t]``, or -1.  ``top=None`` means N, a larger ``top`` is N.  One launch, no synchronisation, no host copy."""
    if form not in SPAN_FORMS:
        raise ValueError(f"span_rank: form={form!r} (expected one of {sorted(SPAN_FORMS)})")
    if not torch.is_tensor(scores) or not torch.is_tensor(spans) or (gt is not None and not torch.is_tensor(gt)):
        raise ValueError("span_rank: scores, spans and gt must be tensors")
    if scores.dim() not in (2, 3) or spans.shape != scores.shape + (2,):
        raise ValueError(f"span_rank: scores {tuple(scores.shape)} / spans {tuple(spans.shape)} (expected [R, N] or [B, Q, N] and [..., N, 2])")
    if gt is not None and gt.shape != scores.shape[:-1] + (2,):
        raise ValueError(f"span_rank: gt {tuple(gt.shape)} for scores {tuple(scores.shape)} (expected [..., 2] rows of (start, end))")
    if scores.dtype != torch.float32:
        raise ValueError(f"span_rank: scores must be float32 (got {scores.dtype})")
    for name, t in (("spans", spans), ("gt", gt)):
        if t is not None and not t.dtype.is_floating_point:
            raise ValueError(f"span_rank: {name} must be a floating-point tensor (got {t.dtype})")
    lead, N = tuple(scores.shape[:-1]), scores.shape[-1]
    if N > SPAN_RANK_MAX:
        raise ValueError(f"span_rank: N={N} proposals per row (at most {SPAN_RANK_MAX})")
    nms_iou, hit_iou = span_rank_keywords("span_rank", top, nms_iou, hit_iou if gt is not None else ())
    top = N if top is None else min(int(top), N)
    T, dev = len(hit_iou), scores.device
    R = math.prod(lead)
    keep = torch.empty(lead + (top,), dtype=torch.int32, device=dev)
    n_keep = torch.empty(lead, dtype=torch.int32, device=dev)
    keep_iou = torch.empty(lead + (top,), dtype=torch.float32, device=dev) if gt is not None else None
    first_hit = torch.empty(lead + (T,), dtype=torch.int32, device=dev) if gt is not None else None
    order = torch.empty(lead + (N,), dtype=torch.int32, device=dev) if return_order else None
    if N > 0 and R > 0:
        hip.check(hip.lib().rv_span_rank(hip.ptr(scores.contiguous()), hip.ptr(spans.float().contiguous()), SPAN_FORMS[form], R, N, top, nms_iou,
                                         hip.ptr(gt.float().contiguous()) if gt is not None else None, hip.ptr(_hit_table(hit_iou, dev)) if T else None, T,
                                         hip.ptr(order), hip.ptr(keep), hip.ptr(n_keep), hip.ptr(keep_iou), hip.ptr(first_hit if T else None), hip.stream()),
                  "rv_span_rank")
    elif R > 0:                                          # no proposals: nothing kept, no hit (no launch)
        n_keep.zero_()
        if first_hit is not None:
            first_hit.fill_(-1)
    return SpanRank(keep, n_keep, keep_iou, first_hit, order)


SPAN_PROPOSE_MAX_LEVELS = 8
SPAN_PROPOSE_MAX_FRAMES = 1 << 20
SPAN_PROPOSE_LEVELS = (0.5, 0.6, 0.7, 0.8, 0.9)
SpanProposals = collections.namedtuple("SpanProposals", "spans n_spans n_found windows smoothed")


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _f32(v):
    """A Python float rounded to float32 (inf when it is out of range)."""
    try:
        return struct.unpack("f", struct.pack("f", v))[0]
    except OverflowError:
        return math.copysign(math.inf, v)


def _flag(who, name, v):
    """The refusal of an on / off keyword -> 0 / 1."""
    if not (isinstance(v, (bool, numbers.Integral)) and v in (0, 1)):
        raise ValueError(f"{who}: {name}={v!r} must be True or False")
    return int(bool(v))


def _rows_f32(*tensors):
    """The f32-contiguous form of each tensor (None stays None), what the kernels read.  The caller keeps what comes back referenced until its call is
    queued: two temporaries dropped one after the other would share one block of the allocator."""
    return tuple(None if t is None else t.float().contiguous() for t in tensors)


def _shape(t):
    return tuple(t.shape) if torch.is_tensor(t) else "?"


def _valid_rows(who, valid, like, expected):
    """The one check of a ``valid``: a bool, uint8 or floating-point tensor with the shape of one of the tensors ``like``; ``expected`` is how the caller's
    refusal describes them -> whether it has the shape of the first."""
    if not torch.is_tensor(valid) or not all(torch.is_tensor(t) for t in like) or all(valid.shape != t.shape for t in like):
        raise ValueError(f"{who}: valid {tuple(valid.shape) if torch.is_tensor(valid) else type(valid).__name__} (expected a tensor of {expected})")
    if not (valid.dtype in (torch.bool, torch.uint8) or valid.dtype.is_floating_point):
        raise ValueError(f"{who}: valid must be bool, uint8 or floating point (got {valid.dtype})")
    return valid.shape == like[0].shape


def _rows_per_valid(who, valid, mask, sims, rpm):
    """``span_refine``'s and ``span_anchors``' ``valid``: None, of the mask's shape (a row per mask row: rpm) or of ``sims``' shape (a row per row: 1) ->
    rows per validity row."""
    if valid is None or _valid_rows(who, valid, (mask, sims), f"mask's shape {tuple(mask.shape)}, a validity row per mask row, or of sims' shape "
                                                           f"{tuple(sims.shape)}, one per row"):
        return rpm
    return 1


def span_propose_keywords(who, levels=SPAN_PROPOSE_LEVELS, relative=True, smooth=1, gap=0, min_len=1, max_len=None, max_spans=256):
    """The keyword refusals of ``span_propose`` (raised before any device is looked for) -> (levels as a tuple of floats, relative as 0 / 1, smooth, gap,
    min_len, max_len with None as 0, max_spans) as ``rv_span_propose`` takes them."""
    try:
        levels = tuple(float(v) for v in levels)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: levels={levels!r} must be a sequence of numbers") from None
    if not 1 <= len(levels) <= SPAN_PROPOSE_MAX_LEVELS:
        raise ValueError(f"{who}: {len(levels)} levels (1 to {SPAN_PROPOSE_MAX_LEVELS})")
    _flag(who, "relative", relative)
    as_f32 = [_f32(v) for v in levels]                   # what the kernel compares
    for i, v in enumerate(as_f32):
        if not math.isfinite(v):
            raise ValueError(f"{who}: level {levels[i]} is not a finite float32")
        if i and not v > as_f32[i - 1]:
            raise ValueError(f"{who}: levels={levels} must be strictly ascending (as float32)")
        if relative and not 0.0 <= v < 1.0:
            raise ValueError(f"{who}: relative level {levels[i]} outside [0, 1)")
    if not (_is_int(smooth) and 1 <= smooth <= 65 and smooth % 2 == 1):
        raise ValueError(f"{who}: smooth={smooth!r} must be an odd integer in [1, 65]")
    if not (_is_int(gap) and 0 <= gap <= 63):
        raise ValueError(f"{who}: gap={gap!r} must be an integer in [0, 63]")
    if not (_is_int(min_len) and 1 <= min_len < 2 ** 31):
        raise ValueError(f"{who}: min_len={min_len!r} must be a positive integer")
    if max_len is not None and not (_is_int(max_len) and min_len <= max_len < 2 ** 31):
        raise ValueError(f"{who}: max_len={max_len!r} must be None or an integer >= min_len={min_len}")
    if not (_is_int(max_spans) and 1 <= max_spans <= SPAN_RANK_MAX):
        raise ValueError(f"{who}: max_spans={max_spans!r} must be an integer in [1, {SPAN_RANK_MAX}]")
    return tuple(as_f32), int(bool(relative)), int(smooth), int(gap), int(min_len), 0 if max_len is None else int(max_len), int(max_spans)


def span_propose_shapes(who, sims, mask):
    """The tensor refusals of ``span_propose`` -> (leading shape, R, rows per mask row, L)."""
    if not torch.is_tensor(sims) or not torch.is_tensor(mask):
        raise ValueError(f"{who}: sims and mask must be tensors")
    if sims.dim() not in (2, 3) or mask.dim() != 2 or mask.shape[-1] != sims.shape[-1]:
        raise ValueError(f"{who}: sims {tuple(sims.shape)} / mask {tuple(mask.shape)} (expected [R, L] or [B, Q, L] and [R, L] / [B, L])")
    lead, L = tuple(sims.shape[:-1]), sims.shape[-1]
    R, M = math.prod(lead), mask.shape[0]
    if min(R, L, M) < 1 or (sims.dim() == 3 and M != lead[0]) or R % M != 0:
        raise ValueError(f"{who}: sims {tuple(sims.shape)} / mask {tuple(mask.shape)} (one mask row per video: a whole number of rows of sims for each)")
    if L > SPAN_PROPOSE_MAX_FRAMES:
        raise ValueError(f"{who}: L={L} frames (at most {SPAN_PROPOSE_MAX_FRAMES})")
    if not sims.dtype.is_floating_point:
        raise ValueError(f"{who}: sims must be a floating-point tensor (got {sims.dtype})")
    if mask.dtype.is_complex:
        raise ValueError(f"{who}: mask must be bool, integer or floating point (got {mask.dtype})")
    return lead, R, R // M, L


def span_propose(sims, mask, *, levels=SPAN_PROPOSE_LEVELS, relative=True, smooth=1, gap=0, min_len=1, max_len=None, max_spans=256, return_windows=False,
                 return_smoothed=False):
    """Candidate spans from similarity rows on the device (``rv_span_propose``): sims f32 [R,L] or [B,Q,L] (``frame_cosine`` / ``frame_cosine_multi``'s
    rows), mask [R,L] / [B,L] of any bool, integer or float dtype (its row sum is the duration; with fewer rows than sims each serves a whole number of
    consecutive rows) -> SpanProposals(spans f32 [...,max_spans,2] as (centre, width) with NaN padding, n_spans i32 [...], n_found i32 [...], windows i32
    [...,max_spans,2] with (-1, -1) padding, smoothed f32 [...,L]); ``windows`` and ``smoothed`` are None unless asked for, and ``smoothed`` is written
    inside each row's duration only (NaN elsewhere).  The row is box-smoothed over ``smooth`` frames and thresholded at every level (``relative``: a
    fraction of the way from the row's smallest to its largest value); a maximal stretch above a threshold, gaps of at most ``gap`` frames closed, is a
    span if its length lies in [min_len, max_len] and the next level has no identical one.  Highest level first, then ascending start;
    ``n_found > n_spans`` shows that ``max_spans`` cut the list.  One launch (a mask that is not f32 adds a cast kernel, ``return_smoothed`` a fill), no
    synchronisation, no host copy.  The full rule stands in include/revision_hip.h."""
    return _span_propose("span_propose", sims, mask, "none", None, False, (levels, relative, smooth, gap, min_len, max_len, max_spans), return_windows,
                         return_smoothed)


def _span_propose(who, sims, mask, validity, valid, skip_nan, keywords, return_windows, return_smoothed):
    """One body for ``span_propose`` (``validity`` "none": ``rv_span_propose``), ``span_propose_masked`` ("mask": ``valid`` is None or has the mask's shape)
    and ``span_propose_masked_rows`` ("rows": ``valid`` has ``sims``' shape); each calls its own entry."""
    lv, relative, smooth, gap, min_len, max_len, N = span_propose_keywords(who, *keywords)
    if validity != "none":
        skip_nan = skip_nan_flag(who, skip_nan)
    lead, R, rpm, L = span_propose_shapes(who, sims, mask)
    if validity == "rows":
        span_rows_valid(who, valid, sims)
    elif validity == "mask":
        window_select_valid(who, valid, mask)
    if sims.dtype != torch.float32:
        raise ValueError(f"{who}: sims must be float32 (got {sims.dtype})")
    dev = sims.device
    spans = torch.empty(lead + (N, 2), dtype=torch.float32, device=dev)
    n_spans = torch.empty(lead, dtype=torch.int32, device=dev)
    n_found = torch.empty(lead, dtype=torch.int32, device=dev)
    windows = torch.empty(lead + (N, 2), dtype=torch.int32, device=dev) if return_windows else None
    smoothed = torch.full(lead + (L,), float("nan"), dtype=torch.float32, device=dev) if return_smoothed else None
    table = (hip.C.c_float * len(lv))(*lv)
    sims, mask, valid = _rows_f32(sims, mask, valid)
    rule = (R, rpm, L, table, len(lv), relative, smooth, gap, min_len, max_len, N)
    outs = (hip.ptr(spans), hip.ptr(n_spans), hip.ptr(n_found), hip.ptr(windows), hip.ptr(smoothed), hip.stream())
    if validity == "none":
        hip.check(hip.lib().rv_span_propose(hip.ptr(sims), hip.ptr(mask), *rule, *outs), "rv_span_propose")
    elif validity == "rows":
        hip.chain_check(hip.chain_lib().rvc_span_propose_masked_rows(hip.ptr(sims), hip.ptr(mask), hip.ptr(valid), 1, *rule, skip_nan, *outs),
                        "rvc_span_propose_masked_rows")
    else:
        hip.chain_check(hip.chain_lib().rvc_span_propose_masked(hip.ptr(sims), hip.ptr(mask), hip.ptr(valid), *rule, skip_nan, *outs), "rvc_span_propose_masked")
    return SpanProposals(spans, n_spans, n_found, windows, smoothed)


WINDOW_SELECT_MAX = 2048
WindowSelection = collections.namedtuple("WindowSelection", "select n_select n_windows scores bounds order hit_rank")


def window_select_keywords(who, win, stride, keep, k=3, min_sep=1):
    """The keyword refusals of ``window_select`` that need no tensor (raised before any device is looked for) -> the five as ints."""
    for name, v in (("win", win), ("stride", stride), ("keep", keep), ("k", k), ("min_sep", min_sep)):
        if not (_is_int(v) and 1 <= v < 2 ** 31):
            raise ValueError(f"{who}: {name}={v!r} must be a positive integer")
    if win < stride:
        raise ValueError(f"{who}: win={win} frames with stride={stride} (stride <= win)")
    if k > 64:
        raise ValueError(f"{who}: k={k} must be in [1, 64]")
    return int(win), int(stride), int(keep), int(k), int(min_sep)


def window_select_capacity(who, L, win, stride, min_sep=1):
    """Wcap = max(1, ceil(L / (win // stride)) - 1), the most windows a row of L frames can have; refuses win > L, more than 2048 windows and
    min_sep > Wcap."""
    if win > L:
        raise ValueError(f"{who}: win={win} frames for rows of L={L}")
    hop = win // stride
    cap = max(1, -(-L // hop) - 1)
    if cap > WINDOW_SELECT_MAX:
        raise ValueError(f"{who}: L={L}, win={win}, stride={stride} give up to {cap} windows (at most {WINDOW_SELECT_MAX})")
    if min_sep > cap:
        raise ValueError(f"{who}: min_sep={min_sep} must be in [1, {cap}] (the most windows a row of L={L} can have)")
    return cap


def window_select_gt(who, gt, lead):
    if gt is None:
        return
    if not torch.is_tensor(gt) or gt.shape != lead + (2,):
        raise ValueError(f"{who}: gt {tuple(gt.shape) if torch.is_tensor(gt) else type(gt).__name__} (expected {lead + (2,)}: rows of (start, end) in frames)")
    if not gt.dtype.is_floating_point:
        raise ValueError(f"{who}: gt must be a floating-point tensor (got {gt.dtype})")


def window_select(sims, mask, *, win, stride, keep, k=3, min_sep=1, gt=None, return_scores=False, return_bounds=False, return_order=False):
    """Choose the recursion's windows from similarity rows on the device (``rv_window_select``): sims f32 [R,L] or [B,Q,L] (``frame_cosine`` /
    ``frame_cosine_multi``'s rows), mask [R,L] / [B,L] of any bool, integer or float dtype (its row sum is the duration; with fewer rows than sims each
    serves a whole number of consecutive rows), gt [...,2] rows of (start, end) in frames or None -> WindowSelection(select i32 [...,keep] ascending
    with -1 padding, n_select i32 [...], n_windows i32 [...], scores f32 [...,Wcap] with NaN padding, bounds i32 [mask rows,Wcap,2] as (lo, hi) with
    (-1, -1) padding, order i32 [...,Wcap] with -1 padding, hit_rank i32 [...]); ``scores``, ``bounds`` and ``order`` are None unless asked for,
    ``hit_rank`` unless ``gt`` is given.  The windows are ``stage2.cut_windows``' for ``clip_length = win``; a window's score is the sum of its ``k``
    largest sims; the windows are taken in rank order, a taken one removing the others within ``min_sep`` indices of it, then topped up in rank order;
    ``select`` is the first ``min(keep, n_windows)`` of that sequence sorted, ``hit_rank`` the first place of the sequence whose window overlaps gt.
    ``Wcap = max(1, ceil(L / (win // stride)) - 1)``; a ``keep`` above it is Wcap.  One launch (a mask that is not f32 adds a cast kernel), no
    synchronisation, no host copy.  The full rule stands in include/revision_hip.h."""
    who = "window_select"
    win, stride, keep, k, min_sep = window_select_keywords(who, win, stride, keep, k, min_sep)
    return _window_select(who, sims, mask, gt, None, win, stride, keep, min_sep, return_scores, return_bounds, return_order, lambda p: hip.check(
        hip.lib().rv_window_select(p.sims, p.mask, p.R, p.rpm, p.L, win, stride, k, p.keep, min_sep, p.Wcap, p.gt, p.select, p.n_select, p.n_windows, p.scores,
                                   p.bounds, p.order, p.hit_rank, hip.stream()), "rv_window_select"))


def _window_select(who, sims, mask, gt, valid, win, stride, keep, min_sep, return_scores, return_bounds, return_order, launch, candidates=False):
    """``window_select``, ``window_select_clipped`` and ``window_select_frames``: the tensor refusals, the outputs and the f32 rows of all three; ``launch``
    calls the function's own entry with the pointers and sizes it is handed; ``candidates``: the selection has an ``n_candidates``."""
    lead, R, rpm, L = span_propose_shapes(who, sims, mask)
    Wcap = window_select_capacity(who, L, win, stride, min_sep)
    window_select_gt(who, gt, lead)
    window_select_valid(who, valid, mask)
    if sims.dtype != torch.float32:
        raise ValueError(f"{who}: sims must be float32 (got {sims.dtype})")
    keep = min(keep, Wcap)
    dev = sims.device
    select = torch.empty(lead + (keep,), dtype=torch.int32, device=dev)
    n_select = torch.empty(lead, dtype=torch.int32, device=dev)
    n_windows = torch.empty(lead, dtype=torch.int32, device=dev)
    n_candidates = torch.empty(lead, dtype=torch.int32, device=dev) if candidates else None
    scores = torch.empty(lead + (Wcap,), dtype=torch.float32, device=dev) if return_scores else None
    bounds = torch.empty((R // rpm, Wcap, 2), dtype=torch.int32, device=dev) if return_bounds else None
    order = torch.empty(lead + (Wcap,), dtype=torch.int32, device=dev) if return_order else None
    hit_rank = torch.empty(lead, dtype=torch.int32, device=dev) if gt is not None else None
    sims, mask, valid, gt = _rows_f32(sims, mask, valid, gt)
    launch(types.SimpleNamespace(sims=hip.ptr(sims), mask=hip.ptr(mask), valid=hip.ptr(valid), gt=hip.ptr(gt), R=R, rpm=rpm, L=L, keep=keep, Wcap=Wcap,
                                 select=hip.ptr(select), n_select=hip.ptr(n_select), n_windows=hip.ptr(n_windows), n_candidates=hip.ptr(n_candidates),
                                 scores=hip.ptr(scores), bounds=hip.ptr(bounds), order=hip.ptr(order), hit_rank=hip.ptr(hit_rank)))
    if candidates:
        return FrameWindowSelection(select, n_select, n_windows, scores, bounds, order, hit_rank, n_candidates)
    return WindowSelection(select, n_select, n_windows, scores, bounds, order, hit_rank)


WINDOW_GATHER_MAX_FRAMES = 1 << 16
_GATHER_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def window_gather_keywords(who, win, stride, num_frames):
    """The keyword refusals of ``window_gather`` that need no tensor (raised before any device is looked for) -> the three as ints."""
    for name, v in (("win", win), ("stride", stride), ("num_frames", num_frames)):
        if not (_is_int(v) and 1 <= v < 2 ** 31):
            raise ValueError(f"{who}: {name}={v!r} must be a positive integer")
    if win < stride:
        raise ValueError(f"{who}: win={win} frames with stride={stride} (stride <= win)")
    if num_frames > WINDOW_GATHER_MAX_FRAMES:
        raise ValueError(f"{who}: num_frames={num_frames} (at most {WINDOW_GATHER_MAX_FRAMES})")
    return int(win), int(stride), int(num_frames)


def window_gather_dtypes(who, video_dtype, out_dtype):
    """(the output dtype, the flavour of the library that runs the call): ``out_dtype=None`` is the video's dtype when that is 16-bit, else the default
    library's operand type.  Each library reads and writes f32 and its OWN 16-bit type, so a call that names both 16-bit types is refused."""
    if video_dtype not in _GATHER_DTYPES:
        raise ValueError(f"{who}: video must be float32, float16 or bfloat16 (got {video_dtype})")
    if out_dtype is None:
        out_dtype = video_dtype if video_dtype != torch.float32 else hip.op_dtype()
    if out_dtype not in _GATHER_DTYPES:
        raise ValueError(f"{who}: out_dtype must be float32, float16 or bfloat16 (got {out_dtype!r})")
    sixteen = {t for t in (video_dtype, out_dtype) if t != torch.float32}
    if len(sixteen) == 2:
        raise ValueError(f"{who}: {video_dtype} features cannot become {out_dtype}: the {hip.flavour_of(video_dtype)} library converts between float32 "
                         f"and its own 16-bit type only (no cross-type 16-bit conversion); pass float32 features, or out_dtype={video_dtype}")
    return out_dtype, hip.flavour_of(sixteen.pop() if sixteen else None)


def window_gather(video, select, *, win, stride, num_frames, mask=None, out_dtype=None, return_index=False):
    """The recursion's window tensor from features that live on the device (``rv_window_gather``): video [L,d] or [B,L,d] (f32 or 16-bit operands; a
    view with a frame stride above d is read in place), select i32 [keep], [R,keep] or [B,Q,keep] - ``window_select``'s ``select`` as it lies, -1
    padding included, or any other window indices - mask [L] / [B,L] or None (its row sum is the duration; None: every frame counts) -> frames
    [...,keep,num_frames,d] in ``out_dtype`` (None: the video's dtype when it is 16-bit, else the default library's operand type), and with
    ``return_index`` the sampled frame of every output row as well, i32 [...,keep,num_frames].  Window i is ``stage2.cut_windows``' for ``clip_length =
    win`` and its frames are that function's ``np.linspace(start, end, num_frames, dtype=int32)``, so with a full mask ``frames[..., n, :, :]`` is
    ``video[cut_windows(...)[1][select[..., n]]]`` cast to ``out_dtype``; an entry outside the row's windows (the -1 padding) gives zeros and index -1.
    With [B,L,d] features the R rows of ``select`` belong to the videos in consecutive groups of R / B.  One launch (a mask that is not f32 adds a cast
    kernel), no synchronisation, no host copy.  The full rule stands in include/revision_hip.h."""
    who = "window_gather"
    win, stride, F = window_gather_keywords(who, win, stride, num_frames)
    return _window_gather(who, video, select, mask, win, stride, F, out_dtype, return_index, None)


def _window_gather(who, video, select, mask, win, stride, F, out_dtype, return_index, rule):
    """``window_gather`` (``rule`` None: ``rv_window_gather``, a ``select`` is needed) and ``window_gather_clipped`` (``rule``: the window rule handed to
    ``rv_window_gather_rule``, where ``select=None`` means every window in order): one body."""
    every = rule is not None and select is None
    if not torch.is_tensor(video) or not (every or torch.is_tensor(select)) or (mask is not None and not torch.is_tensor(mask)):
        raise ValueError(f"{who}: video, select and mask must be tensors")
    bad_video = video.dim() not in (2, 3) or min(video.shape) == 0
    bad_select = not every and (not 1 <= select.dim() <= 3 or min(select.shape) == 0)
    if rule is None:
        if bad_video or bad_select:
            raise ValueError(f"{who}: video {tuple(video.shape)} / select {tuple(select.shape)} (expected [L, d] or [B, L, d] and [keep], [R, keep] or [B, Q, keep])")
    elif bad_video:
        raise ValueError(f"{who}: video {tuple(video.shape)} (expected [L, d] or [B, L, d])")
    elif bad_select:
        raise ValueError(f"{who}: select {tuple(select.shape)} (expected [keep], [R, keep] or [B, Q, keep])")
    M = video.shape[0] if video.dim() == 3 else 1
    L, d = video.shape[-2:]
    if every:
        lead, keep, R = tuple(video.shape[:-2]), clipped_window_count(L, win), M      # (win <= L below: at least one window, keep >= 1)
    else:
        if select.dtype != torch.int32:
            raise ValueError(f"{who}: select must be int32 (got {select.dtype})")
        lead, keep = tuple(select.shape[:-1]), select.shape[-1]
        R = math.prod(lead)
        if (select.dim() == 3 and (video.dim() != 3 or lead[0] != M)) or R % M != 0:
            raise ValueError(f"{who}: video {tuple(video.shape)} / select {tuple(select.shape)} (a whole number of rows of select for each video)")
    if mask is not None:
        if mask.shape != tuple(video.shape[:-1]):
            raise ValueError(f"{who}: mask {tuple(mask.shape)} for video {tuple(video.shape)} (expected {tuple(video.shape[:-1])})")
        if mask.dtype.is_complex:
            raise ValueError(f"{who}: mask must be bool, integer or floating point (got {mask.dtype})")
    if L > SPAN_PROPOSE_MAX_FRAMES:
        raise ValueError(f"{who}: L={L} frames (at most {SPAN_PROPOSE_MAX_FRAMES})")
    if win > L:
        raise ValueError(f"{who}: win={win} frames for rows of L={L}")
    out_dtype, flavour = window_gather_dtypes(who, video.dtype, out_dtype)
    if video.stride(-1) != 1 or video.stride(-2) < d or (video.dim() == 3 and M > 1 and video.stride(0) != L * video.stride(-2)):
        video = video.contiguous()
    dev = video.device
    frames = torch.empty(lead + (keep, F, d), dtype=out_dtype, device=dev)
    index = torch.empty(lead + (keep, F), dtype=torch.int32, device=dev) if return_index else None
    mask, = _rows_f32(mask)
    select = None if every else select.contiguous()
    args = (hip.ptr(video), hip.dtype_code(video), video.stride(-2), hip.ptr(mask), hip.ptr(select), R, R // M, L, d, win, stride, keep, F, hip.ptr(frames),
            hip.dtype_code(frames), hip.ptr(index))
    if rule is None:
        hip.check(hip.lib(flavour).rv_window_gather(*args, hip.stream()), "rv_window_gather")
    else:
        hip.check(hip.lib(flavour).rv_window_gather_rule(*args, rule, hip.stream()), "rv_window_gather_rule")
    return (frames, index) if return_index else frames


def clipped_window_count(L, win):
    """How many windows ``stage1.cut_windows`` makes of ``L`` frames for ``clip_length = win``: max(0, ceil(L / (win // 2)) - 1)."""
    return max(0, -(-L // (win // 2)) - 1)


def clipped_window_void(L, win):
    """Whether the last of those windows starts behind its end (``(i * win) // 2 > L - 1``: an odd ``win`` only, first at L = 15 for win = 5 and at
    L = 195625 for win = 625).  The host's ``np.linspace`` indexes past the array there; the device stores zeros."""
    W = clipped_window_count(L, win)
    return W > 0 and (W - 1) * win // 2 > L - 1


def window_gather_clipped(video, *, win, num_frames, select=None, mask=None, out_dtype=None, return_index=False):
    """The stage-1 driver's window tensor from features that live on the device (``rv_window_gather_rule`` with the clipped rule): video [L,d] or
    [B,L,d] (f32 or 16-bit operands; a view with a frame stride above d is read in place), select None - every window in order, nothing uploaded - or
    i32 [keep], [R,keep] or [B,Q,keep] as ``window_gather`` takes it, mask [L] / [B,L] or None -> frames [W,num_frames,d] / [B,W,num_frames,d] with
    ``W = clipped_window_count(L, win)`` (with ``select``: [...,keep,num_frames,d]) in ``out_dtype`` (None: as ``window_gather``), and with
    ``return_index`` the sampled frame of every output row as well.  Window i is ``stage1.cut_windows``' for ``clip_length = win``: frames
    ``np.linspace((i * win) // 2, min((i * win) // 2 + win, D - 1), num_frames, dtype=int32)``, half-overlapping, the last ones clipped and not shifted
    back, so with a full mask ``frames`` is ``video[cut_windows(L, ...)]`` cast to ``out_dtype``.  A window past a masked row's duration, an entry of
    ``select`` outside the row's windows and a void window (``clipped_window_void``) give zeros and index -1.  One launch (a mask that is not f32 adds a
    cast kernel), no synchronisation, no host copy.  The full rule stands in include/revision_hip.h."""
    who = "window_gather_clipped"
    win, _, F = window_gather_keywords(who, win, 2, num_frames)
    return _window_gather(who, video, select, mask, win, 2, F, out_dtype, return_index, hip.RV_WINDOWS_CLIPPED)


def clipped_window_solid(L, win):
    """How many of ``clipped_window_count(L, win)`` windows are not void (``(i * win) // 2 <= L - 1``): the void ones are a suffix, so these are the
    indices below the result - what ``window_select_clipped`` reports as ``n_windows``."""
    return min(clipped_window_count(L, win), (2 * L - 1) // win + 1) if L >= 1 else 0


def window_select_clipped(sims, mask, *, win, keep, k=3, min_sep=1, gt=None, return_scores=False, return_bounds=False, return_order=False):
    """Choose the stage-1 driver's windows from similarity rows on the device (``rvx_window_select_clipped`` of the companion library): the arguments
    and the WindowSelection of ``window_select``, under ``stage1.cut_windows``' rule for ``clip_length = win`` - half-overlapping windows
    ``[(i * win) // 2, min((i * win) // 2 + win, D - 1)]``, the last ones clipped and not shifted back, so an index means the same window as in
    ``window_gather_clipped``.  A void window (``clipped_window_void``) is no candidate: ``n_windows`` counts the others (``clipped_window_solid``),
    and a void index appears in neither ``select`` nor ``order``.  ``Wcap = max(1, ceil(L / (win // 2)) - 1)``; a ``keep`` above it is Wcap.  One
    launch (a mask that is not f32 adds a cast kernel), no synchronisation, no host copy.  The full rule stands in include/revision_hip_ext.h."""
    who = "window_select_clipped"
    win, _, keep, k, min_sep = window_select_keywords(who, win, 2, keep, k, min_sep)
    return _window_select(who, sims, mask, gt, None, win, 2, keep, min_sep, return_scores, return_bounds, return_order, lambda p: hip.ext_check(
        hip.ext_lib().rvx_window_select_clipped(p.sims, p.mask, p.R, p.rpm, p.L, win, k, p.keep, min_sep, p.Wcap, p.gt, p.select, p.n_select, p.n_windows,
                                                p.scores, p.bounds, p.order, p.hit_rank, hip.stream()), "rvx_window_select_clipped"))


WINDOW_RULES = {"shifted": hip.RV_WINDOWS_SHIFTED, "clipped": hip.RV_WINDOWS_CLIPPED}
WINDOW_FRAME_SETS = {"all": hip.RV_FRAMES_ALL, "sampled": hip.RV_FRAMES_SAMPLED}
WINDOW_SELECT_MAX_SAMPLED = hip.RVC_MAX_SAMPLED
FrameWindowSelection = collections.namedtuple("FrameWindowSelection", WindowSelection._fields + ("n_candidates",))


def window_select_frames_keywords(who, rule, win, stride, keep, frames="all", num_frames=None, k=3, min_sep=1):
    """The keyword refusals of ``window_select_frames`` that need no tensor (raised before any device is looked for) -> (rule code, win, stride, keep,
    frame set code, F, k, min_sep) as ``rvc_window_select_frames`` takes them: the clipped rule has stride 2 (None is 2), the shifted rule needs one;
    ``frames="sampled"`` needs ``num_frames`` in [1, 1024], ``frames="all"`` takes none."""
    if not isinstance(rule, str) or rule not in WINDOW_RULES:
        raise ValueError(f"{who}: rule={rule!r} (expected one of {sorted(WINDOW_RULES)})")
    if not isinstance(frames, str) or frames not in WINDOW_FRAME_SETS:
        raise ValueError(f"{who}: frames={frames!r} (expected one of {sorted(WINDOW_FRAME_SETS)})")
    if rule == "clipped":
        if stride is not None and not (_is_int(stride) and stride == 2):
            raise ValueError(f"{who}: stride={stride!r} with rule='clipped' (its windows overlap by half: stride 2, or None)")
        stride = 2
    elif stride is None:
        raise ValueError(f"{who}: rule='shifted' needs a stride")
    win, stride, keep, k, min_sep = window_select_keywords(who, win, stride, keep, k, min_sep)
    if frames == "sampled":
        if not (_is_int(num_frames) and 1 <= num_frames <= WINDOW_SELECT_MAX_SAMPLED):
            raise ValueError(f"{who}: num_frames={num_frames!r} sampled frames per window must be an integer in [1, {WINDOW_SELECT_MAX_SAMPLED}]")
    elif num_frames is not None:
        raise ValueError(f"{who}: num_frames={num_frames!r} with frames='all' (every frame of a window counts: no num_frames)")
    return WINDOW_RULES[rule], win, stride, keep, WINDOW_FRAME_SETS[frames], int(num_frames or 0), k, min_sep


def window_select_valid(who, valid, mask):
    """The refusals of ``valid``: None, or a bool, uint8 or floating-point tensor of ``mask``'s shape."""
    if valid is not None:
        _valid_rows(who, valid, (mask,), f"mask's shape {_shape(mask)}")


def window_select_frames(sims, mask, *, rule, win, stride=None, keep, frames="all", num_frames=None, valid=None, k=3, min_sep=1, gt=None, return_scores=False,
                         return_bounds=False, return_order=False):
    """``window_select`` (``rule="shifted"``, with its ``stride``) and ``window_select_clipped`` (``rule="clipped"``) with a say in which frames of a
    window count (``rvc_window_select_frames`` of the chain library): the same sims, mask and gt -> FrameWindowSelection(select, n_select, n_windows,
    scores, bounds, order, hit_rank, n_candidates i32 [...]).  ``frames="all"`` scores a window on its every frame; ``frames="sampled"`` on the
    ``num_frames`` frames ``window_gather`` / ``window_gather_clipped`` hand on for the same ``num_frames`` (at most 1024; a frame sampled twice counts
    twice).  ``valid`` [mask's shape] (bool, uint8 or float; None: every frame) hides the frames where it is 0: their sims are never looked at, and the
    duration stays the mask's.  A window's score is the sum of its ``min(k, usable)`` best usable entries; a window without a usable entry is no
    candidate - NaN in ``scores``, its geometry in ``bounds``, absent from ``select`` and ``order`` - while ``n_windows`` still counts it;
    ``n_select = min(keep, n_candidates)``.  With ``frames="all"`` and ``valid=None`` every field equals the other two functions' bit for bit.  One
    launch (a mask or a valid that is not f32 adds a cast kernel), no synchronisation, no host copy.  The full rule stands in
    include/revision_hip_chain.h."""
    who = "window_select_frames"
    rule, win, stride, keep, frames, F, k, min_sep = window_select_frames_keywords(who, rule, win, stride, keep, frames, num_frames, k, min_sep)
    return _window_select(who, sims, mask, gt, valid, win, stride, keep, min_sep, return_scores, return_bounds, return_order, lambda p: hip.chain_check(
        hip.chain_lib().rvc_window_select_frames(p.sims, p.mask, p.valid, p.R, p.rpm, p.L, rule, win, stride, frames, F, k, p.keep, min_sep, p.Wcap, p.gt,
                                                 p.select, p.n_select, p.n_windows, p.n_candidates, p.scores, p.bounds, p.order, p.hit_rank, hip.stream()),
        "rvc_window_select_frames"), candidates=True)


MaskedSpanScores = collections.namedtuple("MaskedSpanScores", "scores windows n_usable")


def skip_nan_flag(who, skip_nan):
    """The refusal of ``skip_nan`` (raised before any device is looked for) -> 0 / 1."""
    return _flag(who, "skip_nan", skip_nan)


def span_scores_masked_checks(who, sims, spans, mask, valid=None, skip_nan=False, k=3, pooling="topk", temperature=0.01):
    """The refusals of ``span_scores_masked`` (raised before any device is looked for) -> (leading shape, rows, rows per mask row, L, N, mode, k,
    temperature, skip_nan) as ``rvc_span_scores_masked`` takes them."""
    if pooling not in SPAN_POOLINGS:
        raise ValueError(f"{who}: pooling={pooling!r} (expected one of {sorted(SPAN_POOLINGS)})")
    skip_nan = skip_nan_flag(who, skip_nan)
    if not torch.is_tensor(sims) or not torch.is_tensor(spans) or not torch.is_tensor(mask):
        raise ValueError(f"{who}: sims, spans and mask must be tensors")
    if (sims.dim() not in (2, 3) or spans.dim() != sims.dim() + 1 or spans.shape[:-2] != sims.shape[:-1] or spans.shape[-1] != 2
            or mask.shape != (sims.shape[0], sims.shape[-1])):
        raise ValueError(f"{who}: sims {tuple(sims.shape)} / spans {tuple(spans.shape)} / mask {tuple(mask.shape)} (expected [R, L], [R, N, 2] and [R, L], "
                         f"or [B, Q, L], [B, Q, N, 2] and [B, L])")
    if sims.dtype != torch.float32:
        raise ValueError(f"{who}: sims must be float32 (got {sims.dtype})")
    if not spans.dtype.is_floating_point:
        raise ValueError(f"{who}: spans must be a floating-point tensor (got {spans.dtype})")
    if mask.dtype.is_complex:
        raise ValueError(f"{who}: mask must be bool, integer or floating point (got {mask.dtype})")
    window_select_valid(who, valid, mask)
    lead, L, N = tuple(sims.shape[:-1]), sims.shape[-1], spans.shape[-2]
    rows = math.prod(lead)
    if min(rows, L) < 1:
        raise ValueError(f"{who}: empty sims {tuple(sims.shape)}")
    if rows > 65535:
        raise ValueError(f"{who}: {rows} rows (at most 65535 per call)")
    if pooling == "topk" and not (_is_int(k) and 1 <= k <= 64):
        raise ValueError(f"{who}: k={k!r} must be an integer in [1, 64]")
    try:
        temperature = float(temperature)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: temperature={temperature!r} must be a number") from None
    if pooling == "attention" and (temperature == 0.0 or not math.isfinite(temperature)):
        raise ValueError(f"{who}: temperature={temperature} must be finite and not 0")
    return lead, rows, rows // mask.shape[0], L, N, SPAN_POOLINGS[pooling], int(k) if pooling == "topk" else 1, temperature, skip_nan


def span_scores_masked(sims, spans, mask, *, valid=None, skip_nan=False, k=3, pooling="topk", temperature=0.01, return_windows=False, return_usable=False):
    """``span_scores`` / ``span_scores_multi`` over the frames that count (``rvc_span_scores_masked`` of the chain library): sims f32 [R,L] with spans
    [R,N,2] and mask [R,L], or sims f32 [B,Q,L] with spans [B,Q,N,2] and mask [B,L] -> MaskedSpanScores(scores f32 [...,N], windows i32 [...,N,2],
    n_usable i32 [...,N]); ``windows`` and ``n_usable`` are None unless asked for.  ``valid`` [mask's shape] (bool, uint8 or float; None: every frame)
    hides the frames where it is 0, ``skip_nan`` the frames whose similarity is NaN (a zeroed feature row); a hidden frame's similarity is never looked
    at, and the duration and the windows stay the mask's.  A window's score is the sum of its ``min(k, usable)`` best usable frames (``"topk"``) or the
    softmax pooling over its usable frames (``"attention"``); a non-empty window without a usable frame scores NaN, an empty one 0.  With
    ``valid=None`` and ``skip_nan=False`` scores and windows equal the other two functions' bit for bit.  One launch (a mask or a valid that is not
    f32 adds a cast kernel), no synchronisation, no host copy.  The full rule stands in include/revision_hip_chain.h."""
    return _span_scores_masked("span_scores_masked", sims, spans, mask, False, valid, skip_nan, k, pooling, temperature, return_windows, return_usable)


def _span_scores_masked(who, sims, spans, mask, rows, valid, skip_nan, k, pooling, temperature, return_windows, return_usable):
    """``span_scores_masked`` (``valid`` None or of the mask's shape) and ``span_scores_masked_rows`` (``rows``: ``valid`` of ``sims``' shape), each with its
    own entry: one body."""
    lead, nrows, rpm, L, N, mode, k, temperature, skip_nan = span_scores_masked_checks(who, sims, spans, mask, None if rows else valid, skip_nan, k, pooling,
                                                                                      temperature)
    if rows:
        span_rows_valid(who, valid, sims)
    dev = sims.device
    scores = torch.empty(lead + (N,), dtype=torch.float32, device=dev)
    win = torch.empty(lead + (N, 2), dtype=torch.int32, device=dev) if return_windows else None
    usable = torch.empty(lead + (N,), dtype=torch.int32, device=dev) if return_usable else None
    if N > 0:
        sims, spans, mask, valid = _rows_f32(sims, spans, mask, valid)
        rule = (nrows, rpm, L, N, mode, k, temperature, skip_nan, hip.ptr(scores), hip.ptr(win), hip.ptr(usable), hip.stream())
        if rows:
            hip.chain_check(hip.chain_lib().rvc_span_scores_masked_rows(hip.ptr(sims), hip.ptr(spans), hip.ptr(mask), hip.ptr(valid), 1, *rule),
                            "rvc_span_scores_masked_rows")
        else:
            hip.chain_check(hip.chain_lib().rvc_span_scores_masked(hip.ptr(sims), hip.ptr(spans), hip.ptr(mask), hip.ptr(valid), *rule), "rvc_span_scores_masked")
    return MaskedSpanScores(scores, win, usable)


def span_propose_masked(sims, mask, *, valid=None, skip_nan=False, levels=SPAN_PROPOSE_LEVELS, relative=True, smooth=1, gap=0, min_len=1, max_len=None,
                        max_spans=256, return_windows=False, return_smoothed=False):
    """``span_propose`` from the frames that count (``rvc_span_propose_masked`` of the chain library): the same sims, mask, keywords and
    SpanProposals.  ``valid`` [mask's shape] (bool, uint8 or float; None: every frame) hides the frames where it is 0, ``skip_nan`` the frames whose
    similarity is NaN.  A usable frame is smoothed over the usable frames of its box alone (their sum divided by their count), a hidden frame's smoothed
    value is NaN: it is left out of the row's range, is never above a threshold and breaks a run unless ``gap`` closes it (a run's length counts the
    hidden frames inside it).  A row without a usable frame gives no span.  The duration stays the mask's.  With ``valid=None`` and ``skip_nan=False``
    every field equals ``span_propose``'s bit for bit.  One launch (a mask or a valid that is not f32 adds a cast kernel, ``return_smoothed`` a fill),
    no synchronisation, no host copy.  The full rule stands in include/revision_hip_chain.h."""
    return _span_propose("span_propose_masked", sims, mask, "mask", valid, skip_nan, (levels, relative, smooth, gap, min_len, max_len, max_spans), return_windows,
                         return_smoothed)


WINDOWS_VALID_MAX_KEEP = 2048
WindowsValid = collections.namedtuple("WindowsValid", "valid n_valid")


def windows_valid_checks(who, select, mask, rule, win, stride=None, frames="all", num_frames=None, valid=None, return_count=False):
    """The refusals of ``windows_valid`` (raised before any device is looked for) -> (rule code, win, stride, frame set code, F, leading shape, R, rows
    per mask row, L, keep) as ``rvc_windows_valid`` takes them."""
    rule, win, stride, _, frames, F, _, _ = window_select_frames_keywords(who, rule, win, stride, 1, frames, num_frames)
    if not torch.is_tensor(select) or not torch.is_tensor(mask):
        raise ValueError(f"{who}: select and mask must be tensors")
    if select.dim() not in (2, 3) or mask.dim() != 2:
        raise ValueError(f"{who}: select {tuple(select.shape)} / mask {tuple(mask.shape)} (expected [R, keep] or [B, Q, keep] and [R, L] / [B, L])")
    if select.dtype != torch.int32:
        raise ValueError(f"{who}: select must be int32 (got {select.dtype})")
    lead, keep, (M, L) = tuple(select.shape[:-1]), select.shape[-1], mask.shape
    R = math.prod(lead)
    if min(R, keep, M, L) < 1 or (select.dim() == 3 and M != lead[0]) or R % M != 0:
        raise ValueError(f"{who}: select {tuple(select.shape)} / mask {tuple(mask.shape)} (one mask row per video: a whole number of rows of select for each)")
    if keep > WINDOWS_VALID_MAX_KEEP:
        raise ValueError(f"{who}: keep={keep} entries per row (at most {WINDOWS_VALID_MAX_KEEP})")
    if L > SPAN_PROPOSE_MAX_FRAMES:
        raise ValueError(f"{who}: L={L} frames (at most {SPAN_PROPOSE_MAX_FRAMES})")
    if win > L:
        raise ValueError(f"{who}: win={win} frames for rows of L={L}")
    if mask.dtype.is_complex:
        raise ValueError(f"{who}: mask must be bool, integer or floating point (got {mask.dtype})")
    window_select_valid(who, valid, mask)
    _flag(who, "return_count", return_count)
    return rule, win, stride, frames, F, lead, R, R // M, L, keep


def windows_valid(select, mask, *, rule, win, stride=None, frames="all", num_frames=None, valid=None, return_count=False):
    """A window selection as the validity rows the ``_rows`` span functions take (``rvc_windows_valid`` of the chain library): select i32 [R,keep] with
    mask [R,L], or select i32 [B,Q,keep] with mask [B,L] (with fewer mask rows than rows of select each serves a whole number of consecutive rows) ->
    WindowsValid(valid f32 [...,L] over ``select``'s leading shape, n_valid i32 [...] or None unless ``return_count``).  ``select`` is
    ``window_select_frames``' as it lies, -1 padding included, or window indices from anywhere (the LLM's answers, a retrieval log): an entry outside the
    row's windows names nothing, order and duplicates do not matter.  ``rule``, ``win``, ``stride``, ``frames`` and ``num_frames`` are
    ``window_select_frames``' and mean the same windows and the same frames of a window.  ``valid[r, t]`` is 1 where frame ``t`` lies inside the mask's
    duration, in the frame set of a named window and - with ``valid`` [mask's shape] (bool, uint8 or float) given - where that is not 0; else 0.  One
    launch (a mask or a valid that is not f32 adds a cast kernel), no synchronisation, no host copy.  The full rule stands in
    include/revision_hip_chain.h."""
    rule, win, stride, frames, F, lead, R, rpm, L, keep = windows_valid_checks("windows_valid", select, mask, rule, win, stride, frames, num_frames, valid,
                                                                               return_count)
    dev = select.device
    out = torch.empty(lead + (L,), dtype=torch.float32, device=dev)
    n_valid = torch.empty(lead, dtype=torch.int32, device=dev) if return_count else None
    select = select.contiguous()
    mask, valid = _rows_f32(mask, valid)
    hip.chain_check(hip.chain_lib().rvc_windows_valid(hip.ptr(select), hip.ptr(mask), hip.ptr(valid), R, rpm, L, rule, win, stride, frames, F, keep, hip.ptr(out),
                                                      hip.ptr(n_valid), hip.stream()), "rvc_windows_valid")
    return WindowsValid(out, n_valid)


def span_rows_valid(who, valid, sims):
    """The refusals of a per-row ``valid``: a bool, uint8 or floating-point tensor of ``sims``' shape."""
    _valid_rows(who, valid, (sims,), f"sims' shape {_shape(sims)}: a validity row per row")


def span_scores_masked_rows(sims, spans, mask, *, valid, skip_nan=False, k=3, pooling="topk", temperature=0.01, return_windows=False, return_usable=False):
    """``span_scores_masked`` with a validity row per ROW (``rvc_span_scores_masked_rows`` of the chain library): the same sims, spans, mask, keywords
    and MaskedSpanScores, with ``valid`` of ``sims``' shape ([R,L] or [B,Q,L]; bool, uint8 or float) - on the [B,Q,L] layout every query has its own
    usable frames, what ``windows_valid`` makes of a per-query window selection, while the duration stays its video's.  Each (b, q) equals
    ``span_scores_masked`` on that row alone bit for bit.  One launch (a mask or a valid that is not f32 adds a cast kernel), no synchronisation, no
    host copy.  The full rule stands in include/revision_hip_chain.h."""
    return _span_scores_masked("span_scores_masked_rows", sims, spans, mask, True, valid, skip_nan, k, pooling, temperature, return_windows, return_usable)


def span_propose_masked_rows(sims, mask, *, valid, skip_nan=False, levels=SPAN_PROPOSE_LEVELS, relative=True, smooth=1, gap=0, min_len=1, max_len=None,
                             max_spans=256, return_windows=False, return_smoothed=False):
    """``span_propose_masked`` with a validity row per ROW (``rvc_span_propose_masked_rows`` of the chain library): the same sims, mask, keywords and
    SpanProposals, with ``valid`` of ``sims``' shape ([R,L] or [B,Q,L]; bool, uint8 or float).  Each (b, q) equals ``span_propose_masked`` on that row
    alone bit for bit.  One launch (a mask or a valid that is not f32 adds a cast kernel, ``return_smoothed`` a fill), no synchronisation, no host
    copy.  The full rule stands in include/revision_hip_chain.h."""
    return _span_propose("span_propose_masked_rows", sims, mask, "rows", valid, skip_nan, (levels, relative, smooth, gap, min_len, max_len, max_spans),
                         return_windows, return_smoothed)


SPAN_REFINE_MAX_RADIUS = 64
SPAN_REFINE_MAX_MARGIN = 128
RefinedSpans = collections.namedtuple("RefinedSpans", "spans windows contrast contrast0")


def span_refine_keywords(who, radius, margin, min_len=1, form="cxw", return_windows=False, return_contrast=False):
    """The keyword refusals of ``span_refine`` (raised before any device is looked for) -> (form code, radius, margin, min_len) as ``rvc_span_refine``
    takes them."""
    if not isinstance(form, str) or form not in SPAN_FORMS:
        raise ValueError(f"{who}: form={form!r} (expected one of {sorted(SPAN_FORMS)})")
    if not (_is_int(radius) and 1 <= radius <= SPAN_REFINE_MAX_RADIUS):
        raise ValueError(f"{who}: radius={radius!r} must be an integer in [1, {SPAN_REFINE_MAX_RADIUS}]")
    if not (_is_int(margin) and 1 <= margin <= SPAN_REFINE_MAX_MARGIN):
        raise ValueError(f"{who}: margin={margin!r} must be an integer in [1, {SPAN_REFINE_MAX_MARGIN}]")
    if not (_is_int(min_len) and 1 <= min_len < 2 ** 31):
        raise ValueError(f"{who}: min_len={min_len!r} must be a positive integer")
    _flag(who, "return_windows", return_windows)
    _flag(who, "return_contrast", return_contrast)
    return SPAN_FORMS[form], int(radius), int(margin), int(min_len)


def span_refine_checks(who, sims, spans, mask, valid=None):
    """The tensor refusals of ``span_refine`` (raised before any device is looked for) -> (leading shape, rows, rows per mask row, rows per validity
    row, L, N).  ``valid`` has the mask's shape (a row per mask row) or ``sims``' shape (a row per row)."""
    if not torch.is_tensor(spans):
        raise ValueError(f"{who}: sims, spans and mask must be tensors")
    lead, rows, rpm, L = span_propose_shapes(who, sims, mask)
    if spans.dim() != sims.dim() + 1 or spans.shape[:-2] != sims.shape[:-1] or spans.shape[-1] != 2:
        raise ValueError(f"{who}: sims {tuple(sims.shape)} / spans {tuple(spans.shape)} (expected [R, L] and [R, N, 2], or [B, Q, L] and [B, Q, N, 2])")
    if sims.dtype != torch.float32:
        raise ValueError(f"{who}: sims must be float32 (got {sims.dtype})")
    if not spans.dtype.is_floating_point:
        raise ValueError(f"{who}: spans must be a floating-point tensor (got {spans.dtype})")
    if rows > 65535:
        raise ValueError(f"{who}: {rows} rows (at most 65535 per call)")
    return lead, rows, rpm, _rows_per_valid(who, valid, mask, sims, rpm), L, spans.shape[-2]


def span_refine(sims, spans, mask, *, form="cxw", radius, margin, min_len=1, valid=None, return_windows=False, return_contrast=False):
    """Refine spans' bounds on the device (``rvc_span_refine`` of the chain library), the stage behind the ranking: sims f32 [R,L] or [B,Q,L] (cosine
    rows), spans [...,N,2] as (centre, width) (``form="cxw"``) or (start, end) (``"xx"``) in fractions of the duration - kept proposals, an LLM's
    answers, a retrieval log - mask [R,L] / [B,L] -> RefinedSpans(spans f32 [...,N,2], windows i32 [...,N,2], contrast f32 [...,N], contrast0 f32
    [...,N]); ``windows`` is None unless ``return_windows``, the contrasts unless ``return_contrast``.  Every span's frame window [lo, hi) (the rule of
    ``span_scores``, cut at the duration) is moved to the pair (a, b) with ``|a - lo| <= radius``, ``|b - hi| <= radius`` and ``b - a >= min_len`` that
    has the largest contrast: the mean of the usable frames inside minus the mean of the usable frames within ``margin`` frames outside, on
    similarities quantised to 2^-24 so that the sums are exact.  Ties go to the pair nearest the original one, which is always a candidate; a span
    with no usable frame inside or outside any candidate stays where it is (``contrast`` NaN).  ``valid`` (bool, uint8 or float; None: every frame)
    hides the frames where it is 0 - of the mask's shape it is a row per mask row, of ``sims``' shape a row per row; a NaN similarity is never
    usable.  The result is ALWAYS (centre, width) in ``span_propose``'s encoding, so ``span_scores`` on it recovers ``windows``; a void span (NaN, empty,
    outside the duration) gives NaN, (-1, -1) and NaN contrasts; ``contrast0`` is the original pair's contrast.  One launch (a mask or a valid that is
    not f32 adds a cast kernel), no synchronisation, no host copy.  The full rule stands in include/revision_hip_chain.h."""
    who = "span_refine"
    code, radius, margin, min_len = span_refine_keywords(who, radius, margin, min_len, form, return_windows, return_contrast)
    lead, rows, rpm, rpv, L, N = span_refine_checks(who, sims, spans, mask, valid)
    dev = sims.device
    out = torch.empty(lead + (N, 2), dtype=torch.float32, device=dev)
    win = torch.empty(lead + (N, 2), dtype=torch.int32, device=dev) if return_windows else None
    contrast = torch.empty(lead + (N,), dtype=torch.float32, device=dev) if return_contrast else None
    contrast0 = torch.empty(lead + (N,), dtype=torch.float32, device=dev) if return_contrast else None
    if N > 0:
        sims, spans, mask, valid = _rows_f32(sims, spans, mask, valid)
        hip.chain_check(hip.chain_lib().rvc_span_refine(hip.ptr(sims), hip.ptr(spans), code, hip.ptr(mask), hip.ptr(valid), rpv, rows, rpm, L, N, radius, margin,
                                                        min_len, hip.ptr(out), hip.ptr(win), hip.ptr(contrast), hip.ptr(contrast0), hip.stream()),
                        "rvc_span_refine")
    return RefinedSpans(out, win, contrast, contrast0)


SPAN_ANCHORS_MAX_SCALES = 8
SPAN_ANCHORS_MAX_PEAK = 64
SPAN_ANCHOR_SCORES = {"mean": hip.RVC_ANCHORS_MEAN, "contrast": hip.RVC_ANCHORS_CONTRAST}
SpanAnchors = collections.namedtuple("SpanAnchors", "spans scores n_spans n_found windows scale")


def span_anchors_keywords(who, scales, score="contrast", peak=2, min_usable=1, max_spans=256, return_windows=False, return_scale=False):
    """The keyword refusals of ``span_anchors`` (raised before any device is looked for) -> (scales as a tuple of (len, stride, margin) triples with
    the defaults filled in, mode code, peak, min_usable, max_spans) as ``rvc_span_anchors`` takes them."""
    if isinstance(scales, (str, bytes)) or not isinstance(scales, collections.abc.Sequence):
        raise ValueError(f"{who}: scales={scales!r} must be a sequence of ints, (len, stride) or (len, stride, margin) tuples")
    if not 1 <= len(scales) <= SPAN_ANCHORS_MAX_SCALES:
        raise ValueError(f"{who}: {len(scales)} scales (1 to {SPAN_ANCHORS_MAX_SCALES})")
    if not isinstance(score, str) or score not in SPAN_ANCHOR_SCORES:
        raise ValueError(f"{who}: score={score!r} (expected one of {sorted(SPAN_ANCHOR_SCORES)})")
    triples = []
    for sc in scales:
        sc = (sc,) if _is_int(sc) else sc
        if not (isinstance(sc, (tuple, list)) and 1 <= len(sc) <= 3 and all(_is_int(v) for v in sc)):
            raise ValueError(f"{who}: scale {sc!r} must be an int, (len, stride) or (len, stride, margin) of ints")
        length = int(sc[0])
        if not 1 <= length < 2 ** 31:
            raise ValueError(f"{who}: scale {tuple(sc)!r} has len={length} (a positive integer)")
        stride = int(sc[1]) if len(sc) > 1 else max(1, length // 4)
        margin = int(sc[2]) if len(sc) > 2 else max(1, length // 2)
        if not 1 <= stride <= length:
            raise ValueError(f"{who}: scale {tuple(sc)!r} has stride={stride} (an integer in [1, len={length}])")
        if not 1 <= margin < 2 ** 31:
            raise ValueError(f"{who}: scale {tuple(sc)!r} has margin={margin} (a positive integer)")
        triples.append((length, stride, margin))
    if not (_is_int(peak) and 0 <= peak <= SPAN_ANCHORS_MAX_PEAK):
        raise ValueError(f"{who}: peak={peak!r} must be an integer in [0, {SPAN_ANCHORS_MAX_PEAK}]")
    if not (_is_int(min_usable) and 1 <= min_usable < 2 ** 31):
        raise ValueError(f"{who}: min_usable={min_usable!r} must be a positive integer")
    if not (_is_int(max_spans) and 1 <= max_spans <= SPAN_RANK_MAX):
        raise ValueError(f"{who}: max_spans={max_spans!r} must be an integer in [1, {SPAN_RANK_MAX}]")
    _flag(who, "return_windows", return_windows)
    _flag(who, "return_scale", return_scale)
    return tuple(triples), SPAN_ANCHOR_SCORES[score], int(peak), int(min_usable), int(max_spans)


def span_anchors_checks(who, sims, mask, valid=None):
    """The tensor refusals of ``span_anchors`` (raised before any device is looked for) -> (leading shape, rows, rows per mask row, rows per validity
    row, L).  ``valid`` has the mask's shape (a row per mask row) or ``sims``' shape (a row per row), as ``span_refine`` takes it."""
    lead, rows, rpm, L = span_propose_shapes(who, sims, mask)
    return lead, rows, rpm, _rows_per_valid(who, valid, mask, sims, rpm), L


def span_anchors(sims, mask, *, scales, score="contrast", peak=2, min_usable=1, valid=None, max_spans=256, return_windows=False, return_scale=False):
    """Multi-scale sliding-window proposals on the device (``rvc_span_anchors`` of the chain library), the chain's second generator beside
    ``span_propose``: sims f32 [R,L] or [B,Q,L] (cosine rows), mask [R,L] / [B,L] -> SpanAnchors(spans f32 [...,max_spans,2] as (centre, width) with
    NaN padding, scores f32 [...,max_spans] with NaN padding, n_spans i32 [...], n_found i32 [...], windows i32 [...,max_spans,2] with (-1, -1)
    padding, scale i32 [...,max_spans] with -1 padding); ``windows`` and ``scale`` are None unless asked for.  ``scales`` is a sequence of up to 8
    window lengths in frames, or of (len, stride) or (len, stride, margin) tuples (``stride = max(1, len // 4)``, ``margin = max(1, len // 2)``
    where left out).  Every scale's windows start at 0, stride, 2 stride, .. inside the duration, with one more flush with its end where that leaves
    frames over.  ``score="mean"``: the mean of a window's usable frames; ``"contrast"``: that mean minus the mean of the usable frames within
    ``margin`` frames outside - ``span_refine``'s contrast, on similarities quantised to 2^-24 so that the sums are exact.  A window needs
    ``min_usable`` usable frames (and, for a contrast, one outside).  Within a scale a window is kept when none of the ``peak`` windows on either
    side scores higher (ties: the earlier one stays, so a flat stretch gives one span); scales do not suppress each other - ``span_rank``'s NMS does.
    Spans come in (scale, start) order; if a row has more peaks than ``max_spans`` (``n_found > n_spans``) the best-scoring ``max_spans`` are the ones
    kept.  ``valid`` (bool, uint8 or float; None: every frame) hides the frames where it is 0 - of the mask's shape it is a row per mask row, of
    ``sims``' shape a row per row; a NaN similarity is never usable.  Unlike ``span_propose``'s relative levels nothing depends on the row's range of
    values.  One launch (a mask or a valid that is not f32 adds a cast kernel), no synchronisation, no host copy; the kernel's workspace comes from
    torch's caching allocator.  The full rule stands in include/revision_hip_chain.h."""
    who = "span_anchors"
    table, mode, peak, min_usable, N = span_anchors_keywords(who, scales, score, peak, min_usable, max_spans, return_windows, return_scale)
    lead, rows, rpm, rpv, L = span_anchors_checks(who, sims, mask, valid)
    if sims.dtype != torch.float32:
        raise ValueError(f"{who}: sims must be float32 (got {sims.dtype})")
    dev = sims.device
    spans = torch.empty(lead + (N, 2), dtype=torch.float32, device=dev)
    scores = torch.empty(lead + (N,), dtype=torch.float32, device=dev)
    n_spans = torch.empty(lead, dtype=torch.int32, device=dev)
    n_found = torch.empty(lead, dtype=torch.int32, device=dev)
    windows = torch.empty(lead + (N, 2), dtype=torch.int32, device=dev) if return_windows else None
    scale = torch.empty(lead + (N,), dtype=torch.int32, device=dev) if return_scale else None
    flat = (hip.C.c_int32 * (3 * len(table)))(*(min(v, 2 ** 31 - 1) for t in table for v in t))
    lib = hip.chain_lib()
    nbytes = lib.rvc_span_anchors_workspace(L, flat, len(table), rows)
    if nbytes < 0:
        hip.chain_check(int(nbytes), "rvc_span_anchors_workspace")
    work = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
    sims, mask, valid = _rows_f32(sims, mask, valid)
    hip.chain_check(lib.rvc_span_anchors(hip.ptr(sims), hip.ptr(mask), hip.ptr(valid), rpv, rows, rpm, L, flat, len(table), mode, peak, min_usable, N,
                                         hip.ptr(spans), hip.ptr(scores), hip.ptr(n_spans), hip.ptr(n_found), hip.ptr(windows), hip.ptr(scale), hip.ptr(work),
                                         work.numel(), hip.stream()), "rvc_span_anchors")
    return SpanAnchors(spans, scores, n_spans, n_found, windows, scale)


def proposal_slice(a, b, T):
    """(lo, hi) of ``range(T)[a : b + 1]`` for a >= 0 as ``rv_proposal_cosine`` cuts it: lo = min(a, T), hi = min(b + 1, T); hi <= lo is an empty slice."""
    return min(a, T), min(b + 1, T)


def proposal_cosine(windows, text, proposals, *, k):
    """``topk_cosine`` of ragged proposals in one launch (``rv_proposal_cosine``): windows [W,T,d] (f32 or 16-bit operands), text [d], proposals an
    int32 device tensor [P,3] of (window, a, b) - or a Python list of such triples, uploaded through a pinned buffer - -> f32 [P], entry p the score
    ``topk_cosine(windows[window][a : b + 1][None], text, k)[0]`` of the slice: column norms over the slice's frames, the sum of its min(k, length)
    largest ``<f_t, text / norm>`` (``k <= 0``: their mean).  A proposal whose window lies outside [0, W), whose ``a`` is negative or whose slice is empty
    gives NaN and reads nothing.  One launch (none for P = 0), no synchronisation, no host copy of the scores.  The full rule and the (d, T) for which a
    score is bit for bit ``topk_cosine``'s stand in include/revision_hip.h."""
    who = "proposal_cosine"
    if not _is_int(k) or not -2 ** 31 <= k < 2 ** 31:
        raise ValueError(f"{who}: k={k!r} must be an integer (<= 0: the mean)")
    if not torch.is_tensor(windows) or not torch.is_tensor(text):
        raise ValueError(f"{who}: windows and text must be tensors")
    if windows.dim() != 3 or min(windows.shape) == 0 or text.shape != (windows.shape[2],):
        raise ValueError(f"{who}: windows {tuple(windows.shape)} / text {tuple(text.shape)} (expected [W, T, d] and [d])")
    if windows.dtype not in _GATHER_DTYPES or not text.dtype.is_floating_point:
        raise ValueError(f"{who}: windows must be float32, float16 or bfloat16 and text floating point (got {windows.dtype}, {text.dtype})")
    if torch.is_tensor(proposals):
        if proposals.dim() != 2 or proposals.shape[1] != 3 or proposals.dtype != torch.int32:
            raise ValueError(f"{who}: proposals {tuple(proposals.shape)} {proposals.dtype} (expected an int32 tensor [P, 3] of (window, a, b))")
    else:
        try:
            rows = [tuple(t) for t in proposals]
        except TypeError:
            raise ValueError(f"{who}: proposals must be an int32 tensor [P, 3] or a list of (window, a, b) triples") from None
        if any(len(t) != 3 or not all(_is_int(v) and -2 ** 31 <= v < 2 ** 31 for v in t) for t in rows):
            raise ValueError(f"{who}: proposals must be (window, a, b) triples of int32 integers")
        from .ops import h2d                   # (ops imports this module: at call time both are complete)
        proposals = h2d(torch.tensor(rows, dtype=torch.int32).view(-1, 3), windows.device)
    W, T, d = windows.shape
    P = proposals.shape[0]
    out = torch.empty(P, dtype=torch.float32, device=windows.device)
    if P > 0:
        windows = windows.contiguous()
        if windows.data_ptr() % 16:
            windows = windows.clone()            # (the 16-byte loads; torch's own allocations are aligned)
        hip.check(_score_lib(windows).rv_proposal_cosine(hip.ptr(windows), hip.dtype_code(windows), hip.ptr(text.float().contiguous()), hip.ptr(proposals.contiguous()),
                                                         P, W, T, d, int(k), hip.ptr(out), hip.stream()), "rv_proposal_cosine")
    return out


def attn_pool(text_embeds, video_embeds, temperature):
    """``_attention_pooling`` (similarity.py:96-113) on the device: text [Nt,d], video [Nv,T,d] (16-bit operands or f32) -> f32 [Nv,Nt,d] =
    ``sum_t softmax_t(<f_t, text_j> / temperature) f_t``."""
    if text_embeds.dim() != 2 or video_embeds.dim() != 3 or text_embeds.shape[1] != video_embeds.shape[2]:
        raise ValueError(f"attn_pool: text {tuple(text_embeds.shape)} / video {tuple(video_embeds.shape)}")
    Nv, T, d = video_embeds.shape
    Nt = text_embeds.shape[0]
    out = torch.empty(Nv, Nt, d, dtype=torch.float32, device=video_embeds.device)
    hip.check(_score_lib(video_embeds).rv_attn_pool(hip.ptr(video_embeds.contiguous()), hip.dtype_code(video_embeds), hip.ptr(text_embeds.float().contiguous()), Nv, T, d, Nt,
                                                    float(temperature), hip.ptr(out), hip.stream()), "rv_attn_pool")
    return out
