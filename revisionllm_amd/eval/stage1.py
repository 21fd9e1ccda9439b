"""Stage-1 (dense / sparse) grounding driver for one query: half-overlapping windows, batches of windows straight into
``inference()`` (LLM batch > 1), ``"From a to b."`` parsing, IoU and entropy / cosine scores; and the same on the device for features that stay
there (``gather_windows``, ``proposal_cosines``, ``score_query_device``, ``run_query_device``: the driver's ``--device_features``); and the LLM on a
selection of the windows only (``clip_stage_windows``, ``windows_from_retrieval``, ``gather_selected``, ``expand_selected``, ``score_query_selected``,
``run_query_selected``: the driver's ``--clip_prefilter_keep`` / ``--retrieval_path``), with records of the same schema.

Counterpart of revisionllm/eval/eval_nlq_negative.py:224-337.  (The reference file imports ``vtimellm.*`` and cannot run
as shipped - SURVEY section 2 #12 - so this follows the cited lines; its ``iou`` helper is pinned by
tests/golden/g9_driver.json.)
"""
import math
import numbers
import re

import numpy as np
import torch

from .. import ops
from ..inference import inference
from ..model.adapter import pad_sequences_1d

QUESTIONS = {"mad_grounding": "During which frames can we see {}?", "ego_assertive": "During which frames {}?",
             "ego_question": "Find the start and end time of the Query from the Video.\nQuery: {}"}  # negative.py:127-131


def cut_windows(ctx_l, debug_window=125, feature_fps=5, num_frames=250):
    """Windows every ``clip_length // 2`` frames, no back-shift (negative.py:224-235)."""
    clip_length = debug_window * feature_fps
    num_window = math.ceil(ctx_l / (clip_length // 2)) - 1
    idx = []
    for i in range(num_window):
        start = max(i * clip_length // 2, 0)
        end = min(i * clip_length // 2 + clip_length, ctx_l - 1)
        idx.append(np.linspace(start, end, num_frames, dtype=np.int32))
    return np.stack(idx) if idx else np.zeros((0, num_frames), np.int32)


def iou(outputs, gt, num_frames_clip, num_frames_video, scores, plus_baseline=False):
    """Same signature / result as negative.py:79-112 -> ({window: (from, to)}, [iou], [kept scores])."""
    frames, keep, clip_frames = [], [], {}
    for i, output in enumerate(outputs):
        if plus_baseline and i == len(outputs) - 1:
            i = 0
        m = re.search(r"(\d+) (to|and) (\d+)", output)
        if not m:
            continue
        a, b = float(m.group(1)), float(m.group(3))
        if a == num_frames_clip - 1 and b == num_frames_clip - 1:
            continue
        if a == b:
            a, b = max(0, a - 1), min(num_frames_video, b + 1)
        clip_frames[i] = (int(a), int(b))
        frames.append((int(i * num_frames_clip // 2 + a), int(i * num_frames_clip // 2 + b)))
        if len(scores) > 0:
            keep.append(scores[i])
    s, e = gt
    ious = []
    for f, t in frames:
        f, t = f / num_frames_video, t / num_frames_video
        inter = max(0, min(t, e) - max(f, s))
        ious.append(round(inter / (max(t, e) - min(f, s)), 2))
    return clip_frames, ious, keep


def score_query(features, answers, ent, query_cls, timestamps, duration, num_frames=250, debug_window=125, score="mean_entropy",
                score_merge="multiply", normalize=True, topk_pool=False, plus_baseline=False):
    """Host epilogue of one query (negative.py:299-337): answers -> proposals + IoU, cosine score of every proposal, score merge.
    ``ent``: one raw entropy statistic per window (max or mean over its decode steps; [] for --score cosine_sim)."""
    gt = (timestamps[0] / duration, timestamps[1] / duration)
    num_frames_video = int(duration * num_frames / debug_window)
    frames, ious, ent = iou(answers, gt, num_frames, num_frames_video, ent, plus_baseline)
    cos = []
    for k, (a, b) in frames.items():
        prop = features[k][a:b + 1]
        cos.append(float(ops.topk_cosine(prop[None], query_cls, min(prop.shape[0], 3) if topk_pool else 0)[0]))
    if normalize:
        if cos:
            cos = [c / max(cos) for c in cos]
        if ent:
            ent = [e / max(ent) for e in ent]
    if "entropy" in score:
        if score_merge == "add":
            scores = [c - e for c, e in zip(cos, ent)]
        elif score_merge == "multiply":
            scores = [c / e for c, e in zip(cos, ent)]
        else:
            scores = [-e for e in ent]
    else:
        scores = cos
    return answers, {"iou": ious, "scores": scores}


def _clipped_geometry(who, features_dev, debug_window, feature_fps):
    """The refusals of the device routes over ``cut_windows``' geometry -> clip_length as an int."""
    clip_length = debug_window * feature_fps
    if not (isinstance(clip_length, numbers.Real) and not isinstance(clip_length, bool) and math.isfinite(clip_length) and clip_length == int(clip_length)
            and clip_length >= 2):
        raise ValueError(f"{who}: debug_window * feature_fps = {clip_length!r} must be a whole number of frames, at least 2")
    clip_length = int(clip_length)
    if not torch.is_tensor(features_dev) or features_dev.dim() != 2 or min(features_dev.shape) == 0 or not features_dev.dtype.is_floating_point:
        raise ValueError(f"{who}: features {tuple(features_dev.shape) if torch.is_tensor(features_dev) else type(features_dev).__name__} "
                         f"(expected a floating-point tensor [ctx_l, d])")
    ctx_l = features_dev.shape[0]
    if ctx_l < clip_length or ops.clipped_window_void(ctx_l, clip_length):
        raise ValueError(f"{who}: ctx_l={ctx_l} frames for windows of {clip_length} (a video shorter than one window, or one whose last window starts "
                         f"behind its end) - take the host route (cut_windows + WindowStager.stage_windows)")
    return clip_length


def gather_windows(features_dev, *, debug_window=125, feature_fps=5, num_frames=250, dtype=None):
    """``cut_windows`` + the host gather for features that are already on the device: features_dev [ctx_l, d] (f32 or 16-bit operands) ->
    [W, num_frames, d] in ``dtype`` (None: ``ops.window_gather``'s default), equal to ``features[cut_windows(ctx_l, debug_window, feature_fps,
    num_frames)]`` cast to ``dtype`` (``rv_window_gather_rule``: one launch, every window, nothing uploaded, no synchronisation).
    ``debug_window * feature_fps`` must be a whole number of frames, at least 2 and at most ctx_l, and no window void (``ops.clipped_window_void``: the
    host route indexes past the array there)."""
    clip_length = _clipped_geometry("stage1.gather_windows", features_dev, debug_window, feature_fps)
    return ops.window_gather_clipped(features_dev, win=clip_length, num_frames=num_frames, out_dtype=dtype)


def proposal_cosines(features, frames, query_cls, topk_pool):
    """The cosine score of every proposal of ``iou``'s ``frames`` dict {window: (a, b)}: features [W,T,d] (device) -> the list of Python floats that the
    loop in ``score_query`` produces, from ONE launch (``ops.proposal_cosine``) and ONE ``.tolist()`` instead of a launch and a host synchronisation per
    proposal.  A proposal the loop would not score - an empty slice, a window past W - sends the whole query through that loop, per proposal, so the
    exception is the host route's."""
    if not frames:
        return []
    W, T = features.shape[0], features.shape[1]
    triples = [(k, a, b) for k, (a, b) in frames.items()]
    for k, a, b in triples:
        lo, hi = ops.proposal_slice(a, b, T)
        if not (0 <= k < W and a >= 0 and hi > lo):
            return _proposal_cosines_each(features, frames, query_cls, topk_pool)
    return ops.proposal_cosine(features, query_cls, triples, k=3 if topk_pool else 0).tolist()


def _proposal_cosines_each(features, frames, query_cls, topk_pool):
    """``score_query``'s loop: one ``ops.topk_cosine`` and one ``float()`` per proposal."""
    cos = []
    for k, (a, b) in frames.items():
        prop = features[k][a:b + 1]
        cos.append(float(ops.topk_cosine(prop[None], query_cls, min(prop.shape[0], 3) if topk_pool else 0)[0]))
    return cos


def _merge_scores(cos, ent, score, score_merge, normalize):
    """``score_query``'s max-normalisation and entropy merge (negative.py:318-336) in Python floats -> the record's ``scores``."""
    if normalize:
        if cos:
            cos = [c / max(cos) for c in cos]
        if ent:
            ent = [e / max(ent) for e in ent]
    if "entropy" in score:
        if score_merge == "add":
            return [c - e for c, e in zip(cos, ent)]
        if score_merge == "multiply":
            return [c / e for c, e in zip(cos, ent)]
        return [-e for e in ent]
    return cos


def score_query_device(features, answers, ent, query_cls, timestamps, duration, num_frames=250, debug_window=125, score="mean_entropy",
                       score_merge="multiply", normalize=True, topk_pool=False, plus_baseline=False):
    """``score_query`` with the proposals' cosine scores from ``proposal_cosines``: the same parameters, the same result.  The max-normalisation and the
    entropy merge stay here in Python floats (float64 arithmetic on a few dozen numbers: on the device it would change the records)."""
    gt = (timestamps[0] / duration, timestamps[1] / duration)
    num_frames_video = int(duration * num_frames / debug_window)
    frames, ious, ent = iou(answers, gt, num_frames, num_frames_video, ent, plus_baseline)
    cos = proposal_cosines(features, frames, query_cls, topk_pool)
    return answers, {"iou": ious, "scores": _merge_scores(cos, ent, score, score_merge, normalize)}


def run_query(model, tokenizer, features, query_feats, query_cls, sentence, timestamps, duration, batch=8, num_frames=250,
              debug_window=125, score="mean_entropy", score_merge="multiply", normalize=True, topk_pool=False,
              prompt="mad_grounding", plus_baseline=False):
    """features [W,T,768] (device).  Returns (answers, info) with info = {'iou': [...], 'scores': [...]} (negative.py:337).
    The reference's own loop: one ``inference()`` per batch of windows, entropy statistics from the returned scores."""
    answers, ent = answer_windows(model, tokenizer, features, query_feats, sentence, batch, score, prompt)
    return score_query(features, answers, ent, query_cls, timestamps, duration, num_frames, debug_window, score, score_merge, normalize, topk_pool,
                       plus_baseline)


def run_query_device(model, tokenizer, features, query_feats, query_cls, sentence, timestamps, duration, batch=8, num_frames=250,
                     debug_window=125, score="mean_entropy", score_merge="multiply", normalize=True, topk_pool=False,
                     prompt="mad_grounding", plus_baseline=False):
    """``run_query`` with ``score_query_device`` as its epilogue (the driver's ``--device_features``): the same parameters, the same result."""
    answers, ent = answer_windows(model, tokenizer, features, query_feats, sentence, batch, score, prompt)
    return score_query_device(features, answers, ent, query_cls, timestamps, duration, num_frames, debug_window, score, score_merge, normalize, topk_pool,
                              plus_baseline)


def clip_stage_windows(features_dev, query_cls, *, debug_window=125, feature_fps=5, keep, num_frames=250, dtype=None, k=3, min_sep=1):
    """The stage-1 pre-filter and the staging of its windows in one pass over features that are on the device: features_dev [ctx_l, d], query_cls [d]
    (host or device) -> (the sorted Python list of the ``keep`` windows of ``cut_windows``' geometry that ``similarity.select_windows_clipped`` chooses,
    the window tensor [len(list), num_frames, d] in ``dtype``, row j equal to ``gather_windows(...)[list[j]]``).  Three launches - the cosine row,
    ``rvx_window_select_clipped``, ``rv_window_gather_rule`` fed from the device ``select`` row - and the gather is enqueued BEFORE the ``.tolist()`` of
    that row, the one device -> host copy, as ``stage2.clip_stage_windows`` does.  The refusals are ``gather_windows``'."""
    who = "stage1.clip_stage_windows"
    from . import similarity
    clip_length = _clipped_geometry(who, features_dev, debug_window, feature_fps)
    if not (isinstance(keep, numbers.Integral) and not isinstance(keep, bool) and keep >= 1):
        raise ValueError(f"{who}: keep={keep!r} must be a positive integer")
    query_cls = query_cls if torch.is_tensor(query_cls) else torch.from_numpy(np.ascontiguousarray(query_cls))
    if query_cls.dim() != 1 or query_cls.shape[0] != features_dev.shape[1] or not query_cls.dtype.is_floating_point:
        raise ValueError(f"{who}: features {tuple(features_dev.shape)} / query_cls {tuple(query_cls.shape)} {query_cls.dtype} (expected [ctx_l, d] and a floating-point [d])")
    dev, ctx_l = features_dev.device, features_dev.shape[0]
    sel = similarity.select_windows_clipped(ops.h2d(query_cls, dev)[None], features_dev[None], torch.ones(1, ctx_l, device=dev), win=clip_length, keep=keep,
                                            k=k, min_sep=min_sep)
    row = sel.select[0]
    frames = ops.window_gather_clipped(features_dev, win=clip_length, num_frames=num_frames, select=row, out_dtype=dtype)
    windows = [i for i in row.tolist() if i >= 0]                   # ascending, the -1 padding behind them: the first len(list) windows of frames
    return windows, frames[:len(windows)]


def clip_stage_windows_frames(features_dev, query_cls, *, debug_window=125, feature_fps=5, keep, num_frames=250, dtype=None, k=3, min_sep=1,
                              score_frames="sampled", valid=None):
    """``clip_stage_windows`` with the windows scored on the frames the LLM is handed: ``score_frames="sampled"`` ranks a window by the ``num_frames``
    frames the gather samples of it (the selection's F is the gather's ``num_frames``), ``"all"`` by its every frame as ``clip_stage_windows`` does;
    ``valid`` [ctx_l] (bool, uint8 or float, host or device; None: every frame) hides frames from the scores, and a window without a usable frame is
    not chosen.  The same three launches (``similarity.select_windows_frames`` under the clipped rule in the middle), the same result, and the gather
    is still enqueued BEFORE the ``.tolist()`` of the ``select`` row, the one device -> host copy."""
    who = "stage1.clip_stage_windows_frames"
    from . import similarity
    from .stage2 import _frames_keywords
    clip_length = _clipped_geometry(who, features_dev, debug_window, feature_fps)
    if not (isinstance(keep, numbers.Integral) and not isinstance(keep, bool) and keep >= 1):
        raise ValueError(f"{who}: keep={keep!r} must be a positive integer")
    query_cls = query_cls if torch.is_tensor(query_cls) else torch.from_numpy(np.ascontiguousarray(query_cls))
    if query_cls.dim() != 1 or query_cls.shape[0] != features_dev.shape[1] or not query_cls.dtype.is_floating_point:
        raise ValueError(f"{who}: features {tuple(features_dev.shape)} / query_cls {tuple(query_cls.shape)} {query_cls.dtype} (expected [ctx_l, d] and a floating-point [d])")
    valid = _frames_keywords(who, score_frames, valid, features_dev)
    dev, ctx_l = features_dev.device, features_dev.shape[0]
    sel = similarity.select_windows_frames(ops.h2d(query_cls, dev)[None], features_dev[None], torch.ones(1, ctx_l, device=dev), rule="clipped", win=clip_length,
                                           keep=keep, frames=score_frames, num_frames=num_frames if score_frames == "sampled" else None,
                                           valid=None if valid is None else ops.h2d(valid, dev), k=k, min_sep=min_sep)
    row = sel.select[0]
    frames = ops.window_gather_clipped(features_dev, win=clip_length, num_frames=num_frames, select=row, out_dtype=dtype)
    windows = [i for i in row.tolist() if i >= 0]                   # ascending, the -1 padding behind them: the first len(list) windows of frames
    return windows, frames[:len(windows)]


def gather_selected(features_dev, windows, *, debug_window=125, feature_fps=5, num_frames=250, dtype=None):
    """``gather_windows`` for a list of window indices that the host already has (``windows_from_retrieval``): -> [len(windows), num_frames, d], row j
    equal to ``gather_windows(...)[windows[j]]``.  The list is uploaded as the ``select`` row of the same launch; no synchronisation."""
    who = "stage1.gather_selected"
    clip_length = _clipped_geometry(who, features_dev, debug_window, feature_fps)
    W = ops.clipped_window_count(features_dev.shape[0], clip_length)
    windows = list(windows)
    if not windows or any(not (isinstance(i, numbers.Integral) and not isinstance(i, bool) and 0 <= i < W) for i in windows):
        raise ValueError(f"{who}: windows={windows!r} must be a non-empty list of indices in [0, {W})")
    row = ops.h2d(torch.tensor(windows, dtype=torch.int32), features_dev.device)
    return ops.window_gather_clipped(features_dev, win=clip_length, num_frames=num_frames, select=row, out_dtype=dtype)


def windows_from_retrieval(frames, n_windows, buffer=0):
    """The stage-1 window indices that a stage-2 record retrieves, by the rule of ``metrics.merge_stage1_stage2``'s ``ranges``: frames = the record's
    ``info["frames"]`` ({key: (f, t)} in stage-2 window units, or a list of such pairs), n_windows = the movie's stage-1 window count -> the distinct
    indices of ``range(max(0, int(.4 * f) - buffer), min(int(.4 * t) + buffer, n_windows - 1))`` over all pairs, ascending.  Host code."""
    pairs = list(frames.values()) if isinstance(frames, dict) else list(frames)
    out = set()
    for f, t in pairs:
        out.update(range(max(0, int(.4 * f) - buffer), min(int(.4 * t) + buffer, n_windows - 1)))
    return sorted(out)


def expand_selected(answers, ent, windows, n_windows):
    """The answers of a run over the windows ``windows`` (ascending, distinct, in [0, n_windows)) as a run over all ``n_windows`` would record them:
    -> (answers of length n_windows, ent of length n_windows or []).  A window that did not run answers ``"Not Present"`` (``metrics.NOT_PRESENT[0]``:
    no proposal), and its entropy slot holds NaN, which ``iou()`` never reads (it keeps the slots of parsed answers only)."""
    from .metrics import NOT_PRESENT
    windows = list(windows)
    if len(answers) != len(windows) or (len(ent) not in (0, len(windows))):
        raise ValueError(f"expand_selected: {len(answers)} answers and {len(ent)} entropy statistics for {len(windows)} windows")
    if windows != sorted(set(windows)) or (windows and not 0 <= windows[0] <= windows[-1] < n_windows):
        raise ValueError(f"expand_selected: windows={windows!r} must be ascending, distinct and in [0, {n_windows})")
    full = [NOT_PRESENT[0]] * n_windows
    full_ent = [float("nan")] * n_windows if len(ent) else []
    for j, w in enumerate(windows):
        full[w] = answers[j]
        if full_ent:
            full_ent[w] = ent[j]
    return full, full_ent


def score_query_selected(features_sel, windows, n_windows, answers_sel, ent_sel, query_cls, timestamps, duration, num_frames=250, debug_window=125,
                         score="mean_entropy", score_merge="multiply", normalize=True, topk_pool=False, plus_baseline=False):
    """``score_query_device`` for a query whose LLM ran on a selection: features_sel [len(windows), T, d] (row j = window ``windows[j]``), answers_sel /
    ent_sel one entry per selected window, n_windows the movie's window count.  The answers are expanded (``expand_selected``) and ``iou()`` runs on them
    unchanged, so the window indices in proposals and IoUs are the TRUE ones; proposal (window, a, b) is scored on row ``windows.index(window)`` of the
    selected tensor through ``proposal_cosines``; normalisation and merge as ``score_query``.  -> (the expanded answers, {"iou", "scores", "windows"}):
    the record ``score_query_device`` writes for the full tensor with the other windows' answers replaced by ``"Not Present"``."""
    windows = [int(w) for w in windows]
    answers, ent = expand_selected(answers_sel, ent_sel, windows, n_windows)
    gt = (timestamps[0] / duration, timestamps[1] / duration)
    num_frames_video = int(duration * num_frames / debug_window)
    frames, ious, ent = iou(answers, gt, num_frames, num_frames_video, ent, plus_baseline)
    row = {w: j for j, w in enumerate(windows)}
    cos = proposal_cosines(features_sel, {row[w]: ab for w, ab in frames.items()}, query_cls, topk_pool)
    return answers, {"iou": ious, "scores": _merge_scores(cos, ent, score, score_merge, normalize), "windows": windows}


def run_query_selected(model, tokenizer, features_sel, windows, n_windows, query_feats, query_cls, sentence, timestamps, duration, batch=8, num_frames=250,
                       debug_window=125, score="mean_entropy", score_merge="multiply", normalize=True, topk_pool=False, prompt="mad_grounding",
                       plus_baseline=False):
    """``run_query_device`` on a selection: ``answer_windows`` on the selected tensor, then ``score_query_selected``."""
    answers, ent = answer_windows(model, tokenizer, features_sel, query_feats, sentence, batch, score, prompt)
    return score_query_selected(features_sel, windows, n_windows, answers, ent, query_cls, timestamps, duration, num_frames, debug_window, score, score_merge,
                                normalize, topk_pool, plus_baseline)


def answer_windows(model, tokenizer, features, query_feats, sentence, batch=8, score="mean_entropy", prompt="mad_grounding"):
    """The LLM part of ``run_query``: -> (the answer of every window, one raw entropy statistic per window or [])."""
    query = "<video>\n" + QUESTIONS[prompt].format(sentence)
    answers, ent = [], []
    for g in range(math.ceil(features.shape[0] / batch)):
        feat = features[g * batch: min((g + 1) * batch, features.shape[0])]
        qf = None
        if query_feats is not None:
            qf = pad_sequences_1d(query_feats[None].repeat(feat.shape[0], 1, 1), dtype=query_feats.dtype, device=query_feats.device)
        ans, out = inference(model, feat, qf, query, tokenizer, return_list=True)
        answers.extend(ans)
        if "entropy" in score:
            st = ops.entropy_stats(torch.stack(out["scores"], 1))
            col = 0 if score == "max_entropy" else 2
            ent.extend(float(e[col]) for e in st)
    return answers, ent


def launch_query_steps(model, tokenizer, features, query_feats, sentence, batch=8, score="mean_entropy", prompt="mad_grounding",
                       max_new_tokens=64, server=None):
    """The LLM part of ``run_query`` as a step generator (``revisionllm_amd.sched``): every batch of windows is one generate whose prefill
    rides in the ``serve.DecodeServer``'s batched passes and whose rows decode in its merged steps (``--in_flight`` of the stage-1 driver;
    the pipeline bench.py's stage-1 workloads time).  Nothing is waited for here beyond what ``generate_steps`` yields.
    -> (device tokens [W, G], device step entropies [W, G], prompt ids, stop string): ``collect_query`` turns them into answers."""
    from ..inference import _prompt_ids
    query = "<video>\n" + QUESTIONS[prompt].format(sentence)
    toks, ents = [], []
    ids1, stop_str = _prompt_ids(query, tokenizer, 1)
    for g in range(math.ceil(features.shape[0] / batch)):
        feat = features[g * batch: min((g + 1) * batch, features.shape[0])]
        qf = None
        if query_feats is not None:
            qf = pad_sequences_1d(query_feats[None].repeat(feat.shape[0], 1, 1), dtype=query_feats.dtype, device=query_feats.device)
        out = yield from model.generate_steps(ids1.repeat(feat.shape[0], 1), images=feat, query_feats=qf, do_sample=True, temperature=0.05, num_beams=1,
                                              max_new_tokens=max_new_tokens, return_dict_in_generate=True, server=server)
        toks.append(out["sequences"][:, ids1.shape[1]:])
        ents.append(out["entropy"])
    width = max(t.shape[1] for t in toks)
    pad = lambda t: torch.nn.functional.pad(t, (0, width - t.shape[1]))      # noqa: E731 - generates of one query may stop at different steps
    return torch.cat([pad(t) for t in toks]), torch.cat([pad(e) for e in ents]), [int(t.shape[1]) for t in toks for _ in range(t.shape[0])], stop_str


def collect_query(model, tokenizer, launched, score="mean_entropy"):
    """Host side of ``launch_query_steps``: decode the answers (inference.py:61-70) and take the entropy statistic of every window over
    ALL the steps its batch's generate ran - like the reference, whose ``get_entropy_statistics`` sees the batch's whole ``scores`` tuple
    (negative.py:291-298): a row that finished early keeps contributing the steps it spent emitting the pad id.  -> (answers, ent)."""
    tok, ent, produced, stop_str = launched
    tok, ent = tok.cpu(), ent.cpu()
    model.engine.check_handoff_status()
    answers, stats = [], []
    for j in range(tok.shape[0]):
        g = produced[j]
        text = tokenizer.batch_decode([tok[j, :g].tolist()], skip_special_tokens=True)[0].strip()
        if text.endswith(stop_str):
            text = text[:-len(stop_str)]
        answers.append(text.strip())
        if "entropy" in score:
            e = ent[j, :g]
            stats.append(float(e.max()) if score == "max_entropy" else float(e.mean()))
    return answers, stats
