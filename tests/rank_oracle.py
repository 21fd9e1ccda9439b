"""The definition of ``rv_span_rank`` (include/revision_hip.h) a second time, in numpy float32, operation by operation, one plain Python loop per row:
rank order, greedy temporal NMS, top-M, IoU against a ground-truth span and first hits.  Every f32 operation is one numpy float32 operation (IEEE, rounded
on its own), so the kernel's integer outputs must EQUAL this module's and ``keep_iou`` must have its bits (one correctly rounded division).  Nothing here
follows the kernel's structure: the order is Python's stable ``sorted`` on a (nan, -score) key, NMS is the textbook loop over a list.

``rank64`` is the same rule written independently in Python floats (float64) - for inputs on which every operation is exact it must agree with ``rank``
(tests/test_rank_host_logic.py holds the two against each other)."""
import math

import numpy as np

F = np.float32
ZERO, HALF = F(0.0), F(0.5)


def bounds(span, form):
    """(start, end) as float32 scalars: form 1 is (centre, width) -> (c - 0.5 w, c + 0.5 w), each operation rounded."""
    a, b = F(span[0]), F(span[1])
    if form == 1:
        hw = HALF * b
        return a - hw, a + hw
    return a, b


def solid(s, e):
    return bool(np.isfinite(s) and np.isfinite(e) and e > s)


def overlap(sa, ea, sb, eb):
    """(inter, union) of two solid spans in float32."""
    d = min(ea, eb) - max(sa, sb)
    inter = d if d > ZERO else ZERO
    return inter, ((ea - sa) + (eb - sb)) - inter


def rank_order(scores):
    """Descending score, ties (-0 against +0 too) to the smaller index, NaN after every number: Python's sort is stable and -0.0 == 0.0."""
    s = [float(x) for x in scores]
    return sorted(range(len(s)), key=lambda i: (1, 0.0) if math.isnan(s[i]) else (0, -s[i]))


def rank_row(scores, spans, form, top, nms_iou, gt=None, hit_iou=()):
    """One row -> dict(order [N], keep [top], n_keep, keep_iou [top] | None, first_hit [T] | None)."""
    N = len(scores)
    nms = F(nms_iou)
    with np.errstate(all="ignore"):
        b = [bounds(spans[i], form) for i in range(N)]
        ok = [solid(*x) for x in b]
        order = rank_order(scores)
        dead = [False] * N
        kept = []
        for a, i in enumerate(order):
            if dead[i]:
                continue
            kept.append(i)
            if len(kept) == top:
                break
            if not ok[i]:
                continue
            for j in order[a + 1:]:
                if dead[j] or not ok[j]:
                    continue
                inter, uni = overlap(b[i][0], b[i][1], b[j][0], b[j][1])
                if inter > nms * uni:
                    dead[j] = True
        out = dict(order=np.array(order, dtype=np.int32), keep=np.array(kept + [-1] * (top - len(kept)), dtype=np.int32), n_keep=len(kept),
                   keep_iou=None, first_hit=None)
        if gt is not None:
            gs, ge = F(gt[0]), F(gt[1])
            iou = np.zeros(top, dtype=np.float32)
            if solid(gs, ge):
                for p, i in enumerate(kept):
                    if ok[i]:
                        inter, uni = overlap(b[i][0], b[i][1], gs, ge)
                        iou[p] = inter / uni if uni > ZERO else ZERO
            out["keep_iou"] = iou
            fh = []
            for t in hit_iou:
                hits = [p for p in range(len(kept)) if iou[p] > F(t)]
                fh.append(hits[0] if hits else -1)
            out["first_hit"] = np.array(fh, dtype=np.int32)
    return out


def rank(scores, spans, form, top, nms_iou, gt=None, hit_iou=()):
    """scores [R,N], spans [R,N,2], gt [R,2] | None (numpy float32) -> dict of stacked arrays (n_keep i32 [R]; absent parts None)."""
    scores, spans = np.asarray(scores, dtype=np.float32), np.asarray(spans, dtype=np.float32)
    rows = [rank_row(scores[r], spans[r], form, top, nms_iou, None if gt is None else np.asarray(gt, dtype=np.float32)[r], hit_iou)
            for r in range(scores.shape[0])]
    out = {k: np.stack([row[k] for row in rows]) for k in ("order", "keep")}
    out["n_keep"] = np.array([row["n_keep"] for row in rows], dtype=np.int32)
    for k in ("keep_iou", "first_hit"):
        out[k] = None if gt is None else np.stack([row[k] for row in rows])
    return out


def rank64(scores, spans, top, nms_iou, gt=None, hit_iou=()):
    """An independent float64 statement for (start, end) spans without voids or NaNs: argsort by repeated maximum, NMS by IoU = inter / union compared as
    ``inter / union > nms`` on exact inputs.  -> (order, keep, first_hit) as lists per row."""
    res = []
    for r in range(len(scores)):
        s = [float(x) for x in scores[r]]
        sp = [(float(a), float(b)) for a, b in spans[r]]
        left, order = list(range(len(s))), []
        while left:
            best = left[0]
            for i in left[1:]:
                if s[i] > s[best]:
                    best = i
            order.append(best)
            left.remove(best)

        def iou(a, b):
            inter = max(0.0, min(a[1], b[1]) - max(a[0], b[0]))
            union = (a[1] - a[0]) + (b[1] - b[0]) - inter
            return inter / union if union > 0 else 0.0
        alive, keep = list(order), []
        while alive and len(keep) < top:
            i = alive.pop(0)
            keep.append(i)
            alive = [j for j in alive if not iou(sp[i], sp[j]) > nms_iou]
        fh = None
        if gt is not None:
            g = (float(gt[r][0]), float(gt[r][1]))
            ious = [iou(sp[i], g) for i in keep]
            fh = [next((p for p, u in enumerate(ious) if u > t), -1) for t in hit_iou]
        res.append((order, keep + [-1] * (top - len(keep)), fh))
    return res
