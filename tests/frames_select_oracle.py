"""The rule of ``rvc_window_select_frames`` (include/revision_hip_chain.h) a second time in numpy float32 with Python loops: the windows of either
rule (tests/window_oracle.py, tests/stage1_prefilter_oracle.py), a window's frame set - every frame, or ``np.linspace(lo, hi - 1, F, dtype=int32)`` -
the entries ``valid`` leaves, their top-k sum in rank order add by add with ties to the smaller POSITION, the candidates, the two passes over the
candidates with the separation counted in window indices, and the ascending sort.  ``select`` is what tests/test_gpu_frames_select.py compares the
kernel with; ``brute_select`` is an independently written statement of the whole selection that tests/test_frames_select_host_logic.py holds
``select`` to.  Nothing here is used by the package."""
import math

import numpy as np

import stage1_prefilter_oracle as PO
import window_oracle as WO

F32 = np.float32
SHIFTED, CLIPPED = 0, 1
ALL, SAMPLED = 0, 1


def capacity(L, win, stride):
    return WO.capacity(L, win, stride)


def windows(D, rule, win, stride):
    """[(lo, hi)] of the row's windows by its geometry (the clipped rule: the non-void ones)."""
    if rule == CLIPPED:
        assert stride == 2
        return PO.windows(D, win)
    return [(lo, hi) for _, _, lo, hi in WO.windows(D, win, stride)]


def sample_indices(lo, hi, num_frames):
    """The frames the gather hands on of window [lo, hi): stage1 / stage2 ``cut_windows``' own expression."""
    return np.linspace(lo, hi - 1, num_frames, dtype=np.int32)


def frame_set(lo, hi, frames, num_frames):
    """The entries of the window's frame set in position order."""
    return [int(t) for t in sample_indices(lo, hi, num_frames)] if frames == SAMPLED else list(range(lo, hi))


def _entry_key(item):
    j, v = item
    return (0, 0.0) if math.isnan(v) else (1, -v)                    # NaN first, then the larger value; sorted() is stable: then the smaller position


def window_score(s, vrow, entries, k):
    """-> (score, n): the sum of the min(k, n) first usable entries in rank order, accumulated from +0, each add rounded to float32; n usable entries."""
    usable = [(j, float(s[t])) for j, t in enumerate(entries) if vrow is None or not vrow[t] == 0]       # (a NaN in valid is not 0)
    acc = F32(0.0)
    with np.errstate(all="ignore"):
        for _, v in sorted(usable, key=_entry_key)[:k]:
            acc = F32(acc + F32(v))
    return acc, len(usable)


def sequence(scores, cand, min_sep):
    """The selection sequence over the candidates: pass 1 over their rank order with the separation rule on window INDICES, pass 2 the rest."""
    order = [i for i in WO.rank_order(scores) if cand[i]]
    alive = [True] * len(scores)
    seq = []
    for i in order:
        if not alive[i]:
            continue
        seq.append(i)
        for j in range(max(0, i - min_sep + 1), min(len(scores), i + min_sep)):
            alive[j] = False
    took = set(seq)
    return seq + [i for i in order if i not in took]


def select(sims, mask, rule, win, stride, frames, num_frames, k, keep, min_sep, valid=None, gt=None):
    """sims [R, L], mask [R / rpm, L], valid [R / rpm, L] or None, gt [R, 2] or None -> dict of select [R, keep], n_select [R], n_windows [R],
    n_candidates [R], win_scores [R, Wcap], bounds [R / rpm, Wcap, 2], order [R, Wcap], hit_rank [R] (None without gt) and D [R] (a list)."""
    sims = np.asarray(sims, dtype=F32)
    mask = np.asarray(mask, dtype=F32)
    valid = None if valid is None else np.asarray(valid, dtype=F32)
    R, L = sims.shape
    M = mask.shape[0]
    rpm = R // M
    Wcap = capacity(L, win, stride)
    nan = np.uint32(WO.NAN_BITS).view(F32)
    out = dict(select=np.full((R, keep), -1, np.int32), n_select=np.zeros(R, np.int32), n_windows=np.zeros(R, np.int32), n_candidates=np.zeros(R, np.int32),
               win_scores=np.full((R, Wcap), nan, F32), bounds=np.full((M, Wcap, 2), -1, np.int32), order=np.full((R, Wcap), -1, np.int32),
               hit_rank=None if gt is None else np.full(R, -1, np.int32), D=[])
    for r in range(R):
        D = WO.duration(mask[r // rpm])
        out["D"].append(D)
        wins = windows(D, rule, win, stride)
        W = len(wins)
        vrow = None if valid is None else valid[r // rpm]
        scored = [window_score(sims[r], vrow, frame_set(lo, hi, frames, num_frames), k) for lo, hi in wins]
        cand = [n > 0 for _, n in scored]
        scores = np.array([sc if n > 0 else nan for sc, n in scored], dtype=F32)
        seq = sequence(scores, cand, min_sep)
        C = sum(cand)
        n = min(keep, C)
        assert len(seq) == C
        out["n_windows"][r], out["n_candidates"][r], out["n_select"][r] = W, C, n
        out["win_scores"][r, :W] = scores
        for i, (lo, hi) in enumerate(wins):
            out["bounds"][r // rpm, i] = (lo, hi)
        out["order"][r, :C] = seq
        out["select"][r, :n] = sorted(seq[:n])
        if gt is not None:
            for p, i in enumerate(seq):
                if WO.covers(wins[i][0], wins[i][1], gt[r][0], gt[r][1]):
                    out["hit_rank"][r] = p
                    break
    return out


def brute_select(row, vrow, D, rule, win, stride, frames, num_frames, k, keep, min_sep):
    """The selection of one row stated on its own, in float64 comparisons on float32 sums: -> (sorted chosen windows, the whole sequence, the number of
    geometric windows)."""
    hop = win // stride
    geo = []
    i = 0
    while i < math.ceil(D / hop) - 1:                                  # windows by their definition
        s = i * win // stride
        e = min(s + win, D - 1)
        if rule == SHIFTED:
            if e - s < win:
                s = e - win
            geo.append((max(s, 0), e))
        elif s <= e:
            geo.append((s, e))
        i += 1
    score = {}
    for i, (s, e) in enumerate(geo):
        if frames == SAMPLED:
            ts = [int(math.floor(x)) for x in np.linspace(float(s), float(e), num_frames)]      # (non-negative: floor is what the int32 cast does)
        else:
            ts = list(range(s, e + 1))
        vals = [row[t] for t in ts if vrow is None or vrow[t] != 0]
        if not vals:
            continue
        nans = [v for v in vals if math.isnan(v)]
        nums = sorted((v for v in vals if not math.isnan(v)), reverse=True)   # (equal values add the same bits whichever comes first, +-0 included)
        acc = F32(0.0)
        with np.errstate(all="ignore"):
            for v in (nans + nums)[:k]:
                acc = F32(acc + F32(v))
        score[i] = float(acc)
    cands = sorted(score)

    def earlier(a, b):
        x, y = score[a], score[b]
        if math.isnan(x) or math.isnan(y):
            return (math.isnan(y) and not math.isnan(x)) or (math.isnan(x) == math.isnan(y) and a < b)
        return x > y or (x == y and a < b)

    def best(c):
        top = None
        for i in c:
            if top is None or earlier(i, top):
                top = i
        return top
    seq, dry = [], False
    while len(seq) < len(cands):
        rest = [i for i in cands if i not in seq]
        if not dry:
            free = [i for i in rest if all(abs(i - j) >= min_sep for j in seq)]
            if free:
                seq.append(best(free))
                continue
            dry = True
        seq.append(best(rest))
    return sorted(seq[:keep]), seq, len(geo)
