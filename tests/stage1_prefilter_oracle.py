"""The rule of ``rvx_window_select_clipped`` (include/revision_hip_ext.h) a second time in numpy float32 with Python loops: the clipped window rule
in integers with the void windows left out, and - from tests/window_oracle.py, which states them for ``rv_window_select`` - the duration, the top-k sum
in rank order add by add, the stable ``sorted`` on the rank key, the two passes and the ascending sort.  ``select`` is what
tests/test_gpu_stage1_prefilter.py compares the kernel with; ``brute_select`` is an independently written statement of the whole selection that
tests/test_stage1_prefilter_host_logic.py holds ``select`` to.  Nothing here is used by the package."""
import math

import numpy as np

import window_oracle as WO

F = np.float32


def capacity(L, win):
    return max(1, -(-L // (win // 2)) - 1)


def all_windows(D, win):
    """[(s, e)] of EVERY index of stage1.cut_windows' range for a row of D frames, void ones (s > e) included."""
    out = []
    for i in range(max(0, -(-D // (win // 2)) - 1)):
        s = (i * win) // 2
        out.append((s, min(s + win, D - 1)))
    return out


def windows(D, win):
    """[(lo, hi)] of the row's candidates: the non-void windows, frames [lo, hi).  The void ones must be a suffix of the index range (an index then
    means the same window with and without them); this asserts it."""
    every = all_windows(D, win)
    solid = [s <= e for s, e in every]
    n = sum(solid)
    assert solid == [True] * n + [False] * (len(every) - n), (D, win)
    return [(s, e + 1) for s, e in every[:n]]


def select(sims, mask, win, k, keep, min_sep, gt=None):
    """sims [R, L], mask [R / rpm, L], gt [R, 2] or None -> dict of select [R, keep], n_select [R], n_windows [R], win_scores [R, Wcap], bounds
    [R / rpm, Wcap, 2], order [R, Wcap], hit_rank [R] (None without gt) and D [R] (a list)."""
    sims = np.asarray(sims, dtype=F)
    mask = np.asarray(mask, dtype=F)
    R, L = sims.shape
    M = mask.shape[0]
    rpm = R // M
    Wcap = capacity(L, win)
    out = dict(select=np.full((R, keep), -1, np.int32), n_select=np.zeros(R, np.int32), n_windows=np.zeros(R, np.int32),
               win_scores=np.full((R, Wcap), np.uint32(WO.NAN_BITS).view(F), F), bounds=np.full((M, Wcap, 2), -1, np.int32),
               order=np.full((R, Wcap), -1, np.int32), hit_rank=None if gt is None else np.full(R, -1, np.int32), D=[])
    for r in range(R):
        D = WO.duration(mask[r // rpm])
        out["D"].append(D)
        wins = windows(D, win)
        W = len(wins)
        scores = np.array([WO.window_score(sims[r], lo, hi, k) for lo, hi in wins], dtype=F)
        seq = WO.sequence(scores, min_sep)
        n = min(keep, W)
        out["n_windows"][r], out["n_select"][r] = W, n
        out["win_scores"][r, :W] = scores
        for i, (lo, hi) in enumerate(wins):
            out["bounds"][r // rpm, i] = (lo, hi)
        out["order"][r, :W] = seq
        out["select"][r, :n] = sorted(seq[:n])
        if gt is not None:
            for p, i in enumerate(seq):
                if WO.covers(wins[i][0], wins[i][1], gt[r][0], gt[r][1]):
                    out["hit_rank"][r] = p
                    break
    return out


def brute_select(row, D, win, k, keep, min_sep):
    """The selection of one row stated on its own, in float64 comparisons on float32 sums: -> (sorted chosen windows, the whole sequence)."""
    cands = []
    i = 0
    while True:                                                      # windows by their definition: index i exists while i < ceil(D / hop) - 1
        if i >= math.ceil(D / (win // 2)) - 1:
            break
        s = i * win // 2
        e = min(s + win, D - 1)
        if s <= e:
            cands.append(i)
        i += 1
    score = {}
    for i in cands:
        s = i * win // 2
        vals = [row[t] for t in range(s, min(s + win, D - 1) + 1)]
        nans = [v for v in vals if math.isnan(v)]
        nums = sorted((v for v in vals if not math.isnan(v)), reverse=True)   # (equal values add the same bits whichever comes first, +-0 included)
        acc = F(0.0)
        with np.errstate(all="ignore"):
            for v in (nans + nums)[:k]:
                acc = F(acc + F(v))
        score[i] = float(acc)

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
    return sorted(seq[:keep]), seq
