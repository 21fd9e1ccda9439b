"""The rule of ``rv_window_select`` (include/revision_hip.h) a second time in numpy float32 with Python loops: the window rule in integers, the top-k
sum in rank order add by add, a stable ``sorted`` on the rank key, the two passes and the ascending sort.  ``select`` is what
tests/test_gpu_window_select.py compares the kernel with; ``brute`` is an independently written statement of the selection ("repeatedly take the
best-ranked untaken window not within min_sep of a taken one; when none is left, take the best-ranked untaken") that
tests/test_window_host_logic.py holds ``sequence`` to.  Nothing here is used by the package."""
import math

import numpy as np

F = np.float32
NAN_BITS = 0x7fc00000


def duration(mask_row):
    """D of a 0 / 1 mask row (its sum is exact in any order)."""
    L = len(mask_row)
    dur = F(np.asarray(mask_row, dtype=np.float64).sum())
    if not np.isfinite(dur):
        return 0
    return min(L, max(0, int(np.floor(dur))))


def capacity(L, win, stride):
    return max(1, -(-L // (win // stride)) - 1)


def windows(D, win, stride):
    """[(s, e, lo, hi)] of a row of D frames: (s, e) as cut_windows' ``times``, frames [lo, hi)."""
    hop = win // stride
    out = []
    for i in range(max(0, -(-D // hop) - 1)):
        s = (i * win) // stride
        e = min(s + win, D - 1)
        if e - s < win:
            s = e - win
        out.append((s, e, max(s, 0), e + 1))
    return out


def _frame_key(item):
    t, v = item
    return (0, 0.0) if math.isnan(v) else (1, -v)                    # NaN first, then the larger value; sorted() is stable: then the smaller index


def window_score(s, lo, hi, k):
    """The sum of the min(k, hi - lo) first frames in rank order, accumulated from 0, each add rounded to float32."""
    frames = sorted(((t, float(s[t])) for t in range(lo, hi)), key=_frame_key)
    acc = F(0.0)
    with np.errstate(all="ignore"):
        for t, _ in frames[:min(k, hi - lo)]:
            acc = F(acc + F(s[t]))
    return acc


def rank_order(scores):
    """Window indices by descending score; ties (-0 against +0 included) to the smaller index, NaN after every number, NaNs by index."""
    return sorted(range(len(scores)), key=lambda i: (1, 0.0) if math.isnan(float(scores[i])) else (0, -float(scores[i])))


def sequence(scores, min_sep):
    """The selection sequence: pass 1 over the rank order with the separation rule, pass 2 the rest in rank order."""
    order = rank_order(scores)
    alive = [True] * len(order)
    seq = []
    for i in order:
        if not alive[i]:
            continue
        seq.append(i)
        for j in range(max(0, i - min_sep + 1), min(len(order), i + min_sep)):            # every j with |i - j| < min_sep
            alive[j] = False
    took = set(seq)
    return seq + [i for i in order if i not in took]


def brute(scores, min_sep):
    """The selection stated on its own, one window per step."""
    W = len(scores)

    def earlier(a, b):                                               # a ranks before b
        x, y = float(scores[a]), float(scores[b])
        if math.isnan(x) or math.isnan(y):
            return (math.isnan(y) and not math.isnan(x)) or (math.isnan(x) == math.isnan(y) and a < b)
        return x > y or (x == y and a < b)

    def best(cands):
        top = None
        for c in cands:
            if top is None or earlier(c, top):
                top = c
        return top
    seq, dry = [], False
    while len(seq) < W:
        rest = [i for i in range(W) if i not in seq]
        if not dry:
            free = [i for i in rest if all(abs(i - j) >= min_sep for j in seq)]
            if free:
                seq.append(best(free))
                continue
            dry = True
        seq.append(best(rest))
    return seq


def covers(lo, hi, gs, ge):
    gs, ge = F(gs), F(ge)
    if not (np.isfinite(gs) and np.isfinite(ge)) or not ge > gs:
        return False
    return bool(F(lo) < ge and F(hi) > gs)


def select(sims, mask, win, stride, k, keep, min_sep, gt=None):
    """sims [R, L], mask [R / rpm, L], gt [R, 2] or None -> dict of select [R, keep], n_select [R], n_windows [R], win_scores [R, Wcap], bounds
    [R / rpm, Wcap, 2], order [R, Wcap], hit_rank [R] (None without gt) and D [R] (a list)."""
    sims = np.asarray(sims, dtype=F)
    mask = np.asarray(mask, dtype=F)
    R, L = sims.shape
    M = mask.shape[0]
    rpm = R // M
    Wcap = capacity(L, win, stride)
    out = dict(select=np.full((R, keep), -1, np.int32), n_select=np.zeros(R, np.int32), n_windows=np.zeros(R, np.int32),
               win_scores=np.full((R, Wcap), np.uint32(NAN_BITS).view(F), F), bounds=np.full((M, Wcap, 2), -1, np.int32),
               order=np.full((R, Wcap), -1, np.int32), hit_rank=None if gt is None else np.full(R, -1, np.int32), D=[])
    for r in range(R):
        D = duration(mask[r // rpm])
        out["D"].append(D)
        wins = windows(D, win, stride)
        W = len(wins)
        scores = np.array([window_score(sims[r], lo, hi, k) for _, _, lo, hi in wins], dtype=F)
        seq = sequence(scores, min_sep)
        n = min(keep, W)
        out["n_windows"][r], out["n_select"][r] = W, n
        out["win_scores"][r, :W] = scores
        for i, (_, _, lo, hi) in enumerate(wins):
            out["bounds"][r // rpm, i] = (lo, hi)
        out["order"][r, :W] = seq
        out["select"][r, :n] = sorted(seq[:n])
        if gt is not None:
            for p, i in enumerate(seq):
                if covers(wins[i][2], wins[i][3], gt[r][0], gt[r][1]):
                    out["hit_rank"][r] = p
                    break
    return out
