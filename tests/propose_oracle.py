"""The rule of ``rv_span_propose`` (include/revision_hip.h) a second time in numpy float32, operation by operation: Python loops per row, ``np.float32``
adds in the stated order and the textbook run scan.  ``propose`` is what tests/test_gpu_propose.py compares the kernel with; ``brute`` is an
independently written statement of the same rule (every frame pair judged straight from the definition, duplicates against ALL higher levels) that
tests/test_propose_host_logic.py holds ``propose`` to.  Nothing here is used by the package."""
import numpy as np

F = np.float32
NAN_BITS = 0x7fc00000


def duration(mask_row):
    """(dur as float32, D) of a 0 / 1 mask row (its sum is exact in any order)."""
    L = len(mask_row)
    dur = F(np.asarray(mask_row, dtype=np.float64).sum())
    if not np.isfinite(dur):
        return dur, 0
    return dur, min(L, max(0, int(np.floor(dur))))


def smooth_row(s, D, smooth):
    """s'[0:D]: the adds in ascending order, then one division."""
    h = smooth // 2
    out = np.empty(D, dtype=F)
    s = np.asarray(s, dtype=F)
    with np.errstate(all="ignore"):
        inner = np.arange(h, D - h)                      # frames whose window is whole: the same adds in the same order, all frames at once
        if inner.size:
            acc = s[inner - h].copy()
            for o in range(1, 2 * h + 1):
                acc = np.add(acc, s[inner - h + o], dtype=F)
            out[inner] = np.divide(acc, F(2 * h + 1), dtype=F)
        for t in [t for t in range(D) if t < h or t >= D - h]:
            a, b = max(0, t - h), min(D - 1, t + h)
            acc = F(s[a])
            for j in range(a + 1, b + 1):
                acc = F(acc + F(s[j]))
            out[t] = F(acc / F(b - a + 1))
    return out


def thresholds(sp, levels, relative):
    """theta_l as float32 (None when the row has no number: then nothing is above)."""
    levels = [F(v) for v in levels]
    if not relative:
        return levels
    nums = sp[~np.isnan(sp)]
    if nums.size == 0:
        return None
    mx, mn = F(nums.max()), F(nums.min())
    with np.errstate(all="ignore"):
        return [F(mn + F(lv * F(mx - mn))) for lv in levels]


def runs_of(above, gap):
    """The textbook scan: (lo, hi) of every run of a boolean row, gaps of at most ``gap`` not-above frames closed."""
    runs, lo, last = [], None, None
    for t, a in enumerate(above):
        if not a:
            continue
        if lo is None:
            lo = t
        elif t - last - 1 > gap:
            runs.append((lo, last + 1))
            lo = t
        last = t
    if lo is not None:
        runs.append((lo, last + 1))
    return runs


def encode(lo, hi, dur):
    """(centre, width) of the window (lo, hi) as float32, each operation rounded on its own."""
    lo, hi, dur = F(lo), F(hi), F(dur)
    with np.errstate(all="ignore"):
        return F(F(F(lo + hi) * F(0.5)) / dur), F(F(F(hi - lo) - F(0.5)) / dur)


def row_runs(s, mask_row, levels, relative, smooth, gap, min_len, max_len):
    """-> (surviving runs in output order, s', dur, D)."""
    dur, D = duration(mask_row)
    sp = smooth_row(np.asarray(s, dtype=F), D, smooth)
    theta = thresholds(sp, levels, relative) if D else None
    T = len(levels)
    per_level = []
    for l in range(T):
        with np.errstate(invalid="ignore"):
            above = (sp > theta[l]) if theta is not None else np.zeros(D, dtype=bool)
        per_level.append(runs_of(above, gap))
    out = []
    for l in range(T - 1, -1, -1):
        nxt = set(per_level[l + 1]) if l < T - 1 else set()
        for lo, hi in per_level[l]:
            n = hi - lo
            if n < min_len or (max_len > 0 and n > max_len) or (lo, hi) in nxt:
                continue
            out.append((lo, hi))
    return out, sp, dur, D


def propose(sims, mask, levels, relative=1, smooth=1, gap=0, min_len=1, max_len=0, N=256):
    """sims [R,L], mask [R / rpm, L] -> dict(spans f32 [R,N,2] (NaN padding), windows i64 [R,N,2] ((-1, -1) padding), n_spans, n_found i64 [R],
    smoothed: list of R float32 arrays of length D, D: list)."""
    sims = np.asarray(sims, dtype=F)
    mask = np.asarray(mask)
    R, L = sims.shape
    rpm = R // mask.shape[0]
    assert rpm * mask.shape[0] == R and mask.shape[1] == L
    spans = np.full((R, N, 2), np.nan, dtype=F)
    spans.view(np.uint32)[...] = NAN_BITS
    windows = np.full((R, N, 2), -1, dtype=np.int64)
    n_spans, n_found = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    smoothed, Ds = [], []
    for r in range(R):
        runs, sp, dur, D = row_runs(sims[r], mask[r // rpm], levels, relative, smooth, gap, min_len, max_len)
        n_found[r] = len(runs)
        n_spans[r] = min(len(runs), N)
        for i, (lo, hi) in enumerate(runs[:N]):
            windows[r, i] = (lo, hi)
            spans[r, i] = encode(lo, hi, dur)
        smoothed.append(sp)
        Ds.append(D)
    return dict(spans=spans, windows=windows, n_spans=n_spans, n_found=n_found, smoothed=smoothed, D=Ds)


def brute(s, mask_row, levels, relative, smooth, gap, min_len, max_len):
    """The rule judged pair by pair: (lo, hi) is a run of level l when both end frames are above, no stretch of more than ``gap`` not-above frames lies
    inside, and the ``gap + 1`` frames on either side (as far as the row goes) are all not above.  A run goes when ANY higher level has the same pair.
    Smoothing and thresholds are restated with float32 array arithmetic (cumulative order kept by an explicit left fold)."""
    dur, D = duration(mask_row)
    s = np.asarray(s, dtype=F)
    h = smooth // 2
    sp = np.empty(D, dtype=F)
    with np.errstate(all="ignore"):
        for t in range(D):
            win = s[max(0, t - h):min(D - 1, t + h) + 1]
            acc = win[0]
            for v in win[1:]:
                acc = np.add(acc, v, dtype=F)
            sp[t] = np.divide(acc, F(len(win)), dtype=F)
        finite_any = D > 0 and not np.all(np.isnan(sp))
        T = len(levels)
        above = np.zeros((T, D), dtype=bool)
        if finite_any or not relative:
            for l, lv in enumerate(levels):
                if relative:
                    mx, mn = np.nanmax(sp), np.nanmin(sp)
                    theta = np.add(mn, np.multiply(F(lv), np.subtract(mx, mn, dtype=F), dtype=F), dtype=F)
                else:
                    theta = F(lv)
                above[l] = np.greater(sp, theta)
    is_run = [set() for _ in range(T)]
    for l in range(T):
        ab = above[l]
        for lo in range(D):
            for hi in range(lo + 1, D + 1):
                if not (ab[lo] and ab[hi - 1]):
                    continue
                if ab[max(0, lo - gap - 1):lo].any() or ab[hi:hi + gap + 1].any():
                    continue
                inside = ab[lo:hi]
                longest = cur = 0
                for v in inside:
                    cur = 0 if v else cur + 1
                    longest = max(longest, cur)
                if longest <= gap:
                    is_run[l].add((lo, hi))
    out = []
    for l in range(T - 1, -1, -1):
        higher = set().union(*is_run[l + 1:]) if l < T - 1 else set()
        for lo, hi in sorted(is_run[l]):
            n = hi - lo
            if n >= min_len and not (max_len > 0 and n > max_len) and (lo, hi) not in higher:
                out.append((lo, hi))
    return out
