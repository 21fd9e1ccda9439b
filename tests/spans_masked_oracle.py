"""The rules of ``rvc_span_scores_masked`` and ``rvc_span_propose_masked`` (include/revision_hip_chain.h) a second time in numpy float32 with Python
loops, operation by operation.  The parts the masked entries leave as they were come from the oracles of the unmasked ones: the window rule
(tests/similarity_oracle.py), the duration, the thresholds, the run scan and the span encoding (tests/propose_oracle.py), the frame order
(tests/frames_select_oracle.py).  ``span_scores`` and ``propose`` are what tests/test_gpu_spans_masked.py compares the kernels with; ``attention64`` is
the float64 statement of the attention mode its one tolerance is measured from; ``brute`` is an independently written statement of the masked proposal
rule that tests/test_spans_masked_host_logic.py holds ``propose`` to.  Nothing here is used by the package."""
import numpy as np
import torch

import frames_select_oracle as FO
import propose_oracle as PO
import similarity_oracle as SO

F = np.float32
NAN_BITS = 0x7fc00000
QNAN = np.uint32(NAN_BITS).view(F)
TOPK, ATTENTION = 0, 1


def usable(s, vrow, skip_nan):
    """The usable frames of a row as booleans: valid is None or valid[t] != 0 (the float32 comparison: -0 hides, NaN does not), and under skip_nan
    s[t] == s[t]."""
    s = np.asarray(s, dtype=F)
    with np.errstate(invalid="ignore"):
        u = np.ones(len(s), dtype=bool) if vrow is None else np.asarray(vrow, dtype=F) != F(0)
        if skip_nan:
            u = u & (s == s)
    return u


# ------------------------------------------------------------------ span scores ------------------------------------------------------------------
def attention_f32(vals, tau):
    """sum_t softmax_t(v / tau) v_t over the given values in float32: the maximum (a NaN makes it NaN), then both sums in order, then one division."""
    tau = F(tau)
    with np.errstate(all="ignore"):
        x = [F(F(v) / tau) for v in vals]
        mx = QNAN if any(np.isnan(v) for v in x) else F(max(x))
        z, zs = F(0), F(0)
        for v, xv in zip(vals, x):
            e = np.exp(F(xv - mx), dtype=F)
            z = F(z + e)
            zs = F(zs + F(e * F(v)))
        return F(zs / z)


def attention64(vals, tau):
    """The same sum in float64 (tau as the float32 the kernel is handed)."""
    v = np.asarray(vals, dtype=np.float64)
    if np.isnan(v).any():
        return np.float64("nan")
    x = v / np.float64(F(tau))
    e = np.exp(x - x.max())
    return (e * v).sum() / e.sum()


def span_scores(sims, spans, mask, valid=None, skip_nan=0, mode=TOPK, k=3, temperature=0.01, f64=False):
    """sims [R,L], spans [R,N,2], mask [R / rpm, L], valid [R / rpm, L] or None -> dict(scores f32 [R,N] (float64 with ``f64``: the attention mode's
    float64 statement), windows i64 [R,N,2], n_usable i64 [R,N])."""
    sims = np.asarray(sims, dtype=F)
    mask = np.asarray(mask, dtype=F)
    R, L = sims.shape
    N = spans.shape[1]
    rpm = R // mask.shape[0]
    win = SO.windows(torch.from_numpy(np.array(spans, dtype=F)), torch.from_numpy(np.repeat(mask, rpm, axis=0))).numpy()
    scores = np.zeros((R, N), dtype=np.float64 if f64 else F)
    n_usable = np.zeros((R, N), dtype=np.int64)
    for r in range(R):
        u = usable(sims[r], None if valid is None else valid[r // rpm], skip_nan)
        for n in range(N):
            lo, hi = int(win[r, n, 0]), int(win[r, n, 1])
            if (lo, hi) == SO.NAN_WINDOW:
                scores[r, n] = QNAN
                continue
            if hi <= lo:
                continue
            frames = [(t, float(sims[r, t])) for t in range(lo, hi) if u[t]]
            n_usable[r, n] = len(frames)
            if not frames:
                scores[r, n] = QNAN
            elif mode == TOPK:
                acc = F(0.0)
                with np.errstate(all="ignore"):
                    for _, v in sorted(frames, key=FO._entry_key)[:k]:
                        acc = F(acc + F(v))
                scores[r, n] = acc
            else:
                vals = [F(v) for _, v in frames]
                scores[r, n] = attention64(vals, temperature) if f64 else attention_f32(vals, temperature)
    return dict(scores=scores, windows=win, n_usable=n_usable)


# ------------------------------------------------------------------ proposals ------------------------------------------------------------------
def smooth_row(s, u, D, smooth):
    """s'[0:D]: for a usable t the usable frames of its box added in ascending order from the first usable one, divided by their count; NaN for a
    hidden t."""
    h = smooth // 2
    s = np.asarray(s, dtype=F)
    out = np.empty(D, dtype=F)
    out.view(np.uint32)[...] = NAN_BITS
    with np.errstate(all="ignore"):
        for t in range(D):
            if not u[t]:
                continue
            acc, cnt = None, 0
            for j in range(max(0, t - h), min(D - 1, t + h) + 1):
                if u[j]:
                    acc = F(s[j]) if acc is None else F(acc + F(s[j]))
                    cnt += 1
            out[t] = F(acc / F(cnt))
    return out


def row_runs(s, mask_row, vrow, skip_nan, levels, relative, smooth, gap, min_len, max_len):
    """-> (surviving runs in output order, s', dur, D): propose_oracle.row_runs with the masked smoothing in the place of the plain one."""
    dur, D = PO.duration(mask_row)
    u = usable(np.asarray(s, dtype=F)[:D], None if vrow is None else np.asarray(vrow)[:D], skip_nan)
    sp = smooth_row(s, u, D, smooth)
    theta = PO.thresholds(sp, levels, relative) if D else None
    T = len(levels)
    per_level = []
    for l in range(T):
        with np.errstate(invalid="ignore"):
            above = (sp > theta[l]) if theta is not None else np.zeros(D, dtype=bool)
        per_level.append(PO.runs_of(above, gap))
    out = []
    for l in range(T - 1, -1, -1):
        nxt = set(per_level[l + 1]) if l < T - 1 else set()
        for lo, hi in per_level[l]:
            n = hi - lo
            if n < min_len or (max_len > 0 and n > max_len) or (lo, hi) in nxt:
                continue
            out.append((lo, hi))
    return out, sp, dur, D


def propose(sims, mask, levels, valid=None, skip_nan=0, relative=1, smooth=1, gap=0, min_len=1, max_len=0, N=256):
    """sims [R,L], mask [R / rpm, L], valid [R / rpm, L] or None -> the dict of propose_oracle.propose."""
    sims = np.asarray(sims, dtype=F)
    mask = np.asarray(mask)
    R, L = sims.shape
    rpm = R // mask.shape[0]
    assert rpm * mask.shape[0] == R and mask.shape[1] == L
    spans = np.empty((R, N, 2), dtype=F)
    spans.view(np.uint32)[...] = NAN_BITS
    windows = np.full((R, N, 2), -1, dtype=np.int64)
    n_spans, n_found = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    smoothed, Ds = [], []
    for r in range(R):
        runs, sp, dur, D = row_runs(sims[r], mask[r // rpm], None if valid is None else valid[r // rpm], skip_nan, levels, relative, smooth, gap, min_len,
                                    max_len)
        n_found[r] = len(runs)
        n_spans[r] = min(len(runs), N)
        for i, (lo, hi) in enumerate(runs[:N]):
            windows[r, i] = (lo, hi)
            spans[r, i] = PO.encode(lo, hi, dur)
        smoothed.append(sp)
        Ds.append(D)
    return dict(spans=spans, windows=windows, n_spans=n_spans, n_found=n_found, smoothed=smoothed, D=Ds)


def brute(s, mask_row, vrow, skip_nan, levels, relative, smooth, gap, min_len, max_len):
    """The masked rule judged pair by pair, in the manner of propose_oracle.brute: the smoothed value of a frame is the left fold over the similarities
    its box keeps after the hidden ones are struck out, over how many it keeps; a hidden frame has none and is above nothing; (lo, hi) is a run of
    level l when both end frames are above, no stretch of more than ``gap`` not-above frames - hidden or low alike - lies inside, and the ``gap + 1``
    frames on either side are all not above.  A run goes when ANY higher level has the same pair."""
    dur, D = PO.duration(mask_row)
    s = np.asarray(s, dtype=F)
    h = smooth // 2
    hidden = [(vrow is not None and float(vrow[t]) == 0.0) or (bool(skip_nan) and bool(np.isnan(s[t]))) for t in range(D)]
    sp = np.full(D, np.nan, dtype=F)
    with np.errstate(all="ignore"):
        for t in range(D):
            if hidden[t]:
                continue
            kept = [s[j] for j in range(max(0, t - h), min(D - 1, t + h) + 1) if not hidden[j]]
            acc = kept[0]
            for v in kept[1:]:
                acc = np.add(acc, v, dtype=F)
            sp[t] = np.divide(acc, F(len(kept)), dtype=F)
        T = len(levels)
        above = np.zeros((T, D), dtype=bool)
        if (D > 0 and not np.all(np.isnan(sp))) or not relative:
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
                longest = cur = 0
                for v in ab[lo:hi]:
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


# ------------------------------------------------------------------ shared inputs ------------------------------------------------------------------
def bumpy(R, L, seed):
    """Rows like cosine rows: a slow wave, plateaus and noise, values in about [-0.2, 0.9] (deterministic)."""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(L, dtype=np.float64)[None, :]
    rows = 0.3 + 0.25 * np.sin(t / (7.0 + rng.random((R, 1)) * 23.0) + rng.random((R, 1)) * 6.0) + 0.08 * rng.standard_normal((R, L))
    for r in range(R):
        for _ in range(3):
            a = int(rng.integers(0, L))
            rows[r, a:a + int(rng.integers(1, max(2, L // 6)))] += 0.3
    return rows.astype(F)


def durations(L, Ds):
    return (np.arange(L)[None, :] < np.asarray(Ds)[:, None]).astype(F)


def fixed_spans(R, N, seed):
    """(centre, width) rows that cover short, long, empty, whole-row, negative-end and non-finite spans."""
    rng = np.random.default_rng(2000 + seed)
    sp = np.stack([rng.random((R, N)), rng.random((R, N)) * 0.6], axis=-1).astype(F)
    special = [(0.5, 1.0), (0.5, 2.5), (-0.2, 0.1), (0.5, 0.0), (np.nan, 0.1), (0.3, np.inf), (0.0, 0.01), (1.0, 0.01), (0.25, -0.1)]
    for i, cw in enumerate(special[:N]):
        sp[:, i] = cw
    return sp


def attention_cases():
    """The inputs of the GPU module's attention comparisons: [(name, sims, spans, mask, valid, skip_nan)].  Shared with the host module, which measures
    the float32 statement's own distance from float64 on them."""
    cases = []
    for L, Ds in ((1, [1, 0]), (63, [63, 62]), (64, [64, 1]), (65, [65, 64]), (300, [300, 299]), (1000, [1000, 999])):
        R = 2 * 3
        sims = bumpy(R, L, L)
        mask = durations(L, Ds)
        sims[np.repeat(mask, 3, axis=0) == 0] = np.nan
        valid = np.ones((2, L), dtype=F)
        valid[0, ::2] = 0
        valid[1, L // 3:L // 3 + max(1, L // 5)] = 0
        planted = sims.copy()
        planted[:, 1::7] = np.nan
        spans = fixed_spans(R, 24, L)
        cases.append((f"L{L} valid", sims, spans, mask, valid, 0))
        cases.append((f"L{L} skip_nan", planted, spans, mask, None, 1))
        cases.append((f"L{L} both", planted, spans, mask, valid, 1))
    return cases


def rel_err(a, b):
    """max |a - b| over the entries where b is a number, relative to the largest |b| among them (0 when there is none)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = ~np.isnan(b)
    if not ok.any():
        return 0.0
    scale = np.abs(b[ok]).max()
    return float(np.abs(a[ok] - b[ok]).max() / (scale if scale > 0 else 1.0))
