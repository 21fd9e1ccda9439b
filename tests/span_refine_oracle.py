"""The rule of ``rvc_span_refine`` (include/revision_hip_chain.h) a second time in numpy: float32 for the window rule, the quantisation and the span
encoding, int64 sums, float64 contrasts, Python loops over the candidates.  ``refine`` is what tests/test_gpu_span_refine.py compares the kernel with;
it takes its sums from prefix arrays.  ``brute`` states the choice independently - every S and C recomputed from scratch per candidate, the order
written as a sort key - and tests/test_span_refine_host_logic.py holds ``refine`` to it.  Nothing here is used by the package."""
import math

import numpy as np

F = np.float32
NAN_BITS = 0x7fc00000
QNAN = np.uint32(NAN_BITS).view(F)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
XX, CXW = 0, 1


def duration_frames(dur, L):
    """D = min(L, floor(dur)); none for a sum that is not finite or below 1."""
    dur = F(dur)
    if not (np.isfinite(dur) and dur >= F(1)):
        return 0
    return L if dur >= F(L) else int(math.floor(float(dur)))


def _sat(v):
    return int(min(max(float(v), I32_MIN), I32_MAX))


def window(u, v, form, dur, L):
    """The span (u, v) -> (lo, hi) of ``rv_span_scores``' rule over the array length L, or None for a non-finite scaled bound."""
    u, v, dur = F(u), F(v), F(dur)
    with np.errstate(all="ignore"):
        if form == CXW:
            hw = F(F(0.5) * v)
            x1, x2 = F(u - hw), F(u + hw)
        else:
            x1, x2 = u, v
        p1, p2 = F(x1 * dur), F(x2 * dur)
    if not (np.isfinite(p1) and np.isfinite(p2)):
        return None
    start = max(0, _sat(np.floor(p1)))
    end = _sat(np.ceil(p2))
    lo = min(start, L)
    hi = max(end + L, 0) if end < 0 else min(end, L)
    return lo, hi


def quantise(s):
    """f32 similarities -> int64 q = rint(clamp(s, -1, 1) * 2^24) (exact product, ties to even); 0 where s is NaN (such a frame is never usable)."""
    s = np.asarray(s, dtype=F)
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(s, F(-1)), F(1))
        p = c * F(16777216.0)
    assert p.dtype == F
    return np.where(np.isnan(p), 0, np.rint(np.where(np.isnan(p), F(0), p).astype(np.float64))).astype(np.int64)


def usable(s, vrow, D):
    """Frame t < D is usable when valid is None or valid[t] != 0 (f32: -0 hides, NaN does not) and s[t] is a number."""
    s = np.asarray(s, dtype=F)
    u = np.zeros(len(s), dtype=bool)
    with np.errstate(invalid="ignore"):
        u[:D] = (s[:D] == s[:D]) if vrow is None else ((np.asarray(vrow, dtype=F)[:D] != F(0)) & (s[:D] == s[:D]))
    return u


def contrast(Sin, Cin, Sout, Cout):
    """J in float64, the two divisions and the subtraction rounded each on its own."""
    return np.float64(Sin) / np.float64(Cin) - np.float64(Sout) / np.float64(Cout)


def encode(a, b, dur):
    """``rv_span_propose``'s (centre, width) of the window [a, b)."""
    dur = F(dur)
    with np.errstate(all="ignore"):
        return F(F(F(F(a) + F(b)) * F(0.5)) / dur), F(F(F(F(b) - F(a)) - F(0.5)) / dur)


def candidates(lo0, hi0, D, radius, min_len):
    for a in range(max(0, lo0 - radius), min(lo0 + radius, D - 1) + 1):
        for b in range(max(1, hi0 - radius), min(hi0 + radius, D) + 1):
            if b - a >= min_len or (a, b) == (lo0, hi0):
                yield a, b


def refine_row(s, vrow, dur, L, spans, form, radius, margin, min_len, choose=None):
    """One row -> (out_spans f32 [N,2], windows i64 [N,2], contrast f32 [N], contrast0 f32 [N])."""
    N = len(spans)
    out = np.full((N, 2), QNAN, dtype=F)
    win = np.full((N, 2), -1, dtype=np.int64)
    con = np.full(N, QNAN, dtype=F)
    con0 = np.full(N, QNAN, dtype=F)
    D = duration_frames(dur, L)
    u = usable(s, vrow, D)
    q = np.where(u, quantise(np.where(u, np.asarray(s, dtype=F), F(0))), 0)
    PS = np.concatenate([[0], np.cumsum(q)]).astype(np.int64)
    PC = np.concatenate([[0], np.cumsum(u.astype(np.int64))])

    def J(a, b):
        x, y = max(0, a - margin), min(D, b + margin)
        Cin, Cout = PC[b] - PC[a], (PC[a] - PC[x]) + (PC[y] - PC[b])
        if not (Cin > 0 and Cout > 0):
            return None
        return contrast(PS[b] - PS[a], Cin, (PS[a] - PS[x]) + (PS[y] - PS[b]), Cout)
    for n in range(N):
        w = window(spans[n][0], spans[n][1], form, dur, L)
        if w is None:
            continue
        lo0, hi0 = min(w[0], D), min(w[1], D)
        if hi0 <= lo0:
            continue
        if choose is not None:
            a, b, j, j0 = choose(s, vrow, D, lo0, hi0, radius, margin, min_len)
        else:
            best = None
            for a, b in candidates(lo0, hi0, D, radius, min_len):
                j = J(a, b)
                if j is None:
                    continue
                d = abs(a - lo0) + abs(b - hi0)
                if best is None or j > best[0] or (j == best[0] and (d, a, b) < best[1:]):
                    best = (j, d, a, b)
            j0 = J(lo0, hi0)
            a, b, j = (best[2], best[3], best[0]) if best is not None else (lo0, hi0, None)
        win[n] = (a, b)
        out[n] = encode(a, b, dur)
        con[n] = QNAN if j is None else F(j)
        con0[n] = QNAN if j0 is None else F(j0)
    return out, win, con, con0


def brute_choice(s, vrow, D, lo0, hi0, radius, margin, min_len):
    """The choice for one span with nothing shared between candidates: each S and C is a fresh Python sum over its own interval, and the order is one
    sort key (-J, distance, a, b) -> (a, b, J or None, J of the original pair or None)."""
    s = np.asarray(s, dtype=F)

    def frames(x, y):
        seg = s[x:y]
        with np.errstate(invalid="ignore"):
            ok = ~np.isnan(seg) if vrow is None else (~np.isnan(seg) & ~(np.asarray(vrow[x:y], dtype=F) == F(0)))
        vals = np.rint((np.clip(seg[ok], F(-1), F(1)) * F(16777216.0)).astype(np.float64)).astype(np.int64)
        return int(vals.sum()), int(ok.sum())

    def J(a, b):
        Sin, Cin = frames(a, b)
        S1, C1 = frames(max(0, a - margin), a)
        S2, C2 = frames(b, min(D, b + margin))
        if Cin <= 0 or C1 + C2 <= 0:
            return None
        return float(np.float64(Sin) / np.float64(Cin) - np.float64(S1 + S2) / np.float64(C1 + C2))
    found = []
    for a in range(0, D):
        for b in range(1, D + 1):
            if abs(a - lo0) > radius or abs(b - hi0) > radius:
                continue
            if b - a < min_len and (a, b) != (lo0, hi0):
                continue
            j = J(a, b)
            if j is not None:
                found.append((-j, abs(a - lo0) + abs(b - hi0), a, b))
    j0 = J(lo0, hi0)
    if not found:
        return lo0, hi0, None, j0
    mj, _, a, b = min(found)
    return a, b, -mj, j0


def mask_sum(mask_row):
    """The duration of a 0 / 1 mask row: exact in f32 whatever the order."""
    return F(np.asarray(mask_row, dtype=F).sum(dtype=np.float64))


def refine(sims, spans, form, mask, valid, rpv, radius, margin, min_len=1, brute=False):
    """sims [R,L], spans [R,N,2], mask [R / rpm, L] of 0 / 1, valid [R / rpv, L] or None -> dict(spans f32 [R,N,2], windows i64 [R,N,2], contrast f32
    [R,N], contrast0 f32 [R,N])."""
    sims = np.asarray(sims, dtype=F)
    spans = np.asarray(spans, dtype=F)
    mask = np.asarray(mask, dtype=F)
    R, L = sims.shape
    rpm = R // mask.shape[0]
    rows = [refine_row(sims[r], None if valid is None else np.asarray(valid, dtype=F)[r // rpv], mask_sum(mask[r // rpm]), L, spans[r], form, radius, margin,
                       min_len, brute_choice if brute else None) for r in range(R)]
    return dict(spans=np.stack([x[0] for x in rows]), windows=np.stack([x[1] for x in rows]), contrast=np.stack([x[2] for x in rows]),
                contrast0=np.stack([x[3] for x in rows]))
