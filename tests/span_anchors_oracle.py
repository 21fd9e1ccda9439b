"""The rule of ``rvc_span_anchors`` (include/revision_hip_chain.h) a second time in numpy: float32 for the duration and the span encoding, int64 sums,
float64 scores, Python loops over the anchors.  ``anchors`` is what tests/test_gpu_span_anchors.py compares the kernel with; it takes its sums from
prefix arrays and walks the peak and capacity rules as loops.  ``brute=True`` states the rule independently - every S and C recomputed from scratch per
anchor, the peak and capacity orders written as sort keys - and tests/test_span_anchors_host_logic.py holds ``anchors`` to it.  Duration, usable frames,
quantisation and encoding are tests/span_refine_oracle.py's (the two kernels state them separately; the oracles share one statement, and the round-trip
tests hold each kernel to ``rv_span_scores``).  Nothing here is used by the package."""
import numpy as np

import span_refine_oracle as RO

F = np.float32
QNAN = RO.QNAN
MEAN, CONTRAST = 0, 1


def anchor_starts(D, length, stride):
    """The starts of one scale's anchors over D frames: i * stride while the anchor fits and, where that leaves frames over, D - length."""
    if length > D:
        return []
    starts = list(range(0, D - length + 1, stride))
    if (D - length) % stride != 0:
        starts.append(D - length)
    return starts


def _scores_prefix(s, vrow, D, starts, length, margin, mode, min_usable):
    """J (float64) or None per anchor, from prefix arrays."""
    u = RO.usable(s, vrow, D)
    q = np.where(u, RO.quantise(np.where(u, np.asarray(s, dtype=F), F(0))), 0)
    PS = np.concatenate([[0], np.cumsum(q)]).astype(np.int64)
    PC = np.concatenate([[0], np.cumsum(u.astype(np.int64))])
    out = []
    for a in starts:
        b = a + length
        Cin = PC[b] - PC[a]
        if Cin < min_usable:
            out.append(None)
            continue
        if mode == MEAN:
            out.append(np.float64(PS[b] - PS[a]) / np.float64(Cin))
            continue
        x, y = max(0, a - margin), min(D, b + margin)
        Cout = (PC[a] - PC[x]) + (PC[y] - PC[b])
        out.append(RO.contrast(PS[b] - PS[a], Cin, (PS[a] - PS[x]) + (PS[y] - PS[b]), Cout) if Cout > 0 else None)
    return out


def _scores_brute(s, vrow, D, starts, length, margin, mode, min_usable):
    """The same with nothing shared between anchors: each S and C is a fresh sum over its own interval."""
    s = np.asarray(s, dtype=F)

    def frames(x, y):
        seg = s[x:y]
        with np.errstate(invalid="ignore"):
            ok = ~np.isnan(seg) if vrow is None else (~np.isnan(seg) & ~(np.asarray(vrow[x:y], dtype=F) == F(0)))
        vals = np.rint((np.clip(seg[ok], F(-1), F(1)) * F(16777216.0)).astype(np.float64)).astype(np.int64)
        return int(vals.sum()), int(ok.sum())
    out = []
    for a in starts:
        b = a + length
        Sin, Cin = frames(a, b)
        if Cin < min_usable:
            out.append(None)
        elif mode == MEAN:
            out.append(np.float64(Sin) / np.float64(Cin))
        else:
            S1, C1 = frames(max(0, a - margin), a)
            S2, C2 = frames(b, min(D, b + margin))
            out.append(np.float64(Sin) / np.float64(Cin) - np.float64(S1 + S2) / np.float64(C1 + C2) if C1 + C2 > 0 else None)
    return out


def anchors_row(s, vrow, dur, L, scales, mode, peak, min_usable, max_spans, brute=False):
    """One row -> (spans f32 [N,2], scores f32 [N], n_spans, n_found, windows i64 [N,2], scale i64 [N])."""
    N = max_spans
    spans = np.full((N, 2), QNAN, dtype=F)
    scores = np.full(N, QNAN, dtype=F)
    win = np.full((N, 2), -1, dtype=np.int64)
    scl = np.full(N, -1, dtype=np.int64)
    D = RO.duration_frames(dur, L)
    peaks = []                                            # (J, scale, index, a, b)
    for k, (length, stride, margin) in enumerate(scales):
        starts = anchor_starts(D, length, stride)
        J = (_scores_brute if brute else _scores_prefix)(s, vrow, D, starts, length, margin, mode, min_usable)
        if brute:
            order = sorted((i for i in range(len(starts)) if J[i] is not None), key=lambda i: (-J[i], i))
            place = {i: p for p, i in enumerate(order)}
            for i in order:
                if not any(j != i and abs(j - i) <= peak and place[j] < place[i] for j in order):
                    peaks.append((J[i], k, i, starts[i], starts[i] + length))
        else:
            for i in range(len(starts)):
                if J[i] is None:
                    continue
                beaten = False
                for j in range(max(0, i - peak), min(len(starts) - 1, i + peak) + 1):
                    if j != i and J[j] is not None and (J[j] > J[i] or (J[j] == J[i] and j < i)):
                        beaten = True
                        break
                if not beaten:
                    peaks.append((J[i], k, i, starts[i], starts[i] + length))
    n_found = len(peaks)
    if n_found > N:
        if brute:
            kept = sorted(sorted(peaks, key=lambda p: (-p[0], p[1], p[2]))[:N], key=lambda p: (p[1], p[2]))
        else:
            # the N-th largest score, everything above it, and the first of those equal to it
            cut = sorted((p[0] for p in peaks), reverse=True)[N - 1]
            room = N - sum(1 for p in peaks if p[0] > cut)
            kept = []
            for p in sorted(peaks, key=lambda p: (p[1], p[2])):
                if p[0] > cut:
                    kept.append(p)
                elif p[0] == cut and room > 0:
                    kept.append(p)
                    room -= 1
    else:
        kept = sorted(peaks, key=lambda p: (p[1], p[2]))
    for n, (j, k, i, a, b) in enumerate(kept):
        spans[n] = RO.encode(a, b, dur)
        scores[n] = F(j)
        win[n] = (a, b)
        scl[n] = k
    return spans, scores, len(kept), n_found, win, scl


def normal_scales(scales):
    """ints, (len, stride) or (len, stride, margin) -> triples, with the defaults of ``ops.span_anchors``."""
    out = []
    for sc in scales:
        sc = (sc,) if isinstance(sc, (int, np.integer)) else tuple(sc)
        length = int(sc[0])
        stride = int(sc[1]) if len(sc) > 1 else max(1, length // 4)
        margin = int(sc[2]) if len(sc) > 2 else max(1, length // 2)
        out.append((length, stride, margin))
    return out


def anchors(sims, mask, valid, rpv, scales, mode=CONTRAST, peak=2, min_usable=1, max_spans=256, brute=False):
    """sims [R,L], mask [R / rpm, L] of 0 / 1, valid [R / rpv, L] or None -> dict(spans f32 [R,N,2], scores f32 [R,N], n_spans i64 [R], n_found i64 [R],
    windows i64 [R,N,2], scale i64 [R,N])."""
    sims = np.asarray(sims, dtype=F)
    mask = np.asarray(mask, dtype=F)
    R, L = sims.shape
    rpm = R // mask.shape[0]
    scales = normal_scales(scales)
    rows = [anchors_row(sims[r], None if valid is None else np.asarray(valid, dtype=F)[r // rpv], RO.mask_sum(mask[r // rpm]), L, scales, mode, peak,
                        min_usable, max_spans, brute) for r in range(R)]
    return dict(spans=np.stack([x[0] for x in rows]), scores=np.stack([x[1] for x in rows]), n_spans=np.array([x[2] for x in rows], dtype=np.int64),
                n_found=np.array([x[3] for x in rows], dtype=np.int64), windows=np.stack([x[4] for x in rows]), scale=np.stack([x[5] for x in rows]))


def planted_rows():
    """The 50 rows of the issue behind this generator: 0.02 noise, a 40-frame plateau of +0.2 and one frame at 1.0 away from it -> (sims [50,1000],
    plateau starts [50])."""
    rng = np.random.default_rng(0)
    rows, los = [], []
    for _ in range(50):
        s = (0.02 * rng.standard_normal(1000)).astype(F)
        lo = 10 * int(rng.integers(10, 80))
        s[lo:lo + 40] += F(0.2)
        while True:
            p = int(rng.integers(0, 1000))
            if not lo - 60 <= p < lo + 100:
                break
        s[p] = 1.0
        rows.append(s)
        los.append(lo)
    return np.stack(rows), np.array(los)


PLANTED_SCALES = ((20, 5, 10), (40, 10, 20), (80, 20, 40))
