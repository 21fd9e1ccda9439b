"""rvc_windows_valid, rvc_span_scores_masked_rows and rvc_span_propose_masked_rows (the chain library's entries behind ``ops.windows_valid``,
``ops.span_scores_masked_rows`` / ``ops.span_propose_masked_rows`` and ``eval.similarity``'s ``windows_valid`` / ``ground_queries_in_windows``: the fine
half of the grounding chain run per query inside the windows the coarse half chose) against tests/windows_valid_oracle.py - the rule restated in
numpy with Python loops - and against the entries without ``_rows`` on each row alone.  Everything is compared in integers and bits; nothing here has a
tolerance.  tests/test_windows_valid_host_logic.py holds the oracle itself to a brute-force set union and to both ``cut_windows``.

Every direct call writes into sentinel-filled buffers with 64 elements on either side of each output, at a 16-byte aligned and at an unaligned
address (the zero fill and the count split a row at its 16-byte boundaries).  ``select`` and ``mask`` sit between fences that would change the result
if they were read: window 0 around ``select``, ones around ``mask``.  ``valid_in`` holds NaN - "not hidden" - at every frame no named window covers and
from D on.  The kernels are f32 / i32 only and the chain library has one build, so the kernel items run once (``kdev``); the items that go through the
flavoured libraries (the cosine rows, the ranking) run in both builds (``dev``)."""
import ctypes

import numpy as np
import pytest
import torch

import frames_select_oracle as FO
import spans_masked_oracle as MO
import windows_valid_oracle as VO
from test_gpu_spans_masked import LEVELS, _same_proposals, bits, dev, flav, hide, kdev, run_propose, run_scores, spans_for, up  # noqa: F401

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
F = np.float32
PAD = 64
INT32_MAX = 2 ** 31 - 1
RULES = {VO.SHIFTED: "shifted", VO.CLIPPED: "clipped"}


class Fenced:
    """``n`` elements inside a sentinel-filled buffer, ``off`` elements past a 16-byte boundary."""

    def __init__(self, n, dtype, dev, off=0, fill=None):
        self.n, self.off = n, off
        self.sentinel = -12345 if dtype == torch.int32 else -777.25
        self.buf = torch.full((n + 2 * PAD + off,), self.sentinel if fill is None else fill, dtype=dtype, device=dev)
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + (PAD + self.off) * self.buf.element_size())

    def put(self, x):
        self.buf[PAD + self.off:PAD + self.off + self.n] = torch.from_numpy(np.ascontiguousarray(x).ravel()).to(self.buf.device)
        return self

    def take(self, shape):
        b, a = self.buf.cpu(), PAD + self.off
        assert bool((b[:a] == self.sentinel).all()) and bool((b[a + self.n:] == self.sentinel).all()), "a write outside the output"
        return b[a:a + self.n].reshape(shape).numpy()


def durations(L, Ds):
    return (np.arange(L)[None, :] < np.asarray(Ds)[:, None]).astype(F)


def run_valid(dev, select, mask, valid_in, rule, win, stride, frames, nf, count=True, off=0):
    from revisionllm_amd import hip
    select = np.ascontiguousarray(select, dtype=np.int32)
    R, keep = select.shape
    M, L = mask.shape
    sel = Fenced(R * keep, torch.int32, dev, fill=0).put(select)                        # (a read outside names window 0)
    msk = Fenced(M * L, torch.float32, dev, fill=1.0).put(np.asarray(mask, dtype=F))    # (a read outside lengthens the duration)
    vin = up(dev, valid_in)
    out = Fenced(R * L, torch.float32, dev, off)
    n = Fenced(R, torch.int32, dev) if count else None
    rc = hip.chain_lib().rvc_windows_valid(sel.ptr, msk.ptr, hip.ptr(vin), R, R // M, L, rule, win, stride, frames, nf, keep, out.ptr, n.ptr if count else None,
                                           hip.stream())
    hip.chain_check(rc, "rvc_windows_valid")
    torch.cuda.synchronize()
    return dict(valid=out.take((R, L)), n_valid=n.take((R,)) if count else None)


def poisoned(valid_in, ref, mask, rpm):
    """``valid_in`` with NaN wherever no row of the mask row has a covered frame (and from D on): a value there must not matter."""
    if valid_in is None:
        return None
    v = np.array(valid_in, dtype=F)
    M, L = v.shape
    covered = np.zeros((M, L), bool)
    raw = VO.windows_valid(ref["select"], mask, *ref["geometry"], None)["valid"]
    for r in range(raw.shape[0]):
        covered[r // rpm] |= raw[r] != 0
    v[~covered] = NAN
    return v


def check_valid(dev, select, mask, rule, win, stride, frames=VO.ALL, nf=0, valid_in=None, what=""):
    """With the count and without it, at an aligned and an unaligned output, bit for bit against the oracle -> (got, ref)."""
    select = np.ascontiguousarray(select, dtype=np.int32)
    rpm = select.shape[0] // mask.shape[0]
    valid_in = poisoned(valid_in, dict(select=select, geometry=(rule, win, stride, frames, nf)), mask, rpm)
    ref = VO.windows_valid(select, mask, rule, win, stride, frames, nf, valid_in)
    what = f"{what} R={select.shape[0]} keep={select.shape[1]} L={mask.shape[1]} rule={rule} win={win} stride={stride} frames={frames} F={nf} valid_in={valid_in is not None}"
    got = None
    for count, off in ((True, 0), (False, 0), (True, 1), (True, 3), (False, 2)):
        g = run_valid(dev, select, mask, valid_in, rule, win, stride, frames, nf, count, off)
        a, b = bits(g["valid"]), bits(ref["valid"])
        assert np.array_equal(a, b), (what, count, off, "valid", np.argwhere(a != b)[:6].tolist())
        if count:
            assert np.array_equal(g["n_valid"], ref["n_valid"]), (what, off, "n_valid", g["n_valid"][:8].tolist(), ref["n_valid"][:8].tolist())
        got = got or g
    return got, ref


def some_select(rng, R, keep, cap):
    """Entries from -2 to two past the most windows a row can have: names, padding, duplicates, no order."""
    return rng.integers(-2, cap + 2, (R, keep)).astype(np.int32)


def some_valid_in(rng, M, L):
    return rng.choice(np.array([1.0, 1.0, 0.0, -0.0, NAN, 2.0], dtype=F), (M, L))


# ------------------------------------------------------------------ rows and durations ------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_lengths_and_durations(kdev, L):
    rng = np.random.default_rng(L)
    mask = durations(L, [L, L - 1, 1, 0])
    for rule, win, stride in ((VO.SHIFTED, max(1, L // 5), 1 if L < 4 else 2), (VO.SHIFTED, max(3, L // 3) if L >= 3 else 1, 3 if L >= 3 else 1),
                              (VO.CLIPPED, max(2, L // 6), 2)):
        if win > L or win < stride:
            continue
        cap = FO.capacity(L, win, stride)
        select = some_select(rng, 4, 6, cap)
        for valid_in in (None, some_valid_in(rng, 4, L)):
            got, ref = check_valid(kdev, select, mask, rule, win, stride, valid_in=valid_in, what="lengths")
            assert ref["D"] == [L, L - 1, 1, 0] and not got["valid"][3].any() and not got["valid"][2, 1:].any()
            assert not got["valid"][1, L - 1:].any()                                            # the frame at D stays 0
        check_valid(kdev, select, mask, rule, win, stride, VO.SAMPLED, 7, some_valid_in(rng, 4, L), "lengths, sampled")


def test_a_long_row(kdev):
    L, win, stride = 20000, 625, 5
    rng = np.random.default_rng(2)
    mask = durations(L, [L, L - 1])
    cap = FO.capacity(L, win, stride)
    select = np.sort(rng.choice(cap, (2, 20), replace=False).astype(np.int32), axis=1)
    select[1, -3:] = -1
    valid_in = np.ones((2, L), dtype=F)
    valid_in[:, ::16] = 0
    got, ref = check_valid(kdev, select, mask, VO.SHIFTED, win, stride, valid_in=valid_in, what="long")
    assert all(2000 < n < 20 * (win + 1) for n in ref["n_valid"].tolist())
    check_valid(kdev, select, mask, VO.SHIFTED, win, stride, VO.SAMPLED, 250, None, "long, sampled")
    check_valid(kdev, select, mask, VO.CLIPPED, win, 2, VO.SAMPLED, 250, None, "long, clipped")


@pytest.mark.parametrize("R", [1, 4, 5, 260])
def test_row_counts(kdev, R):
    L, win, stride = 70, 12, 3
    rng = np.random.default_rng(R)
    mask = durations(L, rng.integers(0, L + 1, R))
    select = some_select(rng, R, 5, FO.capacity(L, win, stride))
    check_valid(kdev, select, mask, VO.SHIFTED, win, stride, valid_in=some_valid_in(rng, R, L), what="rows")
    check_valid(kdev, select, mask, VO.CLIPPED, win, 2, VO.SAMPLED, 5, None, what="rows")


def test_three_rows_per_mask_row_and_the_bqk_layout(kdev):
    from revisionllm_amd import ops
    L, B, Q, keep, win, stride = 150, 4, 3, 4, 20, 2
    rng = np.random.default_rng(17)
    mask = durations(L, [150, 149, 64, 1])
    valid_in = some_valid_in(rng, B, L)
    select = some_select(rng, B * Q, keep, FO.capacity(L, win, stride))
    got, ref = check_valid(kdev, select, mask, VO.SHIFTED, win, stride, valid_in=valid_in, what="rpm=3")
    for r in (0, 3, 9):                                                                 # a mask row's rows alone give the same bits
        alone = run_valid(kdev, select[r:r + 3], mask[r // 3:r // 3 + 1], valid_in[r // 3:r // 3 + 1], VO.SHIFTED, win, stride, VO.ALL, 0)
        assert np.array_equal(bits(alone["valid"]), bits(got["valid"][r:r + 3])) and np.array_equal(alone["n_valid"], got["n_valid"][r:r + 3])
    s, m = torch.from_numpy(select).to(kdev).view(B, Q, keep), up(kdev, mask)
    with np.errstate(invalid="ignore"):
        shown = valid_in != 0
    for v, vref in ((torch.from_numpy(valid_in).to(kdev), ref), (torch.from_numpy(shown).to(kdev), None), (torch.from_numpy(shown.astype(np.uint8)).to(kdev), None),
                    (None, None)):
        for mm in (m, m.bool(), m.long()):
            out = ops.windows_valid(s, mm, rule="shifted", win=win, stride=stride, valid=v, return_count=True)
            want = vref or VO.windows_valid(select, mask, VO.SHIFTED, win, stride, VO.ALL, 0, None if v is None else shown.astype(F))
            assert out.valid.shape == (B, Q, L) and out.valid.dtype == torch.float32 and out.n_valid.shape == (B, Q) and out.n_valid.dtype == torch.int32
            assert np.array_equal(bits(out.valid.cpu().numpy().reshape(B * Q, L)), bits(want["valid"]))
            assert np.array_equal(out.n_valid.cpu().numpy().ravel(), want["n_valid"])
    bare = ops.windows_valid(s.view(B * Q, keep), m, rule="shifted", win=win, stride=stride)
    assert bare.n_valid is None and bare.valid.shape == (B * Q, L) and torch.equal(bare.valid.view(torch.int32), out.valid.view(B * Q, L).view(torch.int32))
    sampled = ops.windows_valid(s, m, rule="clipped", win=win, frames="sampled", num_frames=5, return_count=True)
    want = VO.windows_valid(select, mask, VO.CLIPPED, win, 2, VO.SAMPLED, 5)
    assert np.array_equal(bits(sampled.valid.cpu().numpy().reshape(B * Q, L)), bits(want["valid"])) and sampled.n_valid.cpu().numpy().ravel().tolist() == want["n_valid"].tolist()


# ------------------------------------------------------------------ selections ------------------------------------------------------------------
def test_selections(kdev):
    L, win, stride = 300, 40, 4
    mask = durations(L, [300, 211, 300])
    W = [len(FO.windows(D, VO.SHIFTED, win, stride)) for D in (300, 211, 300)]
    assert W == [29, 21, 29]
    rng = np.random.default_rng(5)
    vin = some_valid_in(rng, 3, L)
    one = np.array([[7], [20], [-1]], dtype=np.int32)
    got, ref = check_valid(kdev, one, mask, VO.SHIFTED, win, stride, what="keep=1")
    assert ref["n_valid"].tolist() == [41, 41, 0]
    every = np.stack([np.arange(29), np.arange(29), np.arange(29)]).astype(np.int32)          # keep = W_r; row 1 names 8 windows it does not have
    got, ref = check_valid(kdev, every, mask, VO.SHIFTED, win, stride, valid_in=vin, what="keep=W")
    got, ref = check_valid(kdev, every, mask, VO.SHIFTED, win, stride, what="keep=W")
    assert ref["n_valid"].tolist() == [300, 211, 300]                                            # every window named: every frame of the duration
    wide = np.full((3, 2048), -1, dtype=np.int32)
    wide[0, :5], wide[1, 1000:1003], wide[2, 2047] = [3, 4, 9, 10, 28], [20, 0, 5], 28
    check_valid(kdev, wide, mask, VO.SHIFTED, win, stride, valid_in=vin, what="keep=2048")
    odd = np.array([[-1, -7, 29, INT32_MAX, 5], [21, -2 ** 31, 20, 2048, -1], [INT32_MAX, 29, -1, -7, 30]], dtype=np.int32)
    got, ref = check_valid(kdev, odd, mask, VO.SHIFTED, win, stride, what="entries that name nothing")
    assert ref["n_valid"].tolist() == [41, 41, 0]
    same = check_valid(kdev, np.array([[5, 9, 12]] * 3, np.int32), mask, VO.SHIFTED, win, stride, valid_in=vin)[0]
    for sel in ([[12, 9, 5]], [[9, 9, 5, 12, 5, 5, 12]], [[12, -1, 5, 40, 9, -1]]):                # descending, duplicates, padding in between
        other = check_valid(kdev, np.array(sel * 3, np.int32), mask, VO.SHIFTED, win, stride, valid_in=vin, what=str(sel))[0]
        assert np.array_equal(bits(other["valid"]), bits(same["valid"])) and np.array_equal(other["n_valid"], same["n_valid"])


# ------------------------------------------------------------------ window rules ------------------------------------------------------------------
def test_window_rules(kdev):
    # shifted: the last windows are shifted back to end at D - 1; a win / stride that does not divide; win = L
    for L, D, win, stride in ((100, 100, 30, 3), (100, 93, 30, 3), (100, 100, 10, 3), (97, 97, 25, 7), (64, 64, 64, 2), (64, 63, 64, 4), (50, 50, 50, 50)):
        mask = durations(L, [D])
        wins = FO.windows(D, VO.SHIFTED, win, stride)
        for i in sorted({0, len(wins) // 2, len(wins) - 2, len(wins) - 1} & set(range(len(wins)))):
            got, ref = check_valid(kdev, [[i]], mask, VO.SHIFTED, win, stride, what=f"shifted window {i}")
            assert np.flatnonzero(got["valid"][0]).tolist() == list(range(wins[i][0], wins[i][1]))
        if wins:
            assert wins[-1][1] == D and (len(wins) < 2 or wins[-1][0] == max(0, D - 1 - win))
        check_valid(kdev, [list(range(len(wins) + 1))], mask, VO.SHIFTED, win, stride, VO.SAMPLED, 4, what="shifted, sampled")
    # clipped: even and odd win; win 5 at D 15 has the void window 6 (naming it names nothing), at D 16 window 6 is the one frame [15, 16)
    for L, D, win in ((40, 40, 8), (40, 33, 8), (15, 15, 5), (16, 16, 5), (16, 15, 5), (41, 41, 7), (30, 30, 2)):
        mask = durations(L, [D])
        wins = FO.windows(D, VO.CLIPPED, win, 2)
        for i in sorted({0, len(wins) - 1, len(wins), len(wins) + 1} & set(range(len(wins) + 2))):
            got, ref = check_valid(kdev, [[i]], mask, VO.CLIPPED, win, 2, what=f"clipped window {i}")
            assert np.flatnonzero(got["valid"][0]).tolist() == (list(range(*wins[i])) if i < len(wins) else [])
        check_valid(kdev, [list(range(len(wins) + 2))[::-1]], mask, VO.CLIPPED, win, 2, VO.SAMPLED, 3, what="clipped, sampled")
    assert len(FO.windows(15, VO.CLIPPED, 5, 2)) == 6 and FO.windows(16, VO.CLIPPED, 5, 2)[6] == (15, 16)


def test_bounds_identity(kdev):
    """``valid`` from ``select = [i]`` is ``[bounds[i, 0], bounds[i, 1])`` of the selection's own ``bounds`` cut at D, for every window of a row."""
    from revisionllm_amd import ops
    L = 230
    mask = up(kdev, durations(L, [230, 199]))
    sims = up(kdev, MO.bumpy(2, L, 4))
    for rule, win, stride in (("shifted", 33, 4), ("clipped", 33, None), ("clipped", 24, None)):
        sel = ops.window_select_frames(sims, mask, rule=rule, win=win, stride=stride, keep=3, return_bounds=True)
        Wcap = sel.bounds.shape[1]
        each = torch.arange(Wcap, dtype=torch.int32, device=kdev).view(1, Wcap, 1).expand(2, Wcap, 1).contiguous()
        out = ops.windows_valid(each, mask, rule=rule, win=win, stride=stride, return_count=True)
        b, D, v = sel.bounds.cpu(), [230, 199], out.valid.cpu()
        for r in range(2):
            for i in range(Wcap):
                lo, hi = b[r, i].tolist()
                want = torch.zeros(L)
                if i < int(sel.n_windows[r]):
                    want[lo:min(hi, D[r])] = 1
                assert torch.equal(v[r, i], want) and int(out.n_valid[r, i]) == int(want.sum()), (rule, win, r, i)


# ------------------------------------------------------------------ frame sets and valid_in ------------------------------------------------------------------
def test_sampled_frame_sets(kdev):
    L, win, stride = 700, 300, 5
    mask = durations(L, [700, 651])
    select = np.array([[0, 3, 6], [5, -1, 1]], dtype=np.int32)
    rng = np.random.default_rng(9)
    for nf in (1, 2, 250, 301, 400, 1024):                                               # (a window has 301 frames: 400 and 1024 sample frames twice)
        got, ref = check_valid(kdev, select, mask, VO.SHIFTED, win, stride, VO.SAMPLED, nf, some_valid_in(rng, 2, L) if nf % 2 else None, f"F={nf}")
        check_valid(kdev, select, mask, VO.CLIPPED, win, 2, VO.SAMPLED, nf, None, f"F={nf}")
    assert VO.windows_valid(select, mask, VO.SHIFTED, win, stride, VO.SAMPLED, 1)["n_valid"].tolist() == [3, 2]
    # the linspace ends at hi - 1: with F = 2 the two frames of a window are its first and its last
    got, _ = check_valid(kdev, [[2]], durations(L, [700]), VO.SHIFTED, win, stride, VO.SAMPLED, 2)
    assert np.flatnonzero(got["valid"][0]).tolist() == [120, 420]
    short = durations(40, [40])
    got, _ = check_valid(kdev, [[1, 2]], short, VO.SHIFTED, 6, 2, VO.SAMPLED, 250, what="F far above the window's length")
    assert np.flatnonzero(got["valid"][0]).tolist() == list(range(3, 13))


def test_valid_in_values(kdev):
    """-0.0 and 0.0 hide a frame; NaN, -1, 2 and 1e-45 do not."""
    L, win, stride = 140, 20, 2
    mask = durations(L, [L, 100])
    valid_in = np.resize(np.array([-0.0, NAN, -1.0, 2.0, 1e-45, 0.0, 1.0], dtype=F), (2, L))
    assert valid_in[0, 4] != 0 and np.signbit(valid_in[0, 0])
    every = np.arange(13, dtype=np.int32)[None].repeat(2, 0)
    got, ref = check_valid(kdev, every, mask, VO.SHIFTED, win, stride, valid_in=valid_in, what="valid_in values")
    assert got["valid"][0].tolist() == [0.0 if t % 7 in (0, 5) else 1.0 for t in range(L)] and got["n_valid"][1] == sum(1 for t in range(100) if t % 7 not in (0, 5))
    assert not np.signbit(got["valid"]).any() and set(np.unique(bits(got["valid"])).tolist()) == {0, 0x3f800000}
    check_valid(kdev, every[:, 3:6], mask, VO.SHIFTED, win, stride, VO.SAMPLED, 9, valid_in, "valid_in values, sampled")


# ------------------------------------------------------------------ the _rows entries ------------------------------------------------------------------
def run_scores_rows(dev, sims, spans, mask, valid, rpv, skip, mode, k, tau, full=True):
    from revisionllm_amd import hip
    R, L = sims.shape
    N = spans.shape[1]
    s, p, m, v = up(dev, sims), up(dev, spans), up(dev, mask), up(dev, valid)
    o = dict(scores=Fenced(R * N, torch.float32, dev), windows=Fenced(R * N * 2, torch.int32, dev) if full else None,
             n_usable=Fenced(R * N, torch.int32, dev) if full else None)
    ptr = lambda x: x.ptr if x is not None else None                                            # noqa: E731
    rc = hip.chain_lib().rvc_span_scores_masked_rows(hip.ptr(s), hip.ptr(p), hip.ptr(m), hip.ptr(v), rpv, R, R // mask.shape[0], L, N, mode, k, float(tau), int(skip),
                                                     ptr(o["scores"]), ptr(o["windows"]), ptr(o["n_usable"]), hip.stream())
    hip.chain_check(rc, "rvc_span_scores_masked_rows")
    torch.cuda.synchronize()
    shapes = dict(scores=(R, N), windows=(R, N, 2), n_usable=(R, N))
    return {k_: (x.take(shapes[k_]) if x is not None else None) for k_, x in o.items()}


def run_propose_rows(dev, sims, mask, valid, rpv, skip, levels=LEVELS, relative=1, smooth=1, gap=0, min_len=1, max_len=0, N=64):
    from revisionllm_amd import hip
    R, L = sims.shape
    s, m, v = up(dev, sims), up(dev, mask), up(dev, valid)
    o = dict(spans=Fenced(R * N * 2, torch.float32, dev), n_spans=Fenced(R, torch.int32, dev), n_found=Fenced(R, torch.int32, dev),
             windows=Fenced(R * N * 2, torch.int32, dev), smoothed=Fenced(R * L, torch.float32, dev))
    table = (ctypes.c_float * len(levels))(*levels)
    rc = hip.chain_lib().rvc_span_propose_masked_rows(hip.ptr(s), hip.ptr(m), hip.ptr(v), rpv, R, R // mask.shape[0], L, table, len(levels), relative, smooth, gap,
                                                      min_len, max_len, N, int(skip), o["spans"].ptr, o["n_spans"].ptr, o["n_found"].ptr, o["windows"].ptr,
                                                      o["smoothed"].ptr, hip.stream())
    hip.chain_check(rc, "rvc_span_propose_masked_rows")
    torch.cuda.synchronize()
    shapes = dict(spans=(R, N, 2), n_spans=(R,), n_found=(R,), windows=(R, N, 2), smoothed=(R, L))
    return {k_: x.take(shapes[k_]) for k_, x in o.items()}


def rows_case(B, Q, L, seed):
    """sims [B Q, L] with NaN from D on, NaN / +-inf under each ROW's hidden frames and a few NaN at usable ones; mask [B, L]; a validity row per row and
    one per mask row."""
    rng = np.random.default_rng(seed)
    mask = MO.durations(L, ([L, L - 1, 64, 1] * B)[:B])
    per_row = (rng.random((B * Q, L)) < 0.6).astype(F)
    per_row[0] = 0                                                                      # a row with nothing usable
    per_row[-1] = 1
    per_mask = (rng.random((B, L)) < 0.6).astype(F)
    sims = MO.bumpy(B * Q, L, seed)
    sims[np.repeat(mask, Q, axis=0) == 0] = NAN
    sims[:, 5::13] = NAN
    return sims, mask, per_row, per_mask


def poison(sims, valid):
    out = sims.copy()
    p = np.resize(np.array([NAN, INF, -INF], dtype=F), sims.shape)
    out[valid == 0] = p[valid == 0]
    return out


def same_dict(a, b, what):
    for name in a:
        x, y = a[name], b[name]
        same = np.array_equal(bits(x), bits(y)) if x.dtype == F else np.array_equal(x, y)
        assert same, (what, name)


SCORE_MODES = ((MO.TOPK, 1, 1.0), (MO.TOPK, 3, 1.0), (MO.ATTENTION, 3, 0.01))


@pytest.mark.parametrize("Q", [1, 3])
def test_score_rows_entry_equals_the_existing_entry(kdev, Q):
    B, L, N = 4, 150, 13
    sims, mask, per_row, per_mask = rows_case(B, Q, L, 30 + Q)
    spans = np.concatenate([spans_for(L, int(mask[b].sum()), Q, b)[:, :N] for b in range(B)])
    for mode, k, tau in SCORE_MODES:
        for skip in (0, 1):
            # rpv = rpm: the existing entry, every output
            s = poison(sims, np.repeat(per_mask, Q, axis=0))
            same_dict(run_scores_rows(kdev, s, spans, mask, per_mask, Q, skip, mode, k, tau), run_scores(kdev, s, spans, mask, per_mask, skip, mode, k, tau),
                      ("rpv=rpm", mode, k, skip))
            same_dict(run_scores_rows(kdev, s, spans, mask, None, Q, skip, mode, k, tau), run_scores(kdev, s, spans, mask, None, skip, mode, k, tau),
                      ("valid=NULL", mode, k, skip))
            # rpv = 1: each (b, q) is the existing entry on that row alone, under its video's mask row and its own validity row
            s = poison(sims, per_row)
            got = run_scores_rows(kdev, s, spans, mask, per_row, 1, skip, mode, k, tau)
            bare = run_scores_rows(kdev, s, spans, mask, per_row, 1, skip, mode, k, tau, full=False)
            assert np.array_equal(bits(bare["scores"]), bits(got["scores"]))
            for r in range(B * Q):
                alone = run_scores(kdev, s[r:r + 1], spans[r:r + 1], mask[r // Q:r // Q + 1], per_row[r:r + 1], skip, mode, k, tau)
                same_dict({n: v[r:r + 1] for n, v in got.items()}, alone, ("rpv=1", mode, k, skip, r))
            ref = MO.span_scores(s[:Q], spans[:Q], np.repeat(mask[:1], Q, axis=0), per_row[:Q], skip, mode, k, tau)
            assert np.array_equal(got["n_usable"][:Q], ref["n_usable"]) and (got["n_usable"][0] == 0).all()
            if Q > 1:                                                                   # the rows of a video differ: the row's own validity was read
                assert not np.array_equal(got["n_usable"][1], got["n_usable"][2])


@pytest.mark.parametrize("Q", [1, 3])
def test_propose_rows_entry_equals_the_existing_entry(kdev, Q):
    B, L = 4, 300
    sims, mask, per_row, per_mask = rows_case(B, Q, L, 40 + Q)
    for kw in (dict(smooth=1), dict(smooth=5, gap=2, N=16), dict(smooth=65, gap=63, relative=0, levels=(0.2, 0.4))):
        for skip in (0, 1):
            s = poison(sims, np.repeat(per_mask, Q, axis=0))
            same_dict(run_propose_rows(kdev, s, mask, per_mask, Q, skip, **kw), run_propose(kdev, s, mask, per_mask, skip, **kw), ("rpv=rpm", kw, skip))
            same_dict(run_propose_rows(kdev, s, mask, None, Q, skip, **kw), run_propose(kdev, s, mask, None, skip, **kw), ("valid=NULL", kw, skip))
            s = poison(sims, per_row)
            got = run_propose_rows(kdev, s, mask, per_row, 1, skip, **kw)
            for r in range(B * Q):
                alone = run_propose(kdev, s[r:r + 1], mask[r // Q:r // Q + 1], per_row[r:r + 1], skip, **kw)
                same_dict({n: v[r:r + 1] for n, v in got.items()}, alone, ("rpv=1", kw, skip, r))
            assert got["n_found"][0] == 0                                              # (row 0 has no usable frame)
            if skip or kw["smooth"] == 1:                                               # (else a NaN every 13 frames sits in every smoothing box)
                assert got["n_found"].sum() > 0
            ref = MO.propose(s[:Q], np.repeat(mask[:1], Q, axis=0), kw.get("levels", LEVELS), valid=per_row[:Q], skip_nan=skip,
                             **{"N": 64, **{n: v for n, v in kw.items() if n != "levels"}})
            assert np.array_equal(got["n_found"][:Q], ref["n_found"]) and np.array_equal(got["windows"][:Q], ref["windows"])


def test_the_rows_functions_on_both_layouts(kdev):
    from revisionllm_amd import ops
    B, Q, L, N = 2, 3, 150, 13
    sims, mask, per_row, _ = rows_case(B, Q, L, 50)
    sims = poison(sims, per_row)
    spans = np.concatenate([spans_for(L, int(mask[b].sum()), Q, b)[:, :N] for b in range(B)])
    s, p, m = up(kdev, sims).view(B, Q, L), up(kdev, spans).view(B, Q, N, 2), up(kdev, mask)
    ref = run_scores_rows(kdev, sims, spans, mask, per_row, 1, 1, MO.TOPK, 3, 1.0)
    pref = run_propose_rows(kdev, sims, mask, per_row, 1, 1, smooth=3, gap=1, N=32)
    for v in (torch.from_numpy(per_row).to(kdev), torch.from_numpy(per_row != 0).to(kdev), torch.from_numpy(per_row.astype(np.uint8)).to(kdev),
              torch.from_numpy(per_row).to(kdev).half()):
        v = v.view(B, Q, L)
        out = ops.span_scores_masked_rows(s, p, m.bool(), valid=v, skip_nan=True, return_windows=True, return_usable=True)
        assert isinstance(out, ops.MaskedSpanScores) and out.scores.shape == (B, Q, N) and out.windows.shape == (B, Q, N, 2)
        assert np.array_equal(bits(out.scores.cpu().numpy().reshape(B * Q, N)), bits(ref["scores"]))
        assert np.array_equal(out.windows.cpu().numpy().reshape(B * Q, N, 2), ref["windows"]) and np.array_equal(out.n_usable.cpu().numpy().reshape(B * Q, N), ref["n_usable"])
        prop = ops.span_propose_masked_rows(s, m, valid=v, skip_nan=True, smooth=3, gap=1, max_spans=32, return_windows=True)
        assert isinstance(prop, ops.SpanProposals) and prop.smoothed is None and prop.spans.shape == (B, Q, 32, 2)
        assert np.array_equal(bits(prop.spans.cpu().numpy().reshape(B * Q, 32, 2)), bits(pref["spans"])) and np.array_equal(prop.n_found.cpu().numpy().ravel(), pref["n_found"])
        assert np.array_equal(prop.windows.cpu().numpy().reshape(B * Q, 32, 2), pref["windows"])
    # the [R, L] layout: a mask row per row
    m6 = m.repeat_interleave(Q, 0)
    flat = ops.span_scores_masked_rows(s.view(B * Q, L), p.view(B * Q, N, 2), m6, valid=torch.from_numpy(per_row).to(kdev), skip_nan=True)
    assert flat.windows is None and flat.n_usable is None and np.array_equal(bits(flat.scores.cpu().numpy()), bits(ref["scores"]))
    flat = ops.span_propose_masked_rows(s.view(B * Q, L), m6, valid=torch.from_numpy(per_row).to(kdev), skip_nan=True, smooth=3, gap=1, max_spans=32)
    assert np.array_equal(bits(flat.spans.cpu().numpy()), bits(pref["spans"]))
    # a validity row of ones per row is valid = None of the entry without _rows
    ones = torch.ones(B, Q, L, device=kdev)
    a, b = ops.span_scores_masked_rows(s, p, m, valid=ones, return_usable=True), ops.span_scores_masked(s, p, m, return_usable=True)
    assert torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32)) and torch.equal(a.n_usable, b.n_usable)
    _same_proposals(ops.span_propose_masked_rows(s, m, valid=ones, smooth=3), ops.span_propose_masked(s, m, smooth=3), "ones")
    assert ops.span_scores_masked_rows(s, p[:, :, :0], m, valid=ones).scores.shape == (B, Q, 0)


# ------------------------------------------------------------------ end to end ------------------------------------------------------------------
def movie(B, Q, L, d, seed, distractor=True):
    """Background frames; per (video, query) a TRUE stretch of 40 frames near the query's text and, in another part of the movie, a short distractor of
    5 frames that is nearer still -> text [B, Q, d], video [B, L, d], true [B, Q, 2] and distractor [B, Q, 2] as (first frame, end)."""
    g = torch.Generator().manual_seed(seed)
    text = torch.nn.functional.normalize(torch.randn(B, Q, d, generator=g), dim=-1)
    video = torch.nn.functional.normalize(torch.randn(B, L, d, generator=g), dim=-1)
    true, false = torch.zeros(B, Q, 2), torch.zeros(B, Q, 2)
    for b in range(B):
        for q in range(Q):
            a = 60 + 150 * q + 10 * b
            video[b, a:a + 40] = torch.nn.functional.normalize(text[b, q] + 0.06 * torch.randn(40, d, generator=g), dim=-1)
            true[b, q] = torch.tensor([a, a + 40.0])
            z = a + 75
            if distractor:
                video[b, z:z + 5] = torch.nn.functional.normalize(text[b, q] + 0.01 * torch.randn(5, d, generator=g), dim=-1)
            false[b, q] = torch.tensor([z, z + 5.0])
    return text, video, true, false


def _same_tuple(a, b, what):
    assert type(a) is type(b), what
    for x, y, name in zip(a, b, a._fields):
        assert (x is None) == (y is None), (what, name)
        if x is None:
            continue
        if not torch.is_tensor(x):
            _same_tuple(x, y, (what, name))
            continue
        raw = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t          # noqa: E731
        assert x.shape == y.shape and torch.equal(raw(x), raw(y)), (what, name)


@pytest.mark.parametrize("multi", [False, True])
def test_ground_queries_in_windows_equals_its_stages(dev, multi):
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval.similarity import Grounding, WindowedGrounding, ground_queries_in_windows, ground_queries_masked
    B, Q, L, d, win, stride = 2, 3, 520, 64, 60, 3
    text, video, true, _ = movie(B, Q, L, d, 7, distractor=False)
    if not multi:
        text, true = text[:, 1], true[:, 1]
    t, v = text.to(dev), video.to(hip.op_dtype()).to(dev)
    m = torch.ones(B, L, device=dev)
    m[1, 500:] = 0
    hidden = torch.ones(B, L, dtype=torch.bool, device=dev)
    hidden[:, ::9] = False
    gt = (true / m.sum(-1).cpu().view((-1,) + (1,) * (true.dim() - 1))).to(dev)
    kw = dict(top=5, nms_iou=0.5, smooth=3, gap=1, min_len=2, max_spans=64, return_windows=True)
    sims = (ops.frame_cosine_multi if multi else ops.frame_cosine)(t, v)

    def by_hand(selection, select, frames, nf, valid, skip, gt_):
        wv = ops.windows_valid(select, m, rule="shifted", win=win, stride=stride, frames=frames, num_frames=nf, valid=valid, return_count=True)
        prop = ops.span_propose_masked_rows(sims, m, valid=wv.valid, skip_nan=skip, smooth=3, gap=1, min_len=2, max_spans=64, return_windows=True)
        sc = ops.span_scores_masked_rows(sims, prop.spans, m, valid=wv.valid, skip_nan=skip).scores
        rank = ops.span_rank(sc, prop.spans, top=5, nms_iou=0.5, gt=gt_)
        held = (rank.keep >= 0) & (rank.keep < prop.n_spans.unsqueeze(-1))
        at = rank.keep.clamp(min=0).long()
        nan = torch.full((), NAN, device=dev)
        spans = torch.where(held.unsqueeze(-1), torch.gather(prop.spans, -2, at.unsqueeze(-1).expand(at.shape + (2,))), nan)
        return WindowedGrounding(Grounding(spans, torch.where(held, torch.gather(sc, -1, at), nan), held.sum(-1, dtype=torch.int32), prop, rank), selection,
                                 wv.valid, wv.n_valid)
    # keep: the selection runs here, on the same cosine rows
    for frames, nf, valid, skip, gt_ in (("all", None, None, False, None), ("sampled", 16, hidden, True, gt), ("all", None, hidden.float(), False, gt)):
        got = ground_queries_in_windows(t, v, m, rule="shifted", win=win, stride=stride, keep=4, frames=frames, num_frames=nf, select_k=2, min_sep=2, valid=valid,
                                        skip_nan=skip, gt=gt_, **kw)
        gt_frames = None if gt_ is None else gt_ * m.sum(-1).view((-1,) + (1,) * (gt_.dim() - 1))
        sel = ops.window_select_frames(sims, m, rule="shifted", win=win, stride=stride, keep=4, frames=frames, num_frames=nf, valid=valid, k=2, min_sep=2,
                                       gt=gt_frames)
        _same_tuple(got, by_hand(sel, sel.select, frames, nf, valid, skip, gt_), (frames, nf, skip))
        assert got.selection.n_select.min() >= 1 and int(got.n_valid.min()) > 0 and got.valid.shape == sims.shape
        if gt_ is not None:
            assert bool((got.selection.hit_rank == 0).all())                                # the best window holds frames of the true stretch
    # select: windows from anywhere
    given = torch.tensor([3, 4, -1, 40], dtype=torch.int32, device=dev).expand(tuple(sims.shape[:-1]) + (4,)).contiguous()
    got = ground_queries_in_windows(t, v, m, rule="shifted", win=win, stride=stride, select=given, valid=hidden, skip_nan=True, gt=gt, **kw)
    _same_tuple(got, by_hand(None, given, "all", None, hidden, True, gt), "select")
    assert got.selection is None
    # every window named, every frame of a window, no valid: ground_queries_masked without valid
    W = ops.window_select_capacity("test", L, win, stride)
    every = torch.arange(W, dtype=torch.int32, device=dev).expand(tuple(sims.shape[:-1]) + (W,)).contiguous()
    got = ground_queries_in_windows(t, v, m, rule="shifted", win=win, stride=stride, select=every, gt=gt, **kw)
    assert torch.equal(got.n_valid, m.sum(-1).int().view((-1,) + (1,) * (got.n_valid.dim() - 1)).expand_as(got.n_valid))
    _same_tuple(got.grounding, ground_queries_masked(t, v, m, gt=gt, **kw), "every window")
    xx = torch.stack((got.grounding.spans[..., 0] - got.grounding.spans[..., 1] / 2, got.grounding.spans[..., 0] + got.grounding.spans[..., 1] / 2), -1)
    assert bool(((xx[~torch.isnan(xx)] >= 0) & (xx[~torch.isnan(xx)] <= 1)).all())


def _kept_windows(g):
    """(lo, hi) of every kept place that holds a proposal: [n, 2] with the row of each in front -> list of (row index tuple, lo, hi)."""
    keep, n, win = g.rank.keep.cpu(), g.n_keep.cpu(), g.proposals.windows.cpu()
    out = []
    for idx in np.ndindex(*keep.shape[:-1]):
        for p in range(int(n[idx])):
            lo, hi = win[idx][int(keep[idx][p])].tolist()
            out.append((idx, lo, hi))
    return out


def test_planted_stretches_and_per_query_selections(dev):
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval.similarity import ground_queries, ground_queries_in_windows
    B, Q, L, d, win, stride = 2, 2, 400, 64, 50, 5
    text, video, true, false = movie(B, Q, L, d, 11)
    t, v, m = text.to(dev), video.to(hip.op_dtype()).to(dev), torch.ones(B, L, device=dev)
    kw = dict(top=5, nms_iou=0.5, gap=0, min_len=2, return_windows=True)
    plain = ground_queries(t, v, m, **kw)
    first = plain.proposals.windows.cpu()[torch.arange(B)[:, None], torch.arange(Q)[None, :], plain.rank.keep.cpu()[..., 0].long()]
    assert bool(((first[..., 0] >= false[..., 0] - 1) & (first[..., 1] <= false[..., 1] + 1)).all()), (first, false)       # the distractor ranks first
    # the windows that lie inside [true - 50, true + 60): they cover the true stretch and stay clear of the distractor 75 frames on
    hop = win // stride
    select = torch.full((B, Q, 8), -1, dtype=torch.int32)
    for b in range(B):
        for q in range(Q):
            a = int(true[b, q, 0])
            names = [i for i in range(ops.window_select_capacity("test", L, win, stride)) if i * hop >= a - 50 and i * hop + win + 1 <= a + 60]
            assert 2 <= len(names) <= 8
            select[b, q, :len(names)] = torch.tensor(names, dtype=torch.int32)
    got = ground_queries_in_windows(t, v, m, rule="shifted", win=win, stride=stride, select=select.to(dev), **kw)
    valid = got.valid.cpu()
    for b in range(B):
        for q in range(Q):
            assert not bool(valid[b, q, int(false[b, q, 0]):int(false[b, q, 1])].any()) and bool(valid[b, q, int(true[b, q, 0]):int(true[b, q, 1])].all())
    kept = _kept_windows(got.grounding)
    assert len(kept) >= B * Q and all(bool(valid[idx][lo:hi].all()) for idx, lo, hi in kept)                 # no span touches a frame with valid == 0
    first = got.grounding.proposals.windows.cpu()[torch.arange(B)[:, None], torch.arange(Q)[None, :], got.grounding.rank.keep.cpu()[..., 0].long()].float()
    inter = (torch.minimum(first[..., 1], true[..., 1]) - torch.maximum(first[..., 0], true[..., 0])).clamp(min=0)
    iou = inter / ((first[..., 1] - first[..., 0]) + 40 - inter)
    assert bool((iou > 0.7).all()), iou                                                                    # the true stretch, first
    # per-query selections: the two queries of a video, given disjoint windows, get disjoint answers - also with ONE text for both
    same_text = t[:, :1].expand(B, Q, d).contiguous()
    halves = torch.full((B, Q, 6), -1, dtype=torch.int32)
    halves[:, 0, :6] = torch.arange(0, 6, dtype=torch.int32)                            # frames [0, 101)
    halves[:, 1, :6] = torch.arange(20, 26, dtype=torch.int32)                          # frames [200, 301)
    got = ground_queries_in_windows(same_text, v, m, rule="shifted", win=win, stride=stride, select=halves.to(dev), **kw)
    kept = _kept_windows(got.grounding)
    q0 = [(lo, hi) for idx, lo, hi in kept if idx[1] == 0]
    q1 = [(lo, hi) for idx, lo, hi in kept if idx[1] == 1]
    assert q0 and q1 and all(hi <= 101 for _, hi in q0) and all(200 <= lo and hi <= 301 for lo, hi in q1)
    assert got.n_valid.cpu().tolist() == [[101, 101]] * B and not bool((got.valid[:, 0] * got.valid[:, 1]).any())


def test_the_windowed_calls_do_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the calls: with the stream kept busy by work queued before them, an event recorded just before
    has not completed when they return."""
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval.similarity import ground_queries_in_windows, windows_valid
    B, Q, L, d, win, stride = 2, 3, 520, 64, 60, 3
    text, video, true, _ = movie(B, Q, L, d, 8)
    t, v, m = text.to(dev), video.to(hip.op_dtype()).to(dev), torch.ones(B, L, device=dev)
    hidden = torch.ones(B, L, dtype=torch.bool, device=dev)
    hidden[:, ::16] = False
    gt = (true / L).to(dev)
    given = torch.tensor([3, 4, -1, 40], dtype=torch.int32, device=dev).expand(B, Q, 4).contiguous()
    rows = ops.frame_cosine_multi(t, v)

    def calls():
        a = ground_queries_in_windows(t, v, m, rule="shifted", win=win, stride=stride, keep=4, frames="sampled", num_frames=16, valid=hidden, skip_nan=True, gt=gt,
                                      top=5, smooth=3, gap=1)
        b = ground_queries_in_windows(t[:, 0], v, m.bool(), rule="clipped", win=win, select=given[:, 0].contiguous(), top=5)
        w = windows_valid(given, m, rule="shifted", win=win, stride=stride, valid=hidden, return_count=True)
        p = ops.span_propose_masked_rows(rows, m, valid=w.valid.bool(), smooth=3)
        s = ops.span_scores_masked_rows(rows, p.spans, m, valid=w.valid, return_usable=True)
        return (a.grounding.spans, a.grounding.scores, a.selection.select, a.selection.hit_rank, a.valid, a.n_valid, b.grounding.spans, b.n_valid, w.valid, w.n_valid,
                p.spans, s.scores, s.n_usable)
    want = calls()                                                                     # (warm: libraries loaded, allocator blocks cached)
    a = torch.ones(8192, 8192, device=dev)
    c = torch.empty_like(a)
    torch.mm(a, a, out=c)
    torch.cuda.synchronize()
    for _ in range(12):                                                                # ~1.1 TFLOP of f32 each: tens of milliseconds of queued work
        torch.mm(a, a, out=c)
    ev = torch.cuda.Event()
    ev.record()
    got = calls()
    still_busy = not ev.query()
    torch.cuda.synchronize()
    assert still_busy, "the windowed calls returned only after the work queued before them had finished: they synchronised"
    raw = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int16) if x.dtype.itemsize == 2 else x      # noqa: E731
    for x, y in zip(got, want):
        assert torch.equal(raw(x), raw(y))
