"""rv_window_select (the kernel behind ``ops.window_select`` / ``eval.similarity.select_windows`` / ``eval.stage2.clip_grounding_windows``: the
recursion's windows chosen from a cosine row in one launch) against tests/window_oracle.py, the rule restated in numpy float32 with Python loops.  The
oracle IS the rule, so ``select``, ``n_select``, ``n_windows``, ``bounds``, ``order`` and ``hit_rank`` must be equal and ``win_scores`` must have the
oracle's bits; no case is left out and there is no tolerance.  tests/test_window_host_logic.py holds the oracle itself to a brute-force statement of
the selection and to ``stage2.cut_windows``.

Every direct call writes into buffers with 64 sentinel elements on either side of each output; the surroundings are compared bitwise.  In every case
the frames of ``sims`` from D on are NaN: a read past the duration would show in a score.  Every case runs twice: with every optional output (the
greedy walk then runs over all windows) and with none (the walk stops at ``keep`` taken); ``select`` must not change.  The kernel is f32 only, and
the module runs in both builds because each library carries its own copy of it."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import window_oracle as WO
from helpers import fl

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")
PAD = 64
NAN, INF = float("nan"), float("inf")
F = np.float32


@pytest.fixture(scope="module", params=[None] if _FORCED else ["f16", "bf16"])
def flav(request, op_flavour):
    from revisionllm_amd import hip
    f = request.param or op_flavour or hip.flavour()
    prev = hip.set_flavour(f)
    yield f
    hip.set_flavour(prev)


@pytest.fixture(scope="module")
def dev(flav):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


# ------------------------------------------------------------------ running the entry ------------------------------------------------------------------
class _Guarded:
    """An output of ``n`` elements inside a sentinel-filled buffer."""

    def __init__(self, n, dtype, dev):
        self.n = n
        self.sentinel = -12345 if dtype == torch.int32 else -777.25
        self.buf = torch.full((n + 2 * PAD,), self.sentinel, dtype=dtype, device=dev)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + PAD * self.buf.element_size())

    def take(self, shape):
        b = self.buf.cpu()
        assert bool((b[:PAD] == self.sentinel).all()) and bool((b[PAD + self.n:] == self.sentinel).all()), "a write outside the output"
        return b[PAD:PAD + self.n].reshape(shape).numpy()


def durations(L, Ds):
    return (np.arange(L)[None, :] < np.asarray(Ds)[:, None]).astype(F)


def fenced(sims, mask):
    """The rows with NaN from each row's duration on (mask [R / rpm, L] of 0 / 1 prefixes)."""
    sims = np.array(sims, dtype=F)
    rpm = sims.shape[0] // mask.shape[0]
    sims[np.repeat(mask, rpm, axis=0) == 0] = NAN
    return sims


def run(dev, sims, mask, win, stride, k, keep, min_sep, gt=None, full=True):
    """The C entry on numpy inputs -> dict like the oracle's (parts not asked for: None), after the sentinel checks."""
    from revisionllm_amd import hip
    R, L = sims.shape
    M = mask.shape[0]
    Wcap = WO.capacity(L, win, stride)
    s = torch.from_numpy(np.ascontiguousarray(sims, dtype=F)).to(dev)
    m = torch.from_numpy(np.ascontiguousarray(mask, dtype=F)).to(dev)
    g = torch.from_numpy(np.ascontiguousarray(gt, dtype=F)).to(dev) if gt is not None else None
    o = dict(select=_Guarded(R * keep, torch.int32, dev), n_select=_Guarded(R, torch.int32, dev), n_windows=_Guarded(R, torch.int32, dev),
             win_scores=_Guarded(R * Wcap, torch.float32, dev) if full else None, bounds=_Guarded(M * Wcap * 2, torch.int32, dev) if full else None,
             order=_Guarded(R * Wcap, torch.int32, dev) if full else None, hit_rank=_Guarded(R, torch.int32, dev) if full and gt is not None else None)
    ptr = lambda x: x.ptr if x is not None else None                                            # noqa: E731
    rc = hip.lib().rv_window_select(hip.ptr(s), hip.ptr(m), R, R // M, L, win, stride, k, keep, min_sep, Wcap, hip.ptr(g) if o["hit_rank"] else None,
                                    ptr(o["select"]), ptr(o["n_select"]), ptr(o["n_windows"]), ptr(o["win_scores"]), ptr(o["bounds"]), ptr(o["order"]),
                                    ptr(o["hit_rank"]), hip.stream())
    hip.check(rc, "rv_window_select")
    torch.cuda.synchronize()
    shapes = dict(select=(R, keep), n_select=(R,), n_windows=(R,), win_scores=(R, Wcap), bounds=(M, Wcap, 2), order=(R, Wcap), hit_rank=(R,))
    return {k_: (v.take(shapes[k_]) if v is not None else None) for k_, v in o.items()}


def same(got, ref, what=""):
    for k_ in ("select", "n_select", "n_windows", "bounds", "order", "hit_rank"):
        if got[k_] is not None:
            assert np.array_equal(got[k_], ref[k_]), (what, k_, np.argwhere(got[k_] != ref[k_])[:4].tolist())
    if got["win_scores"] is not None:
        a, b = got["win_scores"].view(np.uint32), np.ascontiguousarray(ref["win_scores"]).view(np.uint32)
        assert np.array_equal(a, b), (what, "win_scores", np.argwhere(a != b)[:4].tolist())


@functools.lru_cache(maxsize=None)
def _oracle(sims_b, sims_shape, mask_b, mask_shape, gt_b, params):
    """The oracle once per distinct case: both builds' runs share it."""
    sims = np.frombuffer(sims_b, dtype=F).reshape(sims_shape)
    mask = np.frombuffer(mask_b, dtype=F).reshape(mask_shape)
    gt = np.frombuffer(gt_b, dtype=F).reshape(sims_shape[0], 2) if gt_b is not None else None
    return WO.select(sims, mask, *params, gt=gt)


def check(dev, sims, mask, win, stride, k=3, keep=5, min_sep=1, gt=None, what=""):
    """Fence, run with every output and with none, compare both with the oracle -> (got, ref)."""
    sims = fenced(sims, mask)
    Wcap = WO.capacity(sims.shape[1], win, stride)
    keep, min_sep = min(keep, Wcap), min(min_sep, Wcap)
    gt = np.ascontiguousarray(gt, dtype=F) if gt is not None else None
    ref = _oracle(sims.tobytes(), sims.shape, mask.tobytes(), mask.shape, gt.tobytes() if gt is not None else None, (win, stride, k, keep, min_sep))
    got = run(dev, sims, mask, win, stride, k, keep, min_sep, gt)
    same(got, ref, what)
    same(run(dev, sims, mask, win, stride, k, keep, min_sep, None, full=False), ref, what + " (select only)")
    return got, ref


def bumpy(R, L, seed):
    """Rows as a cosine row looks: a few raised stretches of several heights on noise."""
    rng = np.random.default_rng(seed)
    s = rng.normal(0.0, 0.05, (R, L)).astype(F)
    for r in range(R):
        for _ in range(int(rng.integers(1, 6))):
            a = int(rng.integers(0, L))
            s[r, a:a + int(rng.integers(1, max(2, L // 4)))] += F(rng.choice([0.3, 0.5, 0.8, 1.0]))
    return s


def spans_gt(R, L, seed):
    """Ground truths in frames around [0, L): most solid, some outside, some void."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-5, L + 5, R).astype(F)
    gt = np.stack([a, a + rng.integers(-1, max(2, L // 3), R).astype(F)], axis=1)
    return gt


# ------------------------------------------------------------------ sizes and layouts ------------------------------------------------------------------
@pytest.mark.parametrize("L", [10, 11, 12, 64, 128, 129, 130, 131, 132, 133, 300])
@pytest.mark.parametrize("geometry", [(8, 4), (10, 4)])
def test_sizes(dev, geometry, L):
    """hop = 2 in both geometries, (10, 4) with starts that are no multiple of it: D = L, L - 1, win, win + 1, 1 and 0; W_r = 0, 1, 63, 64, 65 among them."""
    win, stride = geometry
    Ds = [L, L - 1, win, min(win + 1, L), 1, 0]
    _, ref = check(dev, bumpy(6, L, L), durations(L, Ds), win, stride, keep=5, min_sep=2, gt=spans_gt(6, L, L), what=f"L={L}")
    assert ref["D"] == Ds and ref["n_windows"].tolist() == [max(0, -(-D // 2) - 1) for D in Ds]
    assert ref["n_windows"][4] == ref["n_windows"][5] == 0 and ref["n_windows"][2] == win // 2 - 1
    if L in (128, 130, 132):
        assert ref["n_windows"][0] == L // 2 - 1 in (63, 64, 65)


def test_the_cap(dev):
    """W_r = 2048 (hop = 1) with the longest greedy walk (keep = W_r, min_sep = 2), and the geometry win = 2, stride = 1, L = 2049 (hop = 2, W_r = 1024)."""
    L = 2049
    sims = bumpy(2, L, 7)
    _, ref = check(dev, sims, durations(L, [L, L - 1]), 2, 2, k=2, keep=2048, min_sep=2, gt=np.array([[2047.5, 2048.0], [5.0, 6.0]]), what="cap")
    assert ref["n_windows"].tolist() == [2048, 2047] and ref["n_select"].tolist() == [2048, 2047] and WO.capacity(L, 2, 2) == 2048
    check(dev, sims, durations(L, [L, 700]), 2, 2, k=1, keep=100, min_sep=1, what="cap, min_sep 1")
    _, ref = check(dev, sims, durations(L, [L, L - 1]), 2, 1, k=3, keep=1024, min_sep=5, gt=np.array([[0.0, 1.0], [2047.0, 2048.0]]), what="stride 1")
    assert ref["n_windows"].tolist() == [1024, 1023]


@pytest.mark.parametrize("win,stride,L", [(70, 5, 300), (130, 5, 300), (130, 1, 131), (625, 5, 3000), (1023, 3, 2100), (1024, 3, 2100), (1100, 5, 1500)])
def test_long_windows(dev, win, stride, L):
    """Windows longer than one and two lane strides, the driver's geometry, and windows of 1024 frames (the last that a wave holds in registers), 1025
    and more (read again from the row in every round)."""
    Ds = [L, L - 1, win + 1, (L + win) // 2]
    for k in (1, 3, 64):
        _, ref = check(dev, bumpy(4, L, win + k), durations(L, Ds), win, stride, k=k, keep=4, min_sep=2, gt=spans_gt(4, L, k), what=f"win={win} k={k}")
    assert ref["n_windows"][0] == WO.capacity(L, win, stride) == {70: 21, 130: 11 if stride == 5 else 1, 625: 23, 1023: 6, 1024: 6, 1100: 6}[win]


@pytest.mark.parametrize("k", [1, 2, 3, 7, 9, 64])
def test_k_around_and_above_the_window_length(dev, k):
    """win = 8: windows of 9 frames, and a shorter first window when D is small; k above the length sums the whole window."""
    L = 40
    _, ref = check(dev, bumpy(3, L, k), durations(L, [40, 9, 5]), 8, 4, k=k, keep=6, what=f"k={k}")
    assert ref["bounds"][0, 0].tolist() == [0, 9] and ref["bounds"][2, 0].tolist() == [0, 5] and ref["n_windows"].tolist() == [19, 4, 2]


@pytest.mark.parametrize("keep", [1, 5, 19, 30, 39])
def test_keep(dev, keep):
    """keep = 1, 5, W_r, above W_r (rows of 40 and 80 frames in a buffer of 80: W_r = 19 and 39)."""
    L = 80
    for min_sep in (1, 3):
        got, ref = check(dev, bumpy(2, L, keep), durations(L, [40, 80]), 8, 4, keep=keep, min_sep=min_sep, what=f"keep={keep}")
        assert ref["n_select"].tolist() == [min(keep, 19), min(keep, 39)]
        for r in range(2):
            n = int(ref["n_select"][r])
            assert (got["select"][r, n:] == -1).all() and (np.diff(got["select"][r, :n]) > 0).all()


@pytest.mark.parametrize("min_sep", [1, 2, 5, 59])
def test_min_sep_on_plateaus(dev, min_sep):
    """Neighbouring windows share a raised stretch, so the best are adjacent: pass 1 spreads them, runs dry, and pass 2 fills in rank order."""
    L = 120
    rng = np.random.default_rng(min_sep)
    sims = rng.normal(0.0, 0.01, (4, L)).astype(F)
    sims[0, 30:50] += 1.0
    sims[1, 0:12] += 1.0
    sims[1, 100:120] += 0.5
    sims[2, 40:44] += 1.0
    sims[2, 60:64] += 1.0
    sims[3, :] = 0.25                                                                        # flat: every window ties, index order
    for keep in (5, 59):
        got, ref = check(dev, sims, durations(L, [L, L, L, L]), 8, 4, keep=keep, min_sep=min_sep, gt=spans_gt(4, L, keep), what=f"min_sep={min_sep}")
        assert ref["n_windows"].tolist() == [59] * 4
        if min_sep > 1:
            first = ref["order"][0, :2]
            assert abs(int(first[0]) - int(first[1])) >= min_sep or min_sep == 59             # spread while pass 1 has windows left
        assert sorted(got["order"][0].tolist()) == list(range(59))
    assert ref["order"][3].tolist() == WO.brute(ref["win_scores"][3], min_sep)


def test_ties_zeros_nans_and_flat_rows(dev):
    L = 64
    sims = np.zeros((7, L), dtype=F)
    sims[0, ::2] = -0.0                                                                       # +0 and -0 windows: ties, the index decides
    sims[0, 20:24] = [0.0, -0.0, -0.0, 0.0]
    sims[1] = np.tile(np.array([0.5, 0.25], F), L // 2)                                       # every window ties
    sims[2] = bumpy(1, L, 3)[0]
    sims[2, 17] = NAN                                                                         # a NaN frame: its windows are NaN and rank last
    sims[3, :] = NAN                                                                          # all NaN
    sims[4, 30:50] = -INF                                                                     # windows of -inf only, and one of +inf (no inf - inf: its NaN's sign is the adder's)
    sims[4, 9] = INF
    sims[5] = -np.abs(bumpy(1, L, 5)[0])                                                      # negative scores
    sims[5, 3] = -0.0
    sims[6] = np.round(bumpy(1, L, 6)[0], 1)                                                  # many exact ties
    gt = np.array([[3.0, 9.0]] * 7)
    for min_sep in (3, 1):
        for k in (1, 3):
            got, ref = check(dev, sims, durations(L, [L] * 7), 8, 4, k=k, keep=9, min_sep=min_sep, gt=gt, what=f"special k={k} sep={min_sep}")
    assert np.isnan(got["win_scores"][3]).all() and got["order"][3].tolist() == list(range(31))
    nan_windows = np.isnan(ref["win_scores"][2]).sum()
    assert 0 < nan_windows < 31 and np.isnan(ref["win_scores"][2][ref["order"][2][31 - nan_windows:]]).all()
    assert got["order"][1].tolist() == list(range(31)) and got["order"][0, 0] == 0


@pytest.mark.parametrize("R", [1, 4, 5, 260])
def test_row_counts(dev, R):
    L = 90
    rng = np.random.default_rng(R)
    check(dev, bumpy(R, L, 40 + R), durations(L, rng.integers(0, L + 1, R)), 10, 4, keep=7, min_sep=2, gt=spans_gt(R, L, R), what=f"R={R}")


def test_three_rows_per_mask_row(dev):
    """rpm = 3: a video's mask row is shared by three rows with different sims; bounds has one entry per mask row."""
    L = 150
    Ds = [150, 129, 64, 0]
    got, ref = check(dev, bumpy(12, L, 3), durations(L, Ds), 10, 4, keep=6, min_sep=3, gt=spans_gt(12, L, 9), what="rpm=3")
    assert ref["D"] == [150] * 3 + [129] * 3 + [64] * 3 + [0] * 3 and got["bounds"].shape == (4, 74, 2)
    assert len({got["select"][r].tobytes() for r in range(3)}) > 1


def test_the_bql_form_and_the_optional_parts(dev):
    from revisionllm_amd import ops
    B, Q, L = 3, 4, 200
    mask = durations(L, [200, 131, 77])
    sims = fenced(bumpy(B * Q, L, 17), mask)
    gt = spans_gt(B * Q, L, 4)
    ref = WO.select(sims, mask, 10, 4, 3, 8, 2, gt=gt)
    s, m, g = torch.from_numpy(sims).view(B, Q, L).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(gt).view(B, Q, 2).to(dev)
    for mk in (m, m.bool(), m.to(torch.int32), m.to(torch.uint8), m.half(), m.double()):
        out = ops.window_select(s, mk, win=10, stride=4, keep=8, min_sep=2, gt=g, return_scores=True, return_bounds=True, return_order=True)
        assert out.select.shape == (B, Q, 8) and out.n_select.shape == (B, Q) == out.n_windows.shape == out.hit_rank.shape
        assert out.scores.shape == (B, Q, 99) == out.order.shape and out.bounds.shape == (B, 99, 2)
        got = dict(select=out.select.cpu().numpy().reshape(B * Q, 8), n_select=out.n_select.cpu().numpy().reshape(-1),
                   n_windows=out.n_windows.cpu().numpy().reshape(-1), win_scores=out.scores.cpu().numpy().reshape(B * Q, 99),
                   bounds=out.bounds.cpu().numpy(), order=out.order.cpu().numpy().reshape(B * Q, 99), hit_rank=out.hit_rank.cpu().numpy().reshape(-1))
        same(got, ref, str(mk.dtype))
    bare = ops.window_select(s, m, win=10, stride=4, keep=8, min_sep=2)
    assert bare.scores is None and bare.bounds is None and bare.order is None and bare.hit_rank is None and torch.equal(bare.select, out.select)
    flat = ops.window_select(s.view(B * Q, L), m, win=10, stride=4, keep=8, min_sep=2)            # [R, L] with fewer mask rows: rpm = R / rows
    assert torch.equal(flat.select, out.select.view(B * Q, 8))
    big = ops.window_select(s, m, win=10, stride=4, keep=5000, min_sep=2)                         # keep above Wcap is Wcap
    assert big.select.shape == (B, Q, 99) and torch.equal(big.n_select, big.n_windows) and int(big.n_windows.max()) == 99
    for b, q in np.ndindex(B, Q):
        W = int(big.n_windows[b, q])
        assert big.select[b, q].tolist() == list(range(W)) + [-1] * (99 - W)


# ------------------------------------------------------------------ ground truths ------------------------------------------------------------------
def test_ground_truths(dev):
    """win = 8, stride = 4, D = 40: windows [2i, 2i + 9) for i < 16 and [31, 40) for the last three.  One peak makes window 10 = [20, 29) the best, then its neighbours."""
    L = 40
    s = np.zeros(L, dtype=F)
    s[24] = 1.0                                                                               # windows 8 .. 12 hold frame 24 and tie: 8, 9, 10, 11, 12 in index order
    gts = [(20.5, 21.0), (24.0, 25.0), (0.0, 2.0), (39.5, 45.0), (40.0, 50.0), (-7.0, 0.0), (-7.0, 0.5), (50.0, 60.0), (NAN, 5.0), (3.0, INF), (-INF, 3.0),
           (9.0, 9.0), (12.0, 3.0), (25.0, 26.0), (16.0, 17.0), (29.0, 30.0), (10.0, 16.0), (0.0, 40.0)]
    sims = np.tile(s, (len(gts), 1))
    for min_sep in (1, 4):
        got, ref = check(dev, sims, durations(L, [L]), 8, 4, k=1, keep=3, min_sep=min_sep, gt=np.array(gts), what=f"gt sep={min_sep}")
    assert ref["order"][0, :5].tolist() == [8, 12, 0, 4, 16] and ref["bounds"][0, 8].tolist() == [16, 25] and ref["bounds"][0, 18].tolist() == [31, 40]
    hr = dict(zip(gts, ref["hit_rank"].tolist()))
    assert hr[(24.0, 25.0)] == 0                                                              # inside the best window
    assert hr[(25.0, 26.0)] == 1                                                              # window 8 ends at 25: hi > gs is strict, window 12 = [24, 33) is next
    assert hr[(16.0, 17.0)] == 0 and hr[(10.0, 16.0)] == 3                                    # window 8 starts at 16: lo < ge is strict; window 4 = [8, 17)
    assert hr[(40.0, 50.0)] == -1 and hr[(-7.0, 0.0)] == -1 and hr[(50.0, 60.0)] == -1        # outside [0, D), touching it
    assert hr[(39.5, 45.0)] >= 0 and hr[(-7.0, 0.5)] == 2
    assert all(hr[g] == -1 for g in gts[8:13])                                                # void
    assert hr[(0.0, 40.0)] == 0
    got1, ref1 = check(dev, sims, durations(L, [L]), 8, 4, k=1, keep=3, min_sep=1, gt=np.array(gts), what="gt sep=1")
    assert ref1["order"][0, :5].tolist() == [8, 9, 10, 11, 12] and ref1["hit_rank"][gts.index((29.0, 30.0))] == 3       # the place is the score rank


def test_a_row_does_not_depend_on_its_batch(dev):
    L = 200
    Ds = [200, 180, 77, 130, 200]
    mask = durations(L, Ds)
    sims = fenced(bumpy(5, L, 23), mask)
    gt = spans_gt(5, L, 2)
    whole = run(dev, sims, mask, 10, 4, 3, 12, 3, gt)
    for r in (0, 2, 4):
        alone = run(dev, sims[r:r + 1], mask[r:r + 1], 10, 4, 3, 12, 3, gt[r:r + 1])
        for k_ in whole:
            a, b = np.ascontiguousarray(whole[k_][r:r + 1]), np.ascontiguousarray(alone[k_])
            assert a.tobytes() == b.tobytes(), (r, k_)
    swapped = run(dev, sims[::-1], mask[::-1], 10, 4, 3, 12, 3, gt[::-1])
    for k_ in whole:
        assert np.ascontiguousarray(whole[k_][::-1]).tobytes() == np.ascontiguousarray(swapped[k_]).tobytes(), k_


# ------------------------------------------------------------------ against the neighbouring kernels ------------------------------------------------------------------
@pytest.mark.parametrize("win,stride,L", [(10, 4, 300), (70, 5, 300), (625, 5, 3000)])
def test_scores_order_and_bounds_against_the_neighbouring_entries(dev, win, stride, L):
    """``win_scores`` = ``ops.span_scores`` on the windows in rv_span_propose's (centre, width) encoding, bit for bit; with min_sep = 1, ``order`` =
    ``ops.span_rank``'s order on those scores; ``bounds`` = ``stage2.cut_windows``' times."""
    from revisionllm_amd import ops
    from revisionllm_amd.eval import stage2
    Ds = [L, L - 7, (L + win) // 2]
    mask = durations(L, Ds)
    sims = fenced(bumpy(3, L, win), mask)
    sims[0, L // 3] = NAN
    s, m = torch.from_numpy(sims).to(dev), torch.from_numpy(mask).to(dev)
    out = ops.window_select(s, m, win=win, stride=stride, keep=10, return_scores=True, return_bounds=True, return_order=True)
    bounds, n = out.bounds.cpu().numpy(), out.n_windows.cpu().numpy()
    Wcap = bounds.shape[1]
    spans = np.full((3, Wcap, 2), NAN, dtype=F)
    for r, D in enumerate(Ds):
        times, _ = stage2.cut_windows(D, win, 1, stride, num_frames=2)
        assert n[r] == len(times) and bounds[r, :n[r]].tolist() == [[max(int(a), 0), int(b) + 1] for a, b in times] and (bounds[r, n[r]:] == -1).all()
        lo, hi, dur = bounds[r, :n[r], 0].astype(F), bounds[r, :n[r], 1].astype(F), F(D)
        spans[r, :n[r], 0] = ((lo + hi) * F(0.5)) / dur
        spans[r, :n[r], 1] = ((hi - lo) - F(0.5)) / dur
    sp = torch.from_numpy(spans).to(dev)
    scores, windows = ops.span_scores(s, sp, m, k=3, return_windows=True)
    assert torch.equal(windows.cpu(), out.bounds.cpu())
    assert torch.equal(scores.view(torch.int32), out.scores.view(torch.int32))
    rank = ops.span_rank(scores, sp, nms_iou=1.0, return_order=True)
    for r in range(3):
        assert torch.equal(rank.order[r, :n[r]].cpu(), out.order[r, :n[r]].cpu()) and bool((out.order[r, n[r]:] == -1).all())
        assert torch.equal(torch.sort(rank.order[r, :10].cpu()).values, out.select[r].cpu())


# ------------------------------------------------------------------ the public calls ------------------------------------------------------------------
def _features(B, L, d, Q, seed, op16):
    g = torch.Generator().manual_seed(seed)
    video = torch.randn(B, L, d, generator=g)
    text = torch.randn(B, Q, d, generator=g)
    for b in range(B):
        for q in range(Q):
            a = 20 + 37 * q + 11 * b
            video[b, a:a + 25 + 9 * q] += 1.5 * text[b, q]                                  # each query has a stretch of its own
    return text, video.to(op16) if op16 is not None else video


def _bits(t):
    return t.cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.cpu()


def test_select_windows_is_the_two_calls_chained(dev):
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import select_windows
    op16 = {"f16": torch.float16, "bf16": torch.bfloat16}[fl()]
    B, L, d, Q = 3, 300, 64, 4
    mask = torch.from_numpy(durations(L, [300, 257, 140])).to(dev)
    kw = dict(win=20, stride=5, keep=6, k=3, min_sep=2, return_scores=True, return_bounds=True, return_order=True)
    for dt in (None, op16):
        text, video = _features(B, L, d, Q, 31, dt)
        gt = torch.tensor([[[30.0, 50.0]] * Q] * B)
        for t, g in ((text.to(dev), gt.to(dev)), (text[:, 0].contiguous().to(dev), gt[:, 0].contiguous().to(dev))):
            out = select_windows(t, video.to(dev), mask, gt=g, **kw)
            sims = (ops.frame_cosine_multi if t.dim() == 3 else ops.frame_cosine)(t.float(), video.to(dev))
            want = ops.window_select(sims, mask, gt=g, **kw)
            assert out.select.shape == t.shape[:-1] + (6,) and out.select.device == dev
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out, want))
            assert int(out.n_select.min()) == 6 and int(out.hit_rank.min()) >= 0
    host = select_windows(text, video, mask.cpu().bool(), **kw)                                    # host tensors: staged, results back on the host
    assert not host.select.is_cuda and not host.scores.is_cuda and host.hit_rank is None
    again = select_windows(text.to(dev), video.to(dev), mask, **kw)
    assert torch.equal(host.select, again.select.cpu()) and torch.equal(_bits(host.scores), _bits(again.scores))


@pytest.mark.parametrize("ab", [(400, 460), (0, 30), (1250, 1300), (700, 1100)])
def test_clip_grounding_windows_finds_a_planted_stretch(dev, ab):
    """Frames [a, b) equal to the query direction, the rest orthogonal to it: the list is sorted, distinct, inside [0, W), of length min(batch, W), and
    holds every window that contains a frame of the stretch when there are no more of them than ``batch``."""
    from revisionllm_amd.eval import stage2
    a, b = ab
    ctx_l, d = 1300, 16
    feats = np.zeros((ctx_l, d), dtype=np.float32)
    feats[:, 1] = 1.0
    feats[a:b] = 0.0
    feats[a:b, 0] = 2.0
    query = np.zeros(d, dtype=np.float32)
    query[0] = 0.5
    geometry = dict(debug_window=20, feature_fps=5, stride=5)                                  # windows of 100 frames every 20: W = 64
    times, frame_idx = stage2.cut_windows(ctx_l, **geometry)
    W = len(times)
    holding = [i for i, (s, e) in enumerate(times) if max(s, 0) < b and e + 1 > a]
    op16 = torch.float16 if fl() == "f16" else torch.bfloat16
    for given in (feats, torch.from_numpy(feats), torch.from_numpy(feats).to(dev), torch.from_numpy(feats).to(dev).to(op16), feats.astype(np.float16)):
        for batch in (len(holding), 40, 64, 100):
            gw = stage2.clip_grounding_windows(given, query, batch=batch, **geometry)
            assert isinstance(gw, list) and all(type(i) is int for i in gw) and gw == sorted(set(gw)) and len(gw) == min(batch, W)
            assert all(0 <= i < W for i in gw) and set(holding) <= set(gw), (batch, holding, gw)
            assert frame_idx[gw].shape == (len(gw), 250)
        spread = stage2.clip_grounding_windows(given, query, batch=8, min_sep=4, **geometry)
        assert len(spread) == 8 and min(np.diff(spread)) >= 4 and len(set(spread) & set(holding)) >= 1


def test_the_calls_do_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the calls: with the stream kept busy by work queued before them, an event recorded just before a
    call has not completed when the call returns (a call that waited for its own kernel would have waited for that work first)."""
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import select_windows
    text, video = _features(4, 300, 64, 3, 77, torch.float16 if fl() == "f16" else torch.bfloat16)
    text, video, mask = text.to(dev), video.to(dev), torch.ones(4, 300, device=dev)
    sims = torch.from_numpy(bumpy(12, 300, 1)).view(4, 3, 300).to(dev)
    gt = torch.tensor([75.0, 150.0]).repeat(4, 3, 1).to(dev)
    one, flags = text[:, 0].contiguous(), mask.bool()
    calls = (lambda: ops.window_select(sims, mask, win=20, stride=5, keep=10, min_sep=2, gt=gt, return_scores=True, return_bounds=True, return_order=True),
             lambda: select_windows(text, video, mask, win=20, stride=5, keep=10, min_sep=3, gt=gt, return_order=True),
             lambda: select_windows(one, video, flags, win=20, stride=5, keep=10))
    for which, call in enumerate(calls):
        want = call()                                                                          # (warm: library loaded, allocator blocks cached)
        a = torch.ones(8192, 8192, device=dev)
        c = torch.empty_like(a)
        torch.mm(a, a, out=c)
        torch.cuda.synchronize()
        for _ in range(12):                                                                    # ~1.1 TFLOP of f32 each: tens of milliseconds of queued work
            torch.mm(a, a, out=c)
        ev = torch.cuda.Event()
        ev.record()
        got = call()
        still_busy = not ev.query()
        torch.cuda.synchronize()
        assert still_busy, f"call {which} returned only after the work queued before it had finished: it synchronised"
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(got, want) if x is not None)
