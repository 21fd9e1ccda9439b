"""rvx_window_select_clipped (the companion library's kernel behind ``ops.window_select_clipped`` / ``eval.similarity.select_windows_clipped`` /
``eval.stage1.clip_stage_windows``: the stage-1 driver's windows chosen from a cosine row in one launch) against tests/stage1_prefilter_oracle.py, the
rule restated in numpy float32 with Python loops.  The oracle IS the rule, so ``select``, ``n_select``, ``n_windows``, ``bounds``, ``order`` and
``hit_rank`` must be equal and ``win_scores`` must have the oracle's bits; no case is left out and there is no tolerance.
tests/test_stage1_prefilter_host_logic.py holds the oracle itself to a brute-force statement of the selection and to ``stage1.cut_windows``.

Every direct call writes into buffers with 64 sentinel elements on either side of each output; the surroundings are compared bitwise.  In every case
the frames of ``sims`` from D on are NaN: a read past the duration would show in a score.  Every case runs twice: with every optional output (the
greedy walk then runs over all windows) and with none (the walk stops at ``keep`` taken); ``select`` must not change.  The kernel is f32 only and the
companion library has one build, so the kernel items run once (``kdev``); the chain items call the flavoured libraries around it and run in both
builds (``dev``)."""
import functools
import os

import numpy as np
import pytest
import torch

import stage1_prefilter_oracle as PO
import window_oracle as WO
from helpers import fl
from test_gpu_window_select import _Guarded, bumpy, durations, fenced, same, spans_gt

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")
NAN, INF = float("nan"), float("inf")
F = np.float32


@pytest.fixture(scope="module")
def kdev(op_flavour):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import hip
    hip.ext_lib()
    return torch.device("cuda:0")


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
    hip.lib(), hip.ext_lib()
    return torch.device("cuda:0")


# ------------------------------------------------------------------ running the entry ------------------------------------------------------------------
def run(dev, sims, mask, win, k, keep, min_sep, gt=None, full=True):
    """The C entry on numpy inputs -> dict like the oracle's (parts not asked for: None), after the sentinel checks."""
    from revisionllm_amd import hip
    R, L = sims.shape
    M = mask.shape[0]
    Wcap = PO.capacity(L, win)
    s = torch.from_numpy(np.ascontiguousarray(sims, dtype=F)).to(dev)
    m = torch.from_numpy(np.ascontiguousarray(mask, dtype=F)).to(dev)
    g = torch.from_numpy(np.ascontiguousarray(gt, dtype=F)).to(dev) if gt is not None else None
    o = dict(select=_Guarded(R * keep, torch.int32, dev), n_select=_Guarded(R, torch.int32, dev), n_windows=_Guarded(R, torch.int32, dev),
             win_scores=_Guarded(R * Wcap, torch.float32, dev) if full else None, bounds=_Guarded(M * Wcap * 2, torch.int32, dev) if full else None,
             order=_Guarded(R * Wcap, torch.int32, dev) if full else None, hit_rank=_Guarded(R, torch.int32, dev) if full and gt is not None else None)
    ptr = lambda x: x.ptr if x is not None else None                                            # noqa: E731
    rc = hip.ext_lib().rvx_window_select_clipped(hip.ptr(s), hip.ptr(m), R, R // M, L, win, k, keep, min_sep, Wcap, hip.ptr(g) if o["hit_rank"] else None,
                                                 ptr(o["select"]), ptr(o["n_select"]), ptr(o["n_windows"]), ptr(o["win_scores"]), ptr(o["bounds"]),
                                                 ptr(o["order"]), ptr(o["hit_rank"]), hip.stream())
    hip.ext_check(rc, "rvx_window_select_clipped")
    torch.cuda.synchronize()
    shapes = dict(select=(R, keep), n_select=(R,), n_windows=(R,), win_scores=(R, Wcap), bounds=(M, Wcap, 2), order=(R, Wcap), hit_rank=(R,))
    return {k_: (v.take(shapes[k_]) if v is not None else None) for k_, v in o.items()}


@functools.lru_cache(maxsize=None)
def _oracle(sims_b, sims_shape, mask_b, mask_shape, gt_b, params):
    sims = np.frombuffer(sims_b, dtype=F).reshape(sims_shape)
    mask = np.frombuffer(mask_b, dtype=F).reshape(mask_shape)
    gt = np.frombuffer(gt_b, dtype=F).reshape(sims_shape[0], 2) if gt_b is not None else None
    return PO.select(sims, mask, *params, gt=gt)


def check(dev, sims, mask, win, k=3, keep=5, min_sep=1, gt=None, what=""):
    """Fence, run with every output and with none, compare both with the oracle -> (got, ref)."""
    sims = fenced(sims, mask)
    Wcap = PO.capacity(sims.shape[1], win)
    keep, min_sep = min(keep, Wcap), min(min_sep, Wcap)
    gt = np.ascontiguousarray(gt, dtype=F) if gt is not None else None
    ref = _oracle(sims.tobytes(), sims.shape, mask.tobytes(), mask.shape, gt.tobytes() if gt is not None else None, (win, k, keep, min_sep))
    got = run(dev, sims, mask, win, k, keep, min_sep, gt)
    same(got, ref, what)
    same(run(dev, sims, mask, win, k, keep, min_sep, None, full=False), ref, what + " (select only)")
    for r in range(sims.shape[0]):                                   # a void index is no candidate
        W = int(ref["n_windows"][r])
        assert got["select"][r].max(initial=-1) < W and got["order"][r].max(initial=-1) < W and W <= Wcap
    return got, ref


# ------------------------------------------------------------------ geometries ------------------------------------------------------------------
@pytest.mark.parametrize("win", [2, 3, 4, 5, 61, 64])
def test_geometries(kdev, win):
    """D = L, L - 1, win, win / 2, 1 and 0 at L = 3 win + 1 and 3 win + 4; the odd ones have void windows at the longer durations."""
    from revisionllm_amd import ops
    for L in (3 * win + 1, 3 * win + 4):
        Ds = [L, L - 1, win, win // 2, 1, 0]
        _, ref = check(kdev, bumpy(6, L, L), durations(L, Ds), win, keep=5, min_sep=2, gt=spans_gt(6, L, L), what=f"win={win} L={L}")
        assert ref["D"] == Ds and ref["n_windows"].tolist() == [ops.clipped_window_solid(D, win) for D in Ds]
        assert ref["n_windows"][4] == ref["n_windows"][5] == 0
        assert [int(n) < ops.clipped_window_count(D, win) for n, D in zip(ref["n_windows"], Ds)] == [ops.clipped_window_void(D, win) for D in Ds]
    assert ops.clipped_window_void(L, win) == (win in (3, 5))                                # (L = 3 win + 4: 13 and 19 frames)


def test_void_suffixes_and_the_one_frame_window(kdev):
    _, ref = check(kdev, bumpy(4, 20, 1), durations(20, [13, 15, 14, 20]), 5, keep=9, min_sep=2, gt=spans_gt(4, 20, 2), what="win=5")
    assert ref["n_windows"].tolist() == [6, 6, 6, 8] and PO.capacity(20, 5) == 9
    assert ref["bounds"][0, 5].tolist() == [12, 13] and ref["bounds"][1, 5].tolist() == [12, 15] and ref["bounds"][1, 6].tolist() == [-1, -1]
    got, ref = check(kdev, bumpy(4, 600, 3), durations(600, [6, 600, 599, 5]), 3, keep=450, min_sep=1, gt=spans_gt(4, 600, 4), what="win=3")
    assert ref["n_windows"].tolist() == [4, 400, 400, 4] and ref["n_select"].tolist() == [4, 400, 400, 4]
    assert ref["bounds"][0, :5].tolist() == [[0, 4], [1, 5], [3, 6], [4, 6], [-1, -1]] and np.isnan(got["win_scores"][1, 400:]).all()
    check(kdev, bumpy(2, 600, 5), durations(600, [600, 301]), 3, k=64, keep=7, min_sep=3, what="win=3 sep=3")


def test_window_counts_up_to_the_cap(kdev):
    """W = 63, 64, 65 (win = 2: W = D - 1), and W = 2048 and 1024 at win = 2, L = 2049 with the longest greedy walk (keep = W, min_sep = 2)."""
    _, ref = check(kdev, bumpy(3, 66, 9), durations(66, [64, 65, 66]), 2, keep=64, min_sep=2, gt=spans_gt(3, 66, 1), what="63..65")
    assert ref["n_windows"].tolist() == [63, 64, 65]
    L = 2049
    sims = bumpy(2, L, 7)
    _, ref = check(kdev, sims, durations(L, [L, 1025]), 2, k=2, keep=2048, min_sep=2, gt=np.array([[2047.5, 2048.0], [5.0, 6.0]]), what="cap")
    assert ref["n_windows"].tolist() == [2048, 1024] and ref["n_select"].tolist() == [2048, 1024] and PO.capacity(L, 2) == 2048
    check(kdev, sims, durations(L, [L, 700]), 2, k=1, keep=100, min_sep=1, what="cap, min_sep 1")


@pytest.mark.parametrize("win", [1023, 1024])
def test_the_register_and_the_reread_path(kdev, win):
    """An unclipped window has win + 1 frames: 1024 (the last that a wave holds in registers) and 1025 (read again from the row in every round)."""
    L = 2600
    Ds = [L, L - 1, win + 1, 1500]
    for k in (1, 3, 64):
        _, ref = check(kdev, bumpy(4, L, win + k), durations(L, Ds), win, k=k, keep=3, min_sep=2, gt=spans_gt(4, L, k), what=f"win={win} k={k}")
    assert ref["n_windows"][0] == 5 and (ref["bounds"][0, 0, 1] - ref["bounds"][0, 0, 0]) == win + 1


@pytest.mark.parametrize("k", [1, 2, 3, 7, 9, 64])
def test_k_around_and_above_the_window_length(kdev, k):
    """win = 8: windows of 9 frames, the last ones of 8, 4 and fewer; k above the length sums the whole window."""
    L = 40
    _, ref = check(kdev, bumpy(4, L, k), durations(L, [40, 37, 9, 34]), 8, k=k, keep=6, what=f"k={k}")
    assert ref["bounds"][0, 8].tolist() == [32, 40] and ref["bounds"][1, 8].tolist() == [32, 37] and ref["bounds"][2, 1].tolist() == [4, 9]
    assert ref["bounds"][3, 7].tolist() == [28, 34] and ref["bounds"][3, 8].tolist() == [-1, -1] and ref["n_windows"].tolist() == [9, 9, 2, 8]


@pytest.mark.parametrize("keep", [1, 8, 9, 10, 19])
def test_keep_around_the_window_count(kdev, keep):
    L = 80
    for min_sep in (1, 3):
        got, ref = check(kdev, bumpy(2, L, keep), durations(L, [40, 80]), 8, keep=keep, min_sep=min_sep, what=f"keep={keep}")
        assert ref["n_select"].tolist() == [min(keep, 9), min(keep, 19)]
        for r in range(2):
            n = int(ref["n_select"][r])
            assert (got["select"][r, n:] == -1).all() and (np.diff(got["select"][r, :n]) > 0).all()


@pytest.mark.parametrize("min_sep", [1, 2, 29])
def test_min_sep_on_plateaus(kdev, min_sep):
    """Neighbouring windows share a raised stretch, so the best are adjacent: pass 1 spreads them, runs dry, and pass 2 fills in rank order."""
    L = 120
    rng = np.random.default_rng(min_sep)
    sims = rng.normal(0.0, 0.01, (4, L)).astype(F)
    sims[0, 30:50] += 1.0
    sims[1, 0:12] += 1.0
    sims[1, 100:120] += 0.5
    sims[2, 40:44] += 1.0
    sims[2, 60:64] += 1.0
    sims[3, :] = 0.25                                                                        # flat: the full windows tie, index order
    for keep in (5, 29):
        got, ref = check(kdev, sims, durations(L, [L] * 4), 8, keep=keep, min_sep=min_sep, gt=spans_gt(4, L, keep), what=f"min_sep={min_sep}")
        assert ref["n_windows"].tolist() == [29] * 4 and sorted(got["order"][0].tolist()) == list(range(29))
        if min_sep == 2:
            assert abs(int(ref["order"][0, 0]) - int(ref["order"][0, 1])) >= 2
    assert ref["order"][3].tolist() == WO.brute(ref["win_scores"][3], min_sep)


def test_ties_zeros_nans_infinities_and_flat_rows(kdev):
    L = 64
    sims = np.zeros((7, L), dtype=F)
    sims[0, ::2] = -0.0
    sims[0, 20:24] = [0.0, -0.0, -0.0, 0.0]
    sims[1] = np.tile(np.array([0.5, 0.25], F), L // 2)
    sims[2] = bumpy(1, L, 3)[0]
    sims[2, 17] = NAN
    sims[3, :] = NAN
    sims[4, 30:50] = -INF
    sims[4, 9] = INF
    sims[5] = -np.abs(bumpy(1, L, 5)[0])
    sims[5, 3] = -0.0
    sims[6] = np.round(bumpy(1, L, 6)[0], 1)
    gt = np.array([[3.0, 9.0]] * 7)
    for min_sep in (3, 1):
        for k in (1, 3):
            got, ref = check(kdev, sims, durations(L, [L] * 7), 8, k=k, keep=9, min_sep=min_sep, gt=gt, what=f"special k={k} sep={min_sep}")
    assert np.isnan(got["win_scores"][3]).all() and got["order"][3].tolist() == list(range(15))
    nan_windows = np.isnan(ref["win_scores"][2]).sum()
    assert 0 < nan_windows < 15 and np.isnan(ref["win_scores"][2][ref["order"][2][15 - nan_windows:]]).all()
    assert got["order"][1].tolist() == list(range(15)) and got["order"][0, 0] == 0


@pytest.mark.parametrize("R", [1, 4, 260])
def test_row_counts(kdev, R):
    L = 90
    rng = np.random.default_rng(R)
    check(kdev, bumpy(R, L, 40 + R), durations(L, rng.integers(0, L + 1, R)), 9, keep=7, min_sep=2, gt=spans_gt(R, L, R), what=f"R={R}")


def test_three_rows_per_mask_row(kdev):
    L = 150
    Ds = [150, 129, 64, 0]
    got, ref = check(kdev, bumpy(12, L, 3), durations(L, Ds), 11, keep=6, min_sep=3, gt=spans_gt(12, L, 9), what="rpm=3")
    assert ref["D"] == [150] * 3 + [129] * 3 + [64] * 3 + [0] * 3 and got["bounds"].shape == (4, 29, 2)
    assert len({got["select"][r].tobytes() for r in range(3)}) > 1


def _as_dict(out, R, keep, Wcap):
    return dict(select=out.select.cpu().numpy().reshape(R, keep), n_select=out.n_select.cpu().numpy().reshape(-1), n_windows=out.n_windows.cpu().numpy().reshape(-1),
                win_scores=out.scores.cpu().numpy().reshape(R, Wcap), bounds=out.bounds.cpu().numpy(), order=out.order.cpu().numpy().reshape(R, Wcap),
                hit_rank=out.hit_rank.cpu().numpy().reshape(-1))


def test_the_bql_form_and_the_optional_parts(kdev):
    from revisionllm_amd import ops
    B, Q, L = 3, 4, 200
    mask = durations(L, [200, 131, 77])
    sims = fenced(bumpy(B * Q, L, 17), mask)
    gt = spans_gt(B * Q, L, 4)
    ref = PO.select(sims, mask, 11, 3, 8, 2, gt=gt)
    Wcap = PO.capacity(L, 11)
    s, m, g = torch.from_numpy(sims).view(B, Q, L).to(kdev), torch.from_numpy(mask).to(kdev), torch.from_numpy(gt).view(B, Q, 2).to(kdev)
    for mk in (m, m.bool(), m.to(torch.int32), m.half()):
        out = ops.window_select_clipped(s, mk, win=11, keep=8, min_sep=2, gt=g, return_scores=True, return_bounds=True, return_order=True)
        assert out.select.shape == (B, Q, 8) and out.n_select.shape == (B, Q) == out.n_windows.shape == out.hit_rank.shape
        assert out.scores.shape == (B, Q, Wcap) == out.order.shape and out.bounds.shape == (B, Wcap, 2)
        same(_as_dict(out, B * Q, 8, Wcap), ref, str(mk.dtype))
    bare = ops.window_select_clipped(s, m, win=11, keep=8, min_sep=2)
    assert bare.scores is None and bare.bounds is None and bare.order is None and bare.hit_rank is None and torch.equal(bare.select, out.select)
    flat = ops.window_select_clipped(s.view(B * Q, L), m, win=11, keep=8, min_sep=2)              # [R, L] with fewer mask rows: rpm = R / rows
    assert torch.equal(flat.select, out.select.view(B * Q, 8))
    big = ops.window_select_clipped(s, m, win=11, keep=5000, min_sep=2)                           # keep above Wcap is Wcap
    assert big.select.shape == (B, Q, Wcap) and torch.equal(big.n_select, big.n_windows)
    assert big.n_windows[:, 0].tolist() == [ops.clipped_window_solid(D, 11) for D in (200, 131, 77)]
    for b, q in np.ndindex(B, Q):
        W = int(big.n_windows[b, q])
        assert big.select[b, q].tolist() == list(range(W)) + [-1] * (Wcap - W)


# ------------------------------------------------------------------ ground truths ------------------------------------------------------------------
def test_ground_truths(kdev):
    """win = 8, D = 40: windows [4 i, 4 i + 9) for i < 8 and [32, 40).  One peak at frame 20 makes windows 3, 4 and 5 tie for the best."""
    L = 40
    s = np.zeros(L, dtype=F)
    s[20] = 1.0
    gts = [(20.5, 21.0), (21.0, 22.0), (25.0, 26.0), (10.0, 14.0), (0.0, 2.0), (39.5, 45.0), (40.0, 50.0), (-7.0, 0.0), (-7.0, 0.5), (50.0, 60.0), (NAN, 5.0),
           (3.0, INF), (-INF, 3.0), (9.0, 9.0), (12.0, 3.0), (0.0, 40.0)]
    sims = np.tile(s, (len(gts), 1))
    for min_sep in (4, 1):
        got, ref = check(kdev, sims, durations(L, [L]), 8, k=1, keep=3, min_sep=min_sep, gt=np.array(gts), what=f"gt sep={min_sep}")
    assert ref["order"][0, :9].tolist() == [3, 4, 5, 0, 1, 2, 6, 7, 8] and ref["bounds"][0, 3].tolist() == [12, 21] and ref["bounds"][0, 8].tolist() == [32, 40]
    hr = dict(zip(gts, ref["hit_rank"].tolist()))
    assert hr[(20.5, 21.0)] == 0                                                              # inside the best window
    assert hr[(21.0, 22.0)] == 1 and hr[(25.0, 26.0)] == 2                                    # windows 3 and 4 end at 21 and 25: hi > gs is strict
    assert hr[(10.0, 14.0)] == 0                                                              # across windows 1, 2 and 3: the best-ranked of them
    assert hr[(0.0, 2.0)] == 3 and hr[(-7.0, 0.5)] == 3 and hr[(39.5, 45.0)] == 8
    assert hr[(40.0, 50.0)] == -1 and hr[(-7.0, 0.0)] == -1 and hr[(50.0, 60.0)] == -1        # outside [0, D), touching it: lo < ge is strict
    assert all(hr[g] == -1 for g in gts[10:15]) and hr[(0.0, 40.0)] == 0                      # void ground truths
    # a ground truth that only a void window's index would cover: win = 3, D = 6 has windows up to [4, 6); index 4 starts at frame 6
    _, ref = check(kdev, np.zeros((2, 9), F), durations(9, [6]), 3, k=1, keep=2, gt=np.array([[6.0, 8.0], [5.5, 8.0]]), what="void window")
    assert ref["hit_rank"].tolist() == [-1, 2] and ref["n_windows"].tolist() == [4, 4]


def test_a_row_does_not_depend_on_its_batch(kdev):
    L = 200
    Ds = [200, 180, 77, 130, 200]
    mask = durations(L, Ds)
    sims = fenced(bumpy(5, L, 23), mask)
    gt = spans_gt(5, L, 2)
    whole = run(kdev, sims, mask, 11, 3, 12, 3, gt)
    for r in (0, 2, 4):
        alone = run(kdev, sims[r:r + 1], mask[r:r + 1], 11, 3, 12, 3, gt[r:r + 1])
        for k_ in whole:
            assert np.ascontiguousarray(whole[k_][r:r + 1]).tobytes() == np.ascontiguousarray(alone[k_]).tobytes(), (r, k_)
    swapped = run(kdev, sims[::-1], mask[::-1], 11, 3, 12, 3, gt[::-1])
    for k_ in whole:
        assert np.ascontiguousarray(whole[k_][::-1]).tobytes() == np.ascontiguousarray(swapped[k_]).tobytes(), k_


# ------------------------------------------------------------------ against the neighbouring kernels ------------------------------------------------------------------
@pytest.mark.parametrize("win,L", [(10, 300), (61, 300), (5, 83), (625, 3000)])
def test_scores_order_and_bounds_against_the_neighbouring_entries(dev, win, L):
    """``win_scores`` = ``ops.span_scores`` on the windows in rv_span_propose's (centre, width) encoding, bit for bit; with min_sep = 1, ``order`` =
    ``ops.span_rank``'s order on those scores; every window that is not clipped (s + win <= D - 1) has the bounds and the score bits of
    ``ops.window_select(..., stride=2)`` - the shifted rule differs in the last windows only."""
    from revisionllm_amd import ops
    Ds = [L, L - 7, (L + win) // 2]
    mask = durations(L, Ds)
    sims = fenced(bumpy(3, L, win), mask)
    sims[0, L // 3] = NAN
    s, m = torch.from_numpy(sims).to(dev), torch.from_numpy(mask).to(dev)
    out = ops.window_select_clipped(s, m, win=win, keep=10, return_scores=True, return_bounds=True, return_order=True)
    bounds, n = out.bounds.cpu().numpy(), out.n_windows.cpu().numpy()
    Wcap = bounds.shape[1]
    spans = np.full((3, Wcap, 2), NAN, dtype=F)
    for r, D in enumerate(Ds):
        assert n[r] == ops.clipped_window_solid(D, win) and bounds[r, :n[r]].tolist() == [list(w) for w in PO.windows(D, win)] and (bounds[r, n[r]:] == -1).all()
        lo, hi, dur = bounds[r, :n[r], 0].astype(F), bounds[r, :n[r], 1].astype(F), F(D)
        spans[r, :n[r], 0] = ((lo + hi) * F(0.5)) / dur
        spans[r, :n[r], 1] = ((hi - lo) - F(0.5)) / dur
    sp = torch.from_numpy(spans).to(dev)
    scores, windows = ops.span_scores(s, sp, m, k=3, return_windows=True)
    assert torch.equal(windows.cpu(), out.bounds.cpu())
    assert torch.equal(scores.view(torch.int32), out.scores.view(torch.int32))
    rank = ops.span_rank(scores, sp, nms_iou=1.0, return_order=True)
    shifted = ops.window_select(s, m, win=win, stride=2, keep=10, return_scores=True, return_bounds=True)
    for r, D in enumerate(Ds):
        assert torch.equal(rank.order[r, :n[r]].cpu(), out.order[r, :n[r]].cpu()) and bool((out.order[r, n[r]:] == -1).all())
        assert torch.equal(torch.sort(rank.order[r, :min(10, n[r])].cpu()).values, out.select[r, :min(10, n[r])].cpu())
        whole = [i for i in range(n[r]) if (i * win) // 2 + win <= D - 1]
        assert len(whole) >= 1 and torch.equal(shifted.bounds[r, whole].cpu(), out.bounds[r, whole].cpu())
        assert torch.equal(shifted.scores[r, whole].cpu().view(torch.int32), out.scores[r, whole].cpu().view(torch.int32))


def _bits(t):
    return t.cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.cpu()


def _op16():
    return torch.float16 if fl() == "f16" else torch.bfloat16


def test_the_gather_takes_the_select_row_as_it_lies(dev):
    """``ops.window_gather_clipped(video, select=select)`` row j is ``features[cut_windows(...)[select[j]]]``; the -1 padding gives zeros."""
    from revisionllm_amd import ops
    from revisionllm_amd.eval import stage1
    L, d, win, nf = 330, 32, 20, 12
    g = torch.Generator().manual_seed(5)
    for dt in (torch.float32, _op16()):
        video = torch.randn(L, d, generator=g).to(dt)
        sims = torch.from_numpy(bumpy(2, L, 8)).to(dev)
        sel = ops.window_select_clipped(sims, torch.ones(1, L, device=dev), win=win, keep=7, min_sep=2)
        short = ops.window_select_clipped(sims, torch.from_numpy(durations(L, [35])).to(dev), win=win, keep=7)       # 3 windows: padding in select
        idx = stage1.cut_windows(L, win, 1, nf)
        for out in (sel, short):
            frames = ops.window_gather_clipped(video.to(dev), win=win, num_frames=nf, select=out.select, out_dtype=dt).cpu()
            for r in range(2):
                for j, w in enumerate(out.select[r].tolist()):
                    want = video[torch.from_numpy(idx[w].astype(np.int64))] if w >= 0 else torch.zeros(nf, d, dtype=dt)
                    assert torch.equal(frames[r, j], want), (dt, r, j, w)
        assert short.n_windows.tolist() == [3, 3] and short.select[0].tolist() == [0, 1, 2, -1, -1, -1, -1]


# ------------------------------------------------------------------ the chain ------------------------------------------------------------------
def _features(B, L, d, Q, seed, op16):
    g = torch.Generator().manual_seed(seed)
    video = torch.randn(B, L, d, generator=g)
    text = torch.randn(B, Q, d, generator=g)
    for b in range(B):
        for q in range(Q):
            a = 20 + 37 * q + 11 * b
            video[b, a:a + 25 + 9 * q] += 1.5 * text[b, q]                                  # each query has a stretch of its own
    return text, video.to(op16) if op16 is not None else video


def test_select_windows_clipped_is_the_two_calls_chained(dev):
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import select_windows_clipped
    B, L, d, Q = 3, 300, 64, 4
    mask = torch.from_numpy(durations(L, [300, 257, 140])).to(dev)
    kw = dict(win=21, keep=6, k=3, min_sep=2, return_scores=True, return_bounds=True, return_order=True)
    for dt in (None, _op16()):
        text, video = _features(B, L, d, Q, 31, dt)
        gt = torch.tensor([[[30.0, 50.0]] * Q] * B)
        for t, g in ((text.to(dev), gt.to(dev)), (text[:, 0].contiguous().to(dev), gt[:, 0].contiguous().to(dev))):
            out = select_windows_clipped(t, video.to(dev), mask, gt=g, **kw)
            sims = (ops.frame_cosine_multi if t.dim() == 3 else ops.frame_cosine)(t.float(), video.to(dev))
            want = ops.window_select_clipped(sims, mask, gt=g, **kw)
            assert out.select.shape == t.shape[:-1] + (6,) and out.select.device == dev
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out, want))
            assert int(out.n_select.min()) == 6 and int(out.hit_rank.min()) >= 0
    host = select_windows_clipped(text, video, mask.cpu().bool(), **kw)                            # host tensors: staged, results back on the host
    assert not host.select.is_cuda and not host.scores.is_cuda and host.hit_rank is None
    again = select_windows_clipped(text.to(dev), video.to(dev), mask, **kw)
    assert torch.equal(host.select, again.select.cpu()) and torch.equal(_bits(host.scores), _bits(again.scores))


@pytest.mark.parametrize("ab", [(400, 460), (0, 30), (1250, 1300), (700, 1100)])
def test_clip_stage_windows_finds_a_planted_stretch(dev, ab):
    """Frames [a, b) equal to the query direction, the rest orthogonal to it: the list is sorted, distinct, of length min(keep, W), holds every window
    that contains a frame of the stretch when there are no more of them than ``keep``, and the tensor is the host route's rows."""
    from revisionllm_amd.eval import stage1
    a, b = ab
    ctx_l, d, nf = 1300, 16, 25
    feats = np.zeros((ctx_l, d), dtype=np.float32)
    feats[:, 1] = 1.0
    feats[:, 2:] = np.random.default_rng(a).normal(size=(ctx_l, d - 2)).astype(np.float32)         # rows differ: a wrong window shows in the tensor
    feats[a:b, 1] = 0.0
    feats[a:b, 0] = 2.0
    query = np.zeros(d, dtype=np.float32)
    query[0] = 0.5
    geometry = dict(debug_window=20, feature_fps=5, num_frames=nf)                                 # windows of 100 frames every 50: W = 25
    idx = stage1.cut_windows(ctx_l, **geometry)
    W = idx.shape[0]
    holding = [i for i in range(W) if i * 50 < b and min(i * 50 + 100, ctx_l - 1) + 1 > a]
    assert W == 25 and 1 <= len(holding) <= 10
    for given in (torch.from_numpy(feats).to(dev), torch.from_numpy(feats).to(dev).to(_op16())):
        full = stage1.gather_windows(given, **geometry)
        for keep in (len(holding), 12, 25, 40):
            windows, tensor = stage1.clip_stage_windows(given, query, keep=keep, **geometry)
            assert isinstance(windows, list) and all(type(i) is int for i in windows) and windows == sorted(set(windows)) and len(windows) == min(keep, W)
            assert all(0 <= i < W for i in windows) and set(holding) <= set(windows), (keep, holding, windows)
            assert tensor.shape == (len(windows), nf, d) and tensor.dtype == full.dtype and torch.equal(tensor, full[windows])
        host = given.float().cpu()[torch.from_numpy(idx[windows].astype(np.int64))]
        assert torch.equal(tensor.float().cpu(), host.to(tensor.dtype).float())
        spread, _ = stage1.clip_stage_windows(given, torch.from_numpy(query).to(dev), keep=6, min_sep=3, **geometry)
        assert len(spread) == 6 and min(np.diff(spread)) >= 3 and len(set(spread) & set(holding)) >= 1
        listed = stage1.gather_selected(given, holding, **geometry)
        assert torch.equal(listed, full[holding])


def test_the_stager_stages_a_selection(dev):
    """``WindowStager.stage_resident_selected`` on the staging stream: a host list (sorted on the way) and the pre-filter's own choice, both rows of
    ``stage_resident_clipped``'s tensor."""
    from revisionllm_amd.data.feature_store import WindowStager
    from revisionllm_amd.eval import stage1
    g = torch.Generator().manual_seed(12)
    feats, q = torch.randn(1300, 16, generator=g).to(dev), torch.randn(16, generator=g)
    geometry = dict(debug_window=20, feature_fps=5, num_frames=25)
    stager = WindowStager(dev, op_dtype=_op16())
    full = stager.stage_resident_clipped(feats, **geometry).wait()
    windows, staged = stager.stage_resident_selected(feats, windows=[7, 2, 11], **geometry)
    assert windows == [2, 7, 11] and torch.equal(staged.wait(), full[windows]) and full.dtype == _op16()
    picked, staged = stager.stage_resident_selected(feats, query_cls=q.numpy(), keep=5, **geometry)
    want, tensor = stage1.clip_stage_windows(feats, q, keep=5, dtype=_op16(), **geometry)
    assert picked == want and len(picked) == 5 and torch.equal(staged.wait(), tensor) and torch.equal(tensor, full[picked])
    for kw in (dict(), dict(windows=[1], query_cls=q, keep=2)):
        with pytest.raises(ValueError, match="stage_resident_selected"):
            stager.stage_resident_selected(feats, **kw, **geometry)


def test_score_query_selected_equals_score_query_device_with_padded_answers(dev):
    from revisionllm_amd.eval import stage1
    W, T, d = 9, 24, 32
    g = torch.Generator().manual_seed(9)
    q = torch.randn(d, generator=torch.Generator().manual_seed(4)).to(dev)
    answers = ["From 3 to 9.", "Not Present", "From 5 to 5.", "From 23 to 23.", "Between 2 and 30", "From 0 to 23.", "From 22 to 22.", "From 1 to 2.", "x"]
    ent = [0.5, 0.7, 0.2, 0.9, 0.4, 0.6, 0.8, 0.3, 0.1]
    for dtype in (torch.float32, _op16()):
        feats = torch.randn(W, T, d, generator=g).to(dtype).to(dev)
        for windows in ([0, 2, 4, 7], [1, 3, 8], list(range(W)), [5]):
            for topk_pool in (True, False):
                for score, merge in (("mean_entropy", "multiply"), ("max_entropy", "add"), ("cosine_sim", "multiply")):
                    for normalize in (True, False):
                        kw = dict(num_frames=T, debug_window=125, score=score, score_merge=merge, normalize=normalize, topk_pool=topk_pool)
                        e = [] if score == "cosine_sim" else ent
                        padded = [a if i in windows else "Not Present" for i, a in enumerate(answers)]
                        want = stage1.score_query_device(feats, padded, e, q, (10.0, 30.0), 300.0, **kw)
                        got = stage1.score_query_selected(feats[windows], windows, W, [answers[i] for i in windows], [e[i] for i in windows] if e else [], q,
                                                          (10.0, 30.0), 300.0, **kw)
                        assert got[0] == want[0] == padded and got[1]["iou"] == want[1]["iou"] and got[1]["scores"] == want[1]["scores"], (windows, kw)
                        assert got[1]["windows"] == windows and sorted(got[1]) == ["iou", "scores", "windows"]


def test_the_calls_do_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the calls: with the stream kept busy by work queued before them, an event recorded just before a
    call has not completed when the call returns (a call that waited for its own kernel would have waited for that work first)."""
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import select_windows_clipped
    text, video = _features(4, 300, 64, 3, 77, _op16())
    text, video, mask = text.to(dev), video.to(dev), torch.ones(4, 300, device=dev)
    sims = torch.from_numpy(bumpy(12, 300, 1)).view(4, 3, 300).to(dev)
    gt = torch.tensor([75.0, 150.0]).repeat(4, 3, 1).to(dev)
    one, flags = text[:, 0].contiguous(), mask.bool()
    calls = (lambda: ops.window_select_clipped(sims, mask, win=21, keep=10, min_sep=2, gt=gt, return_scores=True, return_bounds=True, return_order=True),
             lambda: select_windows_clipped(text, video, mask, win=21, keep=10, min_sep=3, gt=gt, return_order=True),
             lambda: select_windows_clipped(one, video, flags, win=20, keep=10))
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
