"""rvc_window_select_frames (the chain library's kernel behind ``ops.window_select_frames`` / ``eval.similarity.select_windows_frames`` / the two
``clip_stage_windows_frames``: the pre-filter's windows scored on a chosen frame set and on the frames a validity row leaves) against
tests/frames_select_oracle.py, the rule restated in numpy float32 with Python loops.  The oracle IS the rule, so ``select``, ``n_select``,
``n_windows``, ``n_candidates``, ``bounds``, ``order`` and ``hit_rank`` must be equal and ``win_scores`` must have the oracle's bits; there is no
tolerance.  tests/test_frames_select_host_logic.py holds the oracle itself to a brute-force statement of the selection and to both ``cut_windows``.

Every direct call writes into buffers with 64 sentinel elements on either side of each output; the surroundings are compared bitwise.  In every case
the frames of ``sims`` from D on are NaN: a read past the duration would show in a score.  Every case runs twice: with every optional output and with
none; ``select`` must not change.  The kernel is f32 only and the chain library has one build, so the kernel items run once (``kdev``); the items that
call the flavoured libraries around it run in both builds (``dev``).

The one comparison with a tolerance is ``test_sampled_scores_against_window_cosine``: its docstring says where the bound comes from and for which
features the two definitions coincide."""
import functools
import os

import numpy as np
import pytest
import torch

import frames_select_oracle as FO
from helpers import fl
from test_gpu_window_select import _Guarded, bumpy, durations, fenced, spans_gt

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")
NAN, INF = float("nan"), float("inf")
F = np.float32
SHIFTED, CLIPPED, ALL, SAMPLED = FO.SHIFTED, FO.CLIPPED, FO.ALL, FO.SAMPLED
KEYS = ("select", "n_select", "n_windows", "n_candidates", "bounds", "order", "hit_rank")


@pytest.fixture(scope="module")
def kdev(op_flavour):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import hip
    hip.chain_lib()
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
    hip.lib(), hip.ext_lib(), hip.chain_lib()
    return torch.device("cuda:0")


# ------------------------------------------------------------------ running the entry ------------------------------------------------------------------
def call(dev, o, s, m, v, g, R, M, L, rule, win, stride, frames, nf, k, keep, min_sep, Wcap):
    from revisionllm_amd import hip
    ptr = lambda x: x.ptr if x is not None else None                                            # noqa: E731
    return hip.chain_lib().rvc_window_select_frames(hip.ptr(s), hip.ptr(m), hip.ptr(v), R, R // M, L, rule, win, stride, frames, nf, k, keep, min_sep, Wcap,
                                                    hip.ptr(g) if o["hit_rank"] else None, ptr(o["select"]), ptr(o["n_select"]), ptr(o["n_windows"]),
                                                    ptr(o["n_candidates"]), ptr(o["win_scores"]), ptr(o["bounds"]), ptr(o["order"]), ptr(o["hit_rank"]),
                                                    hip.stream())


def run(dev, sims, mask, rule, win, stride, frames, nf, k, keep, min_sep, valid=None, gt=None, full=True):
    """The C entry on numpy inputs -> dict like the oracle's (parts not asked for: None), after the sentinel checks."""
    from revisionllm_amd import hip
    R, L = sims.shape
    M = mask.shape[0]
    Wcap = FO.capacity(L, win, stride)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=F)).to(dev) if x is not None else None      # noqa: E731
    s, m, v, g = up(sims), up(mask), up(valid), up(gt)
    o = dict(select=_Guarded(R * keep, torch.int32, dev), n_select=_Guarded(R, torch.int32, dev), n_windows=_Guarded(R, torch.int32, dev),
             n_candidates=_Guarded(R, torch.int32, dev), win_scores=_Guarded(R * Wcap, torch.float32, dev) if full else None,
             bounds=_Guarded(M * Wcap * 2, torch.int32, dev) if full else None, order=_Guarded(R * Wcap, torch.int32, dev) if full else None,
             hit_rank=_Guarded(R, torch.int32, dev) if full and gt is not None else None)
    hip.chain_check(call(dev, o, s, m, v, g, R, M, L, rule, win, stride, frames, nf, k, keep, min_sep, Wcap), "rvc_window_select_frames")
    torch.cuda.synchronize()
    shapes = dict(select=(R, keep), n_select=(R,), n_windows=(R,), n_candidates=(R,), win_scores=(R, Wcap), bounds=(M, Wcap, 2), order=(R, Wcap),
                  hit_rank=(R,))
    return {k_: (x.take(shapes[k_]) if x is not None else None) for k_, x in o.items()}


def same(got, ref, what=""):
    for k_ in KEYS:
        if got[k_] is not None:
            assert np.array_equal(got[k_], ref[k_]), (what, k_, np.argwhere(got[k_] != ref[k_])[:4].tolist())
    if got["win_scores"] is not None:
        a, b = got["win_scores"].view(np.uint32), np.ascontiguousarray(ref["win_scores"]).view(np.uint32)
        assert np.array_equal(a, b), (what, "win_scores", np.argwhere(a != b)[:4].tolist())


@functools.lru_cache(maxsize=None)
def _oracle(sims_b, sims_shape, mask_b, mask_shape, valid_b, gt_b, params):
    """The oracle once per distinct case."""
    sims = np.frombuffer(sims_b, dtype=F).reshape(sims_shape)
    mask = np.frombuffer(mask_b, dtype=F).reshape(mask_shape)
    valid = np.frombuffer(valid_b, dtype=F).reshape(mask_shape) if valid_b is not None else None
    gt = np.frombuffer(gt_b, dtype=F).reshape(sims_shape[0], 2) if gt_b is not None else None
    return FO.select(sims, mask, *params, valid=valid, gt=gt)


def check(dev, sims, mask, rule, win, stride=2, frames=ALL, nf=0, k=3, keep=5, min_sep=1, valid=None, gt=None, what=""):
    """Fence, run with every output and with none, compare both with the oracle -> (got, ref)."""
    sims = fenced(sims, mask)
    Wcap = FO.capacity(sims.shape[1], win, stride)
    keep, min_sep = min(keep, Wcap), min(min_sep, Wcap)
    gt = np.ascontiguousarray(gt, dtype=F) if gt is not None else None
    valid = np.ascontiguousarray(valid, dtype=F) if valid is not None else None
    what = f"{what} rule={rule} win={win} stride={stride} frames={frames} F={nf} k={k} keep={keep} sep={min_sep} valid={valid is not None}"
    ref = _oracle(sims.tobytes(), sims.shape, mask.tobytes(), mask.shape, valid.tobytes() if valid is not None else None,
                  gt.tobytes() if gt is not None else None, (rule, win, stride, frames, nf, k, keep, min_sep))
    got = run(dev, sims, mask, rule, win, stride, frames, nf, k, keep, min_sep, valid, gt)
    same(got, ref, what)
    same(run(dev, sims, mask, rule, win, stride, frames, nf, k, keep, min_sep, valid, None, full=False), ref, what + " (select only)")
    for r in range(sims.shape[0]):                                   # a non-candidate is in neither list, and the counts are ordered
        W, C = int(ref["n_windows"][r]), int(ref["n_candidates"][r])
        dead = {i for i in range(W) if np.isnan(ref["win_scores"][r, i]) and i not in ref["order"][r, :C]}
        assert C <= W <= Wcap and len(dead) == W - C and not dead & set(got["select"][r].tolist()) and not dead & set(got["order"][r].tolist())
        assert int(got["n_select"][r]) == min(keep, C)
    return got, ref


def every_other(M, L, phase=0):
    v = np.ones((M, L), dtype=F)
    v[:, phase::2] = 0
    return v


def _stride(win):
    return 2 if win < 5 else 5


# ------------------------------------------------------------------ geometries and frame sets ------------------------------------------------------------------
@pytest.mark.parametrize("win", [2, 3, 5, 11, 64])
@pytest.mark.parametrize("rule", [SHIFTED, CLIPPED])
def test_geometries_and_frame_sets(kdev, rule, win):
    """D = L, L - 1, win, 1 and 0; every frame, F = 1, 2, 3, 7, the window's length, and 31 at win = 11 (a frame sampled up to three times: ties go
    to the position); without ``valid`` and with every other frame hidden."""
    L = max(40, 3 * win + 4)
    stride = 2 if rule == CLIPPED else _stride(win)
    Ds = [L, L - 1, win, 1, 0]
    sims, mask, gt = bumpy(5, L, win), durations(L, Ds), spans_gt(5, L, win)
    sims[0, ::5] = sims[0, 1]                                                             # equal values at several frames
    for frames, nf in [(ALL, 0)] + [(SAMPLED, n) for n in (1, 2, 3, 7, win + 1)] + ([(SAMPLED, 31)] if win == 11 else []):
        for valid in (None, every_other(5, L, 1)):
            _, ref = check(kdev, sims, mask, rule, win, stride, frames, nf, keep=5, min_sep=2, valid=valid, gt=gt)
            assert ref["D"] == Ds and ref["n_windows"][3] == ref["n_windows"][4] == 0
            if valid is None:
                assert ref["n_candidates"].tolist() == ref["n_windows"].tolist()


def test_clipped_last_windows_and_the_void_suffix(kdev):
    """win = 5: D = 13 ends in a window of one frame, D = 15 has a void index; win = 3 at D = 600 a long void suffix."""
    valid = np.ones((4, 20), dtype=F)
    valid[0, 12] = 0                                                                       # the one-frame window [12, 13) loses its frame
    valid[3, 15:] = 0
    for frames, nf in ((ALL, 0), (SAMPLED, 3), (SAMPLED, 9)):
        _, ref = check(kdev, bumpy(4, 20, 1), durations(20, [13, 15, 14, 20]), CLIPPED, 5, 2, frames, nf, keep=9, min_sep=2, valid=valid, gt=spans_gt(4, 20, 2))
        assert ref["n_windows"].tolist() == [6, 6, 6, 8] and ref["bounds"][0, 5].tolist() == [12, 13] and ref["n_candidates"][0] == 5
        assert np.isnan(ref["win_scores"][0, 5]) and ref["bounds"][1, 6].tolist() == [-1, -1]
    _, ref = check(kdev, bumpy(2, 600, 3), durations(600, [600, 6]), CLIPPED, 3, 2, SAMPLED, 2, keep=450, valid=every_other(2, 600))
    assert ref["n_windows"].tolist() == [400, 4]


@pytest.mark.parametrize("k", [1, 3, 64])
@pytest.mark.parametrize("rule", [SHIFTED, CLIPPED])
def test_validity_patterns_and_k(kdev, rule, k):
    """A hidden head, interior and tail, every other frame hidden, one usable frame in the row; NaN and +-inf lie under hidden frames only, so no
    score may be NaN or infinite; k = 64 is above every window's usable count."""
    L, win = 120, 11
    valid = np.ones((6, L), dtype=F)
    valid[0, :37] = 0
    valid[1, 40:77] = 0
    valid[2, 90:] = 0
    valid[3] = every_other(1, L)[0]
    valid[4, :] = 0
    valid[4, 63] = 1
    valid[5, 10:20] = np.array([-0.0, NAN, 2.0, -1.0, 0.0, 1e-30, INF, 0.0, 0.5, -0.0], dtype=F)   # -0 hides, everything else that is not 0 shows
    sims = bumpy(6, L, 5 + k)
    hidden = valid == 0
    sims[hidden & (np.arange(L)[None] % 3 == 0)] = NAN
    sims[hidden & (np.arange(L)[None] % 3 == 1)] = INF
    sims[hidden & (np.arange(L)[None] % 3 == 2)] = -INF
    mask = durations(L, [L, L, L, L - 3, L, L])
    for frames, nf in ((ALL, 0), (SAMPLED, 7), (SAMPLED, 12), (SAMPLED, 31)):
        got, ref = check(kdev, sims, mask, rule, win, 2 if rule == CLIPPED else 5, frames, nf, k=k, keep=6, min_sep=2, valid=valid, gt=spans_gt(6, L, k))
        for r in range(6):
            C = int(ref["n_candidates"][r])
            shown = got["win_scores"][r][~np.isnan(got["win_scores"][r])]
            assert len(shown) == C and np.isfinite(shown).all(), (r, "a hidden frame leaked")
        assert 0 < ref["n_candidates"][0] < ref["n_windows"][0] and ref["n_candidates"][4] <= 6 and (frames == SAMPLED or ref["n_candidates"][4] >= 2)


def test_windows_without_a_usable_frame(kdev):
    """win = 8, stride 2, D = 80: windows [4 i, 4 i + 9).  ``valid`` empties windows at the front, in the middle and at the end; ``keep`` lies on
    both sides of n_candidates; min_sep = 2 counts indices across the gap; a ground truth that only a non-candidate covers has no hit; a candidate
    whose score is NaN ranks last among the candidates and in front of no non-candidate."""
    L = 80
    valid = np.ones((1, L), dtype=F)
    valid[0, 0:13] = 0            # windows 0 and 1 ([0, 9), [4, 13)) are empty; window 2 keeps frames 13 .. 16
    valid[0, 36:49] = 0           # windows 9 and 10 ([36, 45), [40, 49))
    valid[0, 68:] = 0             # windows 17 and 18 ([68, 77), [71, 80))
    sims = np.tile(bumpy(1, L, 4), (6, 1))
    sims[:, 50] = 3.0                                                                      # windows 11 and 12 tie for the best
    sims[1, 30] = NAN                                                                      # row 1: windows 6 and 7 have a NaN score, next to nothing
    sims[2, 33] = NAN                                                                      # row 2: windows 7 and 8 ([32, 41)) are NaN-scored, 8 borders the gap
    gt = np.array([[38.0, 40.0], [41.0, 44.0], [0.0, 3.0], [78.0, 80.0], [10.0, 14.0], [44.5, 50.0]])
    for rule in (SHIFTED, CLIPPED):
        for keep in (3, 13, 14, 19):
            for min_sep in (1, 2):
                got, ref = check(kdev, sims, durations(L, [L]), rule, 8, 2, ALL, 0, k=3, keep=keep, min_sep=min_sep, valid=valid, gt=gt)
                dead = [0, 1, 9, 10, 17, 18]
                assert ref["n_windows"].tolist() == [19] * 6 and ref["n_candidates"].tolist() == [13] * 6 and ref["n_select"].tolist() == [min(keep, 13)] * 6
                assert np.isnan(ref["win_scores"][0, dead]).all() and (ref["bounds"][0, [0, 9, 18]] >= 0).all() and (ref["order"][:, 13:] == -1).all()
                if min_sep == 1:                                                           # NaN scores: last of the candidates, by index
                    assert ref["order"][2, 11:13].tolist() == [7, 8] and ref["order"][1, 11:13].tolist() == [6, 7]
                # gt 0 lies in [38, 40): windows 8 (a candidate, [32, 41)) and 9; gt 1 in [41, 44): only 9 and 10; gt 2, 3: only the empty ends
                assert ref["hit_rank"][0] >= 0 and ref["hit_rank"].tolist()[1:4] == [-1, -1, -1] and ref["hit_rank"][4] >= 0 and ref["hit_rank"][5] >= 0
                if min_sep == 2:
                    first = ref["order"][0, :2].tolist()
                    assert abs(first[0] - first[1]) >= 2
    # sampled: F = 2 reads a window's first and last frame only, so a window whose two ends are hidden is no candidate although frames between are usable
    v2 = np.ones((1, L), dtype=F)
    v2[0, [8, 16]] = 0                                                                     # window 2 = [8, 17): both sampled frames hidden
    _, ref = check(kdev, sims[:2], durations(L, [L]), SHIFTED, 8, 2, SAMPLED, 2, keep=19, min_sep=2, valid=v2, gt=gt[:2])
    assert np.isnan(ref["win_scores"][0, 2]) and ref["n_candidates"].tolist() == [18, 18] and 2 not in ref["select"][0]


def test_1024_sampled_frames_and_the_refusal_past_them(kdev):
    """F = 1024 on windows of 6 and 12 frames (every frame is sampled some 170 / 85 times: the top-k are copies of the best frame); 1025 is refused."""
    L = 60
    for rule, win in ((SHIFTED, 5), (CLIPPED, 11)):
        check(kdev, bumpy(2, L, win), durations(L, [L, 41]), rule, win, 2 if rule == CLIPPED else 5, SAMPLED, 1024, k=3, keep=4, valid=every_other(2, L))
        got, ref = check(kdev, bumpy(2, L, win), durations(L, [L, 41]), rule, win, 2 if rule == CLIPPED else 5, SAMPLED, 1024, k=64, keep=4)
    from revisionllm_amd import hip
    one = torch.zeros(64, device=kdev)
    o = dict(select=_Guarded(4, torch.int32, kdev), n_select=_Guarded(1, torch.int32, kdev), n_windows=_Guarded(1, torch.int32, kdev),
             n_candidates=_Guarded(1, torch.int32, kdev), win_scores=None, bounds=None, order=None, hit_rank=None)
    rc = call(kdev, o, one, one, None, None, 1, 1, 60, SHIFTED, 5, 5, SAMPLED, 1025, 3, 4, 1, FO.capacity(60, 5, 5))
    assert rc == -1 and "F=1025 sampled frames per window must be in [1, 1024]" in hip.chain_last_error()
    torch.cuda.synchronize()
    assert all(x.take((x.n,)).tolist() == [x.sentinel] * x.n for x in o.values() if x is not None)      # outputs untouched


@pytest.mark.parametrize("rule", [SHIFTED, CLIPPED])
def test_2048_windows(kdev, rule):
    """W = 2048 (win = 2, stride 2, L = 2049) with every third frame hidden, the longest greedy walk (keep = W, min_sep = 2), sampled F = 2 and all."""
    L = 2049
    valid = np.ones((1, L), dtype=F)
    valid[0, ::3] = 0
    valid[0, 600:640] = 0
    sims = bumpy(2, L, 7)
    _, ref = check(kdev, sims, durations(L, [L]), rule, 2, 2, SAMPLED, 2, k=2, keep=2048, min_sep=2, valid=valid, gt=np.array([[2047.5, 2048.0], [610.0, 620.0]]))
    assert ref["n_windows"].tolist() == [2048, 2048] and 1900 < ref["n_candidates"][0] < 2048 and ref["hit_rank"][1] == -1
    check(kdev, sims, durations(L, [L]), rule, 2, 2, ALL, 0, k=1, keep=100, min_sep=1, valid=valid)


@pytest.mark.parametrize("win", [1023, 1024])
def test_the_register_switch_of_the_all_path_under_valid(kdev, win):
    """An unclipped window has win + 1 frames: 1024 (the last that a wave ranks from registers) and 1025 (read again from the row in every round)."""
    L = 2600
    Ds = [L, L - 1, win + 1, 1500]
    valid = every_other(4, L)
    valid[1, 200:1400] = 0
    valid[2, :] = 0
    valid[2, 5] = 1
    for k in (1, 3, 64):
        for rule in (SHIFTED, CLIPPED):
            _, ref = check(kdev, bumpy(4, L, win + k), durations(L, Ds), rule, win, 2, ALL, 0, k=k, keep=3, min_sep=2, valid=valid, gt=spans_gt(4, L, k))
    assert (ref["bounds"][0, 0, 1] - ref["bounds"][0, 0, 0]) == win + 1
    check(kdev, bumpy(4, L, win), durations(L, Ds), SHIFTED, win, 2, SAMPLED, 250, k=3, keep=3, valid=valid)


@pytest.mark.parametrize("R", [1, 4, 260])
def test_row_counts(kdev, R):
    L = 90
    rng = np.random.default_rng(R)
    valid = (rng.random((R, L)) < 0.6).astype(F)
    for rule, frames, nf in ((SHIFTED, SAMPLED, 4), (CLIPPED, ALL, 0)):
        check(kdev, bumpy(R, L, 40 + R), durations(L, rng.integers(0, L + 1, R)), rule, 9, 2 if rule == CLIPPED else 3, frames, nf, keep=7, min_sep=2,
              valid=valid, gt=spans_gt(R, L, R))


def test_three_rows_per_mask_row_and_row_independence(kdev):
    L = 150
    Ds = [150, 129, 64, 0]
    valid = every_other(4, L)
    valid[1, 30:80] = 0
    sims, mask, gt = bumpy(12, L, 3), durations(L, Ds), spans_gt(12, L, 9)
    got, ref = check(kdev, sims, mask, CLIPPED, 11, 2, SAMPLED, 5, keep=6, min_sep=3, valid=valid, gt=gt, what="rpm=3")
    assert ref["D"] == [150] * 3 + [129] * 3 + [64] * 3 + [0] * 3 and got["bounds"].shape == (4, 29, 2)
    assert len({got["select"][r].tobytes() for r in range(3)}) > 1
    sims = fenced(sims, mask)
    whole = run(kdev, sims, mask, CLIPPED, 11, 2, SAMPLED, 5, 3, 6, 3, valid, gt)
    for r in (0, 3, 9):                                              # a mask row's three rows alone
        alone = run(kdev, sims[r:r + 3], mask[r // 3:r // 3 + 1], CLIPPED, 11, 2, SAMPLED, 5, 3, 6, 3, valid[r // 3:r // 3 + 1], gt[r:r + 3])
        for k_ in whole:
            lo, n = (r // 3, 1) if k_ == "bounds" else (r, 3)
            assert np.ascontiguousarray(whole[k_][lo:lo + n]).tobytes() == np.ascontiguousarray(alone[k_]).tobytes(), (r, k_)


# ------------------------------------------------------------------ the Python surface ------------------------------------------------------------------
def _as_dict(out, R, keep, Wcap):
    return dict(select=out.select.cpu().numpy().reshape(R, keep), n_select=out.n_select.cpu().numpy().reshape(-1), n_windows=out.n_windows.cpu().numpy().reshape(-1),
                n_candidates=out.n_candidates.cpu().numpy().reshape(-1), win_scores=out.scores.cpu().numpy().reshape(R, Wcap), bounds=out.bounds.cpu().numpy(),
                order=out.order.cpu().numpy().reshape(R, Wcap), hit_rank=out.hit_rank.cpu().numpy().reshape(-1))


def test_the_bql_form_the_valid_dtypes_and_the_optional_parts(kdev):
    from revisionllm_amd import ops
    B, Q, L = 3, 4, 200
    mask = durations(L, [200, 131, 77])
    valid = every_other(3, L)
    valid[0, 50:90] = 0
    sims = fenced(bumpy(B * Q, L, 17), mask)
    gt = spans_gt(B * Q, L, 4)
    ref = FO.select(sims, mask, CLIPPED, 11, 2, SAMPLED, 6, 3, 8, 2, valid=valid, gt=gt)
    Wcap = FO.capacity(L, 11, 2)
    s, m, g = torch.from_numpy(sims).view(B, Q, L).to(kdev), torch.from_numpy(mask).to(kdev), torch.from_numpy(gt).view(B, Q, 2).to(kdev)
    v = torch.from_numpy(valid).to(kdev)
    kw = dict(rule="clipped", win=11, keep=8, frames="sampled", num_frames=6, min_sep=2)
    for vk in (v, v.bool(), v.to(torch.uint8), v.half(), v.double()):
        out = ops.window_select_frames(s, m.bool(), valid=vk, gt=g, return_scores=True, return_bounds=True, return_order=True, **kw)
        assert isinstance(out, ops.FrameWindowSelection) and out.select.shape == (B, Q, 8) and out.n_candidates.shape == (B, Q) == out.n_windows.shape
        assert out.scores.shape == (B, Q, Wcap) == out.order.shape and out.bounds.shape == (B, Wcap, 2)
        same(_as_dict(out, B * Q, 8, Wcap), ref, str(vk.dtype))
    bare = ops.window_select_frames(s, m, valid=v, **kw)
    assert bare.scores is None and bare.bounds is None and bare.order is None and bare.hit_rank is None and torch.equal(bare.select, out.select)
    flat = ops.window_select_frames(s.view(B * Q, L), m, valid=v, **kw)
    assert torch.equal(flat.select, out.select.view(B * Q, 8)) and torch.equal(flat.n_candidates, out.n_candidates.view(-1))
    big = ops.window_select_frames(s, m, valid=v, **{**kw, "keep": 5000})                            # keep above Wcap is Wcap
    assert big.select.shape == (B, Q, Wcap) and torch.equal(big.n_select, big.n_candidates)


def _bits(t):
    return t.cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.cpu()


def _equal(a, b):
    return all((x is None and y is None) or torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("win,stride,L", [(10, 5, 300), (61, 2, 300), (5, 2, 83), (625, 5, 3000), (1024, 2, 2600)])
def test_all_frames_without_valid_is_the_existing_selection_bit_for_bit(dev, win, stride, L):
    """``frames="all"``, ``valid=None``: every output equals ``ops.window_select`` (shifted) or ``ops.window_select_clipped`` (clipped), and
    n_candidates == n_windows; ``valid`` all ones changes nothing."""
    from revisionllm_amd import ops
    mask = durations(L, [L, L - 7, (L + win) // 2])
    sims = fenced(bumpy(6, L, win), mask)
    sims[0, L // 3] = NAN
    s, m, g = torch.from_numpy(sims).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(spans_gt(6, L, 3)).to(dev)
    kw = dict(win=win, keep=10, k=3, min_sep=2, gt=g, return_scores=True, return_bounds=True, return_order=True)
    pairs = [(ops.window_select(s, m, stride=stride, **kw), dict(rule="shifted", stride=stride))]
    if stride == 2:
        pairs.append((ops.window_select_clipped(s, m, **kw), dict(rule="clipped")))
    for want, rule in pairs:
        got = ops.window_select_frames(s, m, **rule, **kw)
        assert _equal(got[:7], want) and torch.equal(got.n_candidates, got.n_windows), rule
        ones = ops.window_select_frames(s, m, valid=torch.ones_like(m), **rule, **kw)
        assert _equal(ones, got), rule
        bare = ops.window_select_frames(s, m, **rule, win=win, keep=10, k=3, min_sep=2)
        assert torch.equal(bare.select, want.select) and torch.equal(bare.n_select, want.n_select)


@pytest.mark.parametrize("win,stride,L", [(10, 5, 300), (61, 2, 300), (5, 2, 83), (11, 2, 150)])
def test_sampling_every_frame_is_all_frames(dev, win, stride, L):
    """``frames="sampled"`` with F equal to a window's length: ``np.linspace(s, s + n, n + 1)`` has the step exactly 1.0, so every frame comes once
    and in order, and every unclipped window has the score bits of ``frames="all"``.  Shifted windows all have win + 1 frames (ctx_l > win); the
    clipped rule's length is taken from ``bounds``."""
    from revisionllm_amd import ops
    mask = durations(L, [L, L - 7, (L + win) // 2 + 1])
    sims = fenced(bumpy(3, L, win + 1), mask)
    s, m = torch.from_numpy(sims).to(dev), torch.from_numpy(mask).to(dev)
    v = torch.from_numpy(every_other(3, L)).to(dev)
    for rule in [dict(rule="shifted", stride=stride)] + ([dict(rule="clipped")] if stride == 2 else []):
        for valid in (None, v):
            kw = dict(win=win, keep=10, valid=valid, return_scores=True, return_bounds=True, return_order=True, **rule)
            every = ops.window_select_frames(s, m, **kw)
            length = int((every.bounds[0, 0, 1] - every.bounds[0, 0, 0]))
            assert length == win + 1
            sampled = ops.window_select_frames(s, m, frames="sampled", num_frames=length, **kw)
            whole = (every.bounds[..., 1] - every.bounds[..., 0]) == length
            assert int(whole.sum()) >= 3 and torch.equal(sampled.bounds, every.bounds)
            assert torch.equal(_bits(sampled.scores)[whole.cpu()], _bits(every.scores)[whole.cpu()])
            if bool(whole[every.bounds[..., 0] >= 0].all()):
                assert _equal(sampled, every)


@pytest.mark.parametrize("rule", ["shifted", "clipped"])
def test_valid_is_minus_infinity_where_every_window_keeps_k_frames(dev, rule):
    """With at least k usable frames in every window, hiding a frame is giving it -inf: scores and selection equal ``frames="all"`` on
    ``sims.masked_fill(valid == 0, -inf)`` (a window's top k never reach a -inf then)."""
    from revisionllm_amd import ops
    L, win, k = 300, 20, 3
    mask = durations(L, [L, 250])
    sims = fenced(bumpy(4, L, 8), mask)
    valid = every_other(2, L)
    valid[0, 100:140:3] = 0
    s, m, v = torch.from_numpy(sims).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(valid).to(dev)
    kw = dict(rule=rule, win=win, stride=2, keep=9, k=k, min_sep=2, return_scores=True, return_bounds=True, return_order=True)
    got = ops.window_select_frames(s, m, valid=v, **kw)
    filled = s.masked_fill(v.repeat_interleave(2, 0) == 0, -INF)
    want = ops.window_select_frames(filled, m, **kw)
    assert torch.equal(got.n_candidates, got.n_windows) and _equal(got, want) and bool(torch.isfinite(got.scores[0, :int(got.n_windows[0])]).all())
    old = ops.window_select(filled, m, win=win, stride=2, keep=9, k=k, min_sep=2) if rule == "shifted" else ops.window_select_clipped(filled, m, win=win, keep=9, k=k, min_sep=2)
    assert torch.equal(got.select, old.select)


def _op16():
    return torch.float16 if fl() == "f16" else torch.bfloat16


@pytest.mark.parametrize("win,nf", [(20, 12), (11, 31), (61, 7), (5, 1), (64, 65)])
def test_the_sampled_frames_are_the_gathers(dev, win, nf):
    """The oracle's sample indices (and so the kernel's, which is held to the oracle's scores) are ``ops.window_gather(..., return_index=True)``'s and
    ``ops.window_gather_clipped``'s, window by window."""
    from revisionllm_amd import ops
    L, d = 330, 8
    video = torch.randn(L, d, generator=torch.Generator().manual_seed(win)).to(dev)
    for rule, stride in ((SHIFTED, 2), (SHIFTED, min(win, 5)), (CLIPPED, 2)):
        wins = FO.windows(L, rule, win, stride)
        sel = torch.arange(len(wins), dtype=torch.int32, device=dev)
        if rule == SHIFTED:
            _, idx = ops.window_gather(video, sel, win=win, stride=stride, num_frames=nf, return_index=True)
        else:
            _, idx = ops.window_gather_clipped(video, win=win, num_frames=nf, select=sel, return_index=True)
        want = np.stack([FO.sample_indices(lo, hi, nf) for lo, hi in wins])
        assert np.array_equal(idx.cpu().numpy(), want), (rule, stride)


@pytest.mark.parametrize("rule", ["shifted", "clipped"])
def test_sampled_scores_against_window_cosine(dev, rule):
    """Sampled ``win_scores`` against ``stage2.window_cosine`` on the gathered f32 windows, within (k + 1) * 1e-4 absolute: the project's 1e-4 bound on
    a cosine row entry times the k picked entries, plus its 1e-4 bound on ``rv_topk_cosine``; a top-k sum is k-Lipschitz in the row, so near-ties
    cannot break it.  ``window_cosine`` is the reference's score: it divides every COLUMN by its norm over the window's frames and does not normalise
    the query, where a cosine row divides every FRAME by its norm and the query by its own.  The two are the same number exactly when every frame has
    one norm n and every column one norm c, and |q| = c / n.  Features of +-1 have that: n = sqrt(d), c = sqrt(F) in every window, so the query is
    scaled to |q| = sqrt(F / d).  For other features the two definitions differ by more than rounding and no bound of this kind holds."""
    from revisionllm_amd import ops
    from revisionllm_amd.eval import stage2
    L, d, win, nf, k = 400, 64, 61, 31, 3
    g = torch.Generator().manual_seed(3)
    video = (torch.randint(0, 2, (L, d), generator=g) * 2 - 1).float()
    q = torch.randn(d, generator=g)
    video[120:150] = torch.sign(q) * torch.where(torch.rand(30, d, generator=g) < 0.8, 1.0, -1.0)      # a stretch that leans towards the query
    q = q / q.norm() * (nf / d) ** 0.5
    video, q = video.to(dev), q.to(dev)
    sims = ops.frame_cosine(q[None], video[None])
    mask = torch.ones(1, L, device=dev)
    out = ops.window_select_frames(sims, mask, rule=rule, win=win, stride=2, keep=5, frames="sampled", num_frames=nf, k=k, return_scores=True)
    W = int(out.n_windows[0])
    sel = torch.arange(W, dtype=torch.int32, device=dev)
    if rule == "shifted":
        windows = ops.window_gather(video, sel, win=win, stride=2, num_frames=nf, out_dtype=torch.float32)
    else:
        windows = ops.window_gather_clipped(video, win=win, num_frames=nf, select=sel, out_dtype=torch.float32)
    want = stage2.window_cosine(windows, q, k).cpu()
    got = out.scores[0, :W].cpu()
    err = (got - want).abs().max().item()
    print(f"window_cosine: W={W} max |sampled score - window_cosine| = {err:.3e} (bound {(k + 1) * 1e-4:.1e}), scores {got.min().item():.4f} .. {got.max().item():.4f}")
    assert W >= 10 and err <= (k + 1) * 1e-4
    assert got.max().item() > got.median().item() + 0.1                                     # the planted stretch stands out: the scores are not all alike


# ------------------------------------------------------------------ the chain ------------------------------------------------------------------
def _features(B, L, d, Q, seed, op16):
    g = torch.Generator().manual_seed(seed)
    video = torch.randn(B, L, d, generator=g)
    text = torch.randn(B, Q, d, generator=g)
    for b in range(B):
        for q in range(Q):
            a = 20 + 37 * q + 11 * b
            video[b, a:a + 25 + 9 * q] += 1.5 * text[b, q]
    return text, video.to(op16) if op16 is not None else video


def test_select_windows_frames_is_the_two_calls_chained(dev):
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import select_windows_frames
    B, L, d, Q = 3, 300, 64, 4
    mask = torch.from_numpy(durations(L, [300, 257, 140])).to(dev)
    valid = torch.from_numpy(every_other(3, L)).to(dev)
    kw = dict(rule="clipped", win=21, keep=6, frames="sampled", num_frames=9, k=3, min_sep=2, return_scores=True, return_bounds=True, return_order=True)
    for dt in (None, _op16()):
        text, video = _features(B, L, d, Q, 31, dt)
        video[1, 40:50] = 0                                                                   # zero rows: NaN cosines, hidden by valid
        v = valid.clone()
        v[1, 40:50] = 0
        gt = torch.tensor([[[30.0, 50.0]] * Q] * B)
        for t, g in ((text.to(dev), gt.to(dev)), (text[:, 0].contiguous().to(dev), gt[:, 0].contiguous().to(dev))):
            out = select_windows_frames(t, video.to(dev), mask, valid=v, gt=g, **kw)
            sims = (ops.frame_cosine_multi if t.dim() == 3 else ops.frame_cosine)(t.float(), video.to(dev))
            want = ops.window_select_frames(sims, mask, valid=v, gt=g, **kw)
            assert isinstance(out, ops.FrameWindowSelection) and out.select.shape == t.shape[:-1] + (6,) and out.select.device == dev
            assert _equal(out, want) and bool(torch.isnan(sims[1, ..., 40:50]).all())
            W = int(out.n_windows.view(B, -1)[1, 0])
            assert not bool(torch.isnan(out.scores.view(B, -1, out.scores.shape[-1])[1, :, :W]).any())      # the NaN cosines left no trace
    host = select_windows_frames(text, video, mask.cpu().bool(), valid=v.cpu().bool(), **kw)          # host tensors: staged, results back on the host
    assert not host.select.is_cuda and not host.n_candidates.is_cuda and host.hit_rank is None
    again = select_windows_frames(text.to(dev), video.to(dev), mask, valid=v, **kw)
    assert torch.equal(host.select, again.select.cpu()) and torch.equal(_bits(host.scores), _bits(again.scores))


def test_clip_stage_windows_frames_both_stages(dev):
    """The list is ``select_windows_frames``' row, the tensor is the gather's rows of that list, ``score_frames="all"`` is ``clip_stage_windows``, and a
    planted stretch that only unsampled frames hold is found by "all" and missed by "sampled"; a hidden stretch is not chosen for its own sake."""
    from revisionllm_amd.eval import stage1, stage2
    ctx_l, d, nf = 1300, 16, 5
    feats = np.zeros((ctx_l, d), dtype=np.float32)
    feats[:, 1] = 1.0
    feats[:, 2:] = np.random.default_rng(2).normal(size=(ctx_l, d - 2)).astype(np.float32) * 0.1
    query = np.zeros(d, dtype=np.float32)
    query[0] = 0.5
    for stage, geometry, pick in ((stage1, dict(debug_window=20, feature_fps=5, num_frames=nf), dict(keep=4)),
                                  (stage2, dict(debug_window=20, feature_fps=5, stride=2, num_frames=nf), dict(batch=4))):
        idx = stage.cut_windows(ctx_l, **geometry)
        idx = idx[1] if isinstance(idx, tuple) else idx
        f = feats.copy()
        hit = [t for t in range(405, 420) if t not in set(idx.reshape(-1).tolist())][:6]               # frames no window samples
        f[hit, 0], f[hit, 1] = 2.0, 0.0
        given = torch.from_numpy(f).to(dev)
        every, t_every = stage.clip_stage_windows_frames(given, query, score_frames="all", **geometry, **pick)
        old, t_old = stage.clip_stage_windows(given, query, **geometry, **pick)
        assert every == old and torch.equal(t_every, t_old) and all(type(i) is int for i in every)
        sampled, t_sampled = stage.clip_stage_windows_frames(given, query, **geometry, **pick)
        holding = [i for i in range(idx.shape[0]) if idx[i, 0] <= hit[0] and idx[i, -1] >= hit[-1]]
        assert holding and set(holding) <= set(every) and sampled != every and len(sampled) == 4 == len(every)
        full = torch.from_numpy(f)[torch.from_numpy(idx[sampled].astype(np.int64))]
        assert t_sampled.shape == (4, nf, d) and torch.equal(t_sampled.float().cpu(), full.to(t_sampled.dtype).float())
        valid = np.ones(ctx_l, dtype=bool)
        valid[400:425] = False
        for v in (valid, torch.from_numpy(valid).to(dev), torch.from_numpy(valid).float()):
            hidden, _ = stage.clip_stage_windows_frames(given, query, score_frames="all", valid=v, **geometry, **pick)
            assert hidden == sampled                                                         # without the stretch the rows are alike: ties by index


def test_the_stager_stages_a_sampled_selection(dev):
    from revisionllm_amd.data.feature_store import WindowStager
    from revisionllm_amd.eval import stage1
    g = torch.Generator().manual_seed(12)
    feats, q = torch.randn(1300, 16, generator=g).to(dev), torch.randn(16, generator=g)
    geometry = dict(debug_window=20, feature_fps=5, num_frames=25)
    stager = WindowStager(dev, op_dtype=_op16())
    full = stager.stage_resident_clipped(feats, **geometry).wait()
    picked, staged = stager.stage_resident_selected_frames(feats, query_cls=q.numpy(), keep=5, **geometry)
    want, tensor = stage1.clip_stage_windows_frames(feats, q, keep=5, dtype=_op16(), **geometry)
    assert picked == want and len(picked) == 5 and torch.equal(staged.wait(), tensor) and torch.equal(tensor, full[picked])


def test_the_calls_do_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the calls: with the stream kept busy by work queued before them, an event recorded just before a
    call has not completed when the call returns (a call that waited for its own kernel would have waited for that work first)."""
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import select_windows_frames
    text, video = _features(4, 300, 64, 3, 77, _op16())
    text, video, mask = text.to(dev), video.to(dev), torch.ones(4, 300, device=dev)
    valid = torch.from_numpy(every_other(4, 300)).to(dev)
    sims = torch.from_numpy(bumpy(12, 300, 1)).view(4, 3, 300).to(dev)
    gt = torch.tensor([75.0, 150.0]).repeat(4, 3, 1).to(dev)
    one, flags = text[:, 0].contiguous(), valid.bool()
    calls = (lambda: ops.window_select_frames(sims, mask, rule="shifted", win=21, stride=3, keep=10, frames="sampled", num_frames=8, valid=valid, min_sep=2, gt=gt,
                                              return_scores=True, return_bounds=True, return_order=True),
             lambda: select_windows_frames(text, video, mask, rule="clipped", win=21, keep=10, valid=flags, min_sep=3, gt=gt, return_order=True),
             lambda: select_windows_frames(one, video, mask.bool(), rule="shifted", win=20, stride=5, keep=10, frames="sampled", num_frames=250))
    for which, fn in enumerate(calls):
        want = fn()                                                                            # (warm: library loaded, allocator blocks cached)
        a = torch.ones(8192, 8192, device=dev)
        c = torch.empty_like(a)
        torch.mm(a, a, out=c)
        torch.cuda.synchronize()
        for _ in range(12):                                                                    # ~1.1 TFLOP of f32 each: tens of milliseconds of queued work
            torch.mm(a, a, out=c)
        ev = torch.cuda.Event()
        ev.record()
        got = fn()
        still_busy = not ev.query()
        torch.cuda.synchronize()
        assert still_busy, f"call {which} returned only after the work queued before it had finished: it synchronised"
        assert _equal(got, want)
