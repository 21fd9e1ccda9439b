"""rvc_span_scores_masked and rvc_span_propose_masked (the chain library's kernels behind ``ops.span_scores_masked`` / ``ops.span_propose_masked`` and
``eval.similarity``'s ``forward_clip_matching_masked`` / ``propose_spans_masked`` / ``ground_queries_masked``: the fine half of the grounding chain
over the frames a validity row does not hide and the similarities that are numbers) against tests/spans_masked_oracle.py, the two rules restated in
numpy float32 with Python loops.  The oracle IS the rule: integers, windows, spans, the smoothed row and the top-k scores must have the oracle's bits,
and nothing is excused.  tests/test_spans_masked_host_logic.py holds the oracle itself to a brute-force statement and to the identities of the header.

The one comparison with a tolerance is the attention mode (``test_attention_mode``): the kernel adds a window's terms lane by lane and then across
the lanes, the oracle in frame order.  The bound is 4 x the float32 statement's own distance from float64 on the same inputs
(``spans_masked_oracle.attention_cases``), per temperature - measured here again on the CPU, not a constant; the factor pays for the other summation
order.  Measured on MI355X (profiles/spans_masked_err_{f16,bf16}.log; the kernel is f32 and the same in both builds): kernel against float64 1.53e-7 at
temperature 0.01 and 1.48e-7 at 1, where the float32 statement stands at 2.44e-7 and 6.70e-7 (bounds 9.77e-7 and 2.68e-6).

Every direct call writes into buffers with 64 sentinel elements on either side of each output.  In every case ``sims`` is NaN from D on and NaN or
+-inf sits under every frame ``valid`` hides: a read of either would show.  Every case runs with all optional outputs and with none.  The kernels are
f32 only and the chain library has one build, so the kernel items run once (``kdev``); the items that go through the flavoured libraries (the cosine
rows, the unmasked siblings, the ranking) run in both builds (``dev``)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import spans_masked_oracle as MO
from helpers import fl
from test_gpu_window_select import _Guarded

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")
NAN, INF = float("nan"), float("inf")
F = np.float32
SENTINEL = F(-777.25)
LEVELS = (0.5, 0.6, 0.7, 0.8, 0.9)
TAUS = (0.01, 1.0)


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
    hip.lib(), hip.chain_lib()
    return torch.device("cuda:0")


def _note(line):
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            fh.write(f"  spans_masked {fl()} {line}\n")


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def prepared(sims, mask, valid):
    """NaN from each row's duration on; NaN, +inf and -inf in turn under the frames ``valid`` hides."""
    sims = np.array(sims, dtype=F)
    rpm = sims.shape[0] // mask.shape[0]
    sims[np.repeat(mask, rpm, axis=0) == 0] = NAN
    if valid is not None:
        with np.errstate(invalid="ignore"):
            hidden = np.repeat(np.asarray(valid, dtype=F) == 0, rpm, axis=0)
        poison = np.resize(np.array([NAN, INF, -INF], dtype=F), sims.shape)
        sims[hidden] = poison[hidden]
    return sims


def up(dev, x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F)).to(dev) if x is not None else None


# ------------------------------------------------------------------ span scores ------------------------------------------------------------------
def run_scores(dev, sims, spans, mask, valid, skip, mode, k, tau, full=True):
    from revisionllm_amd import hip
    R, L = sims.shape
    N = spans.shape[1]
    s, p, m, v = up(dev, sims), up(dev, spans), up(dev, mask), up(dev, valid)
    o = dict(scores=_Guarded(R * N, torch.float32, dev), windows=_Guarded(R * N * 2, torch.int32, dev) if full else None,
             n_usable=_Guarded(R * N, torch.int32, dev) if full else None)
    ptr = lambda x: x.ptr if x is not None else None                                            # noqa: E731
    rc = hip.chain_lib().rvc_span_scores_masked(hip.ptr(s), hip.ptr(p), hip.ptr(m), hip.ptr(v), R, R // mask.shape[0], L, N, mode, k, float(tau), int(skip),
                                                ptr(o["scores"]), ptr(o["windows"]), ptr(o["n_usable"]), hip.stream())
    hip.chain_check(rc, "rvc_span_scores_masked")
    torch.cuda.synchronize()
    shapes = dict(scores=(R, N), windows=(R, N, 2), n_usable=(R, N))
    return {k_: (x.take(shapes[k_]) if x is not None else None) for k_, x in o.items()}


@functools.lru_cache(maxsize=None)
def _score_oracle(sims_b, shape, spans_b, N, mask_b, M, valid_b, skip, mode, k, tau, f64):
    sims = np.frombuffer(sims_b, dtype=F).reshape(shape)
    valid = np.frombuffer(valid_b, dtype=F).reshape(M, shape[1]) if valid_b is not None else None
    return MO.span_scores(sims, np.frombuffer(spans_b, dtype=F).reshape(shape[0], N, 2), np.frombuffer(mask_b, dtype=F).reshape(M, shape[1]), valid, skip, mode, k,
                          tau, f64)


def score_oracle(sims, spans, mask, valid, skip, mode, k=3, tau=0.01, f64=False):
    spans, mask = np.ascontiguousarray(spans, dtype=F), np.ascontiguousarray(mask, dtype=F)
    valid = None if valid is None else np.ascontiguousarray(valid, dtype=F)
    return _score_oracle(sims.tobytes(), sims.shape, spans.tobytes(), spans.shape[1], mask.tobytes(), mask.shape[0], None if valid is None else valid.tobytes(),
                         int(skip), mode, k, float(tau), f64)


def check_topk(dev, sims, spans, mask, valid=None, skip=0, k=3, what=""):
    """Top-k mode with every optional output and with none, bit for bit against the oracle -> (got, ref)."""
    sims = prepared(sims, mask, valid)
    ref = score_oracle(sims, spans, mask, valid, skip, MO.TOPK, k)
    what = f"{what} L={sims.shape[1]} k={k} skip={skip} valid={valid is not None}"
    got = run_scores(dev, sims, spans, mask, valid, skip, MO.TOPK, k, 1.0)
    for g in (got, run_scores(dev, sims, spans, mask, valid, skip, MO.TOPK, k, 1.0, full=False)):
        a, b = bits(g["scores"]), bits(ref["scores"])
        assert np.array_equal(a, b), (what, "scores", np.argwhere(a != b)[:4].tolist())
    assert np.array_equal(got["windows"], ref["windows"]), (what, "windows")
    assert np.array_equal(got["n_usable"], ref["n_usable"]), (what, "n_usable", np.argwhere(got["n_usable"] != ref["n_usable"])[:4].tolist())
    return got, ref


def spans_for(L, D, R, seed):
    """(centre, width) rows whose windows over a duration D have 0, 1, 63, 64, 65, 129 and L frames (as far as D goes), next to the fixed ones."""
    sp = MO.fixed_spans(R, 24, seed)
    if D > 0:
        for i, n in enumerate((0, 1, 63, 64, 65, 129, L)):
            lo = (7 * i) % max(1, D - min(n, D) + 1)
            hi = min(D, lo + n)
            sp[:, 9 + i] = ((lo + hi) / 2.0 / D, max(0.0, (hi - lo) - 0.5) / D if hi > lo else 0.0)
    return sp


def patterns(M, L, k):
    """The hidden patterns: head, an interior block astride 63|64, tail, every other frame, exactly one usable, exactly k - 1 usable, none usable."""
    def row(fn):
        v = np.ones((M, L), dtype=F)
        fn(v)
        return v
    out = {"head": row(lambda v: v.__setitem__((slice(None), slice(0, max(1, L // 4))), 0)),
           "block": row(lambda v: v.__setitem__((slice(None), slice(min(60, L // 2), min(68, L // 2 + 8))), 0)),
           "tail": row(lambda v: v.__setitem__((slice(None), slice(L - max(1, L // 3), L)), 0)),
           "other": row(lambda v: v.__setitem__((slice(None), slice(0, L, 2)), 0)),
           "none": np.zeros((M, L), dtype=F)}
    one = np.zeros((M, L), dtype=F)
    one[:, L // 2] = 1
    out["one"] = one
    few = np.zeros((M, L), dtype=F)
    few[:, [(j * 5) % L for j in range(k - 1)]] = 1
    out["k-1"] = few
    return out


@pytest.mark.parametrize("L", [1, 63, 64, 65, 300, 1000])
def test_topk_lengths_durations_windows_and_patterns(kdev, L):
    Ds = [L, L - 1, 1, 0]
    mask = MO.durations(L, Ds)
    sims = MO.bumpy(4, L, L)
    spans = np.concatenate([spans_for(L, D, 1, L) for D in Ds])
    for k in (1, 3, 64):
        check_topk(kdev, sims, spans, mask, None, 0, k, "no valid")
        for name, valid in patterns(4, L, k).items():
            got, ref = check_topk(kdev, sims, spans, mask, valid, 0, k, name)
            if name == "none":
                empty = (ref["windows"][..., 1] <= ref["windows"][..., 0])
                assert (bits(got["scores"])[~empty] == MO.NAN_BITS).all() and (got["n_usable"] == 0).all()
                assert (bits(got["scores"])[empty & (ref["windows"][..., 0] >= 0)] == 0).all()


def test_topk_a_long_row(kdev):
    L = 20000
    mask = MO.durations(L, [L, L - 1])
    valid = np.ones((2, L), dtype=F)
    valid[:, ::16] = 0
    valid[1, 5000:15000] = 0
    spans = np.array([[(0.5, 1.0), (0.5, 0.01), (0.9999, 0.001), (0.25, 0.5), (-0.2, 0.1), (0.5, 0.5)]] * 2, dtype=F)
    check_topk(kdev, MO.bumpy(2, L, 3), spans, mask, valid, 0, 64)
    check_topk(kdev, MO.bumpy(2, L, 3), spans, mask, None, 0, 3)


def test_valid_values_and_skip_nan(kdev):
    """-0.0 hides, NaN / -1 / 2 / 1e-45 do not; a NaN at a usable frame gives NaN with skip_nan off and is skipped with it on; every usable frame NaN
    under skip_nan gives n = 0."""
    L = 130
    mask = MO.durations(L, [L, 100])
    sims = MO.bumpy(2, L, 9)
    valid = np.resize(np.array([-0.0, NAN, -1.0, 2.0, 1e-45, 0.0, 1.0], dtype=F), (2, L))
    assert valid[0, 4] != 0 and np.signbit(valid[0, 0])                                     # (the denormal survives, -0 is -0)
    spans = spans_for(L, L, 2, 5)
    for k in (1, 3):
        got, ref = check_topk(kdev, sims, spans, mask, valid, 0, k, "valid values")
        whole = ref["windows"][0].tolist().index([0, L])
        assert got["n_usable"][0, whole] == sum(1 for t in range(L) if t % 7 not in (0, 5))             # -0.0 and 0.0 hide; NaN, -1, 2 and 1e-45 do not
    planted = sims.copy()
    planted[:, 3::11] = NAN
    for valid_ in (None, valid):
        off, _ = check_topk(kdev, planted, spans, mask, valid_, 0, 3, "planted NaN, skip off")
        on, ref = check_topk(kdev, planted, spans, mask, valid_, 1, 3, "planted NaN, skip on")
        if valid_ is None:
            hit = (ref["windows"][..., 1] - ref["windows"][..., 0] >= 11) & (ref["windows"][..., 0] >= 0)
            assert np.isnan(off["scores"][hit]).all() and not np.isnan(on["scores"][hit]).any() and (on["n_usable"][hit] < off["n_usable"][hit]).all()
    allnan = np.full((2, L), NAN, dtype=F)
    got, ref = check_topk(kdev, allnan, spans, mask, None, 1, 3, "every frame NaN")
    assert (got["n_usable"] == 0).all() and (bits(got["scores"])[ref["windows"][..., 1] > ref["windows"][..., 0]] == MO.NAN_BITS).all()


@pytest.mark.parametrize("R", [1, 4, 260])
def test_topk_row_counts(kdev, R):
    L = 70
    rng = np.random.default_rng(R)
    mask = MO.durations(L, rng.integers(0, L + 1, R))
    valid = (rng.random((R, L)) < 0.7).astype(F)
    check_topk(kdev, MO.bumpy(R, L, R), MO.fixed_spans(R, 9, R), mask, valid, 0, 3, f"R={R}")


def test_three_rows_per_mask_row_row_independence_and_the_bql_layout(kdev):
    from revisionllm_amd import ops
    L, B, Q, N = 150, 4, 3, 13
    rng = np.random.default_rng(17)
    mask = MO.durations(L, [150, 149, 64, 1])
    valid = (rng.random((B, L)) < 0.6).astype(F)
    sims = prepared(MO.bumpy(B * Q, L, 21), mask, valid)
    sims[:, 5::13] = NAN
    spans = MO.fixed_spans(B * Q, N, 4)
    got, ref = check_topk(kdev, sims, spans, mask, valid, 1, 3, "rpm=3")
    for r in (0, 3, 9):                                                                 # a mask row's rows alone give the same bits
        alone = run_scores(kdev, sims[r:r + 3], spans[r:r + 3], mask[r // 3:r // 3 + 1], valid[r // 3:r // 3 + 1], 1, MO.TOPK, 3, 1.0)
        assert np.array_equal(bits(alone["scores"]), bits(got["scores"][r:r + 3])) and np.array_equal(alone["n_usable"], got["n_usable"][r:r + 3])
    s, p, m = up(kdev, sims).view(B, Q, L), up(kdev, spans).view(B, Q, N, 2), up(kdev, mask)
    for v in (torch.from_numpy(valid).to(kdev), torch.from_numpy(valid != 0).to(kdev), torch.from_numpy(valid.astype(np.uint8)).to(kdev),
              torch.from_numpy(valid).to(kdev).half()):
        out = ops.span_scores_masked(s, p, m.bool(), valid=v, skip_nan=True, return_windows=True, return_usable=True)
        assert out.scores.shape == (B, Q, N) and out.windows.shape == (B, Q, N, 2) and out.n_usable.dtype == torch.int32
        assert np.array_equal(bits(out.scores.cpu().numpy().reshape(B * Q, N)), bits(ref["scores"]))
        assert np.array_equal(out.windows.cpu().numpy().reshape(B * Q, N, 2), ref["windows"]) and np.array_equal(out.n_usable.cpu().numpy().reshape(B * Q, N), ref["n_usable"])
    bare = ops.span_scores_masked(s, p, m, valid=torch.from_numpy(valid).to(kdev), skip_nan=True)
    assert bare.windows is None and bare.n_usable is None and torch.equal(bare.scores.view(torch.int32), out.scores.view(torch.int32))
    assert ops.span_scores_masked(s, p[:, :, :0], m).scores.shape == (B, Q, 0)


def test_attention_mode(kdev):
    """The one comparison with a tolerance: see the module docstring.  The NaN pattern, the windows and the usable counts are exact."""
    worst = {tau: 0.0 for tau in TAUS}
    own = {tau: 0.0 for tau in TAUS}
    for tau in TAUS:
        results = []
        for name, sims, spans, mask, valid, skip in MO.attention_cases():
            sims = prepared(sims, mask, valid)
            ref32 = score_oracle(sims, spans, mask, valid, skip, MO.ATTENTION, 3, tau)
            ref64 = score_oracle(sims, spans, mask, valid, skip, MO.ATTENTION, 3, tau, True)
            own[tau] = max(own[tau], MO.rel_err(ref32["scores"], ref64["scores"]))
            got = run_scores(kdev, sims, spans, mask, valid, skip, MO.ATTENTION, 3, tau)
            bare = run_scores(kdev, sims, spans, mask, valid, skip, MO.ATTENTION, 3, tau, full=False)
            assert np.array_equal(bits(got["scores"]), bits(bare["scores"])), (name, tau)
            assert np.array_equal(got["windows"], ref64["windows"]) and np.array_equal(got["n_usable"], ref64["n_usable"]), (name, tau)
            assert np.array_equal(np.isnan(got["scores"]), np.isnan(ref64["scores"])), (name, tau)
            void = (ref64["n_usable"] == 0) & (ref64["windows"][..., 1] > ref64["windows"][..., 0])
            assert (bits(got["scores"])[void] == MO.NAN_BITS).all() and (bits(got["scores"])[(ref64["windows"][..., 1] <= ref64["windows"][..., 0]) & (ref64["windows"][..., 0] >= 0)] == 0).all()
            results.append((name, MO.rel_err(got["scores"], ref64["scores"])))
        worst[tau] = max(e for _, e in results)
        print(f"spans_masked attention tau{tau}: kernel vs float64 rel {worst[tau]:.3e}, float32 statement vs float64 {own[tau]:.3e}, bound {4 * own[tau]:.3e}")
        _note(f"attention tau{tau} kernel vs float64 rel {worst[tau]:.3e} | float32 statement vs float64 {own[tau]:.3e} | asserted bound {4 * own[tau]:.3e}")
    for tau in TAUS:
        assert own[tau] > 0 and worst[tau] < 4 * own[tau], (tau, worst[tau], own[tau])


def test_without_valid_and_skip_nan_the_scores_are_the_unmasked_entries(dev):
    from revisionllm_amd import ops
    L, B, Q, N = 300, 2, 3, 24
    mask = MO.durations(L, [300, 257])
    sims = prepared(MO.bumpy(B * Q, L, 33), mask, None)
    sims[1, 40] = NAN
    s, p, m = up(dev, sims).view(B, Q, L), up(dev, spans_for(L, 257, B * Q, 2)).view(B, Q, N, 2), up(dev, mask)
    for kw in (dict(k=1), dict(k=3), dict(k=64), dict(pooling="attention", temperature=0.01), dict(pooling="attention", temperature=1.0)):
        ref, rwin = ops.span_scores_multi(s, p, m, return_windows=True, **kw)
        got = ops.span_scores_masked(s, p, m, return_windows=True, return_usable=True, **kw)
        assert torch.equal(got.scores.view(torch.int32), ref.view(torch.int32)) and torch.equal(got.windows, rwin), kw
        assert torch.equal(got.n_usable, (rwin[..., 1] - rwin[..., 0]).clamp(min=0)), kw
        ref1, rwin1 = ops.span_scores(s[:, 0].contiguous(), p[:, 0].contiguous(), m, return_windows=True, **kw)
        got1 = ops.span_scores_masked(s[:, 0].contiguous(), p[:, 0].contiguous(), m, valid=torch.ones_like(m), return_windows=True, **kw)
        assert torch.equal(got1.scores.view(torch.int32), ref1.view(torch.int32)) and torch.equal(got1.windows, rwin1), kw


# ------------------------------------------------------------------ proposals ------------------------------------------------------------------
def run_propose(dev, sims, mask, valid, skip, levels=LEVELS, relative=1, smooth=1, gap=0, min_len=1, max_len=0, N=64, full=True):
    from revisionllm_amd import hip
    R, L = sims.shape
    s, m, v = up(dev, sims), up(dev, mask), up(dev, valid)
    o = dict(spans=_Guarded(R * N * 2, torch.float32, dev), n_spans=_Guarded(R, torch.int32, dev), n_found=_Guarded(R, torch.int32, dev) if full else None,
             windows=_Guarded(R * N * 2, torch.int32, dev) if full else None, smoothed=_Guarded(R * L, torch.float32, dev) if full else None)
    ptr = lambda x: x.ptr if x is not None else None                                            # noqa: E731
    table = (ctypes.c_float * len(levels))(*levels)
    rc = hip.chain_lib().rvc_span_propose_masked(hip.ptr(s), hip.ptr(m), hip.ptr(v), R, R // mask.shape[0], L, table, len(levels), relative, smooth, gap, min_len,
                                                 max_len, N, int(skip), ptr(o["spans"]), ptr(o["n_spans"]), ptr(o["n_found"]), ptr(o["windows"]),
                                                 ptr(o["smoothed"]), hip.stream())
    hip.chain_check(rc, "rvc_span_propose_masked")
    torch.cuda.synchronize()
    shapes = dict(spans=(R, N, 2), n_spans=(R,), n_found=(R,), windows=(R, N, 2), smoothed=(R, L))
    return {k_: (x.take(shapes[k_]) if x is not None else None) for k_, x in o.items()}


def check_propose(dev, sims, mask, valid=None, skip=0, what="", **kw):
    """Every optional output and none, bit for bit against the oracle -> (got, ref)."""
    sims = prepared(sims, mask, valid)
    okw = {"N": 64, **{k_: v for k_, v in kw.items() if k_ != "levels"}}
    ref = MO.propose(sims, mask, kw.get("levels", LEVELS), valid=valid, skip_nan=skip, **okw)
    what = f"{what} L={sims.shape[1]} skip={skip} valid={valid is not None} {kw}"
    got = run_propose(dev, sims, mask, valid, skip, **kw)
    for g in (got, run_propose(dev, sims, mask, valid, skip, full=False, **kw)):
        a, b = bits(g["spans"]), bits(ref["spans"])
        assert np.array_equal(g["n_spans"], ref["n_spans"]), (what, "n_spans", g["n_spans"][:8].tolist(), ref["n_spans"][:8].tolist())
        assert np.array_equal(a, b), (what, "spans", np.argwhere(a != b)[:4].tolist())
    assert np.array_equal(got["n_found"], ref["n_found"]) and np.array_equal(got["windows"], ref["windows"]), (what, "n_found / windows")
    for r, (sp, D) in enumerate(zip(ref["smoothed"], ref["D"])):
        assert np.array_equal(bits(got["smoothed"][r, :D]), bits(sp)), (what, "smoothed", r, np.argwhere(bits(got["smoothed"][r, :D]) != bits(sp))[:4].tolist())
        assert (got["smoothed"][r, D:] == SENTINEL).all(), (what, "smoothed past D", r)
    return got, ref


def hide(M, L, *stretches):
    v = np.ones((M, L), dtype=F)
    for a, b in stretches:
        v[:, max(0, a):max(0, b)] = 0
    return v


@pytest.mark.parametrize("L", [64, 65, 256, 257, 512, 513, 1000])
def test_proposals_at_tile_edges(kdev, L):
    Ds = [L, L - 1, 1, 0]
    mask = MO.durations(L, Ds)
    sims = MO.bumpy(4, L, 100 + L)
    edges = [e for e in (64, 256, 512) if e <= L]
    astride = hide(4, L, *[(e - 1, e + 1) for e in edges])
    for smooth in (1, 3, 65):
        for gap in (0, 1):
            check_propose(kdev, sims, mask, astride, 0, "astride the edges", smooth=smooth, gap=gap)
        halo = hide(4, L, *[(e - 3, e - 1) for e in edges], *[(e + 1, e + 30) for e in edges], (0, 2), (L - 2, L), (L - 3, L - 1))
        check_propose(kdev, sims, mask, halo, 0, "the halo and both row ends", smooth=smooth, gap=2, N=32)
    check_propose(kdev, sims, mask, None, 0, "no valid", smooth=3, gap=1)
    check_propose(kdev, sims, mask, np.zeros((4, L), dtype=F), 0, "all hidden", smooth=3, gap=1)
    lonely = np.zeros((4, L), dtype=F)
    lonely[:, ::40] = 1                                                                  # a smoothing box with one usable frame
    check_propose(kdev, sims, mask, lonely, 0, "lonely", smooth=65, gap=63, relative=0, levels=(0.2, 0.4))


def test_a_hidden_frame_inside_a_run_and_hidden_stretches_around_gap(kdev):
    L = 300
    mask = MO.durations(L, [L])
    sims = np.full((1, L), 0.1, dtype=F)
    sims[0, 20:60] = 0.9
    sims[0, 100:260] = 0.8
    for gap, holes, expect in ((0, [(30, 31)], [[20, 30], [31, 60], [100, 260]]), (1, [(30, 31)], [[20, 60], [100, 260]]),
                               (3, [(30, 33), (150, 154)], [[20, 60], [100, 150], [154, 260]]), (63, [(120, 183)], [[20, 260]]),
                               (63, [(120, 184)], [[20, 120], [184, 260]])):               # (gap 63 closes the 40 low frames between the two stretches too)
        got, _ = check_propose(kdev, sims, mask, hide(1, L, *holes), 0, f"gap={gap}", levels=(0.5,), relative=0, gap=gap)
        assert got["windows"][0, :got["n_spans"][0]].tolist() == expect, (gap, holes)
    got, _ = check_propose(kdev, sims, mask, hide(1, L, (30, 31)), 0, "length counts the hidden frame", levels=(0.5,), relative=0, gap=1, min_len=40, max_len=40)
    assert got["windows"][0, 0].tolist() == [20, 60] and got["n_found"][0] == 1


def test_proposal_valid_values(kdev):
    """-0.0 and 0.0 hide a frame, NaN, -1, 2 and 1e-45 do not: the runs of a constant row break at the hidden frames alone."""
    L = 140
    mask = MO.durations(L, [L, 100])
    valid = np.resize(np.array([-0.0, NAN, -1.0, 2.0, 1e-45, 0.0, 1.0], dtype=F), (2, L))
    sims = np.full((2, L), 0.9, dtype=F)
    got, _ = check_propose(kdev, sims, mask, valid, 0, "valid values", levels=(0.5,), relative=0, N=64)
    assert got["windows"][0, :3].tolist() == [[1, 5], [6, 7], [8, 12]] and got["n_found"][0] == 40
    for smooth, gap in ((3, 0), (5, 1)):
        check_propose(kdev, MO.bumpy(2, L, 8), mask, valid, 0, "valid values", smooth=smooth, gap=gap)


@pytest.mark.parametrize("T", [1, 5, 8])
def test_levels_capacity_and_skip_nan(kdev, T):
    L = 520
    mask = MO.durations(L, [L, 519, 300])
    sims = MO.bumpy(3, L, T)
    valid = hide(3, L, (63, 65), (255, 300), (400, 401), (511, 513))
    levels = tuple(0.1 + 0.8 * i / T for i in range(T))
    for relative in (0, 1):
        got, ref = check_propose(kdev, sims, mask, valid, 0, f"T={T}", levels=levels, relative=relative, smooth=3, gap=1, N=64)
        found = int(ref["n_found"][0])
        for N in sorted({max(1, found - 1), max(1, found), found + 1}):
            check_propose(kdev, sims, mask, valid, 0, f"T={T} N around found", levels=levels, relative=relative, smooth=3, gap=1, N=N)
    planted = sims.copy()
    planted[:, 7::23] = NAN
    for smooth in (1, 3, 65):
        check_propose(kdev, planted, mask, None, 1, "skip_nan alone", levels=levels, smooth=smooth, gap=1)
        check_propose(kdev, planted, mask, valid, 1, "skip_nan and valid", levels=levels, smooth=smooth, gap=1)
        check_propose(kdev, planted, mask, valid, 0, "NaN left in", levels=levels, smooth=smooth, gap=1)


@pytest.mark.parametrize("R", [1, 4, 260])
def test_proposal_row_counts_and_rows_per_mask(kdev, R):
    L = 90
    rng = np.random.default_rng(R)
    check_propose(kdev, MO.bumpy(R, L, 60 + R), MO.durations(L, rng.integers(0, L + 1, R)), (rng.random((R, L)) < 0.8).astype(F), 0, f"R={R}", smooth=3, gap=1,
                  N=16)
    if R == 4:
        mask = MO.durations(L, [90, 64, 31, 1])
        valid = (rng.random((4, L)) < 0.8).astype(F)
        sims = MO.bumpy(12, L, 77)
        got, _ = check_propose(kdev, sims, mask, valid, 0, "rpm=3", smooth=5, gap=2, N=16)
        p = prepared(sims, mask, valid)
        alone = run_propose(kdev, p[3:6], mask[1:2], valid[1:2], 0, smooth=5, gap=2, N=16)
        assert np.array_equal(bits(alone["spans"]), bits(got["spans"][3:6])) and np.array_equal(alone["n_found"], got["n_found"][3:6])


def _same_proposals(a, b, what):
    for x, y, name in zip(a, b, a._fields):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            xi, yi = (x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else (x, y)
            assert torch.equal(xi, yi), (what, name)


def test_the_four_identities_against_span_propose(dev):
    from revisionllm_amd import ops
    L, B, Q = 600, 2, 3
    mask = MO.durations(L, [600, 511])
    sims = prepared(MO.bumpy(B * Q, L, 55), mask, None)
    s, m = up(dev, sims).view(B, Q, L), up(dev, mask)
    valid = torch.from_numpy(hide(B, L, (63, 65), (200, 230), (255, 257), (400, 401))).to(dev)
    over = s.masked_fill((valid == 0)[:, None, :].expand(B, Q, L), NAN)
    nans = s.clone()
    nans[..., 9::31] = NAN
    for kw in (dict(smooth=1), dict(smooth=3, gap=1), dict(smooth=65, gap=5, relative=False, levels=(0.2, 0.5)), dict(smooth=1, gap=2, max_spans=7)):
        kw = dict(return_windows=True, return_smoothed=True, **kw)
        ref = ops.span_propose(s, m, **kw)
        _same_proposals(ops.span_propose_masked(s, m, **kw), ref, ("valid=None", kw))
        _same_proposals(ops.span_propose_masked(s, m.bool(), valid=torch.ones_like(m), **kw), ref, ("valid of ones", kw))
        _same_proposals(ops.span_propose_masked(s, m, valid=torch.ones_like(m).bool(), **kw), ref, ("valid of True", kw))
        if kw["smooth"] == 1:
            _same_proposals(ops.span_propose_masked(s, m, valid=valid, **kw), ops.span_propose(over, m, **kw), ("NaN over the hidden frames", kw))
            _same_proposals(ops.span_propose_masked(nans, m, skip_nan=True, **kw), ops.span_propose(nans, m, **kw), ("skip_nan alone", kw))
    bare = ops.span_propose_masked(s, m, valid=valid)
    assert bare.windows is None and bare.smoothed is None and bare.spans.shape == (B, Q, 256, 2) and bare.n_found.shape == (B, Q)


# ------------------------------------------------------------------ the chain ------------------------------------------------------------------
def test_every_proposal_of_the_round_trip_has_a_usable_frame(kdev):
    from revisionllm_amd import ops
    L, R = 700, 5
    rng = np.random.default_rng(3)
    mask = MO.durations(L, [700, 699, 512, 65, 1])
    valid = (rng.random((R, L)) < 0.7).astype(F)
    sims = prepared(MO.bumpy(R, L, 13), mask, valid)
    sims[:, 4::9][valid[:, 4::9] != 0] = NAN
    s, m, v = up(kdev, sims), up(kdev, mask), up(kdev, valid)
    for kw in (dict(smooth=1), dict(smooth=5, gap=3), dict(smooth=65, gap=63)):
        prop = ops.span_propose_masked(s, m, valid=v, skip_nan=True, max_spans=128, return_windows=True, **kw)
        out = ops.span_scores_masked(s, prop.spans, m, valid=v, skip_nan=True, return_windows=True, return_usable=True)
        held = torch.arange(128, device=kdev)[None, :] < prop.n_spans[:, None]
        assert int(prop.n_spans.sum()) > 20 and torch.equal(out.windows[held], prop.windows[held])         # the encoding gives the window back
        assert bool((out.n_usable[held] >= 1).all()) and not bool(torch.isnan(out.scores[held]).any()), kw
        assert bool(torch.isnan(out.scores[~held]).all()) and bool((out.n_usable[~held] == 0).all())


def planted_movie(B, Q, L, d, seed):
    """Background frames, and per (video, query) one stretch of frames along the query's text with two zeroed feature rows inside it."""
    g = torch.Generator().manual_seed(seed)
    text = torch.nn.functional.normalize(torch.randn(B, Q, d, generator=g), dim=-1)
    video = torch.nn.functional.normalize(torch.randn(B, L, d, generator=g), dim=-1)
    gt = torch.zeros(B, Q, 2)
    for b in range(B):
        for q in range(Q):
            a = 40 + 130 * q + 17 * b
            video[b, a:a + 40] = torch.nn.functional.normalize(text[b, q] + 0.05 * torch.randn(40, d, generator=g), dim=-1)
            video[b, [a + 10, a + 25]] = 0
            gt[b, q] = torch.tensor([a, a + 40.0])
    return text, video, gt


def _iou(spans, gt, D):
    xx = torch.stack((spans[..., 0] - spans[..., 1] / 2, spans[..., 0] + spans[..., 1] / 2), -1) * D
    inter = (torch.minimum(xx[..., 1], gt[..., None, 1]) - torch.maximum(xx[..., 0], gt[..., None, 0])).clamp(min=0)
    union = (xx[..., 1] - xx[..., 0]) + (gt[..., None, 1] - gt[..., None, 0]) - inter
    return inter / union


@pytest.mark.parametrize("multi", [False, True])
def test_ground_queries_masked_recovers_stretches_with_zeroed_rows(dev, multi):
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval.similarity import ground_queries, ground_queries_masked
    B, Q, L, d = 2, 3, 450, 64
    text, video, gt = planted_movie(B, Q, L, d, 7)
    if not multi:
        text, gt = text[:, 1], gt[:, 1]
    t, v, m = text.to(dev), video.to(hip.op_dtype()).to(dev), torch.ones(B, L, device=dev)
    kw = dict(top=5, nms_iou=0.5, smooth=3, gap=3, min_len=2)
    plain = ground_queries(t, v, m, **kw)
    masked = ground_queries_masked(t, v, m, skip_nan=True, **kw)
    iou_p, iou_m = _iou(plain.spans.cpu(), gt, L), _iou(masked.spans.cpu(), gt, L)
    # unmasked: whatever overlaps the planted stretch holds a NaN cosine - its score is NaN and it ranks behind every number - or is lost
    on_target = iou_p > 0.5
    assert bool(torch.isnan(plain.scores.cpu()[on_target]).all())
    assert not bool((torch.isfinite(plain.scores.cpu()) & on_target).any())
    # masked: the stretch is the first place, with a number for a score
    assert bool((iou_m[..., 0] > 0.7).all()) and bool(torch.isfinite(masked.scores.cpu()[..., 0]).all()), iou_m[..., 0]
    # ... and equals its four stages chained
    sims = (ops.frame_cosine_multi if multi else ops.frame_cosine)(t, v)
    prop = ops.span_propose_masked(sims, m, skip_nan=True, smooth=3, gap=3, min_len=2)
    sc = ops.span_scores_masked(sims, prop.spans, m, skip_nan=True).scores
    rank = ops.span_rank(sc, prop.spans, top=5, nms_iou=0.5)
    _same_proposals(masked.proposals, prop, "proposals")
    assert torch.equal(masked.rank.keep, rank.keep) and torch.equal(masked.rank.n_keep, rank.n_keep)
    first = rank.keep[..., 0].long()
    assert torch.equal(masked.scores[..., 0].view(torch.int32), torch.gather(sc, -1, first.unsqueeze(-1)).squeeze(-1).view(torch.int32))
    # a validity row that hides the zeroed rows does what skip_nan does
    valid = (video.abs().sum(-1) > 0).to(dev)
    by_valid = ground_queries_masked(t, v, m, valid=valid, **kw)
    assert torch.equal(by_valid.spans.view(torch.int32), masked.spans.view(torch.int32)) and torch.equal(by_valid.scores.view(torch.int32), masked.scores.view(torch.int32))


def test_the_masked_calls_do_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the calls: with the stream kept busy by work queued before them, an event recorded just before
    has not completed when they return."""
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval.similarity import forward_clip_matching_masked, ground_queries_masked, propose_spans_masked
    B, Q, L, d = 2, 3, 450, 64
    text, video, _ = planted_movie(B, Q, L, d, 8)
    t, v, m = text.to(dev), video.to(hip.op_dtype()).to(dev), torch.ones(B, L, device=dev)
    valid = torch.ones(B, L, dtype=torch.bool, device=dev)
    valid[:, ::16] = False
    p = torch.from_numpy(MO.fixed_spans(B * Q, 12, 1)).view(B, Q, 12, 2).to(dev)

    rows = ops.frame_cosine_multi(t, v)

    def calls():
        g = ground_queries_masked(t, v, m, valid=valid, skip_nan=True, top=5, smooth=3, gap=3)
        f = forward_clip_matching_masked(t, v, m, p, valid=valid, skip_nan=True, return_windows=True, return_usable=True)
        s = propose_spans_masked(rows, m, valid=valid, skip_nan=True, smooth=3)
        return g.spans, g.scores, f.scores, f.windows, f.n_usable, s.spans
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
    assert still_busy, "the masked calls returned only after the work queued before them had finished: they synchronised"
    raw = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int16) if x.dtype.itemsize == 2 else x      # noqa: E731
    for x, y in zip(got, want):
        assert torch.equal(raw(x), raw(y))
