"""rvc_span_anchors (the chain library's kernel behind ``ops.span_anchors`` and ``eval.similarity``'s ``propose_anchors`` / ``ground_queries_anchored``:
multi-scale sliding-window proposals, the local peaks of each scale) against tests/span_anchors_oracle.py, the rule restated in numpy.  The rule
works on integers, so the oracle IS the rule: counts, windows, scale indices, span bits and score bits are compared with NO tolerance.
tests/test_span_anchors_host_logic.py holds the oracle itself to a brute-force statement.

Every direct call writes into sentinel-filled buffers with 64 elements on either side of each output, once with every optional output and once with
none, and works in a workspace filled with 0xAB bytes.  Behind every duration ``valid`` holds NaN - "not hidden" - and ``sims`` NaN in the even rows
and 1.0, the largest value there is, in the odd ones: a context cut at L instead of D would show.  NaN and +-inf sit under every frame ``valid``
hides.  The kernel walks a row in tiles of 4096 frames (four per thread), scans in waves of 64 and compacts its anchors in chunks of 1024: the lengths and anchor counts
below lie on both sides of those edges.  The kernel is f32 / i32 only and the chain library has one build, so the kernel items run once (``kdev``);
the end-to-end items go through the flavoured libraries and run in both builds (``dev``)."""
import ctypes

import numpy as np
import pytest
import torch

import span_anchors_oracle as AO
import spans_masked_oracle as MO
from test_gpu_span_refine import durations, prepared
from test_gpu_spans_masked import bits, dev, flav, kdev, up  # noqa: F401
from test_gpu_windows_valid import Fenced, _same_tuple

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
F = np.float32
SHAPES = dict(spans=lambda R, N: (R, N, 2), scores=lambda R, N: (R, N), n_spans=lambda R, N: (R,), n_found=lambda R, N: (R,), windows=lambda R, N: (R, N, 2),
              scale=lambda R, N: (R, N))


def run_anchors(dev, sims, mask, valid, rpv, scales, mode, peak, min_usable, N, full=True):
    from revisionllm_amd import hip
    R, L = sims.shape
    s, m, v = up(dev, sims), up(dev, mask), up(dev, valid)
    flat = [x for t in AO.normal_scales(scales) for x in t]
    table = (ctypes.c_int32 * len(flat))(*flat)
    lib = hip.chain_lib()
    nbytes = lib.rvc_span_anchors_workspace(L, table, len(flat) // 3, R)
    assert nbytes >= (L + 1) * 16 * R
    work = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device=dev)
    o = dict(spans=Fenced(R * N * 2, torch.float32, dev), scores=Fenced(R * N, torch.float32, dev), n_spans=Fenced(R, torch.int32, dev),
             n_found=Fenced(R, torch.int32, dev), windows=Fenced(R * N * 2, torch.int32, dev) if full else None, scale=Fenced(R * N, torch.int32, dev) if full else None)
    ptr = lambda x: x.ptr if x is not None else None                                            # noqa: E731
    rc = lib.rvc_span_anchors(hip.ptr(s), hip.ptr(m), hip.ptr(v), rpv, R, R // mask.shape[0], L, table, len(flat) // 3, mode, peak, min_usable, N, ptr(o["spans"]),
                              ptr(o["scores"]), ptr(o["n_spans"]), ptr(o["n_found"]), ptr(o["windows"]), ptr(o["scale"]), hip.ptr(work), nbytes, hip.stream())
    hip.chain_check(rc, "rvc_span_anchors")
    torch.cuda.synchronize()
    assert bool((work[nbytes:] == 0xAB).all()), "a write behind the workspace"
    return {k: (x.take(SHAPES[k](R, N)) if x is not None else None) for k, x in o.items()}


def compare(got, ref, what):
    for name in ("n_found", "n_spans", "windows", "scale"):
        if got[name] is not None:
            assert np.array_equal(got[name], ref[name]), (what, name, np.argwhere(got[name] != ref[name])[:4].tolist(), got[name][got[name] != ref[name]][:4],
                                                          ref[name][got[name] != ref[name]][:4])
    for name in ("spans", "scores"):
        a, b = bits(got[name]), bits(ref[name])
        assert np.array_equal(a, b), (what, name, np.argwhere(a != b)[:4].tolist())


def check(dev, sims, mask, valid, rpv, scales, mode=AO.CONTRAST, peak=2, min_usable=1, N=256, what="", round_trip=True, bare=True):
    """With every optional output and with none, bit for bit against the oracle; then ``ops.span_scores`` on the spans gives the windows back ->
    (got, ref)."""
    from revisionllm_amd import ops
    sims, valid = prepared(sims, mask, valid, rpv)
    ref = AO.anchors(sims, mask, valid, rpv, scales, mode, peak, min_usable, N)
    what = f"{what} R={sims.shape[0]} L={sims.shape[1]} scales={scales} mode={mode} peak={peak} min_usable={min_usable} N={N} rpv={rpv} valid={valid is not None}"
    got = run_anchors(dev, sims, mask, valid, rpv, scales, mode, peak, min_usable, N)
    compare(got, ref, what)
    if bare:
        compare(run_anchors(dev, sims, mask, valid, rpv, scales, mode, peak, min_usable, N, full=False), ref, what + " without the optional outputs")
    if round_trip and mask.shape[0] == sims.shape[0]:
        back = ops.span_scores(up(dev, np.nan_to_num(sims)), up(dev, got["spans"]), up(dev, mask), return_windows=True)[1].cpu().numpy()
        assert np.array_equal(back, ref["windows"]), (what, "round trip")
    return got, ref


def some_valid(rng, M, L):
    return rng.choice(np.array([1.0, 1.0, 1.0, 1.0, 0.0, -0.0, NAN, 2.0, 1e-45], dtype=F), (M, L))


def stepped(R, L, seed, steps=4):
    """Rows of a few distinct values in runs: equal scores everywhere."""
    rng = np.random.default_rng(seed)
    return (np.repeat(rng.integers(-steps, steps + 1, (R, L // 5 + 1)), 5, axis=1)[:, :L] / (2 * steps)).astype(F)


# ------------------------------------------------------------------ lengths, durations, scales ------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1100, 4095, 4096, 4097])
def test_lengths_and_durations(kdev, L):
    """D = L, L - 1, 1 and 0; len = 1, D and D + 1 (the second scale is row 0's D and row 1's D + 1, the third row 1's D); stride = 1 and len."""
    rng = np.random.default_rng(L)
    Ds = [L, L - 1, 1, 0]
    mask = durations(L, Ds)
    sims = MO.bumpy(4, L, L)
    scales = ((1, 1, 1), (L, 1, 2), (max(1, L - 1), max(1, L - 1), 3), (7, 3, 2), (64, 64, 5), (64, 1, 70))
    for case, (mode, peak) in enumerate(((AO.CONTRAST, 2), (AO.MEAN, 0), (AO.CONTRAST, 1))):
        valid = None if case == 1 else some_valid(rng, 4, L)
        got, ref = check(kdev, sims, mask, valid, 1, scales, mode, peak, 1, 2048, what="lengths")
        assert got["n_found"][3] == 0 and got["n_spans"][3] == 0 and (got["windows"][3] == -1).all() and np.isnan(got["spans"][3]).all()           # D = 0
        if mode == AO.MEAN and L > 2:
            assert got["n_found"][2] == 1 and got["windows"][2, 0].tolist() == [0, 1]                 # D = 1: the one anchor of the scale of length 1
            assert got["n_spans"][0] > 0
        assert (got["windows"][0, :, 1] <= L).all() and (got["windows"][1, :, 1] <= L - 1).all()
    if L > 2:
        with_whole_row = check(kdev, sims, mask, None, 1, ((L, 1, 2), (L - 1, L - 1, 1)), AO.MEAN, 2, 1, 8, what="len = D", bare=False)[0]
        assert with_whole_row["windows"][:2, 0].tolist() == [[0, L], [0, L - 1]] and with_whole_row["n_found"].tolist() == [2, 1, 0, 0]


@pytest.mark.parametrize("S", [1, 8])
def test_strides_the_flush_anchor_and_the_scale_count(kdev, S):
    L, D = 300, 291
    mask = durations(L, [D, 97 * 3, 290])
    sims = MO.bumpy(3, L, 7)
    # 291 = 3 * 97: no flush anchor at stride 97 for rows 0 and 1, one for row 2; (10, 10): 291 - 10 = 281 leaves one over
    scales = ((97, 97, 10), (10, 10, 5), (10, 1, 5), (1, 1, 1), (291, 291, 1), (290, 1, 1), (40, 7, 20), (3, 2, 300))[:S]
    for mode in (AO.CONTRAST, AO.MEAN):
        got, ref = check(kdev, sims, mask, None, 1, scales, mode, 0, 1, 2048, what="strides")                   # peak = 0: every anchor comes back
        assert got["windows"][0, :3].tolist() == [[0, 97], [97, 194], [194, 291]] and got["windows"][2, :3].tolist() == [[0, 97], [97, 194], [193, 290]]
        if S == 8:
            w = got["windows"][0][got["scale"][0] == 1]
            assert w[-1].tolist() == [281, 291] and w[-2].tolist() == [280, 290] and len(w) == 30
            # (the anchor that is the whole duration has no context: no contrast)
            assert sorted(set(got["scale"][0].tolist())) == ([-1, 0, 1, 2, 3, 4, 5, 6, 7] if mode == AO.MEAN else [-1, 0, 1, 2, 3, 5, 6, 7])
        check(kdev, sims, mask, some_valid(np.random.default_rng(S), 3, L), 1, scales, mode, 2, 2, 2048, what="strides, valid")


@pytest.mark.parametrize("peak", [0, 1, 2, 64])
def test_peak_widths_on_flat_staircase_and_stepped_rows(kdev, peak):
    L = 330
    mask = durations(L, [L, L, 300, L])
    sims = np.zeros((4, L), dtype=F)
    sims[0] = 0.25                                                                      # flat: every score ties
    sims[1] = (np.arange(L) // 10 / 64).astype(F)                                       # a staircase up
    sims[2] = sims[1][::-1]
    sims[3] = stepped(1, L, 5)[0]
    scales = ((10, 5, 5), (10, 10, 3), (4, 1, 2), (120, 60, 20))                         # the last scale has 5 anchors: peak = 64 is more than there are
    for mode in (AO.MEAN, AO.CONTRAST):
        got, ref = check(kdev, sims, mask, None, 1, scales, mode, peak, 1, 2048, what="peaks")
        if peak:
            assert got["n_found"][0] == 4 and got["windows"][0, :4].tolist() == [[0, 10], [0, 10], [0, 4], [0, 120]]     # a flat stretch: only its first anchor
    check(kdev, stepped(3, 1100, peak), durations(1100, [1100, 1025, 1024]), None, 1, ((1, 1, 1), (5, 1, 2)), AO.MEAN, peak, 1, 2048, what="stepped, long")


# ------------------------------------------------------------------ validity ------------------------------------------------------------------
def test_valid_values_hidden_anchors_hidden_contexts_and_min_usable(kdev):
    """-0.0 and 0.0 hide a frame; NaN, 2 and 1e-45 do not.  An anchor with no usable frame, one with no usable context, anchors touching 0 and D."""
    L, D = 140, 130
    mask = durations(L, [D] * 4)
    sims = MO.bumpy(4, L, 9)
    valid = np.resize(np.array([-0.0, NAN, 2.0, 1e-45, 0.0, 1.0, 1.0], dtype=F), (4, L))
    valid[1, 40:60] = 0                                                                 # the anchors inside [40, 60) have nothing usable
    valid[2, :] = 0
    valid[2, 50:60] = 1                                                                 # nothing usable outside [50, 60): no context for [50, 60)
    valid[3, :] = 1
    scales = ((10, 10, 5), (10, 5, 200), (5, 1, 3))
    got, ref = check(kdev, sims, mask, valid, 1, scales, AO.CONTRAST, 0, 1, 2048, what="valid values")
    w1 = got["windows"][1][got["scale"][1] == 0].tolist()
    assert [40, 50] not in w1 and [50, 60] not in w1 and [30, 40] in w1 and [60, 70] in w1
    w2 = got["windows"][2][got["scale"][2] == 0].tolist()
    assert [50, 60] not in w2 and w2 == []                                              # (no usable frame in any other anchor of that scale either)
    assert [52, 57] in got["windows"][2][got["scale"][2] == 2].tolist()                 # a shorter anchor has the plateau's other frames as context
    w3 = got["windows"][3][got["scale"][3] == 0].tolist()
    assert w3[0] == [0, 10] and w3[-1] == [120, 130] and len(w3) == 13                  # anchors touching 0 and D: one-sided context
    got, ref = check(kdev, sims, mask, valid, 1, scales, AO.MEAN, 0, 1, 2048, what="valid values, mean")
    assert [50, 60] in got["windows"][2][got["scale"][2] == 0].tolist()                 # the mean needs no context
    for mu in (2, 5, 6, 11):
        check(kdev, sims, mask, valid, 1, scales, AO.CONTRAST, 2, mu, 2048, what="min_usable")
    # NaN and +-inf similarities at usable frames: a NaN is never usable, an infinity clamps
    s2 = sims.copy()
    s2[0, 12:20] = NAN
    s2[0, 33], s2[0, 34], s2[3, 0], s2[3, D - 1] = INF, -INF, INF, -INF
    s2[1, ::3] = NAN
    for mode in (AO.CONTRAST, AO.MEAN):
        check(kdev, s2, mask, None, 1, scales, mode, 2, 1, 2048, what="NaN and inf sims, valid=NULL")
        check(kdev, s2, mask, valid, 1, scales, mode, 2, 3, 2048, what="NaN and inf sims")


# ------------------------------------------------------------------ capacity ------------------------------------------------------------------
def test_capacity_at_and_around_the_number_of_peaks_with_ties_at_the_cut(kdev):
    L = 1100
    mask = durations(L, [L, 1025, 700])
    sims = stepped(3, L, 11)                                                            # few distinct values: the cut falls among equal scores
    scales = ((5, 1, 2), (20, 5, 10))
    for mode, peak in ((AO.MEAN, 0), (AO.CONTRAST, 0), (AO.MEAN, 2)):
        full = AO.anchors(prepared(sims, mask, None, 1)[0], mask, None, 1, scales, mode, peak, 1, 2048)
        nf = int(full["n_found"][0])
        assert nf > (1100 if peak == 0 else 40)
        for N in sorted({1, 2, nf - 1, nf, nf + 1, 2048, nf // 2, 64}):
            got, ref = check(kdev, sims, mask, None, 1, scales, mode, peak, 1, N, what="capacity", bare=N in (1, nf - 1), round_trip=N in (1, nf - 1))
            assert got["n_found"][0] == nf and got["n_spans"][0] == min(nf, N)
            if N < nf:
                kept = np.sort(got["scores"][0, :N].astype(np.float64))[::-1]
                allsc = np.sort(full["scores"][0, :nf].astype(np.float64))[::-1]
                assert np.array_equal(kept, allsc[:N])                                  # truncation is by score
        if peak == 0:
            allsc = np.sort(full["scores"][0, :nf].astype(np.float64))[::-1]
            assert allsc[nf // 2 - 1] == allsc[nf // 2] and allsc[63] == allsc[64]      # tied scores at those cuts
    # more peaks than the largest capacity: 2 x 1100 anchors, every one a peak
    got, ref = check(kdev, sims, mask, None, 1, ((1, 1, 1), (2, 1, 1)), AO.MEAN, 0, 1, 2048, what="capacity, 2048 of more", bare=False)
    assert got["n_found"][0] == 2 * L - 1 and got["n_spans"][0] == 2048 and got["n_found"][2] == 1399 and got["n_spans"][2] == 1399


# ------------------------------------------------------------------ rows ------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 4, 5, 260])
def test_row_counts_and_row_independence(kdev, R):
    L = 70
    rng = np.random.default_rng(R)
    Ds = rng.integers(0, L + 1, R)
    mask, sims, valid = durations(L, Ds), MO.bumpy(R, L, R), some_valid(rng, R, L)
    scales = ((6, 2, 3), (15, 5, 7))
    got, _ = check(kdev, sims, mask, valid, 1, scales, AO.CONTRAST, 2, 1, 24, what="rows")
    ps, pv = prepared(sims, mask, valid, 1)
    for r in sorted({0, R // 2, R - 1}):                                                 # a row alone gives the same bits
        alone = run_anchors(kdev, ps[r:r + 1], mask[r:r + 1], pv[r:r + 1], 1, scales, AO.CONTRAST, 2, 1, 24)
        for name in got:
            assert np.array_equal(bits(alone[name]) if alone[name].dtype == F else alone[name], bits(got[name][r:r + 1]) if got[name].dtype == F else got[name][r:r + 1])


def test_three_rows_per_mask_row_and_both_validity_layouts(kdev):
    L, B, Q = 150, 4, 3
    rng = np.random.default_rng(17)
    Ds = [150, 149, 64, 1]
    mask, sims = durations(L, Ds), MO.bumpy(B * Q, L, 5)
    per_video, per_row = some_valid(rng, B, L), some_valid(rng, B * Q, L)
    scales = ((8, 2, 4), (30, 10, 10))
    a, _ = check(kdev, sims, mask, per_video, Q, scales, what="rpm=3, rpv=3")
    b, _ = check(kdev, sims, mask, per_row, 1, scales, what="rpm=3, rpv=1")
    check(kdev, sims, mask, None, Q, scales, what="rpm=3, valid=NULL")
    assert not np.array_equal(a["windows"], b["windows"])                                # the row's own validity row was read


def test_one_long_row(kdev):
    L = 36000
    mask = durations(L, [L, L - 7])
    sims = MO.bumpy(2, L, 3)
    valid = np.ones((2, L), dtype=F)
    valid[:, ::5] = 0
    scales = ((25, 6, 12), (50, 12, 25), (100, 25, 50), (200, 50, 100), (400, 100, 200), (3000, 5, 3000))
    got, _ = check(kdev, sims, mask, valid, 1, scales, AO.CONTRAST, 2, 1, 2048, what="long", bare=False)
    assert got["n_found"][0] > 1500
    got, _ = check(kdev, sims, mask, None, 1, scales, AO.MEAN, 2, 1, 256, what="long, cut", bare=False)
    assert got["n_found"][0] > 256 and got["n_spans"][0] == 256


# ------------------------------------------------------------------ the wrappers ------------------------------------------------------------------
def test_the_wrapper_on_both_layouts(kdev):
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import propose_anchors
    B, Q, L = 2, 3, 150
    rng = np.random.default_rng(50)
    Ds = [150, 101]
    mask, sims = durations(L, Ds), MO.bumpy(B * Q, L, 6)
    per_video, per_row = (rng.random((B, L)) < 0.7).astype(F), (rng.random((B * Q, L)) < 0.7).astype(F)
    scales = (8, (12, 3), (30, 10, 4))
    s, m = up(kdev, sims).view(B, Q, L), up(kdev, mask)
    for score, mode in (("contrast", AO.CONTRAST), ("mean", AO.MEAN)):
        for valid, rpv in ((per_video, Q), (per_row, 1), (None, Q)):
            ref = AO.anchors(sims, mask, valid, rpv, scales, mode, 1, 2, 40)
            forms = [None] if valid is None else [torch.from_numpy(valid).to(kdev), torch.from_numpy(valid != 0).to(kdev), torch.from_numpy(valid.astype(np.uint8)).to(kdev),
                                                  torch.from_numpy(valid).to(kdev).half()]
            for v in forms:
                if v is not None and rpv == 1:
                    v = v.view(B, Q, L)
                for mm in (m, m.bool()):
                    out = ops.span_anchors(s, mm, scales=scales, score=score, peak=1, min_usable=2, valid=v, max_spans=40, return_windows=True, return_scale=True)
                    assert isinstance(out, ops.SpanAnchors) and out.spans.shape == (B, Q, 40, 2) and out.windows.dtype == torch.int32 and out.scores.shape == (B, Q, 40)
                    assert out.n_spans.shape == (B, Q) and out.n_found.dtype == torch.int32 and out.scale.shape == (B, Q, 40)
                    got = dict(spans=out.spans, scores=out.scores, n_spans=out.n_spans, n_found=out.n_found, windows=out.windows, scale=out.scale)
                    compare({k: x.cpu().numpy().reshape(ref[k].shape) for k, x in got.items()}, ref, (score, rpv))
            bare = ops.span_anchors(s, m, scales=scales, score=score, peak=1, min_usable=2, valid=v, max_spans=40)
            assert bare.windows is None and bare.scale is None and torch.equal(bare.spans.view(torch.int32), out.spans.view(torch.int32))
            assert torch.equal(bare.scores.view(torch.int32), out.scores.view(torch.int32)) and torch.equal(bare.n_found, out.n_found)
        # the spans in span_scores_multi give the windows back
        back = ops.span_scores_multi(s, out.spans, m, return_windows=True)[1]
        assert torch.equal(back, out.windows)
        flat = propose_anchors(s.view(B * Q, L).cpu(), m.cpu(), scales=scales, score=score, peak=1, min_usable=2, max_spans=40, return_windows=True)
        assert flat.spans.device.type == "cpu" and flat.scale is None and np.array_equal(flat.windows.numpy(), ref["windows"])
    # the defaults: contrast, peak 2, 256 spans
    out = ops.span_anchors(s, m, scales=scales)
    compare({k: getattr(out, k).cpu().numpy().reshape(B * Q, *getattr(out, k).shape[2:]) for k in ("spans", "scores", "n_spans", "n_found")} | dict(windows=None, scale=None),
            AO.anchors(sims, mask, None, Q, scales), "defaults")


def _iou(lo, hi, a, b):
    inter = (torch.minimum(hi, b) - torch.maximum(lo, a)).clamp(min=0)
    return inter / ((hi - lo) + (b - a) - inter)


@pytest.mark.parametrize("multi", [False, True])
def test_ground_queries_anchored_equals_its_stages(dev, multi):
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval.similarity import Grounding, RefinedGrounding, ground_queries_anchored, refine_spans
    from test_gpu_windows_valid import movie
    B, Q, L, d = 2, 3, 520, 64
    text, video, true, _ = movie(B, Q, L, d, 7, distractor=False)
    if not multi:
        text, true = text[:, 1], true[:, 1]
    t, v = text.to(dev), video.to(hip.op_dtype()).to(dev)
    m = torch.ones(B, L, device=dev)
    m[1, 500:] = 0
    hidden = torch.ones(B, L, dtype=torch.bool, device=dev)
    hidden[:, 3::50] = False
    sims = (ops.frame_cosine_multi if multi else ops.frame_cosine)(t, v)
    per_query = (torch.rand(sims.shape, generator=torch.Generator().manual_seed(3)) < 0.9).to(dev)
    scales = ((20, 5, 10), (40, 10, 20), (80, 20, 40))
    gt = (true / m.sum(-1).cpu().view((-1,) + (1,) * (true.dim() - 1))).to(dev)
    for valid, score in ((None, "contrast"), (hidden, "contrast"), (hidden.float(), "mean"), (per_query, "contrast")):
        got = ground_queries_anchored(t, v, m, scales=scales, score=score, valid=valid, top=4, nms_iou=0.5, max_spans=64, gt=gt)
        assert isinstance(got, Grounding) and isinstance(got.proposals, ops.SpanAnchors)
        prop = ops.span_anchors(sims, m, scales=scales, score=score, valid=valid, max_spans=64, return_windows=True, return_scale=True)
        _same_tuple(got.proposals, prop, "proposals")
        rank = ops.span_rank(prop.scores, prop.spans, top=4, nms_iou=0.5, form="cxw", gt=gt)
        _same_tuple(got.rank, rank, "rank")
        at = rank.keep.clamp(min=0).long()
        held = (rank.keep >= 0) & (rank.keep < prop.n_spans.unsqueeze(-1))
        assert torch.equal(got.n_keep, held.sum(-1, dtype=torch.int32)) and got.spans.shape == sims.shape[:-1] + (4, 2)
        want_spans = torch.gather(prop.spans, -2, at.unsqueeze(-1).expand(at.shape + (2,)))
        assert torch.equal(got.spans[held].view(torch.int32), want_spans[held].view(torch.int32)) and bool(torch.isnan(got.spans[~held]).all())
        assert torch.equal(got.scores[held].view(torch.int32), torch.gather(prop.scores, -1, at)[held].view(torch.int32))
        # the kernel's answer on these cosine rows is the oracle's
        rows = sims.reshape(-1, L).cpu().numpy()
        vv = None if valid is None else valid.float().reshape(-1, L).cpu().numpy()
        rpv = 1 if valid is not None and valid.shape == sims.shape and valid.shape != m.shape else rows.shape[0] // B
        want = AO.anchors(rows, m.cpu().numpy(), vv, rpv, scales, AO.CONTRAST if score == "contrast" else AO.MEAN, 2, 1, 64)
        compare({k: getattr(prop, k).reshape(want[k].shape).cpu().numpy() for k in want}, want, "on cosine rows")
        if score == "contrast":                                                          # the planted 40-frame stretches rank first, exactly
            first = torch.gather(prop.windows, -2, at[..., :1].unsqueeze(-1).expand(at.shape[:-1] + (1, 2))).squeeze(-2)
            assert torch.equal(first.cpu().long(), true.long()), (first, true)
            assert bool((got.rank.first_hit[..., -1] == 0).all())
        # refined behind the ranking: the stage of ground_queries_refined
        ref = ground_queries_anchored(t, v, m, scales=scales, score=score, valid=valid, top=4, nms_iou=0.5, max_spans=64, gt=gt, radius=8, margin=12, min_len=2)
        assert isinstance(ref, RefinedGrounding)
        _same_tuple(ref.grounding, got, "grounding untouched")
        by_hand = refine_spans(sims, got.spans, m, radius=8, margin=12, min_len=2, valid=valid, return_windows=True, return_contrast=True)
        _same_tuple(ref.refined, by_hand, "refined")
        score_fn = ops.span_scores_masked_rows if rpv == 1 and rows.shape[0] != B else ops.span_scores_masked
        sc = score_fn(sims, by_hand.spans, m, valid=valid, skip_nan=True).scores
        assert torch.equal(ref.scores.view(torch.int32), sc.view(torch.int32))


def test_planted_rows_the_threshold_generator_misses(dev):
    """One frame at 1.0 compresses every relative level, so ``ground_queries`` keeps nothing near a 40-frame plateau of +0.2; the anchored chain ranks
    exactly that plateau first, in every row.  The cosine rows are the planted rows: a two-dimensional feature (s, sqrt(1 - s^2)) against the text
    (1, 0)."""
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval.similarity import ground_queries, ground_queries_anchored
    rows, los = AO.planted_rows()
    B, L = rows.shape
    video = torch.zeros(B, L, 64)
    video[..., 0] = torch.from_numpy(rows)
    video[..., 1] = torch.sqrt(1 - video[..., 0] ** 2)
    text = torch.zeros(B, 64)
    text[:, 0] = 1
    t, v, m = text.to(dev), video.to(hip.op_dtype()).to(dev), torch.ones(B, L, device=dev)
    lo = torch.from_numpy(los).to(dev).float()
    got = ground_queries_anchored(t, v, m, scales=AO.PLANTED_SCALES, score="contrast", peak=2)
    assert bool((got.proposals.n_found == got.proposals.n_spans).all()) and bool((got.proposals.n_found > 30).all())
    first = torch.gather(got.proposals.windows, 1, got.rank.keep[:, :1].long().unsqueeze(-1).expand(B, 1, 2)).squeeze(1)
    assert torch.equal(first.float(), torch.stack((lo, lo + 40), -1)), (first, los)
    # the kept span IS that window for rv_span_scores' rule
    back = ops.span_scores(ops.frame_cosine(t, v), got.spans, m, return_windows=True)[1]
    assert torch.equal(back[:, 0], first)
    inside = ground_queries_anchored(t, v, m, scales=AO.PLANTED_SCALES, score="mean", peak=2)
    w = torch.gather(inside.proposals.windows, 1, inside.rank.keep[:, :1].long().unsqueeze(-1).expand(B, 1, 2)).squeeze(1).float()
    assert bool(((w[:, 0] >= lo) & (w[:, 1] <= lo + 40)).all())                         # mean mode: a span INSIDE the plateau
    base = ground_queries(t, v, m, return_windows=True)
    kept = torch.gather(base.proposals.windows, 1, base.rank.keep.clamp(min=0).long().unsqueeze(-1).expand(-1, -1, 2)).float()
    iou = _iou(lo[:, None], lo[:, None] + 40, kept[..., 0], kept[..., 1])
    held = (base.rank.keep >= 0) & (base.rank.keep < base.proposals.n_spans.unsqueeze(-1))
    assert bool(held.any(-1).all()) and bool((iou[held] < 0.1).all())                   # the threshold chain keeps spans, none of them near the plateau


def test_the_anchor_calls_do_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the calls: with the stream kept busy by work queued before them, an event recorded just before
    has not completed when they return."""
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval.similarity import ground_queries_anchored, propose_anchors
    from test_gpu_windows_valid import movie
    B, Q, L, d = 2, 3, 520, 64
    text, video, true, _ = movie(B, Q, L, d, 8)
    t, v, m = text.to(dev), video.to(hip.op_dtype()).to(dev), torch.ones(B, L, device=dev)
    hidden = torch.ones(B, L, dtype=torch.bool, device=dev)
    hidden[:, ::16] = False
    rows = ops.frame_cosine_multi(t, v)
    scales = ((20, 5, 10), (40, 10, 20), (80, 20, 40))

    def calls():
        a = ground_queries_anchored(t, v, m, scales=scales, valid=hidden, top=5)
        b = ground_queries_anchored(t[:, 0], v, m.bool(), scales=(40,), score="mean", top=3, radius=8, margin=12)
        c = propose_anchors(rows, m, scales=scales, valid=rows > -2, return_windows=True, return_scale=True)
        e = ops.span_anchors(rows, m.bool(), scales=(5, 10), peak=0, max_spans=32)             # more peaks than max_spans: the cut runs
        return (a.spans, a.scores, a.n_keep, a.proposals.windows, a.rank.keep, b.grounding.spans, b.refined.spans, b.refined.windows, b.scores, c.spans, c.scores,
                c.windows, c.scale, c.n_found, e.spans, e.scores, e.n_spans, e.n_found)
    want = calls()                                                                     # (warm: libraries loaded, allocator blocks cached)
    first = torch.gather(want[3], -2, want[4][..., :1].long().unsqueeze(-1).expand(B, Q, 1, 2)).squeeze(-2)
    assert torch.equal(first.cpu().long(), true.long()) and bool((want[17] > 32).all())
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
    assert still_busy, "the anchor calls returned only after the work queued before them had finished: they synchronised"
    raw = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x                      # noqa: E731
    for x, y in zip(got, want):
        assert torch.equal(raw(x), raw(y))
