"""rvc_span_refine (the chain library's kernel behind ``ops.span_refine`` and ``eval.similarity``'s ``refine_spans`` / ``ground_queries_refined``: the
kept spans' bounds moved to the pair with the largest inside / outside contrast) against tests/span_refine_oracle.py, the rule restated in numpy.  The
rule works on integers, so the oracle IS the rule: windows, span bits and contrast bits are compared with NO tolerance.
tests/test_span_refine_host_logic.py holds the oracle itself to a brute-force statement and shows that on a step row it returns the plateau.

Every direct call writes into sentinel-filled buffers with 64 elements on either side of each output, once with every optional output and once with
none.  Behind every duration ``valid`` holds NaN - "not hidden" - and ``sims`` NaN in the even rows and 1.0, the largest value there is, in the odd
ones: a context cut at L instead of D would show.  NaN and +-inf sit under every frame ``valid`` hides.  The kernel is f32 / i32 only and the chain
library has one build, so the kernel items run once (``kdev``); the end-to-end items go through the flavoured libraries and run in both builds
(``dev``)."""
import numpy as np
import pytest
import torch

import span_refine_oracle as RO
import spans_masked_oracle as MO
from test_gpu_spans_masked import bits, dev, flav, kdev, up  # noqa: F401
from test_gpu_windows_valid import Fenced, _same_tuple, movie

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
F = np.float32


def durations(L, Ds):
    return (np.arange(L)[None, :] < np.asarray(Ds)[:, None]).astype(F)


def prepared(sims, mask, valid, rpv):
    """-> (sims, valid) with the fences of the module docstring."""
    sims = np.array(sims, dtype=F)
    R, L = sims.shape
    rpm = R // mask.shape[0]
    behind = np.repeat(mask, rpm, axis=0) == 0
    fill = np.where(np.arange(R)[:, None] % 2 == 0, F(NAN), F(1.0)).astype(F) * np.ones((1, L), dtype=F)
    sims[behind] = fill[behind]
    if valid is not None:
        valid = np.array(valid, dtype=F)
        with np.errstate(invalid="ignore"):
            hidden = np.repeat(valid == 0, rpv, axis=0) & ~behind
        poison = np.resize(np.array([NAN, INF, -INF], dtype=F), sims.shape)
        sims[hidden] = poison[hidden]
        valid[mask[(np.arange(valid.shape[0]) * rpv) // rpm] == 0] = NAN
    return sims, valid


def run_refine(dev, sims, spans, form, mask, valid, rpv, radius, margin, min_len=1, full=True):
    from revisionllm_amd import hip
    R, L = sims.shape
    N = spans.shape[1]
    s, p, m, v = up(dev, sims), up(dev, spans), up(dev, mask), up(dev, valid)
    o = dict(spans=Fenced(R * N * 2, torch.float32, dev), windows=Fenced(R * N * 2, torch.int32, dev) if full else None,
             contrast=Fenced(R * N, torch.float32, dev) if full else None, contrast0=Fenced(R * N, torch.float32, dev) if full else None)
    ptr = lambda x: x.ptr if x is not None else None                                            # noqa: E731
    rc = hip.chain_lib().rvc_span_refine(hip.ptr(s), hip.ptr(p), form, hip.ptr(m), hip.ptr(v), rpv, R, R // mask.shape[0], L, N, radius, margin, min_len,
                                         ptr(o["spans"]), ptr(o["windows"]), ptr(o["contrast"]), ptr(o["contrast0"]), hip.stream())
    hip.chain_check(rc, "rvc_span_refine")
    torch.cuda.synchronize()
    shapes = dict(spans=(R, N, 2), windows=(R, N, 2), contrast=(R, N), contrast0=(R, N))
    return {k: (x.take(shapes[k]) if x is not None else None) for k, x in o.items()}


def check(dev, sims, spans, form, mask, valid, rpv, radius, margin, min_len=1, what="", round_trip=True):
    """With every optional output and with none, bit for bit against the oracle; then ``ops.span_scores`` on the refined spans gives the windows
    back -> (got, ref)."""
    from revisionllm_amd import ops
    sims, valid = prepared(sims, mask, valid, rpv)
    spans = np.ascontiguousarray(spans, dtype=F)
    ref = RO.refine(sims, spans, form, mask, valid, rpv, radius, margin, min_len)
    what = f"{what} R={sims.shape[0]} L={sims.shape[1]} N={spans.shape[1]} form={form} rpv={rpv} radius={radius} margin={margin} min_len={min_len} valid={valid is not None}"
    got = run_refine(dev, sims, spans, form, mask, valid, rpv, radius, margin, min_len)
    assert np.array_equal(got["windows"], ref["windows"]), (what, "windows", np.argwhere(got["windows"] != ref["windows"])[:4].tolist(),
                                                            got["windows"][got["windows"] != ref["windows"]][:4], ref["windows"][got["windows"] != ref["windows"]][:4])
    for name in ("spans", "contrast", "contrast0"):
        a, b = bits(got[name]), bits(ref[name])
        assert np.array_equal(a, b), (what, name, np.argwhere(a != b)[:4].tolist())
    bare = run_refine(dev, sims, spans, form, mask, valid, rpv, radius, margin, min_len, full=False)
    assert np.array_equal(bits(bare["spans"]), bits(ref["spans"])), (what, "spans without the optional outputs")
    if round_trip and mask.shape[0] == sims.shape[0]:
        back = ops.span_scores(up(dev, np.nan_to_num(sims)), up(dev, got["spans"]), up(dev, mask), return_windows=True)[1].cpu().numpy()
        assert np.array_equal(back, ref["windows"]), (what, "round trip")
    return got, ref


def from_pairs(pairs, Ds, form):
    """[R,N] (lo, hi) frame pairs -> spans whose windows they are (a quarter frame inside either bound), in ``form``."""
    pairs = np.asarray(pairs, dtype=np.float64)
    d = np.maximum(np.asarray(Ds, dtype=np.float64), 1)[:, None]
    x1, x2 = (pairs[..., 0] + 0.25) / d, (pairs[..., 1] - 0.25) / d
    return np.stack([x1, x2] if form == RO.XX else [(x1 + x2) / 2, x2 - x1], -1).astype(F)


def some_pairs(rng, R, N, L):
    """Windows of every kind: short and long, leaving the row at either end, behind the duration, empty and reversed."""
    lo = rng.integers(-4, L + 4, (R, N))
    ln = np.where(rng.random((R, N)) < 0.5, rng.integers(-1, 6, (R, N)), rng.integers(1, L + 2, (R, N)))
    return np.stack([lo, lo + ln], -1)


def some_valid(rng, M, L):
    return rng.choice(np.array([1.0, 1.0, 1.0, 0.0, -0.0, NAN, 2.0, 1e-45], dtype=F), (M, L))


# ------------------------------------------------------------------ rows, durations, zones ------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 129, 300])
def test_lengths_and_durations(kdev, L):
    rng = np.random.default_rng(L)
    Ds = [L, L - 1, 1, 0]
    mask = durations(L, Ds)
    sims = MO.bumpy(4, L, L)
    for case, (radius, margin, min_len) in enumerate(((1, 1, 1), (2, 3, 1), (5, 40, 3), (64, 128, 1))):
        N = 9 if radius < 64 else 3
        for form in (RO.XX, RO.CXW):
            spans = from_pairs(some_pairs(rng, 4, N, L), Ds, form)
            spans[0, 0] = (NAN, 0.5)
            spans[1, 0] = (0.5, INF if form == RO.XX else -0.3)                 # not finite / reversed
            spans[2, 0] = from_pairs([[[0, L]]], [1], form)[0, 0]                # the whole array on a row of one frame
            valid = None if (case + form) % 2 else some_valid(rng, 4, L)
            got, ref = check(kdev, sims, spans, form, mask, valid, 1, radius, margin, min_len, what="lengths")
            assert (got["windows"][3] == -1).all() and np.isnan(got["spans"][3]).all()                      # D = 0: every span is void
            assert got["windows"][0, 0].tolist() == [-1, -1] and (form != RO.XX or got["windows"][1, 0].tolist() == [-1, -1])
            w = got["windows"][:3]
            ok = w[..., 0] >= 0
            assert (w[ok][:, 0] < w[ok][:, 1]).all() and all((w[r][w[r][:, 0] >= 0][:, 1] <= Ds[r]).all() for r in range(3))


@pytest.mark.parametrize("radius", [1, 2, 5])
def test_span_lengths_where_the_zones_meet_and_at_the_ends(kdev, radius):
    L, D = 300, 291
    mask = durations(L, [D])
    sims = MO.bumpy(1, L, 7 + radius)
    pairs = []
    for ln in (1, 2, 2 * radius - 1, 2 * radius, 2 * radius + 1, 2 * radius + 2, 64, 150):
        for lo in (0, 1, radius, 100, D - ln - radius, D - ln - 1, D - ln):
            pairs.append((lo, lo + ln))
    pairs += [(0, D), (0, L), (D - 1, L), (-5, 3), (D, L), (D + 2, D + 5)]
    for form in (RO.XX, RO.CXW):
        spans = from_pairs([pairs], [D], form)
        for margin in (1, 3, 128):
            for min_len in (1, 4, 200):
                got, ref = check(kdev, sims, spans, form, mask, None, 1, radius, margin, min_len, what="zones")
    assert got["windows"][0, -2:].tolist() == [[-1, -1], [-1, -1]] and (got["windows"][0, :-2] >= 0).all()
    # min_len above every candidate: the original pair is still one
    ln = got["windows"][0, :-2, 1] - got["windows"][0, :-2, 0]
    orig = np.clip(np.array(pairs[:-2]), 0, D)
    assert ((ln >= 200) | (got["windows"][0, :-2] == orig).all(-1)).all()


def test_a_long_row_and_the_widest_search(kdev):
    L = 20000
    mask = durations(L, [L, L - 7])
    sims = MO.bumpy(2, L, 3)
    pairs = [[(2500, 17500), (0, 15000), (19000, L)], [(5000, 19993), (100, 101), (19900, L)]]
    for form in (RO.XX, RO.CXW):
        spans = from_pairs(pairs, [L, L - 7], form)
        valid = np.ones((2, L), dtype=F)
        valid[:, ::5] = 0
        check(kdev, sims, spans, form, mask, valid if form else None, 1, 64, 128, 1, what="long")
    check(kdev, sims, spans, RO.CXW, mask, None, 1, 64, 1, 1, what="long, margin 1")


@pytest.mark.parametrize("N", [1, 3, 4, 5, 9])
def test_span_counts(kdev, N):
    L = 140
    rng = np.random.default_rng(N)
    Ds = [140, 99, 64]
    spans = from_pairs(some_pairs(rng, 3, N, L), Ds, RO.CXW)
    check(kdev, MO.bumpy(3, L, N), spans, RO.CXW, durations(L, Ds), some_valid(rng, 3, L), 1, 2, 3, what="N")


@pytest.mark.parametrize("R", [1, 3, 260])
def test_row_counts_and_row_independence(kdev, R):
    L, N = 70, 3
    rng = np.random.default_rng(R)
    Ds = rng.integers(0, L + 1, R)
    mask, sims, valid = durations(L, Ds), MO.bumpy(R, L, R), some_valid(rng, R, L)
    spans = from_pairs(some_pairs(rng, R, N, L), Ds, RO.XX)
    got, _ = check(kdev, sims, spans, RO.XX, mask, valid, 1, 2, 3, what="rows")
    ps, pv = prepared(sims, mask, valid, 1)
    for r in sorted({0, R // 2, R - 1}):                                                 # a row alone gives the same bits
        alone = run_refine(kdev, ps[r:r + 1], spans[r:r + 1], RO.XX, mask[r:r + 1], pv[r:r + 1], 1, 2, 3)
        for name in got:
            assert np.array_equal(bits(alone[name]) if alone[name].dtype == F else alone[name], bits(got[name][r:r + 1]) if got[name].dtype == F else got[name][r:r + 1])


def test_three_rows_per_mask_row_and_both_validity_layouts(kdev):
    L, B, Q, N = 150, 4, 3, 5
    rng = np.random.default_rng(17)
    Ds = [150, 149, 64, 1]
    mask, sims = durations(L, Ds), MO.bumpy(B * Q, L, 5)
    spans = from_pairs(some_pairs(rng, B * Q, N, L), np.repeat(Ds, Q), RO.CXW)
    per_video, per_row = some_valid(rng, B, L), some_valid(rng, B * Q, L)
    a, _ = check(kdev, sims, spans, RO.CXW, mask, per_video, Q, 5, 8, what="rpm=3, rpv=3")
    b, _ = check(kdev, sims, spans, RO.CXW, mask, per_row, 1, 5, 8, what="rpm=3, rpv=1")
    check(kdev, sims, spans, RO.CXW, mask, None, Q, 5, 8, what="rpm=3, valid=NULL")
    assert not np.array_equal(a["windows"], b["windows"])                                # the row's own validity row was read


# ------------------------------------------------------------------ validity ------------------------------------------------------------------
def test_valid_values_hidden_frames_and_inadmissible_spans(kdev):
    """-0.0 and 0.0 hide a frame; NaN, 2 and 1e-45 do not.  A span with no usable frame inside any candidate, and one with no usable context."""
    L, D = 140, 130
    mask = durations(L, [D] * 3)
    sims = MO.bumpy(3, L, 9)
    valid = np.resize(np.array([-0.0, NAN, 2.0, 1e-45, 0.0, 1.0, 1.0], dtype=F), (3, L))
    valid[1, 40:60] = 0                                                                 # nothing usable inside [45, 55) within radius 2
    valid[2, :] = 0
    valid[2, 50:60] = 1                                                                 # nothing usable outside [50, 60): no context
    pairs = [[(10, 30), (45, 55), (0, 7)], [(45, 55), (44, 56), (38, 45)], [(50, 60), (48, 62), (52, 58)]]
    spans = from_pairs(pairs, [D] * 3, RO.XX)
    got, ref = check(kdev, sims, spans, RO.XX, mask, valid, 1, 2, 3, what="valid values")
    assert got["windows"][1, 0].tolist() == [45, 55] and np.isnan(got["contrast"][1, 0]) and np.isnan(got["contrast0"][1, 0])      # kept, NaN
    assert got["windows"][2, 1].tolist() == [48, 62] and np.isnan(got["contrast"][2, 1])                # no candidate has context: kept, NaN
    assert np.isnan(got["contrast0"][2, 0]) and not np.isnan(got["contrast"][2, 0])                     # (50, 60) has none, a shorter candidate has
    assert not np.isnan(got["contrast"][0]).any() and not np.isnan(got["contrast"][2, 2])         # (52, 58) has the plateau's other frames as context
    # a NaN similarity is never usable, with valid or without
    s2 = sims.copy()
    s2[0, 12:20] = NAN
    check(kdev, s2, spans, RO.XX, mask, None, 1, 2, 3, what="NaN sims, valid=NULL")


def test_every_tie_break(kdev):
    """Flat rows keep the original pair (distance); two equal plateaus inside one search range: the nearer, then the smaller a, then the smaller b."""
    L = 120
    mask = durations(L, [L] * 4)
    sims = np.zeros((4, L), dtype=F)
    sims[0] = 0.25
    sims[1, 30:40] = 1
    sims[1, 50:60] = 1                                                                  # two equal plateaus, 10 floor frames between
    sims[2] = sims[1]
    sims[3, 20:100:2] = 0.5                                                             # a comb: many equal contrasts
    pairs = [[(10, 20), (0, 5), (100, 120), (55, 56)], [(40, 50), (35, 55), (41, 49), (39, 51)], [(30, 60), (45, 46), (25, 45), (44, 66)],
             [(30, 40), (31, 41), (21, 99), (50, 51)]]
    for form in (RO.XX, RO.CXW):
        spans = from_pairs(pairs, [L] * 4, form)
        for radius, margin in ((5, 3), (12, 10), (64, 128)):
            got, ref = check(kdev, sims, spans, form, mask, None, 1, radius, margin, what="ties")
            assert got["windows"][0].tolist() == [list(p) for p in pairs[0]]
    got, _ = check(kdev, sims, spans, RO.CXW, mask, None, 1, 12, 10, what="ties")
    assert got["windows"][1, 0].tolist() == [30, 40]                                     # (40, 50) between the plateaus: both at distance 20, the smaller a


# ------------------------------------------------------------------ the wrappers ------------------------------------------------------------------
def test_the_wrapper_on_both_layouts(kdev):
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import refine_spans
    B, Q, L, N = 2, 3, 150, 5
    rng = np.random.default_rng(50)
    Ds = [150, 101]
    mask, sims = durations(L, Ds), MO.bumpy(B * Q, L, 6)
    per_video, per_row = (rng.random((B, L)) < 0.7).astype(F), (rng.random((B * Q, L)) < 0.7).astype(F)
    for form, name in ((RO.CXW, "cxw"), (RO.XX, "xx")):
        spans = from_pairs(some_pairs(rng, B * Q, N, L), np.repeat(Ds, Q), form)
        s, p, m = up(kdev, sims).view(B, Q, L), up(kdev, spans).view(B, Q, N, 2), up(kdev, mask)
        for valid, rpv in ((per_video, Q), (per_row, 1), (None, Q)):
            ref = RO.refine(sims, spans, form, mask, valid, rpv, 4, 6, 2)
            forms = [None] if valid is None else [torch.from_numpy(valid).to(kdev), torch.from_numpy(valid != 0).to(kdev), torch.from_numpy(valid.astype(np.uint8)).to(kdev),
                                                  torch.from_numpy(valid).to(kdev).half()]
            for v in forms:
                if v is not None and rpv == 1:
                    v = v.view(B, Q, L)
                for mm in (m, m.bool()):
                    out = ops.span_refine(s, p, mm, form=name, radius=4, margin=6, min_len=2, valid=v, return_windows=True, return_contrast=True)
                    assert isinstance(out, ops.RefinedSpans) and out.spans.shape == (B, Q, N, 2) and out.windows.dtype == torch.int32 and out.contrast.shape == (B, Q, N)
                    assert np.array_equal(out.windows.cpu().numpy().reshape(B * Q, N, 2), ref["windows"])
                    for x, y in ((out.spans, ref["spans"]), (out.contrast, ref["contrast"]), (out.contrast0, ref["contrast0"])):
                        assert np.array_equal(bits(x.cpu().numpy().reshape(y.shape)), bits(y))
            bare = ops.span_refine(s, p, m, form=name, radius=4, margin=6, min_len=2, valid=v)
            assert bare.windows is None and bare.contrast is None and bare.contrast0 is None and torch.equal(bare.spans.view(torch.int32), out.spans.view(torch.int32))
        # the refined spans in span_scores_multi give the windows back
        back = ops.span_scores_multi(s, out.spans, m, return_windows=True)[1]
        assert torch.equal(back, out.windows)
        flat = refine_spans(s.view(B * Q, L).cpu(), p.view(B * Q, N, 2).cpu(), m.cpu(), form=name, radius=4, margin=6, min_len=2, return_windows=True)
        assert flat.spans.device.type == "cpu" and np.array_equal(flat.windows.numpy(), RO.refine(sims, spans, form, mask, None, Q, 4, 6, 2)["windows"])
    assert ops.span_refine(s, p[:, :, :0], m, radius=4, margin=6).spans.shape == (B, Q, 0, 2)


@pytest.mark.parametrize("multi", [False, True])
def test_ground_queries_refined_equals_its_stages_and_finds_planted_plateaus(dev, multi):
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval.similarity import RefinedGrounding, ground_queries_masked, ground_queries_refined, span_cxw_to_xx
    B, Q, L, d = 2, 3, 520, 64
    text, video, true, _ = movie(B, Q, L, d, 7, distractor=False)
    if not multi:
        text, true = text[:, 1], true[:, 1]
    t, v = text.to(dev), video.to(hip.op_dtype()).to(dev)
    m = torch.ones(B, L, device=dev)
    m[1, 500:] = 0
    hidden = torch.ones(B, L, dtype=torch.bool, device=dev)
    hidden[:, 3::50] = False
    kw = dict(top=4, nms_iou=0.5, smooth=9, levels=(0.8,), max_spans=32, return_windows=True)
    sims = (ops.frame_cosine_multi if multi else ops.frame_cosine)(t, v)
    for valid, skip, form in ((None, False, "cxw"), (hidden, True, "cxw"), (hidden.float(), False, "xx")):
        got = ground_queries_refined(t, v, m, radius=8, margin=12, min_len=2, form=form, valid=valid, skip_nan=skip, **kw)
        assert isinstance(got, RefinedGrounding)
        base = ground_queries_masked(t, v, m, valid=valid, skip_nan=skip, min_len=2, **kw)
        _same_tuple(got.grounding, base, "grounding untouched")
        ref = ops.span_refine(sims, base.spans, m, radius=8, margin=12, min_len=2, valid=valid, return_windows=True, return_contrast=True)
        sc = ops.span_scores_masked(sims, ref.spans, m, valid=valid, skip_nan=skip).scores
        _same_tuple(got.refined, ref._replace(spans=span_cxw_to_xx(ref.spans)) if form == "xx" else ref, "refined")
        assert torch.equal(got.scores.view(torch.int32), sc.view(torch.int32)) and got.scores.shape == base.scores.shape
        # the kernel's answer on these cosine rows is the oracle's
        rows = sims.reshape(-1, L).cpu().numpy()
        Q_ = rows.shape[0] // B
        vv = None if valid is None else valid.float().cpu().numpy()
        want = RO.refine(rows, base.spans.reshape(rows.shape[0], -1, 2).cpu().numpy(), RO.CXW, m.cpu().numpy(), vv, Q_, 8, 12, 2)
        assert np.array_equal(got.refined.windows.reshape(want["windows"].shape).cpu().numpy(), want["windows"])
        assert np.array_equal(bits(got.refined.contrast.reshape(want["contrast"].shape).cpu().numpy()), bits(want["contrast"]))
        # the first proposal sits inside the plateau, short of its bounds by the smoothing; the refined one has them exactly
        first = base.proposals.windows.reshape(rows.shape[0], -1, 2).cpu()[torch.arange(rows.shape[0]), base.rank.keep.reshape(rows.shape[0], -1)[:, 0].cpu().long()]
        plateau = true.reshape(-1, 2).long()
        assert bool(((first[:, 0] > plateau[:, 0]) & (first[:, 1] < plateau[:, 1])).all()), (first, plateau)
        assert torch.equal(got.refined.windows.reshape(rows.shape[0], -1, 2)[:, 0].cpu().long(), plateau), (got.refined.windows, plateau)
        assert bool((got.refined.contrast.reshape(rows.shape[0], -1)[:, 0] > got.refined.contrast0.reshape(rows.shape[0], -1)[:, 0]).all())
        pad = torch.isnan(base.spans[..., 0])
        assert bool((got.refined.windows[pad] == -1).all()) and bool(torch.isnan(got.scores[pad]).all())


def test_the_refining_calls_do_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the calls: with the stream kept busy by work queued before them, an event recorded just before
    has not completed when they return."""
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval.similarity import ground_queries_refined, refine_spans
    B, Q, L, d = 2, 3, 520, 64
    text, video, true, _ = movie(B, Q, L, d, 8)
    t, v, m = text.to(dev), video.to(hip.op_dtype()).to(dev), torch.ones(B, L, device=dev)
    hidden = torch.ones(B, L, dtype=torch.bool, device=dev)
    hidden[:, ::16] = False
    rows = ops.frame_cosine_multi(t, v)
    answers = (torch.stack((true[..., 0] - 3, true[..., 1] + 5), -1) / L).unsqueeze(-2).to(dev)                 # an LLM's (start, end) answers, a few frames off

    def calls():
        a = ground_queries_refined(t, v, m, radius=8, margin=12, valid=hidden, skip_nan=True, top=5, smooth=9, gap=1)
        b = ground_queries_refined(t[:, 0], v, m.bool(), radius=64, margin=128, form="xx", top=3)
        c = refine_spans(rows, answers, m, form="xx", radius=8, margin=12, valid=hidden, return_windows=True, return_contrast=True)
        e = ops.span_refine(rows, answers, m.bool(), form="xx", radius=8, margin=12, valid=rows > -2)
        return (a.grounding.spans, a.refined.spans, a.refined.windows, a.refined.contrast, a.scores, b.refined.spans, b.scores, c.spans, c.windows, c.contrast,
                c.contrast0, e.spans)
    want = calls()                                                                     # (warm: libraries loaded, allocator blocks cached)
    assert torch.equal(want[8].cpu(), torch.stack((true[..., 0], true[..., 1]), -1).unsqueeze(-2).int())          # the answers snapped to the stretches
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
    assert still_busy, "the refining calls returned only after the work queued before them had finished: they synchronised"
    raw = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x                      # noqa: E731
    for x, y in zip(got, want):
        assert torch.equal(raw(x), raw(y))
