"""rv_frame_cosine, rv_span_scores and rv_attn_pool (the kernels behind ``eval.similarity.forward_clip_matching`` and ``_attention_pooling``) against the
float64 restatements of tests/similarity_oracle.py, computed on the CPU from the inputs after rounding to the type the kernel reads; f32 features and the
16-bit operands of both builds.  tests/test_similarity_host_logic.py holds the oracle to the reference's outputs (fixture G17).

Bounds.  Cosine rows and top-k scores: the project's COSINE_BOUND (1e-4 absolute, the number test_gpu_rowops_scores_edges.py holds rv_topk_cosine to), times
k / 3 for k > 3.  The softmax forms (rv_attn_pool, the attention mode of rv_span_scores) amplify rounding by 1 / temperature and the project had no number for them:
theirs is 4 x the distance of the reference's own formula evaluated by torch in f32 on the CPU from float64, the worst over this module's inputs per temperature
(REF_F32_ERR below, ``reference_f32_errors`` re-measures it; the factor is for another summation order over the frames)."""
import functools
import os

import pytest
import torch

import similarity_oracle as O
from helpers import feats, fl, rel_err

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")
COSINE_BOUND = 1e-4
LDS_BYTES = 64 * 1024
TAUS_POOL = (0.01, 0.07, 1.0, -1.0)
TAUS_SPAN = (0.01, 1.0)
# max-norm relative distance from float64 of torch's f32 CPU evaluation of similarity.py:105-113 (rv_attn_pool's cases below: T in {1, 64, 65, 300} x d in
# {33, 768} x Nt in {1, 3}, and T = 16312 at d = 8 for temperature 1) and of sum softmax(s / temperature) s over the windows of the span cases, the worst
# over f32-, fp16- and bf16-valued inputs; measured with reference_f32_errors() on the CPU (test_the_f32_reference_distances_.. re-measures them into profiles/similarity_err_*.log next to the kernels' figures)
REF_F32_ERR = {"attn_pool": {0.01: 4.11e-6, 0.07: 9.47e-7, 1.0: 4.42e-6, -1.0: 9.76e-7}, "span_attention": {0.01: 8.55e-7, 1.0: 1.31e-7}}
SOFTMAX_MARGIN = 4.0


def softmax_bound(what, tau):
    return SOFTMAX_MARGIN * REF_F32_ERR[what][tau]


@pytest.fixture(scope="module", params=[None] if _FORCED else ["f16", "bf16"])
def flav(request, op_flavour):
    """Both operand flavours (the module list of conftest.py is fixed, so the module brings its own parameter; REVISION_TEST_FLAVOURS still narrows it)."""
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


def _note(label, value):
    """A line that names the case in the RV_LOG_ERR file (profiles/similarity_err_<flavour>.log)."""
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            fh.write(f"  similarity {fl()} {label} {value:.3e}\n")
    return value


def _abs_err(y, ref, label):
    return _note(label + " abs", float((y.cpu().double() - ref).abs().max()))


def _rel(y, ref, label):
    return _note(label + " rel", rel_err(y.cpu(), ref))


def _rt(x, kind):
    """x (f32) rounded to what the kernel reads: "f16" / "bf16" -> through that type, "f32" -> unchanged."""
    return x if kind == "f32" else x.to(_dt(kind)).float()


def _dt(kind):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[kind]


def _kinds():
    return (fl(), "f32")


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


# ------------------------------------------------------------------ inputs ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clip_like(B, L, d, kind, tag=""):
    """Unit-norm frames that share a component along their video's unit-norm text, as CLIP features do (cosines around 0.3, spread 1 / sqrt(d)), with another
    weight per video (a wrong block offset shows); -> (text f32 [B,d], video as f32 holding ``kind``-representable values [B,L,d])."""
    text = _unit(feats(f"sim.t.{B}.{d}{tag}", (B, d)))
    g = _unit(feats(f"sim.v.{B}.{L}.{d}{tag}", (B, L, d)))
    video = _unit(g + text[:, None, :] * (0.25 + 0.1 * torch.arange(B, dtype=torch.float32))[:, None, None])
    return text, _rt(video, kind)


@functools.lru_cache(maxsize=None)
def pool_inputs(Nv, T, d, Nt, kind):
    """Videos of clip_like frames (each around a text of its own) and Nt texts: the first video's text and texts near it."""
    t0, video = clip_like(Nv, T, d, kind, tag=".pool")
    text = _unit(t0[:1] + 0.5 * _unit(feats(f"sim.pt.{Nt}.{d}", (Nt, d))))
    text[0] = t0[0]
    return text, video


SPAN_L, SPAN_DUR = 200, (200, 130)
SPAN_WINDOWS = [(0, 200), (7, 8), (30, 32), (50, 53), (60, 64), (70, 135), (0, 1), (199, 200), (100, 100), (3, 68), (140, 143), (90, 97)]


@functools.lru_cache(maxsize=None)
def span_inputs():
    """sims [2, 200] like a cosine row, masks of duration 200 and 130 and spans that give windows of 0, 1, 2, 3, 4, 65 and L frames (x1 = (lo + 0.5) / duration,
    x2 = (hi - 0.5) / duration: floor and ceil land on lo and hi whatever the rounding; the empty window is (0.5, 0) at an even duration)."""
    sims = 0.3 + 0.05 * feats("sim.span.sims", (2, SPAN_L))
    mask = torch.zeros(2, SPAN_L)
    spans = torch.zeros(2, len(SPAN_WINDOWS), 2)
    for b, D in enumerate(SPAN_DUR):
        mask[b, :D] = 1
        for n, (lo, hi) in enumerate(SPAN_WINDOWS):
            if hi == lo:
                spans[b, n] = torch.tensor([0.5, 0.0])
            elif (lo, hi) == (0, SPAN_L):
                spans[b, n] = torch.tensor([0.5, 1.0]) if D == SPAN_L else torch.tensor([0.5 * SPAN_L / D, SPAN_L / D])
            else:
                x1, x2 = (lo + 0.5) / D, (hi - 0.5) / D
                spans[b, n] = torch.tensor([(x1 + x2) / 2, x2 - x1])
    win = O.windows(spans, mask)
    lens = set((win[..., 1] - win[..., 0]).clamp_min(0).flatten().tolist())
    assert {0, 1, 2, 3, 4, 65, SPAN_L} <= lens, lens
    return sims, mask, spans, win


def span_tie_inputs():
    """span_inputs with exact ties: in the window (70, 135) the largest value appears twice (frames 80 and 120), in (3, 68) the second largest three times."""
    sims, mask, spans, win = span_inputs()
    sims = sims.clone()
    for b in range(2):
        sims[b, 80] = sims[b, 120] = float(sims[b, 70:135].max()) + 0.01
        second = float(torch.sort(sims[b, 3:68], descending=True).values[1])
        sims[b, 10] = sims[b, 40] = sims[b, 60] = second
    return sims, mask, spans, win


POOL_T, POOL_D, POOL_NT, POOL_NV = (1, 64, 65, 300), (33, 768), (1, 3), 3
POOL_LAST_D = 8
POOL_LAST_T = (LDS_BYTES - 256) // 4 - POOL_LAST_D          # the last (d + T) * 4 + 256 that fits


def reference_f32_errors(kinds=("f32", "f16", "bf16")):
    """The figures behind REF_F32_ERR: torch's f32 CPU evaluation of the reference's formulas against float64 on this module's inputs, the worst per temperature."""
    worst = {"attn_pool": {t: 0.0 for t in TAUS_POOL}, "span_attention": {t: 0.0 for t in TAUS_SPAN}}
    for kind in kinds:
        for T in POOL_T:
            for d in POOL_D:
                for Nt in POOL_NT:
                    text, video = pool_inputs(POOL_NV, T, d, Nt, kind)
                    for tau in TAUS_POOL:
                        worst["attn_pool"][tau] = max(worst["attn_pool"][tau], rel_err(O.attn_pool_f32(text, video, tau), O.attn_pool64(text, video, tau)))
        text, video = pool_inputs(1, POOL_LAST_T, POOL_LAST_D, 1, kind)
        worst["attn_pool"][1.0] = max(worst["attn_pool"][1.0], rel_err(O.attn_pool_f32(text, video, 1.0), O.attn_pool64(text, video, 1.0)))
    for sims, mask, spans, win in (span_inputs(), span_tie_inputs(), long_row_inputs(), fence_inputs()):
        for tau in TAUS_SPAN:
            e = rel_err(O.span_attention_f32(sims, win, tau), O.span_scores64(sims, win, "attention", temperature=tau))
            worst["span_attention"][tau] = max(worst["span_attention"][tau], e)
    return worst


@functools.lru_cache(maxsize=None)
def long_row_inputs():
    """L = 20000 (80 KB of similarities: more than any LDS the kernels ask for), one span over everything and one over the second half."""
    L = 20000
    sims = 0.3 + 0.05 * feats("sim.span.long", (1, L))
    mask = torch.ones(1, L)
    spans = torch.tensor([[[0.5, 1.0], [0.75, 0.5]]])
    win = O.windows(spans, mask)
    assert win[0].tolist() == [[0, L], [L // 2, L]]
    return sims, mask, spans, win


FENCE_L, FENCE_WINDOWS = 96, [(0, 5), (7, 72), (74, 75), (77, 96)]


@functools.lru_cache(maxsize=None)
def fence_inputs():
    """Two rows of 96 similarities, four windows that touch both ends of the row, and NaN in the elements lo - 1 and hi next to every window."""
    L = FENCE_L
    mask = torch.ones(2, L)
    spans = torch.tensor([[((lo + 0.5) / L + (hi - 0.5) / L) / 2, (hi - 0.5) / L - (lo + 0.5) / L] for lo, hi in FENCE_WINDOWS])[None].repeat(2, 1, 1)
    win = O.windows(spans, mask)
    assert win[0].tolist() == [list(w) for w in FENCE_WINDOWS]
    sims = 0.3 + 0.05 * feats("sim.span.fence", (2, L))
    for lo, hi in FENCE_WINDOWS:
        if lo > 0:
            sims[:, lo - 1] = float("nan")
        if hi < L:
            sims[:, hi] = float("nan")
    return sims, mask, spans, win


def test_the_f32_reference_distances_the_softmax_bounds_come_from(dev):
    """Re-measures REF_F32_ERR on this machine's CPU (torch's f32 evaluation of the reference's formulas against float64, this module's inputs) and writes the
    figures into the error log next to the kernels'.  CPUs differ in how torch orders its f32 sums, so the figures need not repeat to the digit: each has to
    stay inside the bound that was derived from it."""
    for what, per_tau in reference_f32_errors().items():
        for tau, e in per_tau.items():
            _note(f"reference f32 (CPU, torch) vs float64, worst over f32 / fp16 / bf16 inputs: {what} tau{tau} rel", e)
            _note(f"... the constant the bound is 4 x of: {what} tau{tau}", REF_F32_ERR[what][tau])
            assert 0 < e < softmax_bound(what, tau), (what, tau, e)


# ------------------------------------------------------------------ rv_frame_cosine ------------------------------------------------------------------
def _cosine(dev, text, video, kind):
    from revisionllm_amd import ops
    return ops.frame_cosine(text.to(dev), video.to(_dt(kind)).to(dev))


@pytest.mark.parametrize("d", [1, 33, 64, 768, 1024])
def test_frame_cosine_widths_and_lengths(dev, d):
    """The generic path (d = 1, 33) and the 16-byte-load path (d = 64, 768, 1024) in both feature types, frame counts around the 32 frames of a block, the
    eight of a wave and the four it keeps in flight, one and three videos."""
    for kind in _kinds():
        for L in (1, 63, 64, 65, 257):
            text, video = clip_like(3, L, d, kind)
            ref = O.frame_cosine64(text, video)
            for B in (1, 3):
                y = _cosine(dev, text[:B], video[:B], kind)
                assert y.shape == (B, L) and y.dtype == torch.float32 and y.device == dev
                assert _abs_err(y, ref[:B], f"frame_cosine {kind} d{d} L{L} B{B}") < COSINE_BOUND, (kind, d, L, B)


def test_frame_cosine_of_a_feature_view_that_is_not_16_byte_aligned(dev):
    """The same values at an address 16-byte loads cannot take: the entry point switches to the generic path and the row is the same within the bound."""
    from revisionllm_amd import ops
    for kind in _kinds():
        text, video = clip_like(3, 65, 64, kind)
        flat = torch.zeros(video.numel() + 1, dtype=_dt(kind), device=dev)
        flat[1:] = video.to(_dt(kind)).to(dev).flatten()
        view = flat[1:].view(3, 65, 64)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        y = ops.frame_cosine(text.to(dev), view)
        assert _abs_err(y, O.frame_cosine64(text, video), f"frame_cosine {kind} unaligned view") < COSINE_BOUND


def test_frame_cosine_zero_frame_zero_text_and_nan_feature(dev):
    """0 / 0 as the reference's divisions give it: a zero frame is NaN alone, a zero text makes its video's row NaN, a NaN feature its frame alone."""
    for kind in _kinds():
        for d in (33, 768):
            text, video = (t.clone() for t in clip_like(3, 65, d, kind))
            video[0, 5] = 0
            text[1] = 0
            video[2, 7, 3] = float("nan")
            ref = O.frame_cosine64(text, video)
            want = torch.zeros(3, 65, dtype=torch.bool)
            want[0, 5] = want[2, 7] = True
            want[1] = True
            assert torch.equal(torch.isnan(ref), want)
            y = _cosine(dev, text, video, kind).cpu()
            assert torch.equal(torch.isnan(y), want), (kind, d)
            assert _abs_err(y[~want], ref[~want], f"frame_cosine {kind} d{d} next to NaN rows") < COSINE_BOUND


def test_frame_cosine_refuses_a_text_row_wider_than_it_stages(dev):
    from revisionllm_amd import hip, ops
    with pytest.raises(hip.HipLibraryError, match="d=8193 exceeds the 8192 columns of the staged text row"):
        ops.frame_cosine(torch.ones(1, 8193, device=dev), torch.ones(1, 2, 8193, device=dev))
    text, video = clip_like(1, 3, 8192, "f32")
    assert _abs_err(_cosine(dev, text, video, "f32"), O.frame_cosine64(text, video), "frame_cosine f32 d8192 L3 B1") < COSINE_BOUND


# ------------------------------------------------------------------ rv_span_scores ------------------------------------------------------------------
def _scores(dev, sims, spans, mask, **kw):
    from revisionllm_amd import ops
    s, w = ops.span_scores(sims.to(dev), spans.to(dev), mask.to(dev), return_windows=True, **kw)
    assert s.dtype == torch.float32 and w.dtype == torch.int32 and s.device == dev and w.device == dev
    return s.cpu(), w.cpu().long()


def _span_ok(y, ref, kw, label):
    """A span result against the oracle where the oracle is a number, by the mode's bound; the NaN pattern exactly."""
    assert torch.equal(torch.isnan(y), torch.isnan(ref)), (label, kw)
    ok = ~torch.isnan(ref)
    if kw.get("pooling", "topk") == "topk":
        assert _abs_err(y[ok], ref[ok], f"span_scores topk {label} k{kw['k']}") < COSINE_BOUND * max(1.0, kw["k"] / 3.0), (label, kw)
    else:
        tau = kw["temperature"]
        assert _rel(y[ok], ref[ok], f"span_scores attention {label} tau{tau}") < softmax_bound("span_attention", tau), (label, kw)


def _span_ref(sims, win, kw):
    return O.span_scores64(sims, win, kw.get("pooling", "topk"), k=kw.get("k", 3), temperature=kw.get("temperature", 0.01))


@pytest.fixture(scope="module")
def g17(golden):
    return {k: torch.from_numpy(v) for k, v in golden.npz("g17_similarity").items()}


def test_forward_clip_matching_gives_the_references_g17_scores(dev, g17):
    """The two G17 calls end to end from f32 device tensors, against the reference's own outputs: scores within COSINE_BOUND, windows, zeros and the NaN
    pattern of the zeroed frame exactly; then from host tensors (staged up, the result back on the host) and through _get_predicted_proposal_feat."""
    from revisionllm_amd.eval.similarity import _get_predicted_proposal_feat, forward_clip_matching
    text, video, mask, spans = g17["text"], g17["video"], g17["mask"], g17["spans"]
    vz = video.clone()
    vz[0, 3] = 0
    for v, key in ((video, "scores"), (vz, "scores_zero_frame")):
        ref = g17[key].double()
        y, win = forward_clip_matching(text.to(dev), v.to(dev), mask.to(dev), spans.to(dev), return_windows=True)
        assert y.device == dev and y.dtype == torch.float32 and win.dtype == torch.int32
        assert torch.equal(win.cpu(), g17["windows"])
        y = y.cpu()
        assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.equal(y == 0, ref == 0)
        ok = ~torch.isnan(ref)
        assert _abs_err(y[ok], ref[ok], f"forward_clip_matching G17 {key}") < COSINE_BOUND
        yh = forward_clip_matching(text, v, mask, spans)
        assert not yh.is_cuda and yh.dtype == torch.float32 and torch.equal(torch.nan_to_num(yh, nan=-7.0), torch.nan_to_num(y, nan=-7.0))
        yp = _get_predicted_proposal_feat(v.to(dev), mask.to(dev).bool(), spans.to(dev).to(torch.float64), _unit(text).to(dev))
        assert torch.equal(torch.isnan(yp.cpu()), torch.isnan(ref)) and _abs_err(yp.cpu()[ok], ref[ok], f"_get_predicted_proposal_feat G17 {key}") < COSINE_BOUND


def test_forward_clip_matching_on_16_bit_features_and_spans(dev, g17):
    """Operand-typed features, spans and an integer mask (cast to f32 on the way in), against the oracle on the rounded values; the result comes back in
    the features' type."""
    from revisionllm_amd.eval.similarity import forward_clip_matching
    text, mask = g17["text"], g17["mask"]
    video, spans = _rt(g17["video"], fl()), _rt(g17["spans"], fl())
    ref, rwin = O.forward_clip_matching64(text, video, mask, spans)
    y, win = forward_clip_matching(text.to(dev), video.to(_dt(fl())).to(dev), mask.to(dev).to(torch.int64), spans.to(_dt(fl())).to(dev), return_windows=True)
    assert y.dtype == _dt(fl()) and y.device == dev and torch.equal(win.cpu().long(), rwin)
    # the f32 score is held to COSINE_BOUND and is then rounded to the features' type: at most half a unit in the last place (p = 11 / 8 significand bits) of the
    # binade the score lies in, element by element - whatever the size of the score
    p = 11 if fl() == "f16" else 8
    half_ulp = torch.pow(2.0, torch.floor(torch.log2(ref.abs() + COSINE_BOUND)) - p)
    err = (y.cpu().double() - ref).abs()
    _note(f"forward_clip_matching {fl()} features: worst (error - half ulp of the result type)", float((err - half_ulp).max()))
    assert bool((err <= COSINE_BOUND + half_ulp).all()), (err - half_ulp).max()


@pytest.mark.parametrize("k", [1, 3, 64])
def test_span_scores_topk_window_lengths_and_ties(dev, k):
    """Windows of 0, 1, 2, 3, 4, 65 and L frames in videos of two durations, k below, at and above the window length; then with exact ties on the first and
    the second place.  Windows exactly, scores within COSINE_BOUND (times k / 3 above 3)."""
    bound = COSINE_BOUND * max(1.0, k / 3.0)
    for name, (sims, mask, spans, win) in (("plain", span_inputs()), ("ties", span_tie_inputs())):
        y, w = _scores(dev, sims, spans, mask, k=k)
        assert torch.equal(w, win)
        ref = O.span_scores64(sims, win, "topk", k=k)
        assert torch.equal(y == 0, ref == 0)
        assert _abs_err(y, ref, f"span_scores topk {name} k{k}") < bound


@pytest.mark.parametrize("tau", TAUS_SPAN)
def test_span_scores_attention_mode(dev, tau):
    for name, (sims, mask, spans, win) in (("plain", span_inputs()), ("ties", span_tie_inputs()), ("L20000", long_row_inputs())):
        y, w = _scores(dev, sims, spans, mask, pooling="attention", temperature=tau)
        assert torch.equal(w, win)
        ref = O.span_scores64(sims, win, "attention", temperature=tau)
        assert torch.equal(y == 0, ref == 0)
        _note(f"span_scores attention tau{tau} asserted bound", softmax_bound("span_attention", tau))
        assert _rel(y, ref, f"span_scores attention {name} tau{tau}") < softmax_bound("span_attention", tau)


def test_span_scores_on_a_row_longer_than_any_lds(dev):
    sims, mask, spans, win = long_row_inputs()
    for k in (3, 64):
        y, w = _scores(dev, sims, spans, mask, k=k)
        assert torch.equal(w, win)
        assert _abs_err(y, O.span_scores64(sims, win, "topk", k=k), f"span_scores topk L20000 k{k}") < COSINE_BOUND * max(1.0, k / 3.0)


def test_span_scores_read_nothing_outside_their_window(dev):
    """sims is a view in the middle of a NaN-filled buffer and every window is fenced by NaN inside its row as well (the elements lo - 1 and hi); windows touch
    both ends of both rows.  A read one element outside a window turns its score NaN."""
    from revisionllm_amd import ops
    sims, mask, spans, win = fence_inputs()
    L, pad = FENCE_L, 37
    buf = torch.full((2 * pad + 2 * L,), float("nan"), device=dev)
    buf[pad:pad + 2 * L] = sims.flatten().to(dev)
    view = buf[pad:pad + 2 * L].view(2, L)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * pad
    for kw in (dict(k=1), dict(k=3), dict(k=64), dict(pooling="attention", temperature=0.01), dict(pooling="attention", temperature=1.0)):
        y, w = ops.span_scores(view, spans.to(dev), mask.to(dev), return_windows=True, **kw)
        assert torch.equal(w.cpu().long(), win)
        assert not torch.isnan(y).any(), (kw, y)
        _span_ok(y.cpu(), _span_ref(sims, win, kw), kw, "fenced")


def test_span_scores_nan_inside_a_window_and_non_finite_spans(dev):
    """A NaN similarity inside a window gives NaN in both modes (k = 1 too: NaN ranks first) and leaves the other windows alone; a span whose scaled bounds
    are not finite gives NaN and the window (-1, -1); finite bounds outside int32 saturate (build-defined)."""
    sims, mask, spans, win = span_inputs()
    sims = sims.clone()
    sims[:, 95] = float("nan")                                    # inside (0, 200), (70, 135) and (90, 97) only
    hit = (win[..., 0] <= 95) & (win[..., 1] > 95)
    assert int(hit[0].sum()) == 3
    for kw in (dict(k=1), dict(k=3), dict(pooling="attention", temperature=0.01), dict(pooling="attention", temperature=1.0)):
        y, _ = _scores(dev, sims, spans, mask, **kw)
        ref = _span_ref(sims, win, kw)
        assert torch.equal(torch.isnan(ref), hit), kw
        _span_ok(y, ref, kw, "next to NaN windows")
    sims, mask = span_inputs()[:2]
    odd = torch.tensor([[float("nan"), 0.1], [0.5, float("inf")], [float("-inf"), 0.1], [3e9, 0.0], [-3e9, 0.0], [0.0, 1e30], [0.5, 1.0]])[None].repeat(2, 1, 1)
    win = O.windows(odd, mask)
    assert win[0].tolist() == [[-1, -1], [-1, -1], [-1, -1], [200, 200], [0, 0], [0, 200], [0, 200]]
    for kw in (dict(k=3), dict(pooling="attention", temperature=1.0)):
        y, w = _scores(dev, sims, odd, mask, **kw)
        assert torch.equal(w, win)
        assert torch.isnan(y[:, :3]).all() and bool((y[:, 3:5] == 0).all())
        _span_ok(y, _span_ref(sims, win, kw), kw, "odd spans")


def test_span_scores_refusals(dev):
    from revisionllm_amd import hip, ops
    sims, mask, spans, _ = span_inputs()
    s, m, p = sims.to(dev), mask.to(dev), spans.to(dev)
    for k in (0, 65):
        with pytest.raises(hip.HipLibraryError, match=r"k=%d must be in \[1, 64\]" % k):
            ops.span_scores(s, p, m, k=k)
    for tau in (0.0, float("inf"), float("nan")):
        with pytest.raises(hip.HipLibraryError, match="temperature must be finite and not 0"):
            ops.span_scores(s, p, m, pooling="attention", temperature=tau)
    with pytest.raises(ValueError):
        ops.span_scores(s, p, m, pooling="mean")
    with pytest.raises(ValueError):
        ops.span_scores(s, p[:1], m)
    with pytest.raises(ValueError):
        ops.span_scores(s.half(), p, m)


# ------------------------------------------------------------------ rv_attn_pool ------------------------------------------------------------------
def _pool(dev, text, video, tau, kind):
    from revisionllm_amd import ops
    y = ops.attn_pool(text.to(dev), video.to(_dt(kind)).to(dev), tau)
    assert y.dtype == torch.float32 and y.device == dev and y.shape == (video.shape[0], text.shape[0], video.shape[2])
    return y.cpu()


@pytest.mark.parametrize("T", POOL_T)
def test_attn_pool_geometries_and_temperatures(dev, T):
    """One frame, frame counts around the 64 lanes and the 256 threads of the softmax, a width that is no multiple of the block, one and three texts, sharp
    (0.01), CLIP's (0.07), flat (1) and negative temperatures."""
    for kind in _kinds():
        for d in POOL_D:
            for Nt in POOL_NT:
                text, video = pool_inputs(POOL_NV, T, d, Nt, kind)
                for tau in TAUS_POOL:
                    e = _rel(_pool(dev, text, video, tau, kind), O.attn_pool64(text, video, tau), f"attn_pool {kind} T{T} d{d} Nt{Nt} tau{tau}")
                    assert e < softmax_bound("attn_pool", tau), (kind, T, d, Nt, tau, e)
    for tau in TAUS_POOL:
        _note(f"attn_pool tau{tau} asserted bound", softmax_bound("attn_pool", tau))


def test_attn_pool_nan_frame_in_one_video_of_three(dev):
    for kind in _kinds():
        text, video = pool_inputs(POOL_NV, 65, 768, 3, kind)
        video = video.clone()
        video[1, 40, 5] = float("nan")
        for tau in (0.01, 1.0):
            ref = O.attn_pool64(text, video, tau)
            assert torch.isnan(ref[1]).all() and not torch.isnan(ref[[0, 2]]).any()
            y = _pool(dev, text, video, tau, kind)
            assert torch.equal(torch.isnan(y), torch.isnan(ref)), (kind, tau)
            assert _rel(y[[0, 2]], ref[[0, 2]], f"attn_pool {kind} tau{tau} next to a NaN video") < softmax_bound("attn_pool", tau)


def test_attn_pool_refusals_and_the_last_accepted_length(dev):
    from revisionllm_amd import hip, ops
    text, video = pool_inputs(1, POOL_LAST_T, POOL_LAST_D, 1, fl())
    assert (POOL_LAST_D + POOL_LAST_T) * 4 + 256 == LDS_BYTES
    e = _rel(_pool(dev, text, video, 1.0, fl()), O.attn_pool64(text, video, 1.0), f"attn_pool {fl()} T{POOL_LAST_T} d{POOL_LAST_D} tau1.0")
    assert e < softmax_bound("attn_pool", 1.0)
    big = torch.zeros(1, POOL_LAST_T + 1, POOL_LAST_D, dtype=_dt(fl()), device=dev)
    with pytest.raises(hip.HipLibraryError, match=r"rv_attn_pool: d \+ T too large for LDS"):
        ops.attn_pool(text.to(dev), big, 1.0)
    for tau in (0.0, float("inf"), float("nan")):
        with pytest.raises(hip.HipLibraryError, match="rv_attn_pool: temperature must be finite and not 0"):
            ops.attn_pool(text.to(dev), big[:, :4], tau)
    with pytest.raises(ValueError):
        ops.attn_pool(text.to(dev)[0], big[:, :4], 1.0)


def test_attention_pooling_contract(dev, g17):
    """The drop-in function on G17's inputs against the reference's outputs (f32), from device and from host tensors, and the type it gives back."""
    from revisionllm_amd.eval.similarity import _attention_pooling
    text, video = g17["text"], g17["video"]
    for key, tau in (("attn_pool_t001", 0.01), ("attn_pool_t1", 1.0)):
        ref = g17[key].double()
        y = _attention_pooling(text.to(dev), video.to(dev), tau)
        assert y.device == dev and y.dtype == torch.float32
        # G17's features are not unit-norm (similarities of +-10): the f32 reference's own distance from float64 bounds what a comparison to it can show
        own = rel_err(ref, O.attn_pool64(text, video, tau))
        assert _rel(y, ref, f"_attention_pooling G17 tau{tau}") < max(2e-5, 4 * own)
        yh = _attention_pooling(text, video, tau)
        assert not yh.is_cuda and torch.equal(yh, y.cpu())
    y16 = _attention_pooling(text.to(dev), video.to(_dt(fl())).to(dev), 1.0)
    assert y16.dtype == _dt(fl()) and y16.device == dev


# ------------------------------------------------------------------ both ------------------------------------------------------------------
def test_two_calls_give_equal_bits(dev):
    from revisionllm_amd import ops
    text, video = clip_like(3, 257, 768, fl())
    t, v = text.to(dev), video.to(_dt(fl())).to(dev)
    a, b = ops.frame_cosine(t, v), ops.frame_cosine(t, v)
    assert torch.equal(a, b)
    sims, mask, spans, _ = span_tie_inputs()
    for kw in (dict(k=3), dict(k=64), dict(pooling="attention", temperature=0.01)):
        assert torch.equal(ops.span_scores(sims.to(dev), spans.to(dev), mask.to(dev), **kw), ops.span_scores(sims.to(dev), spans.to(dev), mask.to(dev), **kw))
    text, video = pool_inputs(POOL_NV, 300, 768, 3, fl())
    t, v = text.to(dev), video.to(_dt(fl())).to(dev)
    assert torch.equal(ops.attn_pool(t, v, 0.01), ops.attn_pool(t, v, 0.01))


def test_forward_clip_matching_does_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the call: with the stream kept busy by work queued before it, an event recorded just before the call
    has not completed when the call returns (a call that waited for its own kernels would have waited for that work first)."""
    from revisionllm_amd.eval.similarity import forward_clip_matching
    text, video = clip_like(3, 257, 768, fl())
    sims, mask, spans, _ = span_inputs()
    t, v = text.to(dev), video.to(_dt(fl())).to(dev)
    m, p = torch.ones(3, 257, device=dev), spans[:1].repeat(3, 1, 1).to(dev)
    want = forward_clip_matching(t, v, m, p, return_windows=True)                 # (warm: libraries loaded, allocator blocks cached)
    a = torch.ones(8192, 8192, device=dev)
    c = torch.empty_like(a)
    torch.mm(a, a, out=c)
    torch.cuda.synchronize()
    for _ in range(12):                                                            # ~1.1 TFLOP of f32 each: tens of milliseconds of queued work
        torch.mm(a, a, out=c)
    ev = torch.cuda.Event()
    ev.record()
    got = forward_clip_matching(t, v, m, p, return_windows=True)
    still_busy = not ev.query()
    torch.cuda.synchronize()
    assert still_busy, "forward_clip_matching returned only after the work queued before it had finished: it synchronised"
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
