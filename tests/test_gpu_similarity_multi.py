"""rv_frame_cosine_multi and rv_span_scores_multi (the kernels behind ``eval.similarity.forward_clip_matching_multi``: Q texts per video, the features read
once) against the float64 restatements of tests/similarity_multi_oracle.py, computed on the CPU from the inputs after rounding to the type the kernel reads;
f32 features and the 16-bit operands of both builds.  tests/test_similarity_multi_host_logic.py holds that oracle to fixture G17 and to the single-text one.

Bounds (the project's own, as tests/test_gpu_similarity.py states them).  Cosine rows and top-k scores: COSINE_BOUND = 1e-4 absolute, times k / 3 for k > 3.
The attention mode of the span kernel: 4 x the distance from float64 of the formula evaluated by torch in f32 on the CPU, the worst over THIS module's span
inputs per temperature (REF_F32_ERR below; ``reference_f32_errors`` re-measures it; never measured from the kernel).

Shapes: the kernel's tile is 128 frames per block (two MFMA tiles of 16 per wave) by 16 queries per MFMA tile, up to 8 tiles (128 queries) per pass over the
features, 4 k per MFMA with a 16-byte-load path (d a multiple of 8 / 4 elements; steps in groups of four, then one by one) and an element-wise one; the cases
sit on those edges."""
import ctypes
import functools
import os

import pytest
import torch

import similarity_multi_oracle as M
import similarity_oracle as O
from helpers import feats, fl, rel_err

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")
COSINE_BOUND = 1e-4
TAUS_SPAN = (0.01, 1.0)
# max-norm relative distance from float64 of torch's f32 CPU evaluation of sum softmax(s / temperature) s over the windows of this module's span cases
# (span_multi_inputs, its tie and NaN variants), measured with reference_f32_errors() on the CPU
REF_F32_ERR = {0.01: 1.62e-7, 1.0: 1.38e-7}
SOFTMAX_MARGIN = 4.0


def softmax_bound(tau):
    return SOFTMAX_MARGIN * REF_F32_ERR[tau]


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
    """A line that names the case in the RV_LOG_ERR file (profiles/similarity_multi_err_<flavour>.log)."""
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            fh.write(f"  similarity_multi {fl()} {label} {value:.3e}\n")
    return value


def _abs_err(y, ref, label):
    return _note(label + " abs", float((y.cpu().double() - ref).abs().max()))


def _rel(y, ref, label):
    return _note(label + " rel", rel_err(y.cpu(), ref))


def _dt(kind):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[kind]


def _rt(x, kind):
    """x (f32) rounded to what the kernel reads: "f16" / "bf16" -> through that type, "f32" -> unchanged."""
    return x if kind == "f32" else x.to(_dt(kind)).float()


def _kinds():
    return (fl(), "f32")


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


# ------------------------------------------------------------------ inputs ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def multi_like(B, Q, L, d, kind, tag=""):
    """Unit-norm frames that share a component along their video's theme, as CLIP features do, with another weight per video (a wrong block offset shows),
    and Q unit-norm texts per video around that theme, all different (a wrong column offset shows)
    -> (text f32 [B,Q,d], video as f32 holding ``kind``-representable values [B,L,d], float64 reference [B,Q,L])."""
    theme = _unit(feats(f"simm.t.{B}.{d}{tag}", (B, d)))
    text = _unit(theme[:, None, :] + 0.5 * _unit(feats(f"simm.q.{B}.{Q}.{d}{tag}", (B, Q, d))))
    g = _unit(feats(f"simm.v.{B}.{L}.{d}{tag}", (B, L, d)))
    video = _rt(_unit(g + theme[:, None, :] * (0.25 + 0.1 * torch.arange(B, dtype=torch.float32))[:, None, None]), kind)
    return text, video, M.frame_cosine_multi64(text, video)


@functools.lru_cache(maxsize=None)
def long_inputs(kind):
    """L = 20000, Q = 5, d = 768 (seeded torch generator: 15 M features)."""
    g = torch.Generator().manual_seed(20000)
    theme = _unit(torch.randn(1, 768, generator=g))
    text = _unit(theme[:, None, :] + 0.5 * _unit(torch.randn(1, 5, 768, generator=g)))
    video = _rt(_unit(_unit(torch.randn(1, 20000, 768, generator=g)) + 0.3 * theme[:, None, :]), kind)
    return text, video, M.frame_cosine_multi64(text, video)


def _cosine(dev, text, video, kind):
    from revisionllm_amd import ops
    y = ops.frame_cosine_multi(text.to(dev), video.to(_dt(kind)).to(dev))
    assert y.shape == (video.shape[0], text.shape[1], video.shape[1]) and y.dtype == torch.float32 and y.device == dev
    return y


def _check_rows(dev, Q, L, d, what):
    for kind in _kinds():
        text, video, ref = multi_like(3, Q, L, d, kind)
        for B in (1, 3):
            y = _cosine(dev, text[:B], video[:B], kind)
            assert _abs_err(y, ref[:B], f"frame_cosine_multi {what} {kind} d{d} L{L} Q{Q} B{B}") < COSINE_BOUND, (kind, d, L, Q, B)


# ------------------------------------------------------------------ rv_frame_cosine_multi ------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200])
def test_cosine_rows_across_frame_tile_edges(dev, L):
    """Frame counts around an MFMA tile's 16 frames, a wave's 32 and a block's 128, on the 16-byte-load path (d = 768) and the element-wise one (d = 33), two
    column tiles."""
    for d in (768, 33):
        _check_rows(dev, 17, L, d, "frame edge")


@pytest.mark.parametrize("Q", [1, 2, 15, 16, 17, 33, 64, 65, 129])
def test_cosine_rows_across_column_tile_edges(dev, Q):
    """Query counts around the 16 columns of a tile, the 1 / 2 / 4 / 8 tiles a pass holds, and (129) the 128 queries after which a second pass begins."""
    for d in (768, 33):
        _check_rows(dev, Q, 65, d, "column edge")


@pytest.mark.parametrize("d", [4, 8, 33, 766, 768, 1000, 1024])
def test_cosine_rows_across_widths(dev, d):
    """k-padding (33, 766: d % 4 != 0), the element-wise path (4 for 16-bit features, 33, 766: whole groups of four steps, single steps and a partial one), the
    16-byte path with nothing but a partial step (4 and 8) and with whole groups (768, 1024); 1000 (f32: 62 steps and a half) has groups, single steps and a partial one."""
    _check_rows(dev, 17, 65, d, "width")


def test_cosine_rows_of_a_long_video(dev):
    for kind in _kinds():
        text, video, ref = long_inputs(kind)
        assert _abs_err(_cosine(dev, text, video, kind), ref, f"frame_cosine_multi {kind} d768 L20000 Q5 B1") < COSINE_BOUND


def test_cosine_rows_of_a_feature_view_that_is_not_16_byte_aligned(dev):
    """The same values at an address 16-byte loads cannot take: the entry point switches to the element-wise path; the rows stay within the bound."""
    from revisionllm_amd import ops
    for kind in _kinds():
        text, video, ref = multi_like(3, 17, 65, 768, kind)
        flat = torch.zeros(video.numel() + 1, dtype=_dt(kind), device=dev)
        flat[1:] = video.to(_dt(kind)).to(dev).flatten()
        view = flat[1:].view(3, 65, 768)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        assert _abs_err(ops.frame_cosine_multi(text.to(dev), view), ref, f"frame_cosine_multi {kind} unaligned view") < COSINE_BOUND


def test_cosine_rows_read_nothing_outside_the_video(dev):
    """The video is a window of a NaN-filled larger buffer (16-byte aligned, so d = 768 keeps its 16-byte loads): a read past the last row's d elements - a
    k-step that is not padded with zeros, a frame index that is not clamped into the video - turns stored entries NaN."""
    from revisionllm_amd import ops
    for kind in _kinds():
        for d in (768, 33, 766):
            text, video, ref = multi_like(3, 17, 65, d, kind)
            pad = 64
            buf = torch.full((2 * pad + video.numel(),), float("nan"), dtype=_dt(kind), device=dev)
            buf[pad:pad + video.numel()] = video.to(_dt(kind)).to(dev).flatten()
            view = buf[pad:pad + video.numel()].view(3, 65, d)
            assert view.is_contiguous() and view.data_ptr() % 16 == 0
            y = ops.frame_cosine_multi(text.to(dev), view)
            assert not torch.isnan(y).any(), (kind, d)
            assert _abs_err(y, ref, f"frame_cosine_multi {kind} d{d} fenced video") < COSINE_BOUND


def test_cosine_rows_write_nothing_outside_their_output(dev):
    """``out`` lies inside a NaN-filled buffer: the result is within the bound and every word around it keeps its bits."""
    from revisionllm_amd import hip
    for kind in _kinds():
        for d in (768, 33):
            B, Q, L = 3, 17, 65
            text, video, ref = multi_like(B, Q, L, d, kind)
            t, v = text.to(dev).contiguous(), video.to(_dt(kind)).to(dev).contiguous()
            unit = torch.empty_like(t)
            pad = 101
            buf = torch.full((2 * pad + B * Q * L,), float("nan"), device=dev)
            before = buf.clone().view(torch.int32)
            out = buf[pad:pad + B * Q * L]
            lib = hip.lib(None if kind == "f32" else v)
            hip.check(lib.rv_frame_cosine_multi(hip.ptr(v), hip.dtype_code(v), hip.ptr(t), B, Q, L, d, hip.ptr(unit), ctypes.c_void_p(out.data_ptr()), hip.stream()),
                      "rv_frame_cosine_multi")
            after = buf.view(torch.int32)
            assert torch.equal(after[:pad], before[:pad]) and torch.equal(after[pad + B * Q * L:], before[pad + B * Q * L:]), (kind, d)
            assert not torch.isnan(out).any()
            assert _abs_err(out.view(B, Q, L), ref, f"frame_cosine_multi {kind} d{d} fenced out") < COSINE_BOUND
            assert _abs_err(unit, _unit(text).double(), f"frame_cosine_multi {kind} d{d} unit texts") < 1e-6


def test_cosine_rows_zero_frame_zero_text_and_nan_feature(dev):
    """0 / 0 as the single-text kernel gives it: a zero frame is NaN in its column for every query, a zero text makes that query's row NaN and no other,
    a NaN feature makes its frame's column NaN alone."""
    for kind in _kinds():
        for d in (33, 768):
            text, video, _ = (t.clone() for t in multi_like(3, 33, 65, d, kind))
            video[0, 5] = 0
            text[1, 17] = 0
            video[2, 7, 3] = float("nan")
            ref = M.frame_cosine_multi64(text, video)
            want = torch.zeros(3, 33, 65, dtype=torch.bool)
            want[0, :, 5] = want[2, :, 7] = True
            want[1, 17] = True
            assert torch.equal(torch.isnan(ref), want)
            y = _cosine(dev, text, video, kind).cpu()
            assert torch.equal(torch.isnan(y), want), (kind, d)
            assert _abs_err(y[~want], ref[~want], f"frame_cosine_multi {kind} d{d} next to NaN rows and columns") < COSINE_BOUND


def test_a_querys_row_does_not_depend_on_q_slot_neighbours_or_batch(dev):
    """Bit for bit: a query alone (Q = 1) gives the row it has among 130, on both sides of a 16-column edge and of the 128-query pass edge; the same text in
    two slots gives equal rows; video 0 of three equals the same video alone; two runs agree."""
    from revisionllm_amd import ops
    for kind in _kinds():
        for d in (768, 33):
            text, video, _ = multi_like(3, 130, 65, d, kind)
            text = text.clone()
            text[:, 20] = text[:, 3]
            text[:, 129] = text[:, 3]
            t, v = text.to(dev), video.to(_dt(kind)).to(dev)
            full = ops.frame_cosine_multi(t, v)
            assert torch.equal(full, ops.frame_cosine_multi(t, v))
            for q in (0, 15, 16, 17, 31, 32, 127, 128, 129):
                assert torch.equal(full[:, q], ops.frame_cosine_multi(t[:, q:q + 1], v)[:, 0]), (kind, d, q)
            assert torch.equal(full[:, 3], full[:, 20]) and torch.equal(full[:, 3], full[:, 129]), (kind, d)
            assert torch.equal(full[:, :33], ops.frame_cosine_multi(t[:, :33], v)) and torch.equal(full[:, 5:70], ops.frame_cosine_multi(t[:, 5:70], v))
            assert torch.equal(full[:1], ops.frame_cosine_multi(t[:1], v[:1])), (kind, d)


def test_cosine_rows_against_the_single_text_kernel(dev):
    """Two kernels, each held to COSINE_BOUND against float64: within twice the bound of each other (their summation orders differ: no bit equality)."""
    from revisionllm_amd import ops
    for kind in _kinds():
        for d in (768, 33):
            text, video, _ = multi_like(3, 17, 200, d, kind)
            t, v = text.to(dev), video.to(_dt(kind)).to(dev)
            y = ops.frame_cosine_multi(t, v)
            for q in (0, 15, 16):
                one = ops.frame_cosine(t[:, q].contiguous(), v)
                assert _abs_err(y[:, q], one.cpu().double(), f"frame_cosine_multi {kind} d{d} q{q} vs rv_frame_cosine") < 2 * COSINE_BOUND


def test_cosine_refusals(dev):
    from revisionllm_amd import hip, ops
    with pytest.raises(hip.HipLibraryError, match=r"at most 65535 \(video, query\) rows per launch \(B=1, Q=65536\)"):
        ops.frame_cosine_multi(torch.ones(1, 65536, 4, device=dev), torch.ones(1, 2, 4, device=dev))
    with pytest.raises(hip.HipLibraryError, match="rv_frame_cosine_multi: dtype must be f32 or"):
        other = torch.bfloat16 if fl() == "f16" else torch.float16
        v = torch.ones(1, 2, 8, device=dev, dtype=other)
        hip.check(hip.lib().rv_frame_cosine_multi(hip.ptr(v), hip.dtype_code(v), hip.ptr(v), 1, 1, 2, 8, hip.ptr(v), hip.ptr(v), hip.stream()), "rv_frame_cosine_multi")
    with pytest.raises(ValueError):
        ops.frame_cosine_multi(torch.ones(2, 8, device=dev), torch.ones(2, 3, 8, device=dev))
    with pytest.raises(ValueError):
        ops.frame_cosine_multi(torch.ones(1, 2, 8, device=dev), torch.ones(2, 3, 8, device=dev))
    # the widest d the single-text kernel takes, and one more (no staged text row here: no limit on d)
    for d in (8192, 8193):
        text, video, ref = multi_like(1, 2, 3, d, "f32")
        assert _abs_err(_cosine(dev, text, video, "f32"), ref, f"frame_cosine_multi f32 d{d} L3 Q2 B1") < COSINE_BOUND


# ------------------------------------------------------------------ rv_span_scores_multi ------------------------------------------------------------------
SPAN_L, SPAN_DUR, SPAN_Q = 200, (200, 130), 3
SPAN_WINDOWS = [(0, 200), (7, 8), (30, 32), (50, 53), (60, 64), (70, 135), (0, 1), (199, 200), (100, 100), (3, 68), (140, 143), (90, 97)]


@functools.lru_cache(maxsize=None)
def span_multi_inputs():
    """The window set of test_gpu_similarity.span_inputs (windows of 0, 1, 2, 3, 4, 65 and L frames in videos of duration 200 and 130), for Q = 3 queries
    per video: every query has a similarity row of its own and the windows in another order (rotated by 4 q), so a (b, q) row taken with another row's
    spans, similarities or duration gives other windows or scores.  -> sims [2,3,200], mask [2,200], spans [2,3,12,2], win [2,3,12,2]."""
    sims = 0.3 + 0.05 * feats("simm.span.sims", (2, SPAN_Q, SPAN_L))
    mask = torch.zeros(2, SPAN_L)
    spans = torch.zeros(2, SPAN_Q, len(SPAN_WINDOWS), 2)
    for b, D in enumerate(SPAN_DUR):
        mask[b, :D] = 1
        for q in range(SPAN_Q):
            for n, (lo, hi) in enumerate(SPAN_WINDOWS[4 * q:] + SPAN_WINDOWS[:4 * q]):
                if hi == lo:
                    spans[b, q, n] = torch.tensor([0.5, 0.0])
                elif (lo, hi) == (0, SPAN_L):
                    spans[b, q, n] = torch.tensor([0.5, 1.0]) if D == SPAN_L else torch.tensor([0.5 * SPAN_L / D, SPAN_L / D])
                else:
                    x1, x2 = (lo + 0.5) / D, (hi - 0.5) / D
                    spans[b, q, n] = torch.tensor([(x1 + x2) / 2, x2 - x1])
    win = M.windows_multi(spans, mask)
    for q in range(SPAN_Q):
        lens = set((win[:, q, :, 1] - win[:, q, :, 0]).clamp_min(0).flatten().tolist())
        assert {0, 1, 2, 3, 4, 65, SPAN_L} <= lens, lens
    assert not torch.equal(win[0], win[1]) and not torch.equal(win[:, 0], win[:, 1])
    return sims, mask, spans, win


def span_multi_tie_inputs():
    """span_multi_inputs with exact ties: in the window (70, 135) the largest value appears twice, in (3, 68) the second largest three times - in every row."""
    sims, mask, spans, win = span_multi_inputs()
    sims = sims.clone()
    for row in sims.view(-1, SPAN_L):
        row[80] = row[120] = float(row[70:135].max()) + 0.01
        second = float(torch.sort(row[3:68], descending=True).values[1])
        row[10] = row[40] = row[60] = second
    return sims, mask, spans, win


def span_attention_f32(sims, win, tau):
    return torch.stack([O.span_attention_f32(sims[:, q], win[:, q], tau) for q in range(sims.shape[1])], dim=1)


def reference_f32_errors():
    """The figures behind REF_F32_ERR: torch's f32 CPU evaluation of the attention-mode formula against float64 on this module's span inputs, per temperature."""
    worst = {t: 0.0 for t in TAUS_SPAN}
    for sims, mask, spans, win in (span_multi_inputs(), span_multi_tie_inputs()):
        for tau in TAUS_SPAN:
            worst[tau] = max(worst[tau], rel_err(span_attention_f32(sims, win, tau), M.span_scores_multi64(sims, win, "attention", temperature=tau)))
    return worst


def test_the_f32_reference_distances_the_softmax_bounds_come_from(dev):
    """Re-measures REF_F32_ERR on this machine's CPU and writes the figures into the error log next to the kernel's.  CPUs differ in how torch orders its
    f32 sums, so the figures need not repeat to the digit: each has to stay inside the bound that was derived from it."""
    for tau, e in reference_f32_errors().items():
        _note(f"reference f32 (CPU, torch) vs float64: span_attention tau{tau} rel", e)
        _note(f"... the constant the bound is 4 x of: span_attention tau{tau}", REF_F32_ERR[tau])
        _note(f"span_scores_multi attention tau{tau} asserted bound", softmax_bound(tau))
        assert 0 < e < softmax_bound(tau), (tau, e)


def _scores(dev, sims, spans, mask, **kw):
    from revisionllm_amd import ops
    s, w = ops.span_scores_multi(sims.to(dev), spans.to(dev), mask.to(dev), return_windows=True, **kw)
    assert s.dtype == torch.float32 and w.dtype == torch.int32 and s.device == dev and w.device == dev
    assert s.shape == spans.shape[:3] and w.shape == spans.shape
    return s, w


def _each_row_is_the_single_kernels(dev, sims, spans, mask, s, w, **kw):
    """The same kernel body: every (b, q) equals rv_span_scores on that query's row bit for bit (NaN patterns included)."""
    from revisionllm_amd import ops
    for q in range(sims.shape[1]):
        s1, w1 = ops.span_scores(sims[:, q].contiguous().to(dev), spans[:, q].contiguous().to(dev), mask.to(dev), return_windows=True, **kw)
        assert torch.equal(s[:, q].view(torch.int32), s1.view(torch.int32)) and torch.equal(w[:, q], w1), (q, kw)


def _span_ok(y, ref, kw, label):
    assert torch.equal(torch.isnan(y), torch.isnan(ref)), (label, kw)
    ok = ~torch.isnan(ref)
    if kw.get("pooling", "topk") == "topk":
        assert _abs_err(y[ok], ref[ok], f"span_scores_multi topk {label} k{kw['k']}") < COSINE_BOUND * max(1.0, kw["k"] / 3.0), (label, kw)
    else:
        tau = kw["temperature"]
        assert _rel(y[ok], ref[ok], f"span_scores_multi attention {label} tau{tau}") < softmax_bound(tau), (label, kw)


def _span_ref(sims, win, kw):
    return M.span_scores_multi64(sims, win, kw.get("pooling", "topk"), k=kw.get("k", 3), temperature=kw.get("temperature", 0.01))


SPAN_MODES = [dict(k=1), dict(k=3), dict(k=64), dict(pooling="attention", temperature=0.01), dict(pooling="attention", temperature=1.0)]


@pytest.mark.parametrize("kw", SPAN_MODES, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_span_scores_multi_window_lengths_ties_and_modes(dev, kw):
    """Q = 3 with each query's own spans, windows of 0, 1, 2, 3, 4, 65 and L frames in videos of two durations; then with exact ties.  Windows exactly (the
    duration is the VIDEO's: a mask row taken by (b, q) instead of b gives other windows), scores by the mode's bound, each row the single kernel's bits."""
    for name, (sims, mask, spans, win) in (("plain", span_multi_inputs()), ("ties", span_multi_tie_inputs())):
        s, w = _scores(dev, sims, spans, mask, **kw)
        assert torch.equal(w.cpu().long(), win), name
        ref = _span_ref(sims, win, kw)
        assert torch.equal(s.cpu() == 0, ref == 0)
        _span_ok(s.cpu(), ref, kw, name)
        _each_row_is_the_single_kernels(dev, sims, spans, mask, s, w, **kw)


def test_span_scores_multi_nan_in_one_querys_window_and_non_finite_spans(dev):
    """A NaN similarity in query 1's row gives NaN for the windows of query 1 that hold it, in both modes, and for no other query; spans whose scaled bounds
    are not finite (query 2 only) give NaN and the window (-1, -1); finite bounds outside int32 saturate."""
    sims, mask, spans, win = span_multi_inputs()
    sims = sims.clone()
    sims[:, 1, 95] = float("nan")                                 # inside (0, 200), (70, 135) and (90, 97) of query 1 only
    hit = torch.zeros(win.shape[:3], dtype=torch.bool)
    hit[:, 1] = (win[:, 1, :, 0] <= 95) & (win[:, 1, :, 1] > 95)
    assert int(hit[0].sum()) == 3
    for kw in (dict(k=1), dict(k=3), dict(pooling="attention", temperature=0.01), dict(pooling="attention", temperature=1.0)):
        s, w = _scores(dev, sims, spans, mask, **kw)
        ref = _span_ref(sims, win, kw)
        assert torch.equal(torch.isnan(ref), hit), kw
        _span_ok(s.cpu(), ref, kw, "next to NaN windows")
        _each_row_is_the_single_kernels(dev, sims, spans, mask, s, w, **kw)
    sims, mask, spans, _ = span_multi_inputs()
    odd = torch.tensor([[float("nan"), 0.1], [0.5, float("inf")], [float("-inf"), 0.1], [3e9, 0.0], [-3e9, 0.0], [0.0, 1e30], [0.5, 1.0]])
    spans = spans[:, :, :7].clone()
    spans[:, 2] = odd
    win = M.windows_multi(spans, mask)
    assert win[0, 2].tolist() == [[-1, -1], [-1, -1], [-1, -1], [200, 200], [0, 0], [0, 200], [0, 200]] and int((win[:, :2] < 0).sum()) == 0
    for kw in (dict(k=3), dict(pooling="attention", temperature=1.0)):
        s, w = _scores(dev, sims, spans, mask, **kw)
        assert torch.equal(w.cpu().long(), win)
        s = s.cpu()
        assert torch.isnan(s[:, 2, :3]).all() and bool((s[:, 2, 3:5] == 0).all()) and not torch.isnan(s[:, :2]).any()
        _span_ok(s, _span_ref(sims, win, kw), kw, "odd spans")


def test_span_scores_multi_refusals(dev):
    from revisionllm_amd import hip, ops
    sims, mask, spans, _ = span_multi_inputs()
    s, m, p = sims.to(dev), mask.to(dev), spans.to(dev)
    for k in (0, 65):
        with pytest.raises(hip.HipLibraryError, match=r"rv_span_scores_multi: k=%d must be in \[1, 64\]" % k):
            ops.span_scores_multi(s, p, m, k=k)
    for tau in (0.0, float("inf"), float("nan")):
        with pytest.raises(hip.HipLibraryError, match="rv_span_scores_multi: temperature must be finite and not 0"):
            ops.span_scores_multi(s, p, m, pooling="attention", temperature=tau)
    with pytest.raises(hip.HipLibraryError, match=r"rv_span_scores_multi: at most 65535 \(video, query\) rows per launch \(B=1, Q=65536\)"):
        ops.span_scores_multi(torch.zeros(1, 65536, 2, device=dev), torch.zeros(1, 65536, 1, 2, device=dev), torch.ones(1, 2, device=dev))
    with pytest.raises(ValueError):
        ops.span_scores_multi(s, p, m, pooling="mean")
    with pytest.raises(ValueError):
        ops.span_scores_multi(s, p[:, :2], m)
    with pytest.raises(ValueError):
        ops.span_scores_multi(s, p, m[:1])
    with pytest.raises(ValueError):
        ops.span_scores_multi(s.half(), p, m)


# ------------------------------------------------------------------ end to end ------------------------------------------------------------------
@pytest.fixture(scope="module")
def g17(golden):
    return {k: torch.from_numpy(v) for k, v in golden.npz("g17_similarity").items()}


def _g17_multi(g17):
    """G17's three texts as Q = 3 against each of its videos; query q of video b scores the video's proposals reversed q times over (its own order)."""
    text = g17["text"][None].repeat(3, 1, 1).contiguous()
    spans = torch.stack([g17["spans"], g17["spans"].flip(1), g17["spans"]], dim=1).contiguous()
    return text, g17["video"], g17["mask"], spans


def test_forward_clip_matching_multi_gives_the_references_g17_scores(dev, g17):
    """[b, q = b] against the reference's own recorded outputs (queries 0 and 2 carry the proposals in G17's order): scores within COSINE_BOUND, windows,
    zeros and the NaN pattern of the zeroed frame exactly; every [b, q] against the oracle; then from host tensors (the result back on the host)."""
    from revisionllm_amd.eval.similarity import forward_clip_matching, forward_clip_matching_multi
    text, video, mask, spans = _g17_multi(g17)
    vz = video.clone()
    vz[0, 3] = 0
    for v, key in ((video, "scores"), (vz, "scores_zero_frame")):
        y, win = forward_clip_matching_multi(text.to(dev), v.to(dev), mask.to(dev), spans.to(dev), return_windows=True)
        assert y.device == dev and y.dtype == torch.float32 and win.dtype == torch.int32 and y.shape == (3, 3, 11) and win.shape == (3, 3, 11, 2)
        ref_all, win_all = M.forward_clip_matching_multi64(text, v, mask, spans)
        assert torch.equal(win.cpu().long(), win_all)
        y = y.cpu()
        rec = g17[key].double()
        for b in range(3):
            got = y[b, b].flip(0) if b == 1 else y[b, b]
            gwin = win[b, b].cpu().flip(0) if b == 1 else win[b, b].cpu()
            assert torch.equal(gwin, g17["windows"][b])
            assert torch.equal(torch.isnan(got), torch.isnan(rec[b])) and torch.equal(got == 0, rec[b] == 0)
            ok = ~torch.isnan(rec[b])
            assert _abs_err(got[ok], rec[b][ok], f"forward_clip_matching_multi G17 {key} video {b}") < COSINE_BOUND
        assert torch.equal(torch.isnan(y), torch.isnan(ref_all))
        ok = ~torch.isnan(ref_all)
        assert _abs_err(y[ok], ref_all[ok], f"forward_clip_matching_multi G17 {key} all pairs") < COSINE_BOUND
        for q in range(3):                                                   # the contract: each query is the single-text call within the cosine bound
            y1, w1 = forward_clip_matching(text[:, q].to(dev), v.to(dev), mask.to(dev), spans[:, q].to(dev), return_windows=True)
            assert torch.equal(w1, win[:, q])
            assert _abs_err(y[:, q][ok[:, q]], y1.cpu().double()[ok[:, q]], f"forward_clip_matching_multi G17 {key} q{q} vs forward_clip_matching") < 2 * COSINE_BOUND
        yh, wh = forward_clip_matching_multi(text, v, mask, spans, return_windows=True)
        assert not yh.is_cuda and not wh.is_cuda and yh.dtype == torch.float32
        assert torch.equal(torch.nan_to_num(yh, nan=-7.0), torch.nan_to_num(y, nan=-7.0)) and torch.equal(wh, win.cpu())
        # attention pooling at temperature 1: d score / d s_t = p_t (1 + (s_t - score) / tau) with |s_t - score| <= 2, so cosines within COSINE_BOUND move
        # the score by at most (1 + 2 / tau) times the bound
        ya = forward_clip_matching_multi(text.to(dev), v.to(dev), mask.to(dev), spans.to(dev), pooling="attention", temperature=1.0)
        ra, _ = M.forward_clip_matching_multi64(text, v, mask, spans, pooling="attention", temperature=1.0)
        assert torch.equal(torch.isnan(ya.cpu()), torch.isnan(ra))
        assert _abs_err(ya.cpu()[ok], ra[ok], f"forward_clip_matching_multi G17 {key} attention tau1") < 3 * COSINE_BOUND


def test_forward_clip_matching_multi_on_16_bit_features_and_spans(dev, g17):
    """Operand-typed features, spans and an integer mask (cast to f32 on the way in), against the oracle on the rounded values; the result comes back in
    the features' type."""
    from revisionllm_amd.eval.similarity import forward_clip_matching_multi
    text, video, mask, spans = _g17_multi(g17)
    video, spans = _rt(video, fl()), _rt(spans, fl())
    ref, rwin = M.forward_clip_matching_multi64(text, video, mask, spans)
    y, win = forward_clip_matching_multi(text.to(dev), video.to(_dt(fl())).to(dev), mask.to(dev).to(torch.int64), spans.to(_dt(fl())).to(dev), return_windows=True)
    assert y.dtype == _dt(fl()) and y.device == dev and torch.equal(win.cpu().long(), rwin)
    # the f32 score is held to COSINE_BOUND and is then rounded to the features' type: at most half a unit in the last place (p = 11 / 8 significand bits) of the
    # binade the score lies in, element by element
    p = 11 if fl() == "f16" else 8
    half_ulp = torch.pow(2.0, torch.floor(torch.log2(ref.abs() + COSINE_BOUND)) - p)
    err = (y.cpu().double() - ref).abs()
    _note(f"forward_clip_matching_multi {fl()} features: worst (error - half ulp of the result type)", float((err - half_ulp).max()))
    assert bool((err <= COSINE_BOUND + half_ulp).all()), (err - half_ulp).max()


def test_forward_clip_matching_multi_does_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the call: with the stream kept busy by work queued before it, an event recorded just before the call
    has not completed when the call returns (a call that waited for its own kernels would have waited for that work first)."""
    from revisionllm_amd.eval.similarity import forward_clip_matching_multi
    text, video, _ = multi_like(3, 17, 200, 768, fl())
    _, mask, spans, _ = span_multi_inputs()
    t, v = text.to(dev), video.to(_dt(fl())).to(dev)
    m, p = torch.ones(3, 200, device=dev), spans[:1, :1].repeat(3, 17, 1, 1).to(dev)
    want = forward_clip_matching_multi(t, v, m, p, return_windows=True)           # (warm: libraries loaded, allocator blocks cached)
    a = torch.ones(8192, 8192, device=dev)
    c = torch.empty_like(a)
    torch.mm(a, a, out=c)
    torch.cuda.synchronize()
    for _ in range(12):                                                            # ~1.1 TFLOP of f32 each: tens of milliseconds of queued work
        torch.mm(a, a, out=c)
    ev = torch.cuda.Event()
    ev.record()
    got = forward_clip_matching_multi(t, v, m, p, return_windows=True)
    still_busy = not ev.query()
    torch.cuda.synchronize()
    assert still_busy, "forward_clip_matching_multi returned only after the work queued before it had finished: it synchronised"
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
