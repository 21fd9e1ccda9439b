"""The rules the span stages share (csrc/grounding.h: span_mask_sum, SPAN_NOT_FINITE / span_slice, span_encode, with duration_frames) hold across the stages on a FRACTIONAL
mask, where the order of the duration sum shows in the duration's bits: the other GPU tests of these stages run on 0 / 1 masks, whose sum is exact in any
order, so they would not see one stage adding its mask row up in another order than the next.

Rows are [2, 2, L] with one mask row per video, L in {1, 63, 64, 65, 255, 256, 257, 1025} (around the wave, around the 256 threads that add the row up, and
more than one pass of them), N in {1, 4, 5} spans a row (a block takes 4: one, none and three idle waves).  Three statements, all at zero tolerance:
  1. ``span_scores_multi``, ``span_scores_masked`` and ``span_refine`` agree on every span's window.  ``span_refine`` runs on constant similarities: every
     contrast is 0, the tie goes to the original pair, so its window is the scores' window cut at the duration - unless that is the whole duration, which
     has no frame outside and is not admissible (then the oracle alone says where the span goes).
  2. ``span_scores(return_windows=True)`` on the spans ``span_propose``, ``span_refine`` and ``span_anchors`` hand back recovers their ``windows``.
  3. Each matches the numpy statement of the rule (tests/span_refine_oracle.py: ``window``, ``duration_frames``, ``encode``, ``refine_row``;
     tests/span_anchors_oracle.py: ``anchors_row``) for the duration ``span_mask_sum`` below
     gives - the kernels' order of the sum, stated in numpy.  ``span_propose`` is the one stage that adds its mask row up the other way (block_mask_sum:
     the wave sums from left to right - rv_span_propose's rule since it was written), so ITS encoding is held to ``left_to_right_sum``; its duration can
     differ from the score kernels' in the last bit, which the encoding's quarter-frame slack absorbs: statement 2 holds for it all the same."""
import numpy as np
import pytest
import torch

import span_anchors_oracle as AO
import span_refine_oracle as RO
from test_gpu_spans_masked import bits, dev, flav, up  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1025)
SPANS = (1, 4, 5)
SCALES = ((4, 1, 2), (16, 4, 8), (33, 5, 7))


def span_mask_sum(row):
    """The span kernels' duration (csrc/grounding.h): thread t of 256 adds the frames t, t + 256, .. in turn, each wave of 64 adds its threads' sums up in a
    butterfly (offsets 32, 16, .., 1), and the four wave sums are added pairwise; every add rounded to f32."""
    row = np.asarray(row, dtype=F)
    part = np.zeros(256, dtype=F)
    for l0 in range(0, len(row), 256):
        chunk = row[l0:l0 + 256]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    w = part.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ o]
    assert w.dtype == F and all((w[i] == w[i, 0]).all() for i in range(4))
    return F(F(w[0, 0] + w[1, 0]) + F(w[2, 0] + w[3, 0]))


def left_to_right_sum(row):
    """block_mask_sum<256>'s order of the same partial sums (csrc/grounding.h): the wave sums added from left to right.  span_propose_kernel's duration, not
    the other span kernels'."""
    row = np.asarray(row, dtype=F)
    part = np.zeros(256, dtype=F)
    for l0 in range(0, len(row), 256):
        chunk = row[l0:l0 + 256]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    w = part.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, np.arange(64) ^ o]
    return F(F(F(w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])


def case(L, N):
    """-> sims [2,2,L] (bumpy), flat [2,2,L] (constant), mask [2,L] (fractional, the second row's sum near 3/4 L and the first's near 1/2 L), spans [2,2,N,2]."""
    rng = np.random.default_rng(1000 * L + N)
    t = np.arange(L, dtype=np.float64)
    sims = (0.4 + 0.3 * np.sin(t[None, None, :] / rng.uniform(3, 9, (2, 2, 1)) + rng.uniform(0, 6, (2, 2, 1))) + 0.05 * rng.standard_normal((2, 2, L))).astype(F)
    flat = np.full((2, 2, L), 0.25, dtype=F)
    mask = (np.array([[0.05], [0.55]]) + rng.uniform(0, 0.9, (2, L)) * np.array([[1.0], [0.45]])).astype(F)
    spans = np.stack([rng.uniform(0.0, 1.0, (2, 2, N)), rng.uniform(0.0, 0.6, (2, 2, N))], -1).astype(F)
    spans[0, 0, 0] = (0.5, 4.0)                                   # the whole row
    spans[1, 1, -1] = (1.2, 0.1)                                  # past the duration
    return sims, flat, mask, spans


def windows_of(spans, dur, L):
    """RO.window for every span of a row -> i64 [N,2], (-1, -1) for a non-finite one."""
    out = []
    for c, w in spans:
        win = RO.window(c, w, RO.CXW, dur, L)
        out.append((-1, -1) if win is None else win)
    return np.array(out, dtype=np.int64)


def test_the_masks_tell_the_orders_of_the_sum_apart():
    """Some of the masks below sum to other bits in another order of the same adds: a stage that summed that way would hand on another duration."""
    told = [(L, N, b) for L in LENGTHS for N in SPANS for b in range(2) if bits(left_to_right_sum(case(L, N)[2][b])) != bits(span_mask_sum(case(L, N)[2][b]))]
    assert len(told) >= 3 and all(L >= 255 for L, _, _ in told), told


@pytest.mark.parametrize("N", SPANS)
@pytest.mark.parametrize("L", LENGTHS)
def test_the_span_stages_agree_on_a_fractional_mask(dev, L, N):
    from revisionllm_amd import ops
    sims, flat, mask, spans = case(L, N)
    durs = [span_mask_sum(mask[b]) for b in range(2)]
    s, c, m, p = up(dev, sims), up(dev, flat), up(dev, mask), up(dev, spans)
    what = f"L={L} N={N}"

    # the windows of the two score entries, against the rule
    scores, win = ops.span_scores_multi(s, p, m, return_windows=True)
    masked = ops.span_scores_masked(s, p, m, return_windows=True, return_usable=True)
    win = win.cpu().numpy()
    rule = np.stack([np.stack([windows_of(spans[b, q], durs[b], L) for q in range(2)]) for b in range(2)])
    assert np.array_equal(win, rule), (what, "span_scores_multi's windows against the rule")
    assert np.array_equal(masked.windows.cpu().numpy(), win), (what, "span_scores_masked's windows")
    assert np.array_equal(bits(masked.scores.cpu().numpy()), bits(scores.cpu().numpy())), (what, "span_scores_masked's scores")
    assert np.array_equal(masked.n_usable.cpu().numpy(), np.maximum(win[..., 1] - win[..., 0], 0)), (what, "usable counts")

    # span_refine on constant rows: the original pair stays; on the bumpy rows: the oracle; both: its spans give its windows back
    kw = dict(radius=3, margin=5, return_windows=True, return_contrast=True)
    for name, rows_np, rows_dev in (("constant", flat, c), ("bumpy", sims, s)):
        got = ops.span_refine(rows_dev, p, m, **kw)
        gw = got.windows.cpu().numpy()
        for b in range(2):
            D = RO.duration_frames(durs[b], L)
            for q in range(2):
                ref = RO.refine_row(rows_np[b, q], None, durs[b], L, spans[b, q], RO.CXW, 3, 5, 1)
                assert np.array_equal(gw[b, q], ref[1]), (what, name, b, q, "span_refine's windows against the oracle")
                assert np.array_equal(bits(got.spans[b, q].cpu().numpy()), bits(ref[0])), (what, name, b, q, "span_refine's spans")
                assert np.array_equal(bits(got.contrast[b, q].cpu().numpy()), bits(ref[2])), (what, name, b, q, "contrast")
                assert np.array_equal(bits(got.contrast0[b, q].cpu().numpy()), bits(ref[3])), (what, name, b, q, "contrast0")
                if name == "constant":
                    for n in range(N):
                        lo0, hi0 = min(win[b, q, n, 0], D), min(win[b, q, n, 1], D)
                        if win[b, q, n, 0] < 0 or hi0 <= lo0:
                            assert tuple(gw[b, q, n]) == (-1, -1), (what, b, q, n, "a void span")
                        elif (lo0, hi0) != (0, D):
                            assert tuple(gw[b, q, n]) == (lo0, hi0), (what, b, q, n, "the scores' window cut at the duration")
        back = ops.span_scores_multi(rows_dev, got.spans, m, return_windows=True)[1].cpu().numpy()
        assert np.array_equal(back, gw), (what, name, "span_scores on span_refine's spans")

    # the two generators: their spans give their windows back, in the encoding of the rule
    prop = ops.span_propose(s, m, levels=(0.3, 0.6), max_spans=16, return_windows=True)
    anch = ops.span_anchors(s, m, scales=SCALES, max_spans=16, return_windows=True, return_scale=True)
    for name, got, sum_of in (("span_propose", prop, left_to_right_sum), ("span_anchors", anch, span_mask_sum)):
        gw, gs = got.windows.cpu().numpy(), got.spans.cpu().numpy()
        back = ops.span_scores_multi(s, got.spans, m, return_windows=True)[1].cpu().numpy()
        assert np.array_equal(back, gw), (what, "span_scores on %s's spans" % name)
        for b in range(2):
            for q in range(2):
                enc = np.array([RO.encode(a, e, sum_of(mask[b])) if a >= 0 else (RO.QNAN, RO.QNAN) for a, e in gw[b, q]], dtype=F)
                assert np.array_equal(bits(gs[b, q]), bits(enc)), (what, name, b, q, "the encoding")
    for b in range(2):
        for q in range(2):
            ref = AO.anchors_row(sims[b, q], None, durs[b], L, SCALES, AO.CONTRAST, 2, 1, 16)
            assert np.array_equal(anch.windows[b, q].cpu().numpy(), ref[4]) and np.array_equal(bits(anch.scores[b, q].cpu().numpy()), bits(ref[1])), (what, b, q, "span_anchors")
            assert (int(anch.n_spans[b, q]), int(anch.n_found[b, q])) == (ref[2], ref[3]) and np.array_equal(anch.scale[b, q].cpu().numpy(), ref[5]), (what, b, q)
