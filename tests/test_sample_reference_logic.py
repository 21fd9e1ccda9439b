"""CPU checks of the float64 sampler reference (tests/sample_oracle.py) and of the case tables the GPU module uses (tests/sample_cases.py): the reference
against oracle/sampling.py on generic rows, against rows worked out by hand, and the margin condition - every mid-step uniform and every mid-step
``top_p`` of every table sits at least sample_oracle.MARGIN from the nearest step, so tests/test_gpu_sample_edges.py needs no excuse for a draw or an
``n_keep``.  No GPU."""
import math

import numpy as np
import pytest
import torch

import sample_cases as cases
from helpers import feats
from sample_oracle import LIST_CAP, MARGIN, Row, mid_step_top_p, mid_step_uniform, processed_f32


def _logits(p):
    return np.log(np.asarray(p, dtype=np.float64)).astype(np.float32)


HAND = _logits([0.5, 0.25, 0.125, 0.125])      # -1, -2, -3, -3 times ln 2, rounded to float32: the probabilities come back to ~1e-7


# ---- against the existing oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [100, 1500])
@pytest.mark.parametrize("T,k,p", [(1.0, 50, 1.0), (0.7, 20, 0.9), (1.0, 0, 0.8)])
def test_reference_agrees_with_the_oracle_on_generic_rows(V, T, k, p):
    """Distinct scores, uniforms away from the steps: the same kept set and the same token.  (T = 0.7: the oracle divides, the reference multiplies
    by the float32 reciprocal as the kernel does - one ulp apart at most, so the kept SET and the token are compared, not the values' bits.)"""
    from oracle import sampling
    x = feats(f"srl.generic.v{V}", (4, V)) * 2.0
    assert all(len(set(r.tolist())) == V for r in x)
    sc = sampling.process_logits(x, T, k, p)
    for b in range(4):
        ref = Row(x[b].numpy(), T, k, p)
        assert sorted(ref.kept) == torch.isfinite(sc[b]).nonzero()[:, 0].tolist()
        assert ref.n_keep == int(torch.isfinite(sc[b]).sum())
        assert np.allclose(ref.scores[ref.kept], sc[b][ref.kept].numpy(), rtol=3e-7, atol=0)
        for rank in sorted({0, 1, ref.n_keep // 2, ref.n_keep - 1}):
            u, hw = mid_step_uniform(ref, rank)
            if hw < 1e-6:
                continue                            # (the oracle's own f32 sums decide such a draw, not the rule)
            tok = int(sampling.select_token(sc[b:b + 1], torch.tensor([u], dtype=torch.float32))[0])
            assert tok == ref.draw(u) == ref.kept[rank], (b, rank)
        ent = -(torch.softmax(sc[b].double(), -1) * torch.log(torch.softmax(sc[b].double(), -1) + 1e-10)).sum()
        assert math.isclose(ref.entropy_proc, float(ent), rel_tol=1e-5)
        raw = torch.softmax(x[b].double(), -1)
        assert math.isclose(ref.entropy_raw, float(-(raw * torch.log(raw + 1e-10)).sum()), rel_tol=1e-9)


def test_processed_scores_multiply_by_the_float32_reciprocal():
    x = feats("srl.recip", (4096,)).numpy()
    got = processed_f32(x, 0.05)
    assert got.dtype == np.float32 and np.array_equal(got, x * (np.float32(1) / np.float32(0.05)))
    assert (got != x / np.float32(0.05)).any()      # why the distinction is made at all


# ---- rows worked out by hand ----------------------------------------------------------------------------------------------------------------------
def test_hand_row_draw_boundaries():
    ref = Row(HAND, 1.0, 0, 1.0)
    assert ref.kept == [0, 1, 2, 3] and ref.n_keep == 4
    assert np.allclose(ref.probs, [0.5, 0.25, 0.125, 0.125], atol=1e-7)
    assert np.allclose(ref.cdf, [0.5, 0.75, 0.875, 1.0], atol=1e-7)
    for u, tok in ((0.0, 0), (0.49, 0), (0.51, 1), (0.74, 1), (0.76, 2), (0.874, 2), (0.876, 3), (0.999, 3), (float(np.nextafter(1.0, 0.0)), 3)):
        assert ref.draw(u) == tok, u
    # "exceeds": a uniform exactly ON a step belongs to the next token
    assert ref.draw(ref.cdf[0]) == 1 and ref.draw(ref.cdf[1]) == 2
    assert math.isclose(ref.entropy_proc, 1.75 * math.log(2), rel_tol=1e-6) and math.isclose(ref.entropy_raw, ref.entropy_proc, rel_tol=1e-12)
    assert ref.threshold == HAND[3]
    u, hw = mid_step_uniform(ref, 1)
    assert math.isclose(u, 0.625, abs_tol=1e-7) and math.isclose(hw, 0.125, abs_tol=1e-7)


def test_hand_row_top_p():
    # ascending cumulative sums: 0.125, 0.25, 0.5, 1.0; what is <= 1 - top_p goes
    assert Row(HAND, 1.0, 0, 0.8).kept == [0, 1, 2]           # 1 - p = 0.2: the last 0.125 goes, 0.25 > 0.2 stays
    assert Row(HAND, 1.0, 0, 0.7).kept == [0, 1]              # 0.3: both 0.125 go
    assert Row(HAND, 1.0, 0, 0.2).kept == [0]                 # 0.8: everything but the largest
    assert Row(HAND, 1.0, 0, 1e-6).kept == [0]                # the largest always stays
    r = Row(HAND, 1.0, 0, 0.7)
    assert np.allclose(r.probs, [2 / 3, 1 / 3], atol=1e-7) and r.threshold == HAND[1]
    assert math.isclose(r.entropy_proc, -(2 / 3) * math.log(2 / 3) - (1 / 3) * math.log(1 / 3), rel_tol=1e-6)
    base = Row(HAND, 1.0, 0, 1.0)
    for n, (mid, hw) in {4: (0.0625, 0.0625), 3: (0.1875, 0.0625), 2: (0.375, 0.125), 1: (0.75, 0.25)}.items():
        tp, got_hw = mid_step_top_p(base, n)
        assert math.isclose(1 - tp, mid, abs_tol=1e-6) and math.isclose(got_hw, hw, abs_tol=1e-6)
        assert Row(HAND, 1.0, 0, tp).n_keep == n


def test_hand_row_ties_signed_zeros_and_top_k():
    # the tie pair (indices 2, 3): the lower index first, in the order and at the k-th place of the list
    assert Row(HAND, 1.0, 3, 1.0).kept == [0, 1, 2]
    wide = Row(np.concatenate([HAND, np.full(80, -50.0, dtype=np.float32)]), 1.0, 0, 1.0)
    assert wide.kept[:4] == [0, 1, 2, 3] and wide.draw(0.80) == 2 and wide.draw(0.95) == 3
    # +-0.0 is a tie: index decides, whatever the sign
    z = np.array([0.0, -1.0, -0.0, 0.0, -0.0], dtype=np.float32)
    assert Row(z, 1.0, 0, 1.0).kept == [0, 2, 3, 4, 1]
    assert Row(-z, 1.0, 0, 1.0).kept == [1, 0, 2, 3, 4]
    assert Row(z, 1.0, 2, 1.0).kept == [0, 2] and Row(z, 0.5, 3, 1.0).kept == [0, 2, 3]
    # wide mode keeps the tie at the k-th place whole, list mode cuts it
    many = np.concatenate([z, np.full(95, -3.0, dtype=np.float32)])
    assert Row(many, 1.0, 65, 1.0).n_keep == 100 and Row(many, 1.0, 64, 1.0).kept == [0, 2, 3, 4, 1] + list(range(5, 64))
    assert LIST_CAP == 64
    # top_k > V keeps V
    r = Row(HAND, 1.0, 10, 1.0)
    assert r.n_keep == 4 and r.kept == [0, 1, 2, 3] and r.list_mode


def test_hand_row_with_masked_entries_draws_a_token_with_mass():
    x = np.array([HAND[0], -np.inf, HAND[1], -np.inf], dtype=np.float32)
    one_below = float(np.nextafter(1.0, 0.0))
    for k in (0, 3, 10):
        ref = Row(x, 1.0, k, 1.0)
        assert ref.kept[:2] == [0, 2] and ref.last_positive == 1
        assert ref.draw(one_below) == 2 and ref.draw(cases.ONE_BELOW) == 2 and ref.draw(0.0) == 0
        assert np.isfinite(ref.scores[ref.draw(one_below)])
    # the clamp itself: a CDF that never exceeds u (forced) still ends on the last token with mass
    ref = Row(x, 1.0, 0, 1.0)
    ref.cdf = [2 / 3, 0.9999999, 0.9999999, 0.9999999]
    assert ref.draw_pos(0.99999995) == 1


# ---- the margin condition over the GPU module's tables --------------------------------------------------------------------------------------------
def _table_ids():
    return [f"list V{V}" for V in cases.LIST_V] + ["n_keep"] + [f"wide V{V}" for V in cases.WIDE_V] + ["ties", "masked", "many rows"]


def _table(name):
    kind, _, v = name.partition(" V")
    return {"list": lambda: cases.list_launches(int(v)), "wide": lambda: cases.wide_launches(int(v)), "n_keep": cases.nkeep_launches,
            "ties": cases.tie_launches, "masked": cases.masked_launches, "many rows": cases.many_rows_launches}[kind]()


@pytest.mark.parametrize("name", _table_ids())
def test_every_step_the_gpu_tables_rely_on_is_at_least_the_margin_wide(name):
    """A condition on the cases, not a measurement: the kernel's f32 sums err by about 64 * 3 * 2^-24 = 1.2e-5 (list path: at most 64 sequential terms
    <= 1, an exp and a divide each; wide path: tree sums), MARGIN = 1e-4 is 8 times that.  No rank of any table is skipped."""
    launches = _table(name)
    assert launches
    for L in launches:
        assert len(L.rows) >= 1
        for ref, rank, u, hw in zip(L.refs, L.ranks, L.us, L.hw):
            assert ref.draw_pos(u) == rank, (L.label, rank, u)
            assert hw is None or (hw >= MARGIN and 0.0 < u < 1.0), (L.label, rank, hw)
            assert hw is not None or u in (0.0, cases.ONE_BELOW, 1.0)
        assert (L.p_hw is None) == (L.top_p == 1.0)
        if L.p_hw is not None:
            assert L.p_hw >= MARGIN, (L.label, L.p_hw)
            assert all(ref.n_keep == L.n_wanted for ref in L.refs), L.label
            assert abs(float(np.float32(L.top_p)) - L.top_p) < 1e-7


def test_the_tables_hold_the_cases_they_are_meant_to():
    # every top_k > V of the list table is there, at every V
    for V in cases.LIST_V:
        ks = {L.top_k for L in cases.list_launches(V)}
        assert ks == set(cases.LIST_K)
        assert len(cases.list_launches(V)) == len(cases.LIST_K) * (1 + 3 + 1)
    # n_keep rows: distinct scores, permutations of one vector
    x = cases.nkeep_rows()
    assert x.shape == (cases.NKEEP_B, cases.NKEEP_V) and len(set(x[0].tolist())) == cases.NKEEP_V
    assert all(sorted(r.tolist()) == sorted(x[0].tolist()) for r in x) and not any(np.array_equal(x[0], r) for r in x[1:])
    for L in cases.nkeep_launches():
        assert len({tuple(ref.kept) for ref in L.refs}) == cases.NKEEP_B
    # the quantised row: a -0.0 below a +0.0 by index, the whole zero group inside the list, and a top_k that lets only the first zero in
    q, above, zeros = cases.tie_quantised_row()
    assert len(zeros) >= 2 and np.signbit(q[zeros[0]]) and not np.signbit(q[zeros[1]]) and zeros[0] < zeros[1]
    assert 1 <= above and above + len(zeros) <= LIST_CAP
    assert Row(q, 1.0, above + len(zeros), 1.0).kept[above:] == zeros and Row(q, 1.0, above + 1, 1.0).kept[above:] == zeros[:1]
    assert (np.round(np.float32(-0.2)) == 0) and np.signbit(np.round(np.float32(-0.2)))      # quantising does produce -0.0
    # masked rows: 10 finite scores each, and a uniform of ONE_BELOW draws the last of them
    m = cases.masked_rows()
    assert (np.isfinite(m).sum(-1) == cases.MASK_FINITE).all()
    for L in cases.masked_launches():
        assert all(np.isfinite(ref.scores[w]) for ref, w in zip(L.refs, L.want))
        if "u=0.99" in L.label or "u=1.0" in L.label:
            assert all(r == cases.MASK_FINITE - 1 for r in L.ranks)
    assert {k for V in cases.WIDE_V for k in cases.wide_top_ks(V)} >= {0, 65, 72, 999, 1000, 1007, 4098, 4099, 4106}
