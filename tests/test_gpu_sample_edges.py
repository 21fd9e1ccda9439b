"""``rv_sample`` (csrc/sample.hip, ``sample_kernel``) through ``ops.sample`` against the float64 per-row reference of tests/sample_oracle.py, at the shapes
its other tests leave out: the candidate-list path at short vocabularies (V below the fast path's 1024, below the list's 64, ``top_k`` > V), exact
``n_keep`` under top-p, wide-path draws, exact ties and signed zeros, rows with masked (-inf) entries, and the entry's refusals.

Nothing is excused: every uniform sits in the middle of a step of the reference's CDF and every ``top_p`` in the middle of a step of its ascending
cumulative sum, each at least sample_oracle.MARGIN = 1e-4 wide on either side (tests/test_sample_reference_logic.py asserts that for the very tables
used here, tests/sample_cases.py), against f32 summation errors of about 1e-5.  So tokens, ``n_keep`` and ``topk_idx`` are compared exactly, and the
values with the tolerances the project already uses for them (TOL below).

Out of scope: a row that is entirely -inf and NaN logits (the kernel's keys assume numbers; neither the reference nor HF defines a draw there).
On masked rows ``n_keep`` itself is not asserted: HF leaves -inf entries inside the top-k "kept" at -inf while the oracle counts finite ones; what
consumers read is the reconstruction of the processed scores (model/revision_llama.py), and that is compared."""
import numpy as np
import pytest
import torch

import sample_cases as cases
from helpers import T as tensor

pytestmark = pytest.mark.gpu

CAP = 64
# (rtol, atol); atol None = torch.allclose's default 1e-8, as test_gpu_kernels.test_sample_and_scores uses for these outputs
TOL = {"val": (1e-6, None), "entropy_proc list": (1e-4, 1e-6), "entropy_proc wide": (2e-4, 1e-5), "entropy_raw": (1e-5, None)}


@pytest.fixture(scope="module")
def dev(op_flavour):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import hip
    hip.lib()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def variants(dev):
    """ctx of the general selection (sample_variant = 0) and of the compacted one (1, the default)."""
    from revisionllm_amd import hip
    return {v: hip.Options(sample_variant=v) for v in (0, 1)}


def _close(got, want, what):
    rtol, atol = TOL[what]
    return torch.allclose(torch.as_tensor(got).double(), torch.as_tensor(want).double(), rtol=rtol, atol=1e-8 if atol is None else atol)


def _sample(dev, L, ctx=None):
    from revisionllm_amd import ops
    o = ops.sample(tensor(L.x).to(dev), tensor(L.u).to(dev), True, L.T, L.top_k, L.top_p, ctx=ctx)
    return {k: v.cpu() for k, v in o.items()}


def _check(L, o, n_keep=True):
    """Every output of one launch against the references of its rows."""
    refs, V = L.refs, L.x.shape[1]
    R = len(refs)
    tok = o["tokens"].long().tolist()
    assert tok == L.want, (L.label, "tokens", [(r, a, b) for r, (a, b) in enumerate(zip(tok, L.want)) if a != b][:8])
    assert (o["topk_idx"] < V).all() and (o["topk_idx"] >= -1).all(), (L.label, "an index outside the vocabulary")
    if n_keep:
        assert o["n_keep"].tolist() == [ref.n_keep for ref in refs], (L.label, "n_keep", o["n_keep"].tolist()[:8], [ref.n_keep for ref in refs][:8])
    list_mode = refs[0].list_mode
    if list_mode:
        K = min(L.top_k, V)
        if L.top_p == 1.0 and n_keep:
            assert (o["n_keep"] == K).all(), (L.label, "n_keep at top_p = 1", o["n_keep"].tolist()[:8], K)
        for r, ref in enumerate(refs):                         # the list holds the K candidates of the top-k filter, the first n_keep of them kept
            assert o["topk_idx"][r, :K].tolist() == ref.after_top_k, (L.label, r, "topk_idx", o["topk_idx"][r, :K].tolist(), ref.after_top_k)
            assert ref.after_top_k[:ref.n_keep] == ref.kept
            assert _close(o["topk_val"][r, :K], ref.s32[ref.after_top_k], "val"), (L.label, r, "topk_val")
        assert (o["topk_idx"][:, K:] == -1).all() and (o["topk_val"][:, K:] == float("-inf")).all(), (L.label, "beyond min(top_k, V)")
    else:
        assert (o["topk_idx"] == -1).all() and (o["topk_val"] == float("-inf")).all(), (L.label, "a candidate list in wide mode")
    thr = np.array([ref.threshold for ref in refs], dtype=np.float32)
    if n_keep:
        assert np.isfinite(thr).all() and torch.isfinite(o["threshold"]).all(), (L.label, "threshold", o["threshold"].tolist()[:8])
    assert _close(o["threshold"], thr, "val"), (L.label, "threshold", o["threshold"].tolist()[:8], thr.tolist()[:8])
    for name, what in (("entropy_proc", "entropy_proc list" if list_mode else "entropy_proc wide"), ("entropy_raw", "entropy_raw")):
        want = [getattr(ref, name) for ref in refs]
        assert torch.isfinite(o[name]).all(), (L.label, name, o[name].tolist()[:8])
        assert _close(o[name], want, what), (L.label, name, o[name].tolist()[:8], want[:8])
    assert all(v.shape[0] == R for v in o.values())


# ---- the list path at short vocabularies ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", cases.LIST_V)
def test_list_path_at_short_vocabularies(dev, variants, V):
    """1 <= top_k <= 64 at V from 1 to 32768, top_k > V included (K = min(top_k, V): nothing beyond it, no index >= V, finite entropies), both
    selections: T = 1 / 0.7 with a top-p that leaves 3 tokens / 0.05; uniforms in the middle of the steps of ranks {0, 1, middle, last kept}."""
    for L in cases.list_launches(V):
        for v, ctx in variants.items():
            _check(L, _sample(dev, L, ctx))


# ---- exact n_keep under top-p ---------------------------------------------------------------------------------------------------------------------------
def test_n_keep_under_top_p_is_exact_on_both_paths(dev, variants):
    """Rows that are permutations of one vector of 300 distinct scores share the steps of the ascending cumulative sum, so one mid-step top_p asks every
    row for the same n_keep (list path, top_k = 64: 1, 2, 17, 63, 64; wide path, top_k = 0: 1, 2, 17, 150, 299 and top_k = 100: 1, 2, 17, 99, 100) while
    the indices differ.  n_keep exact, threshold = the reference's smallest kept score, tokens exact at mid-step uniforms."""
    for L in cases.nkeep_launches():
        for v, ctx in variants.items():
            o = _sample(dev, L, ctx)
            assert o["n_keep"].tolist() == [L.n_wanted] * len(L.refs), (L.label, v, o["n_keep"].tolist())
            _check(L, o)


# ---- wide-path draws ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", cases.WIDE_V)
def test_wide_path_draws_without_exclusions(dev, V):
    """top_k in {0, 65, V - 1, V, V + 7} (the wide ones), T = 0.8, top_p = 1: token and n_keep exact at ranks {0, 1, 10, the last with p >= 2e-4}."""
    for L in cases.wide_launches(V):
        _check(L, _sample(dev, L))


# ---- ties and signed zeros --------------------------------------------------------------------------------------------------------------------------------
def test_ties_and_signed_zeros_follow_the_reference_order(dev, variants):
    """Quantised rows with -0.0 planted below +0.0 (the whole zero group inside the list; only its first member inside; the wide path), a fully tied row and
    two tied maxima: topk_idx in (score descending, index ascending) order with -0.0 == +0.0, and mid-step uniforms inside a tie group draw the
    reference's member."""
    for L in cases.tie_launches():
        for v, ctx in variants.items():
            _check(L, _sample(dev, L, ctx))


@pytest.mark.parametrize("V", [100, 32768])
def test_greedy_on_a_fully_tied_row_returns_index_0(dev, variants, V):
    from revisionllm_amd import ops
    x = tensor(np.stack([cases.tie_flat_row(V)] * 2)).to(dev)
    for ctx in variants.values():
        o = ops.sample(x, None, False, ctx=ctx)
        assert o["tokens"].tolist() == [0, 0]


# ---- masked rows ------------------------------------------------------------------------------------------------------------------------------------------
def _rebuilt_scores(o, L, V):
    """The processed scores as model/revision_llama.py rebuilds them from the kernel's outputs."""
    x = tensor(L.x)
    if not L.top_k or L.top_k > CAP:
        sc = x * float(np.float32(1.0) / np.float32(L.T))
        return sc.masked_fill(sc < o["threshold"][:, None], float("-inf"))
    sc = torch.full((x.shape[0], V + 1), float("-inf"))
    keep = torch.arange(CAP)[None] < o["n_keep"][:, None]
    idx = torch.where(keep, o["topk_idx"], torch.full_like(o["topk_idx"], V)).long()
    return sc.scatter(1, idx, o["topk_val"])[:, :V].contiguous()


def test_masked_rows_never_draw_a_token_without_mass(dev, variants):
    """V = 200 with 10 finite scores, 64 rows a launch, top_k = 50 / 0 / 100, u = 0, mid-step, the largest float32 below 1, and 1.0 itself (which no sum
    exceeds: the clamp, on the list path and in the wide path's fallback): the drawn token has a finite processed score and is the reference's, the entropy holds, and the processed scores rebuilt from the outputs equal the reference's."""
    for L in cases.masked_launches():
        for v, ctx in variants.items():
            o = _sample(dev, L, ctx)
            tok = o["tokens"].long()
            assert (tok >= 0).all() and (tok < cases.MASK_V).all()
            proc = torch.stack([tensor(ref.scores) for ref in L.refs])
            drawn = proc.gather(1, tok[:, None])[:, 0]
            assert torch.isfinite(drawn).all(), (L.label, v, "rows that drew a masked token", (~torch.isfinite(drawn)).nonzero()[:, 0].tolist())
            _check(L, o, n_keep=False)
            assert torch.equal(_rebuilt_scores(o, L, cases.MASK_V), proc), (L.label, v, "rebuilt processed scores")


# ---- degenerate controls ----------------------------------------------------------------------------------------------------------------------------------
def test_a_tiny_top_p_keeps_the_argmax_for_every_uniform(dev, variants):
    from revisionllm_amd import ops
    for V, k in ((100, 50), (100, 0), (1025, 100), (40, 64)):
        x = tensor(cases.list_rows(V, 1.0))
        for uu in (0.0, 0.5, cases.ONE_BELOW):
            for ctx in variants.values():
                o = ops.sample(x.to(dev), torch.full((3,), uu).to(dev), True, 1.0, k, 1e-6, ctx=ctx)
                assert o["tokens"].cpu().long().tolist() == x.argmax(-1).tolist() and o["n_keep"].tolist() == [1, 1, 1], (V, k, uu)
                assert torch.equal(o["threshold"].cpu(), x.amax(-1))


def test_no_uniforms_when_sampling_is_a_uniform_of_zero(dev):
    from revisionllm_amd import ops
    for V, k in ((100, 50), (100, 0), (4099, 7)):
        x = tensor(cases.list_rows(V, 1.0)).to(dev)
        a, b = ops.sample(x, None, True, 0.9, k, 0.95), ops.sample(x, torch.zeros(3, device=dev), True, 0.9, k, 0.95)
        for name in a:
            assert torch.equal(a[name].cpu(), b[name].cpu()), (V, k, name)
        assert a["tokens"].cpu().long().tolist() == x.cpu().argmax(-1).tolist()


def test_257_rows_are_independent(dev):
    """Row indexing: B = 257 rows of V = 64, a rank of its own per row (b mod n_keep), list path and wide path."""
    for L in cases.many_rows_launches():
        _check(L, _sample(dev, L))


def test_the_largest_vocabulary_is_accepted_and_bad_arguments_are_refused(dev):
    from revisionllm_amd import hip, ops
    x = tensor(cases.list_rows(32768, 1.0)).to(dev)
    assert ops.sample(x, None, False)["tokens"].cpu().long().tolist() == x.cpu().argmax(-1).tolist()       # V = 32768 (the list path is in the table above)
    big = torch.zeros(2, 32769, device=dev)
    with pytest.raises(hip.HipLibraryError, match="V=32769 exceeds 32768"):
        ops.sample(big, None, False)
    with pytest.raises(hip.HipLibraryError, match="top_k=-1 must be 0"):
        ops.sample(x, torch.zeros(3, device=dev), True, 1.0, -1, 1.0)
    # ... and at the entry point itself with live buffers: an error status, nothing written
    for logits, V, do_sample, top_k in ((big, 32769, 0, 50), (x, 32768, 1, -1)):
        B = logits.shape[0]
        i32 = lambda *s: torch.full(s, 77, dtype=torch.int32, device=dev)
        f32 = lambda *s: torch.full(s, 7.5, dtype=torch.float32, device=dev)
        outs = [i32(B), f32(B), f32(B), i32(B, CAP), f32(B, CAP), i32(B), f32(B)]
        rc = hip.lib().rv_sample(None, hip.ptr(logits), B, V, hip.ptr(f32(B)), do_sample, 1.0, top_k, 1.0, *[hip.ptr(t) for t in outs], hip.stream())
        torch.cuda.synchronize()
        assert rc != 0
        assert all(bool((t == (77 if t.dtype == torch.int32 else 7.5)).all()) for t in outs)
