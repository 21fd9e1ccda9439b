"""Proposal-query matching and attention pooling on the host: the float64 oracle (tests/similarity_oracle.py) against the reference's outputs in fixture
G17 (tests/golden/make_g17_similarity.py), its f32 window rule against torch's own f32 evaluation of the reference's expressions, the drop-in surface of
``revisionllm_amd.eval.similarity`` and the ABI entries behind it.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import similarity_oracle as O
from revisionllm_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_TOL = 2e-5            # the suite's oracle bound (test_oracle_golden.TOL)
NAMES = ["span_cxw_to_xx", "forward_clip_matching", "_get_predicted_proposal_feat", "_topk_pooling", "_attention_pooling"]
NEW_ENTRIES = ["rv_frame_cosine", "rv_span_scores", "rv_attn_pool"]


@pytest.fixture(scope="module")
def g17(golden):
    return {k: torch.from_numpy(v) for k, v in golden.npz("g17_similarity").items()}


def test_g17_holds_the_cases_it_is_for(g17):
    """The fixture's own shape: durations 40 / 25 / 7, eleven spans per video, an empty window at duration 40 that is one frame at duration 25, a window
    reached through a negative end, and the NaN pattern of the zeroed frame."""
    assert g17["video"].shape == (3, 40, 32) and g17["spans"].shape == (3, 11, 2)
    assert g17["mask"].sum(-1).tolist() == [40, 25, 7]
    win = g17["windows"]
    assert win[0, 2].tolist() == [20, 20] and win[1, 2].tolist() == [12, 13] and float(g17["scores"][0, 2]) == 0.0
    assert win[0, 8].tolist() == [0, 34]                                                  # (-0.2, 0.1): feat[0:-6]
    assert win[2, 10].tolist() == [1, 0] and float(g17["scores"][2, 10]) == 0.0            # negative width at duration 7: nothing
    holds3 = (win[0, :, 0] <= 3) & (win[0, :, 1] > 3)
    assert torch.equal(torch.isnan(g17["scores_zero_frame"][0]), holds3) and int(holds3.sum()) == 4
    assert not torch.isnan(g17["scores_zero_frame"][1:]).any() and not torch.isnan(g17["scores"]).any()


def test_oracle_against_g17(g17):
    """Scores and pooled rows within the suite's oracle bound; windows, zeros and the NaN pattern exactly."""
    text, video, mask, spans = g17["text"], g17["video"], g17["mask"], g17["spans"]
    assert float((O.span_cxw_to_xx64(spans) - g17["xx"].double()).abs().max()) < 1e-7
    got, win = O.forward_clip_matching64(text, video, mask, spans)
    assert torch.equal(win, g17["windows"].long())
    ref = g17["scores"].double()
    assert torch.equal(got == 0, ref == 0)
    assert float((got - ref).abs().max() / ref.abs().max()) < ORACLE_TOL
    vz = video.clone()
    vz[0, 3] = 0
    gz, _ = O.forward_clip_matching64(text, vz, mask, spans)
    rz = g17["scores_zero_frame"].double()
    assert torch.equal(torch.isnan(gz), torch.isnan(rz))
    ok = ~torch.isnan(rz)
    assert float((gz[ok] - rz[ok]).abs().max() / rz[ok].abs().max()) < ORACLE_TOL
    for key, tau in (("attn_pool_t001", 0.01), ("attn_pool_t1", 1.0)):
        r = g17[key].double()
        assert r.shape == (3, 3, 32)
        assert float((O.attn_pool64(text, video, tau) - r).abs().max() / r.abs().max()) < ORACLE_TOL, key
        assert float((O.attn_pool_f32(text, video, tau).double() - r).abs().max() / r.abs().max()) < ORACLE_TOL, key


def test_oracle_modes_on_simple_rows():
    """The two pooling modes, the rank order and the empty / non-finite windows of the oracle on rows small enough to check by hand."""
    sims = torch.tensor([[0.1, 0.5, float("nan"), 0.4, 0.5, -0.2, 0.3, 0.0]])
    win = torch.tensor([[[3, 8], [0, 2], [1, 4], [4, 4], [6, 2], [-1, -1], [3, 5]]])
    top = O.span_scores64(sims, win, "topk", k=3)
    assert top[0, :2].tolist() == pytest.approx([0.4 + 0.5 + 0.3, 0.1 + 0.5], abs=1e-6)
    assert torch.isnan(top[0, 2]) and top[0, 3] == 0 and top[0, 4] == 0 and torch.isnan(top[0, 5])
    assert O.span_scores64(sims, win, "topk", k=1)[0, 6] == pytest.approx(0.5, abs=1e-6)
    att = O.span_scores64(sims, win, "attention", temperature=1.0)
    e = torch.exp(torch.tensor([0.4, 0.5], dtype=torch.float64))
    assert float(att[0, 6]) == pytest.approx(float((e * torch.tensor([0.4, 0.5], dtype=torch.float64)).sum() / e.sum()), abs=1e-6)
    assert torch.isnan(att[0, 2]) and att[0, 3] == 0 and torch.isnan(att[0, 5])
    assert O.rank_order(torch.tensor([1.0, float("nan"), 3.0, 3.0, float("nan")])).tolist() == [1, 4, 2, 3, 0]


def test_window_rule_equals_torchs_f32_evaluation_on_the_integer_grid():
    """10^5 seeded (centre, width, duration) triples with centre and width on the grid i / (2 * duration), where x * duration sits on or next to an integer and
    a wrong rounding moves a floor or a ceiling: the oracle's f32 rule (numpy) gives the start / end torch computes in f32 from the package's span_cxw_to_xx,
    and its (lo, hi) are Python's own slice of range(L)."""
    g = torch.Generator().manual_seed(17)
    n = 100_000
    duration = torch.randint(1, 20001, (n,), generator=g).float()
    ci = torch.randint(-40, 40, (n,), generator=g).float() + torch.randint(0, 2, (n,), generator=g).float() * duration
    wi = 2 * torch.randint(-10, 30, (n,), generator=g).float()            # even: the exact x * duration are (ci -+ wi / 2) / 2, half of them integers
    c = ci / (2 * duration) + (torch.randint(0, 3, (n,), generator=g).float() - 1) * torch.rand(n, generator=g) * (torch.rand(n, generator=g) < 0.3)
    w = wi / (2 * duration)
    from revisionllm_amd.eval.similarity import span_cxw_to_xx
    prop = span_cxw_to_xx(torch.stack([c, w], dim=-1)) * duration[:, None]                  # torch, f32: one rounding per operation
    assert prop.dtype == torch.float32
    start_t = prop[:, 0].floor().to(torch.int32).clamp_min(0).long().numpy()
    end_t = prop[:, 1].ceil().to(torch.int32).long().numpy()
    start, end, finite = O.start_end_f32(c.numpy(), w.numpy(), duration.numpy())
    assert finite.all() and np.array_equal(start, start_t) and np.array_equal(end, end_t)
    on_integer = float((prop == prop.round()).float().mean())           # 70 % of the centres are on the grid and half of their bounds are integers exactly; the f32
    assert on_integer > 0.2, on_integer                                  # roundings of c, w and x move some of them one ulp off - the cases this test is for
    L = torch.randint(1, 20001, (n,), generator=g).numpy()
    lo, hi = O.slice_lo_hi(start, end, L)
    for i in range(n):
        r = range(int(L[i]))[int(start[i]):int(end[i])]
        assert (r.start, r.stop) == (lo[i], hi[i]), (i, start[i], end[i], L[i])
    assert (end < 0).sum() > 100 and (hi <= lo).sum() > 100 and (start > L).sum() > 100 and (end > L).sum() > 100


def test_window_rule_on_non_finite_and_out_of_range_spans():
    mask = torch.ones(1, 10)
    spans = torch.tensor([[[float("nan"), 0.1], [0.5, float("inf")], [float("-inf"), 0.1], [3e9, 0.0], [-3e9, 0.0], [0.0, 1e30], [0.5, 1.0]]])
    win = O.windows(spans, mask)
    assert win[0].tolist() == [[-1, -1], [-1, -1], [-1, -1], [10, 10], [0, 0], [0, 10], [0, 10]]


def test_the_five_names_import_from_both_module_names():
    from revisionllm_amd.eval import similarity
    for n in NAMES:
        assert callable(getattr(similarity, n)), n
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
from revisionllm.eval.similarity import span_cxw_to_xx, forward_clip_matching, _get_predicted_proposal_feat, _topk_pooling, _attention_pooling
import revisionllm_amd.eval.similarity as real
assert forward_clip_matching is real.forward_clip_matching and _attention_pooling is real._attention_pooling
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_positional_signatures_are_the_references():
    from revisionllm_amd.eval import similarity as S
    p = inspect.signature(S.forward_clip_matching).parameters
    assert list(p)[:5] == ["src_cls_txt", "src_vid_appear", "src_vid_appear_mask", "proposal", "is_groundtruth"]
    assert p["proposal"].default is None and p["is_groundtruth"].default is False
    assert {n: p[n].default for n in ("k", "pooling", "temperature", "return_windows")} == dict(k=3, pooling="topk", temperature=0.01, return_windows=False)
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("k", "pooling", "temperature", "return_windows"))
    assert list(inspect.signature(S._get_predicted_proposal_feat).parameters) == ["src_vid_appear", "src_vid_appear_mask", "pred_proposal", "text_cls_features"]
    assert list(inspect.signature(S._attention_pooling).parameters) == ["text_embeds", "video_embeds", "temperature"]
    assert list(inspect.signature(S.span_cxw_to_xx).parameters) == ["cxw_spans"]


def test_new_entries_in_header_ctypes_table_and_both_libraries():
    header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    declared = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", header))
    assert "#define RV_ABI_VERSION 5" in header
    if not all(os.path.exists(p) for p in hip.LIB_PATHS.values()):
        from revisionllm_amd import build
        build.build_library()
    for name in NEW_ENTRIES:
        assert name in declared and name in hip.SIGNATURES, name
        for flavour, path in hip.LIB_PATHS.items():
            assert hasattr(ctypes.CDLL(path), name), (flavour, name)
    # the header's parameter lists and the ctypes table agree in length
    for name in NEW_ENTRIES:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(params.split(",")) == len(hip.SIGNATURES[name][1]), name
    # argument validation runs on the host before any launch
    for flavour in hip.LIB_PATHS:
        lib = hip.lib(flavour)
        one = ctypes.c_void_p(64)
        assert lib.rv_frame_cosine(one, hip.RV_F32, one, 1, 4, 8193, one, None) < 0 and "8192 columns of the staged text row" in hip.last_error()
        assert lib.rv_span_scores(one, one, one, 1, 4, 2, 0, 0, 0.01, one, None, None) < 0 and "k=0 must be in [1, 64]" in hip.last_error()
        assert lib.rv_span_scores(one, one, one, 1, 4, 2, 0, 65, 0.01, one, None, None) < 0 and "k=65 must be in [1, 64]" in hip.last_error()
        assert lib.rv_span_scores(one, one, one, 1, 4, 2, 2, 3, 0.01, one, None, None) < 0 and "mode=2" in hip.last_error()
        assert lib.rv_span_scores(one, one, one, 1, 4, 2, 1, 3, 0.0, one, None, None) < 0 and "temperature must be finite and not 0" in hip.last_error()
        for tau in (0.0, float("inf"), float("nan")):
            assert lib.rv_attn_pool(one, hip.RV_F32, one, 1, 4, 8, 1, tau, one, None) < 0 and "rv_attn_pool: temperature must be finite and not 0" in hip.last_error()
        T = (64 * 1024 - 256) // 4 - 8
        assert lib.rv_attn_pool(one, hip.RV_F32, one, 1, T + 1, 8, 1, 0.01, one, None) < 0 and "rv_attn_pool: d + T too large for LDS" in hip.last_error()
        other = hip.RV_BF16 if flavour == "f16" else hip.RV_F16
        assert lib.rv_frame_cosine(one, other, one, 1, 4, 8, one, None) < 0 and lib.rv_attn_pool(one, other, one, 1, 4, 8, 1, 0.01, one, None) < 0


def test_host_side_refusals_come_before_any_launch():
    """Shape and dtype errors are ValueError, a missing proposal TypeError - on a machine without a GPU too, so before the device is looked for."""
    from revisionllm_amd.eval.similarity import _attention_pooling, _get_predicted_proposal_feat, forward_clip_matching
    text, video, mask, spans = torch.zeros(2, 8), torch.zeros(2, 5, 8), torch.ones(2, 5), torch.zeros(2, 3, 2)
    with pytest.raises(TypeError, match="proposal is None"):
        forward_clip_matching(text, video, mask)
    bad = [dict(text=torch.zeros(2, 7)), dict(text=torch.zeros(8)), dict(video=torch.zeros(2, 5)), dict(video=torch.zeros(3, 5, 8)), dict(mask=torch.ones(2, 4)),
           dict(mask=torch.ones(2, 5, 1)), dict(spans=torch.zeros(2, 3)), dict(spans=torch.zeros(2, 3, 3)), dict(spans=torch.zeros(1, 3, 2)),
           dict(spans=torch.zeros(2, 3, 2, dtype=torch.int64)), dict(video=torch.zeros(2, 5, 8, dtype=torch.int32)), dict(text=torch.zeros(2, 8, dtype=torch.int64)),
           dict(video=torch.zeros(2, 0, 8), mask=torch.ones(2, 0)), dict(spans=[[0.5, 1.0]])]
    for kw in bad:
        a = {**dict(text=text, video=video, mask=mask, spans=spans), **kw}
        with pytest.raises(ValueError):
            forward_clip_matching(a["text"], a["video"], a["mask"], a["spans"])
        with pytest.raises(ValueError):
            _get_predicted_proposal_feat(a["video"], a["mask"], a["spans"], a["text"])
    for kw in (dict(k=0), dict(k=65), dict(k=2.5), dict(pooling="mean"), dict(pooling="attention", temperature=0.0), dict(pooling="attention", temperature=float("nan"))):
        with pytest.raises(ValueError):
            forward_clip_matching(text, video, mask, spans, **kw)
    with pytest.raises(ValueError):
        _attention_pooling(torch.zeros(2, 7), video, 0.01)
    with pytest.raises(ValueError):
        _attention_pooling(torch.zeros(8), video, 0.01)
    for tau in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            _attention_pooling(text, video, tau)
    if not torch.cuda.is_available():                          # device code: a valid call raises instead of falling back to torch on the CPU
        with pytest.raises(hip.HipLibraryError):
            forward_clip_matching(text, video, mask, spans)
        with pytest.raises(hip.HipLibraryError):
            _attention_pooling(text, video, 0.01)


def test_span_cxw_to_xx_on_2d_and_3d_input(g17):
    from revisionllm_amd.eval.similarity import span_cxw_to_xx
    spans = torch.tensor([[0.5, 1.0], [0.3, 0.2]])
    want = torch.tensor([[0.0, 1.0], [0.2, 0.4]])
    assert torch.allclose(span_cxw_to_xx(spans), want, atol=1e-7) and torch.allclose(span_cxw_to_xx(spans[None]), want[None], atol=1e-7)
    assert span_cxw_to_xx(spans).shape == (2, 2) and span_cxw_to_xx(spans[None]).shape == (1, 2, 2)
    assert torch.equal(span_cxw_to_xx(g17["spans"]), g17["xx"])                 # the reference's own f32 result, bit for bit
    assert span_cxw_to_xx(spans.double()).dtype == torch.float64 and span_cxw_to_xx(spans.half()).dtype == torch.float16
    assert span_cxw_to_xx(torch.zeros(2, 3, 4, 2)).shape == (2, 3, 4, 2)
