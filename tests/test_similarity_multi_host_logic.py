"""Several texts per video on the host: the drop-in surface of ``forward_clip_matching_multi``, the two ABI entries behind it (rv_frame_cosine_multi,
rv_span_scores_multi) with every refusal they make before a launch, and the multi-query float64 oracle (tests/similarity_multi_oracle.py) against fixture
G17 and against the single-text oracle it loops over.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

import similarity_multi_oracle as M
import similarity_oracle as O
from revisionllm_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_TOL = 2e-5            # the suite's oracle bound (test_oracle_golden.TOL)
ENTRIES = ["rv_frame_cosine_multi", "rv_span_scores_multi"]
RV_ERR_ARG = -1              # include/revision_hip.h: rv_status


@pytest.fixture(scope="module")
def g17(golden):
    return {k: torch.from_numpy(v) for k, v in golden.npz("g17_similarity").items()}


def g17_multi(g17):
    """G17's three texts as Q = 3 against each of its videos, each query with the video's own eleven proposals: [b, q = b] is the pair G17 records."""
    text = g17["text"][None].repeat(3, 1, 1).contiguous()                  # [B=3, Q=3, d]: text[b, q] = G17's text q
    spans = g17["spans"][:, None].repeat(1, 3, 1, 1).contiguous()          # [B=3, Q=3, N=11, 2]
    return text, g17["video"], g17["mask"], spans


def test_the_new_name_imports_from_both_module_names():
    from revisionllm_amd.eval import similarity
    assert callable(similarity.forward_clip_matching_multi)
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
from revisionllm.eval.similarity import forward_clip_matching_multi, forward_clip_matching
import revisionllm_amd.eval.similarity as real
assert forward_clip_matching_multi is real.forward_clip_matching_multi and forward_clip_matching is real.forward_clip_matching
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_signature():
    from revisionllm_amd.eval import similarity as S
    p = inspect.signature(S.forward_clip_matching_multi).parameters
    assert list(p) == ["src_cls_txt", "src_vid_appear", "src_vid_appear_mask", "proposal", "is_groundtruth", "k", "pooling", "temperature", "return_windows"]
    assert p["is_groundtruth"].default is False
    assert {n: p[n].default for n in ("k", "pooling", "temperature", "return_windows")} == dict(k=3, pooling="topk", temperature=0.01, return_windows=False)
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("k", "pooling", "temperature", "return_windows"))
    assert all(p[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in list(p)[:5])
    # the single-text function is what it was
    q = inspect.signature(S.forward_clip_matching).parameters
    assert list(q) == list(p) and q["proposal"].default is None


def test_entries_in_header_ctypes_table_and_both_libraries():
    header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    declared = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", header))
    assert "#define RV_ABI_VERSION 5" in header
    if not all(os.path.exists(p) for p in hip.LIB_PATHS.values()):
        from revisionllm_amd import build
        build.build_library()
    for name in ENTRIES:
        assert name in declared and name in hip.SIGNATURES, name
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(params.split(",")) == len(hip.SIGNATURES[name][1]), name
        for flavour, path in hip.LIB_PATHS.items():
            assert hasattr(ctypes.CDLL(path), name), (flavour, name)
    assert "similarity.hip" in __import__("revisionllm_amd.build", fromlist=["SOURCES"]).SOURCES


def _refused(rc, message):
    return rc == RV_ERR_ARG and message in hip.last_error()


def test_every_refusal_of_rv_frame_cosine_multi_comes_before_any_launch():
    """Dummy pointers: a call that got as far as a launch would fault, so a clean RV_ERR_ARG with its message shows the check came first."""
    one = ctypes.c_void_p(64)
    for flavour in hip.LIB_PATHS:
        f = hip.lib(flavour).rv_frame_cosine_multi
        good = dict(video=one, dtype=hip.RV_F32, text=one, B=1, Q=2, L=4, d=8, unit=one, out=one)

        def call(**kw):
            a = {**good, **kw}
            return f(a["video"], a["dtype"], a["text"], a["B"], a["Q"], a["L"], a["d"], a["unit"], a["out"], None)
        for name in ("video", "text", "unit", "out"):
            assert _refused(call(**{name: None}), "rv_frame_cosine_multi: bad arguments"), (flavour, name)
        for name in ("B", "Q", "L", "d"):
            for v in (0, -1):
                assert _refused(call(**{name: v}), "rv_frame_cosine_multi: bad arguments"), (flavour, name, v)
        other = hip.RV_BF16 if flavour == "f16" else hip.RV_F16
        want = "rv_frame_cosine_multi: dtype must be f32 or %s" % ("fp16" if flavour == "f16" else "bf16")
        assert _refused(call(dtype=other), want) and _refused(call(dtype=77), want), flavour
        for B, Q in ((65536, 1), (1, 65536), (256, 256), (3, 21846)):
            assert _refused(call(B=B, Q=Q), "rv_frame_cosine_multi: at most 65535 (video, query) rows per launch (B=%d, Q=%d)" % (B, Q)), (flavour, B, Q)


def test_every_refusal_of_rv_span_scores_multi_comes_before_any_launch():
    one = ctypes.c_void_p(64)
    for flavour in hip.LIB_PATHS:
        f = hip.lib(flavour).rv_span_scores_multi
        good = dict(sims=one, spans=one, mask=one, B=1, Q=2, L=4, N=2, mode=0, k=3, tau=0.01, scores=one, windows=None)

        def call(**kw):
            a = {**good, **kw}
            return f(a["sims"], a["spans"], a["mask"], a["B"], a["Q"], a["L"], a["N"], a["mode"], a["k"], a["tau"], a["scores"], a["windows"], None)
        for name in ("sims", "spans", "mask", "scores"):
            assert _refused(call(**{name: None}), "rv_span_scores_multi: bad arguments"), (flavour, name)
        for name in ("B", "Q", "L", "N"):
            for v in (0, -1):
                assert _refused(call(**{name: v}), "rv_span_scores_multi: bad arguments"), (flavour, name, v)
        for mode in (2, -1):
            assert _refused(call(mode=mode), "rv_span_scores_multi: mode=%d must be 0 (top-k) or 1 (attention)" % mode)
        for k in (0, 65):
            assert _refused(call(k=k), "rv_span_scores_multi: k=%d must be in [1, 64]" % k)
        for tau in (0.0, float("inf"), float("-inf"), float("nan")):
            assert _refused(call(mode=1, tau=tau), "rv_span_scores_multi: temperature must be finite and not 0"), tau
        for B, Q in ((65536, 1), (1, 65536), (256, 256)):
            assert _refused(call(B=B, Q=Q), "rv_span_scores_multi: at most 65535 (video, query) rows per launch (B=%d, Q=%d)" % (B, Q)), (flavour, B, Q)


def test_host_side_refusals_come_before_the_device_is_looked_for():
    """Shape and dtype errors are ValueError, a missing proposal TypeError - on a machine without a GPU too."""
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import forward_clip_matching_multi
    text, video, mask, spans = torch.zeros(2, 3, 8), torch.zeros(2, 5, 8), torch.ones(2, 5), torch.zeros(2, 3, 4, 2)
    with pytest.raises(TypeError, match="proposal is None"):
        forward_clip_matching_multi(text, video, mask)
    bad = [dict(text=torch.zeros(2, 8)), dict(text=torch.zeros(2, 3, 7)), dict(text=torch.zeros(3, 3, 8)), dict(text=torch.zeros(2, 0, 8), spans=torch.zeros(2, 0, 4, 2)),
           dict(video=torch.zeros(2, 5)), dict(video=torch.zeros(3, 5, 8)), dict(mask=torch.ones(2, 4)), dict(mask=torch.ones(2, 3, 5)),
           dict(spans=torch.zeros(2, 4, 2)), dict(spans=torch.zeros(2, 3, 4, 3)), dict(spans=torch.zeros(2, 2, 4, 2)), dict(spans=torch.zeros(1, 3, 4, 2)),
           dict(spans=torch.zeros(2, 3, 4, 2, dtype=torch.int64)), dict(video=torch.zeros(2, 5, 8, dtype=torch.int32)), dict(text=torch.zeros(2, 3, 8, dtype=torch.int64)),
           dict(video=torch.zeros(2, 0, 8), mask=torch.ones(2, 0)), dict(mask=torch.ones(2, 5, dtype=torch.complex64)), dict(spans=[[[[0.5, 1.0]]]])]
    for kw in bad:
        a = {**dict(text=text, video=video, mask=mask, spans=spans), **kw}
        with pytest.raises(ValueError, match="forward_clip_matching_multi"):
            forward_clip_matching_multi(a["text"], a["video"], a["mask"], a["spans"])
    for kw in (dict(k=0), dict(k=65), dict(k=2.5), dict(pooling="mean"), dict(pooling="attention", temperature=0.0), dict(pooling="attention", temperature=float("nan"))):
        with pytest.raises(ValueError, match="forward_clip_matching_multi"):
            forward_clip_matching_multi(text, video, mask, spans, **kw)
    with pytest.raises(ValueError, match="frame_cosine_multi"):
        ops.frame_cosine_multi(torch.zeros(2, 8), video)
    with pytest.raises(ValueError, match="span_scores_multi"):
        ops.span_scores_multi(torch.zeros(2, 3, 5), torch.zeros(2, 4, 2), mask)
    with pytest.raises(ValueError, match="span_scores_multi"):
        ops.span_scores_multi(torch.zeros(2, 3, 5), spans, torch.ones(2, 3, 5))
    with pytest.raises(ValueError, match="span_scores_multi"):
        ops.span_scores_multi(torch.zeros(2, 3, 5).half(), spans, mask)
    with pytest.raises(ValueError, match="span_scores_multi"):
        ops.span_scores_multi(torch.zeros(2, 3, 5), spans, mask, pooling="mean")
    if not torch.cuda.is_available():                          # device code: a valid call raises instead of falling back to torch on the CPU
        with pytest.raises(hip.HipLibraryError):
            forward_clip_matching_multi(text, video, mask, spans)


GROUNDING_NAMES = ["topk_pool", "frame_cosine", "SPAN_POOLINGS", "span_scores", "frame_cosine_multi", "span_scores_multi", "SPAN_FORMS", "SPAN_RANK_MAX",
                   "HIT_IOU", "SpanRank", "span_rank_keywords", "span_rank", "SPAN_PROPOSE_MAX_LEVELS", "SPAN_PROPOSE_MAX_FRAMES", "SPAN_PROPOSE_LEVELS",
                   "SpanProposals", "span_propose_keywords", "span_propose_shapes", "span_propose", "WINDOW_SELECT_MAX", "WindowSelection",
                   "window_select_keywords", "window_select_capacity", "window_select_gt", "window_select", "attn_pool"]


def test_ops_hands_out_the_grounding_modules_own_objects():
    """The grounding wrappers live in revisionllm_amd.grounding; every public name of theirs is the same object under ``ops``."""
    from revisionllm_amd import grounding, ops
    for name in GROUNDING_NAMES:
        assert getattr(ops, name) is getattr(grounding, name), name
        if callable(getattr(grounding, name)):
            assert getattr(grounding, name).__module__ == "revisionllm_amd.grounding", name
    assert ops.h2d.__module__ == "revisionllm_amd.ops"
    # ops imports grounding, and grounding takes h2d from ops at call time: importing grounding FIRST, in a fresh interpreter, must work too
    code = f"import sys; sys.path.insert(0, {ROOT!r}); import revisionllm_amd.grounding as g; from revisionllm_amd import ops; assert ops.span_rank is g.span_rank"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0, r.stderr


def test_multi_oracle_against_g17(g17):
    """[b, q = b] is the pair the reference recorded: scores within the suite's oracle bound, windows, zeros and the NaN pattern of the zeroed frame exactly."""
    text, video, mask, spans = g17_multi(g17)
    idx = torch.arange(3)
    for v, key in ((video, "scores"), (video.clone(), "scores_zero_frame")):
        if key == "scores_zero_frame":
            v[0, 3] = 0
        got, win = M.forward_clip_matching_multi64(text, v, mask, spans)
        assert got.shape == (3, 3, 11) and win.shape == (3, 3, 11, 2)
        for q in range(3):
            assert torch.equal(win[:, q], g17["windows"].long())               # the windows depend on the video's duration alone
        ref, diag = g17[key].double(), got[idx, idx]
        assert torch.equal(torch.isnan(diag), torch.isnan(ref)) and torch.equal(diag == 0, ref == 0)
        ok = ~torch.isnan(ref)
        assert float((diag[ok] - ref[ok]).abs().max() / ref[ok].abs().max()) < ORACLE_TOL
        if key == "scores_zero_frame":                                          # a zero frame is NaN for every query of its video, and for no other video
            assert torch.equal(torch.isnan(got[0]), torch.isnan(ref[0])[None].repeat(3, 1)) and not torch.isnan(got[1:]).any()


def test_multi_oracle_is_the_single_text_oracle_per_query(g17):
    text, video, mask, spans = g17_multi(g17)
    spans = spans.clone()
    spans[:, 1] = spans[:, 1].flip(1)                                           # each query its own proposals
    spans[:, 2, :, 1] *= 0.5
    for kw in (dict(), dict(k=1), dict(k=64), dict(pooling="attention", temperature=0.01), dict(pooling="attention", temperature=1.0)):
        got, win = M.forward_clip_matching_multi64(text, video, mask, spans, **kw)
        for q in range(3):
            one, w1 = O.forward_clip_matching64(text[:, q], video, mask, spans[:, q], **kw)
            assert torch.equal(got[:, q], one) and torch.equal(win[:, q], w1), (kw, q)
    cos = M.frame_cosine_multi64(text, video)
    assert cos.shape == (3, 3, 40) and all(torch.equal(cos[:, q], O.frame_cosine64(text[:, q], video)) for q in range(3))
    win = M.windows_multi(spans, mask)
    assert torch.equal(M.span_scores_multi64(cos, win)[:, 1], O.span_scores64(cos[:, 1], win[:, 1]))
