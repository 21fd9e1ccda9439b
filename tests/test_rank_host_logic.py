"""Ranking of scored proposals on the host: the package surface of ``rv_span_rank`` (header, ctypes table, both libraries, every refusal of the C entry
before a launch, the Python-side refusals), the float32 oracle of tests/rank_oracle.py held against an independently written float64 statement and against
hand-made cases, and ``grounding_metrics_ranked`` against ``grounding_metrics_stream``.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import rank_oracle as K
from revisionllm_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_ERR_ARG = -1              # include/revision_hip.h: rv_status
HITS = (0.1, 0.3, 0.5, 0.7, 0.9)


# ------------------------------------------------------------------ surface ------------------------------------------------------------------
def test_the_names_import_from_both_module_names():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import metrics, similarity
    assert callable(similarity.rank_proposals) and callable(metrics.grounding_metrics_ranked) and callable(ops.span_rank)
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
import revisionllm_amd.eval.similarity as real
import revisionllm_amd.eval.metrics as real_m
from revisionllm.eval.similarity import rank_proposals, forward_clip_matching_multi
from revisionllm.eval.metrics import grounding_metrics_ranked, grounding_metrics_stream
import vtimellm.eval.similarity as old
assert rank_proposals is real.rank_proposals and old.rank_proposals is real.rank_proposals
assert grounding_metrics_ranked is real_m.grounding_metrics_ranked and forward_clip_matching_multi is real.forward_clip_matching_multi
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_signatures():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import metrics, similarity
    p = inspect.signature(ops.span_rank).parameters
    assert list(p) == ["scores", "spans", "top", "nms_iou", "form", "gt", "hit_iou", "return_order"]
    assert {n: p[n].default for n in list(p)[2:]} == dict(top=None, nms_iou=1.0, form="cxw", gt=None, hit_iou=HITS, return_order=False)
    q = inspect.signature(similarity.rank_proposals).parameters
    assert list(q) == ["scores", "proposal", "top", "nms_iou", "gt", "hit_iou", "return_order"]
    assert all(q[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(q)[2:])
    assert {n: q[n].default for n in list(q)[2:]} == dict(top=None, nms_iou=1.0, gt=None, hit_iou=HITS, return_order=False)
    m = inspect.signature(metrics.grounding_metrics_ranked).parameters
    assert list(m) == ["keep_iou", "first_hit", "hit_iou"] and m["hit_iou"].default == HITS
    assert ops.SpanRank._fields == ("keep", "n_keep", "keep_iou", "first_hit", "order")


def test_entry_in_header_ctypes_table_and_both_libraries():
    header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    declared = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", header))
    assert "#define RV_ABI_VERSION 5" in header
    if not all(os.path.exists(p) for p in hip.LIB_PATHS.values()):
        from revisionllm_amd import build
        build.build_library()
    assert "rv_span_rank" in declared and "rv_span_rank" in hip.SIGNATURES
    params = re.search(r"\brv_span_rank\s*\(([^)]*)\)", header).group(1)
    assert len(params.split(",")) == len(hip.SIGNATURES["rv_span_rank"][1]) == 16
    for flavour, path in hip.LIB_PATHS.items():
        assert hasattr(ctypes.CDLL(path), "rv_span_rank"), flavour
        assert hip.lib(flavour).rv_abi_version() == 5
    assert "topk" in re.search(r"/\* ---- ranking scored proposals.*?\*/", header, re.S).group(0)      # the header says how its order differs


def _refused(rc, message):
    return rc == RV_ERR_ARG and message in hip.last_error()


def test_every_refusal_of_rv_span_rank_comes_before_any_launch():
    """Dummy pointers: a call that got as far as a launch would fault, so a clean RV_ERR_ARG with its message shows the check came first."""
    one = ctypes.c_void_p(64)
    for flavour in hip.LIB_PATHS:
        f = hip.lib(flavour).rv_span_rank
        good = dict(scores=one, spans=one, form=1, R=2, N=8, top=3, nms=0.5, gt=one, hit=one, T=5, order=one, keep=one, n_keep=one, keep_iou=one, first_hit=one)

        def call(**kw):
            a = {**good, **kw}
            return f(a["scores"], a["spans"], a["form"], a["R"], a["N"], a["top"], a["nms"], a["gt"], a["hit"], a["T"], a["order"], a["keep"], a["n_keep"],
                     a["keep_iou"], a["first_hit"], None)
        for name in ("scores", "spans", "keep", "n_keep"):
            assert _refused(call(**{name: None}), "rv_span_rank: bad arguments"), (flavour, name)
        for name in ("R", "N"):
            for v in (0, -1):
                assert _refused(call(**{name: v}), "rv_span_rank: bad arguments"), (flavour, name, v)
        assert _refused(call(N=2049, top=3), "rv_span_rank: N=2049 proposals per row (at most 2048)")
        for top in (0, -1, 9):
            assert _refused(call(top=top), "rv_span_rank: top=%d must be in [1, N=8]" % top), top
        for form in (2, -1):
            assert _refused(call(form=form), "rv_span_rank: form=%d must be 0 (start, end) or 1 (centre, width)" % form)
        for nms in (-0.5, float("inf"), float("-inf"), float("nan")):
            assert _refused(call(nms=nms), "rv_span_rank: nms_iou must be finite and >= 0"), nms
        for T in (-1, 17):
            assert _refused(call(T=T), "rv_span_rank: T=%d thresholds (at most 16)" % T)
        needs = "rv_span_rank: hit_iou, T > 0, keep_iou and first_hit need gt"
        assert _refused(call(gt=None), needs)                                                        # T > 0 without gt
        assert _refused(call(gt=None, hit=None, T=0, first_hit=None), needs)                         # keep_iou without gt
        assert _refused(call(gt=None, hit=None, T=0, keep_iou=None), needs)                          # first_hit without gt
        assert _refused(call(gt=None, T=0, keep_iou=None, first_hit=None), needs)                    # hit_iou without gt
        assert _refused(call(hit=None), "rv_span_rank: T=5 thresholds without hit_iou")
        assert _refused(call(T=0, hit=None, keep_iou=None), "rv_span_rank: gt with neither thresholds nor keep_iou")


def test_python_side_refusals_come_before_the_device_is_looked_for():
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import rank_proposals
    s, p, g = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, 2), torch.zeros(2, 3, 2)
    bad = [dict(scores=torch.zeros(4)), dict(scores=torch.zeros(2, 3, 4, 1)), dict(spans=torch.zeros(2, 3, 4, 3)), dict(spans=torch.zeros(2, 3, 5, 2)),
           dict(spans=torch.zeros(2, 4, 2)), dict(gt=torch.zeros(2, 2)), dict(gt=torch.zeros(2, 3, 3)), dict(spans=torch.zeros(2, 3, 4, 2, dtype=torch.int64)),
           dict(gt=torch.zeros(2, 3, 2, dtype=torch.int32)), dict(spans=[[0.5, 1.0]]), dict(scores=torch.zeros(2, 2049), spans=torch.zeros(2, 2049, 2), gt=None)]
    keywords = [dict(top=0), dict(top=-3), dict(top=2.5), dict(top=True), dict(nms_iou=-0.1), dict(nms_iou=float("nan")), dict(nms_iou=float("inf")),
                dict(hit_iou=tuple(range(17))), dict(nms_iou=None), dict(nms_iou="x"), dict(hit_iou=("a",)), dict(hit_iou=0.5)]
    for fn, who in ((ops.span_rank, "span_rank"), (rank_proposals, "rank_proposals")):
        for kw in bad:
            a = {**dict(scores=s, spans=p, gt=g), **kw}
            with pytest.raises(ValueError, match=who):
                fn(a["scores"], a["spans"], gt=a["gt"])
        for kw in keywords:
            with pytest.raises(ValueError, match=who):
                fn(s, p, gt=g, **kw)
    assert ops.span_rank_keywords("t", np.int64(3), np.float32(0.5), np.array([0.5, 0.7])) == (0.5, (0.5, 0.7))      # numpy numbers are numbers
    with pytest.raises(ValueError, match="span_rank: form"):
        ops.span_rank(s, p, form="xyxy")
    with pytest.raises(ValueError, match="span_rank: scores must be float32"):
        ops.span_rank(s.half(), p)
    with pytest.raises(ValueError, match="rank_proposals"):
        rank_proposals(s.long(), p)
    if not torch.cuda.is_available():                          # device code: a valid call raises instead of falling back to torch on the CPU
        with pytest.raises(hip.HipLibraryError):
            rank_proposals(s, p, gt=g)


# ------------------------------------------------------------------ the oracle ------------------------------------------------------------------
def test_f32_oracle_equals_an_independent_float64_statement_on_exact_inputs():
    """Bounds that are multiples of 2^-6 in [0, 2], thresholds in {0.25, 0.5, 0.75}: every f32 operation of the rule is exact, so the float64 statement
    (written with a division and a selection sort) must give the same order, keep and first_hit."""
    rng = np.random.default_rng(7)
    for N, top in ((1, 1), (5, 5), (17, 4), (40, 40), (90, 25)):
        for nms in (0.25, 0.5, 0.75):
            R = 6
            a = rng.integers(0, 129, size=(R, N, 2))
            lo, hi = a.min(-1), a.max(-1)
            hi = np.where(hi == lo, lo + 1, hi)
            spans = (np.stack([lo, hi], -1) / 64.0).astype(np.float32)
            scores = rng.integers(-8, 9, size=(R, N)).astype(np.float32) / 4           # many ties
            g = np.sort(rng.integers(0, 129, size=(R, 2)), -1)
            g[:, 1] += 1
            gt = (g / 64.0).astype(np.float32)
            hit = (0.25, 0.5, 0.75)
            got = K.rank(scores, spans, 0, top, nms, gt, hit)
            ref = K.rank64(scores, spans, top, nms, gt, hit)
            for r in range(R):
                assert got["order"][r].tolist() == ref[r][0] and got["keep"][r].tolist() == ref[r][1] and got["first_hit"][r].tolist() == ref[r][2], (N, nms, r)
                assert got["n_keep"][r] == sum(i >= 0 for i in ref[r][1])


def test_greedy_chain_a_suppresses_b_and_c_stays():
    """B would have suppressed C, but B is dead when its turn comes."""
    spans = np.array([[[0.0, 1.0], [0.5, 1.5], [1.0, 2.0]]], dtype=np.float32)      # IoU(A,B) = IoU(B,C) = 1/3, IoU(A,C) = 0
    scores = np.array([[3.0, 2.0, 1.0]], dtype=np.float32)
    out = K.rank(scores, spans, 0, 3, 0.25)
    assert out["keep"].tolist() == [[0, 2, -1]] and out["n_keep"].tolist() == [2] and out["order"].tolist() == [[0, 1, 2]]
    assert K.rank(scores, spans, 0, 3, 0.5)["keep"].tolist() == [[0, 1, 2]]


def test_the_suppression_test_is_strict():
    """inter = 1, union = 2 at threshold 0.5: 1 > 0.5 * 2 is false, the proposal stays; just below the threshold it goes."""
    spans = np.array([[[0.0, 1.5], [0.5, 2.0]]], dtype=np.float32)                  # inter 1, union 2
    scores = np.array([[1.0, 0.0]], dtype=np.float32)
    assert K.rank(scores, spans, 0, 2, 0.5)["keep"].tolist() == [[0, 1]]
    assert K.rank(scores, spans, 0, 2, np.nextafter(np.float32(0.5), np.float32(0))) ["keep"].tolist() == [[0, -1]]
    hit = K.rank(scores, spans, 0, 2, 1.0, np.array([[0.5, 2.0]], dtype=np.float32), (0.5, 0.4999))
    assert hit["keep_iou"].tolist() == [[0.5, 1.0]] and hit["first_hit"].tolist() == [[1, 0]]       # 0.5 > 0.5 is no hit


def test_order_rules_and_void_spans():
    nan, inf = float("nan"), float("inf")
    assert K.rank_order([nan, 1.0, -inf, nan, inf, -0.0, 0.0, 1.0]) == [4, 1, 7, 5, 6, 2, 0, 3]
    spans = np.array([[[0.0, 1.0], [1.0, 0.0], [0.0, 1.0], [0.5, 0.5], [0.0, nan], [0.0, inf], [0.0, 1.0]]], dtype=np.float32)
    scores = np.array([[7, 6, 5, 4, 3, 2, 1]], dtype=np.float32)
    out = K.rank(scores, spans, 0, 7, 0.0, np.array([[0.0, 1.0]], dtype=np.float32), (0.5,))
    assert out["keep"].tolist() == [[0, 1, 3, 4, 5, -1, -1]]                         # the duplicates 2 and 6 go, every void span stays
    assert out["keep_iou"].tolist() == [[1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]] and out["first_hit"].tolist() == [[0]]
    cxw = np.array([[[0.5, 1.0], [0.5, -1.0], [0.5, 1.0], [0.5, 0.0], [nan, 1.0], [inf, 1.0], [0.5, 1.0]]], dtype=np.float32)
    assert K.rank(scores, cxw, 1, 7, 0.0)["keep"].tolist() == [[0, 1, 3, 4, 5, -1, -1]]


# ------------------------------------------------------------------ metrics ------------------------------------------------------------------
def test_grounding_metrics_ranked_is_grounding_metrics_stream():
    """Logs as the drivers write them, from random distinct scores and the oracle's IoUs: both routes give the same dict.  Tolerance: the percentages are
    float64 sums of n terms taken in another order (a count times 100 / n against n additions of 100 / n): n * 2^-52 relative."""
    from revisionllm_amd.eval.metrics import grounding_metrics_ranked, grounding_metrics_stream
    rng = np.random.default_rng(11)
    R, N = 37, 60
    scores = rng.permutation(R * N).reshape(R, N).astype(np.float32) / 64
    c, w = rng.uniform(0.1, 0.9, (R, N)), rng.uniform(0.02, 0.5, (R, N))
    spans = np.stack([c, w], -1).astype(np.float32)
    gt = np.sort(rng.uniform(0, 1, (R, 2)), -1).astype(np.float32)
    full = K.rank(scores, spans, 1, N, 1.0, gt, HITS)
    assert (full["n_keep"] == N).all()
    logs = []
    for r in range(R):
        iou = np.zeros(N)
        iou[full["keep"][r]] = full["keep_iou"][r]                                   # back to proposal order
        logs.append({"info": {"scores": scores[r].tolist(), "iou": iou.tolist()}})
    want = grounding_metrics_stream(logs)
    for conv in (lambda x: x, torch.from_numpy):
        got = grounding_metrics_ranked(conv(full["keep_iou"]), conv(full["first_hit"]), HITS)
        assert set(got) == set(want) and len(got) == 21
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=R * 2.0 ** -52, abs=0), k
    assert 0 < want["R1@0.5"] < want["R50@0.1"] <= 100                                 # the case is not degenerate
    assert grounding_metrics_ranked(torch.zeros(0, 4), torch.zeros(0, 5, dtype=torch.int32)) is None
    with pytest.raises(ValueError, match="grounding_metrics_ranked"):
        grounding_metrics_ranked(full["keep_iou"], full["first_hit"], (0.5,))
