"""Per-frame validity in the fine half of the grounding chain, on the host: the package surface of ``rvc_span_scores_masked`` and
``rvc_span_propose_masked`` (names under both module names, signatures, the chain library's header, ctypes table and exports held to each other with
the new names among them, one source per kernel, every refusal of both C entries before a launch, every Python-side refusal before a device is looked
for) - these fail without the feature.  The rest guards the oracle of tests/spans_masked_oracle.py, which the GPU tests compare the kernels with: its
proposals are held to a brute-force statement, the identities the header states are checked on it, a masked window with at least k usable frames is
held to the unmasked oracle on ``masked_fill(-inf)``, and the float32 attention statement's own distance from float64 - a quarter of the GPU module's
bound - is measured.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import propose_oracle as PO
from helpers import assert_grounding_rule_is_shared
import similarity_oracle as SO
import spans_masked_oracle as MO
from revisionllm_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_ERR_ARG = -1              # include/revision_hip.h: rv_status
MINE = {"rvc_span_scores_masked", "rvc_span_propose_masked"}
F = np.float32
LEVELS = (0.5, 0.6, 0.7, 0.8, 0.9)


# ------------------------------------------------------------------ surface ------------------------------------------------------------------
def test_the_names_import_from_both_module_names():
    from revisionllm_amd import grounding, ops
    from revisionllm_amd.eval import similarity
    for name in ("span_scores_masked", "span_propose_masked", "MaskedSpanScores", "span_scores_masked_checks", "skip_nan_flag"):
        assert getattr(ops, name) is getattr(grounding, name) and getattr(grounding, name).__module__ == "revisionllm_amd.grounding", name
    assert ops.MaskedSpanScores._fields == ("scores", "windows", "n_usable")
    for name in ("forward_clip_matching_masked", "propose_spans_masked", "ground_queries_masked"):
        assert callable(getattr(similarity, name)), name
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
import revisionllm_amd.ops as real_ops
import revisionllm_amd.eval.similarity as real_similarity
from revisionllm.ops import span_scores_masked, span_propose_masked, MaskedSpanScores
from revisionllm.eval.similarity import forward_clip_matching_masked, propose_spans_masked, ground_queries_masked
import vtimellm.ops as old_ops
import vtimellm.eval.similarity as old_similarity
assert span_scores_masked is real_ops.span_scores_masked is old_ops.span_scores_masked
assert span_propose_masked is real_ops.span_propose_masked is old_ops.span_propose_masked and MaskedSpanScores is real_ops.MaskedSpanScores
assert forward_clip_matching_masked is real_similarity.forward_clip_matching_masked is old_similarity.forward_clip_matching_masked
assert propose_spans_masked is real_similarity.propose_spans_masked and ground_queries_masked is old_similarity.ground_queries_masked
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_signatures():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import similarity
    K = inspect.Parameter.KEYWORD_ONLY

    def keywords(fn):
        return {n: p.default for n, p in inspect.signature(fn).parameters.items() if p.kind is K}
    p = inspect.signature(ops.span_scores_masked).parameters
    assert list(p)[:3] == ["sims", "spans", "mask"] and all(p[n].kind is not K for n in list(p)[:3])
    assert keywords(ops.span_scores_masked) == dict(valid=None, skip_nan=False, k=3, pooling="topk", temperature=0.01, return_windows=False,
                                                    return_usable=False)
    p = inspect.signature(ops.span_propose_masked).parameters
    assert list(p)[:2] == ["sims", "mask"] and list(p)[2:4] == ["valid", "skip_nan"]
    assert keywords(ops.span_propose_masked) == {"valid": None, "skip_nan": False, **keywords(ops.span_propose)}
    p = inspect.signature(similarity.forward_clip_matching_masked).parameters
    assert len([n for n in p if p[n].kind is not K]) == 4
    assert keywords(similarity.forward_clip_matching_masked) == dict(valid=None, skip_nan=False, k=3, pooling="topk", temperature=0.01, return_windows=False,
                                                                      return_usable=False)
    assert list(inspect.signature(similarity.propose_spans_masked).parameters)[:4] == ["sims", "mask", "valid", "skip_nan"]
    assert keywords(similarity.propose_spans_masked) == {"valid": None, "skip_nan": False, **keywords(similarity.propose_spans)}
    g, gm = inspect.signature(similarity.ground_queries).parameters, inspect.signature(similarity.ground_queries_masked).parameters
    assert list(gm) == ["text", "video", "mask", "valid", "skip_nan"] + list(g)[3:]
    assert keywords(similarity.ground_queries_masked) == {"valid": None, "skip_nan": False, **keywords(similarity.ground_queries)}
    assert gm["propose_keywords"].kind is inspect.Parameter.VAR_KEYWORD
    # no existing function gained a keyword
    for fn in (ops.span_scores, ops.span_scores_multi, ops.span_propose, similarity.forward_clip_matching, similarity.forward_clip_matching_multi,
               similarity.propose_spans, similarity.ground_queries):
        assert "valid" not in inspect.signature(fn).parameters and "skip_nan" not in inspect.signature(fn).parameters, fn.__name__


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    return {line.split()[-1] for line in nm.stdout.splitlines() if line.split() and line.split()[-2] in "TDBR"}


def test_header_table_and_exports_agree_and_each_kernel_has_one_source():
    from revisionllm_amd import build
    header = open(os.path.join(ROOT, "include", "revision_hip_chain.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(rvc_[a-z0-9_]+)\s*\(", code))
    if not all(os.path.exists(p) for p in [hip.CHAIN_LIB_PATH, hip.EXT_LIB_PATH] + list(hip.LIB_PATHS.values())):
        build.build_library()
    assert declared == set(hip.CHAIN_SIGNATURES) == _exported(hip.CHAIN_LIB_PATH) and MINE <= declared
    assert f"#define RVC_ABI_VERSION {hip.RVC_ABI_VERSION}" in header and hip.RVC_ABI_VERSION == 1
    for name in MINE:
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code).group(1)
        assert len(params.split(",")) == len(hip.CHAIN_SIGNATURES[name][1]), name
    assert len(hip.CHAIN_SIGNATURES["rvc_span_scores_masked"][1]) == 16 and len(hip.CHAIN_SIGNATURES["rvc_span_propose_masked"][1]) == 21
    assert len(hip.SIGNATURES) == 64 and len(hip.EXT_SIGNATURES) == 3                                # no other library gained a symbol
    scores = re.search(r"/\* ---- span scores over the usable frames.*?\*/", header, re.S).group(0)
    for word in ("valid[(r / rpm) * L + t] != 0", "-0 hides", "a NaN in valid does", "sims[r * L + t] == sims[r * L + t]", "never enters any arithmetic",
                 "min(k, n)", "NaN first", "from +0", "skipped, not multiplied by 0", "0x7fc00000", "bit for bit", "rows > 65535", "skip_nan outside {0, 1}",
                 "no global atomics", "no\n * scratch"):
        assert word in scores, word
    propose = re.search(r"/\* ---- span proposals from the usable frames.*?\*/", header, re.S).group(0)
    for word in ("(a) smoothing", "(b) range", "(c) detection", "starting\n *       from the first usable one", "divided by their count", "never above",
                 "counts the hidden frames inside it", "valid = NULL with skip_nan = 0 is rv_span_propose bit for bit", "valid of ones is valid = NULL",
                 "At smooth = 1 the call equals", "At smooth = 1 skip_nan alone changes nothing", "skip_nan outside {0, 1}", "no global atomics", "no scratch"):
        assert word in propose, word
    # one source per kernel: the kernels live in the two headers, the translation units instantiate them
    csrc = os.path.join(ROOT, "revisionllm_amd", "csrc")
    src = {n: open(os.path.join(csrc, n)).read() for n in ("span_scores.h", "span_propose.h", "similarity.hip", "propose.hip", "spans_chain.hip")}
    assert src["span_scores.h"].count("void span_scores_kernel(") == 1 and "template <int MODE, bool MASKED = false>" in src["span_scores.h"]
    assert src["span_propose.h"].count("void span_propose_kernel(") == 1 and "template <bool MASKED = false>" in src["span_propose.h"]
    assert src["span_propose.h"].count("float sp_smooth(") == 1 and "int sat_i32(" not in src["span_scores.h"]
    assert open(os.path.join(csrc, "grounding.h")).read().count("int sat_i32(") == 1                       # (it moved with the window rule, span_slice)
    for helper in ("span_mask_sum", "SPAN_NOT_FINITE", "span_slice", "span_encode"):
        assert_grounding_rule_is_shared(helper, csrc)
    for tu, head in (("similarity.hip", "span_scores.h"), ("propose.hip", "span_propose.h"), ("spans_chain.hip", "span_scores.h"),
                     ("spans_chain.hip", "span_propose.h")):
        assert f'#include "{head}"' in src[tu], (tu, head)
    for tu in ("similarity.hip", "propose.hip", "spans_chain.hip"):
        assert "span_scores_kernel(" not in src[tu] and "span_propose_kernel(" not in src[tu] and "sp_smooth(" not in src[tu], tu
    assert "__global__" not in src["spans_chain.hip"] and "__global__" not in src["propose.hip"]
    assert "spans_chain.hip" in build.CHAIN_SOURCES and "similarity.hip" in build.SOURCES and "propose.hip" in build.SOURCES
    assert {"span_scores.h", "span_propose.h"} <= set(build.HEADERS)


def _refused(rc, message):
    return rc == RV_ERR_ARG and message in hip.chain_last_error()


def test_every_refusal_of_the_score_entry_comes_before_any_launch():
    """Dummy device pointers: a call that got as far as a launch would fault, so a clean RV_ERR_ARG with its message shows the check came first."""
    one = ctypes.c_void_p(64)
    f = hip.chain_lib().rvc_span_scores_masked
    who = "rvc_span_scores_masked: "
    good = dict(sims=one, spans=one, mask=one, valid=one, rows=6, rpm=3, L=100, N=5, mode=0, k=3, temperature=0.01, skip_nan=1, scores=one, windows=one,
                n_usable=one)
    order = list(good)

    def call(**kw):
        a = {**good, **kw}
        return f(*[a[n] for n in order], None)
    for name in ("sims", "spans", "mask", "scores"):
        assert _refused(call(**{name: None}), who + "bad arguments"), name
    for kw in (dict(rows=0), dict(rows=-6), dict(L=0), dict(L=-1), dict(N=0), dict(N=-2)):
        assert _refused(call(**kw), who + "bad arguments"), kw
    for kw in (dict(rpm=0), dict(rpm=-1), dict(rows=7), dict(rows=2, rpm=3), dict(rpm=4)):
        a = {**good, **kw}
        assert _refused(call(**kw), who + "rows=%d with rpm=%d rows per mask row" % (a["rows"], a["rpm"])), kw
    for rows in (65536, 65538 * 3):
        assert _refused(call(rows=rows, rpm=1), who + "at most 65535 rows per launch (rows=%d)" % rows)
    for mode in (-1, 2, 7):
        assert _refused(call(mode=mode), who + "mode=%d must be 0 (top-k) or 1 (attention)" % mode)
    for skip in (-1, 2, 255):
        assert _refused(call(skip_nan=skip), who + "skip_nan=%d must be 0 or 1" % skip)
    for k in (0, -1, 65):
        assert _refused(call(k=k), who + "k=%d must be in [1, 64]" % k)
    for tau in (0.0, -0.0, float("inf"), float("-inf"), float("nan")):
        assert _refused(call(mode=1, temperature=tau), who + "temperature must be finite and not 0"), tau


def test_every_refusal_of_the_proposal_entry_comes_before_any_launch():
    one = ctypes.c_void_p(64)
    f = hip.chain_lib().rvc_span_propose_masked
    who = "rvc_span_propose_masked: "
    table = lambda *v: (ctypes.c_float * len(v))(*v)                                            # noqa: E731
    good = dict(sims=one, mask=one, valid=one, R=6, rpm=3, L=100, levels=table(0.5, 0.7), T=2, relative=1, smooth=3, gap=1, min_len=1, max_len=0, N=16,
                skip_nan=1, spans=one, n_spans=one, n_found=one, windows=one, smoothed=one)
    order = list(good)

    def call(**kw):
        a = {**good, **kw}
        return f(*[a[n] for n in order], None)
    for name in ("sims", "mask", "levels", "spans", "n_spans"):
        assert _refused(call(**{name: None}), who + "bad arguments (a null sims, mask, levels, spans or n_spans)"), name
    for kw in (dict(R=0), dict(R=-3), dict(rpm=0), dict(rpm=-1), dict(R=7), dict(R=2, rpm=3)):
        assert _refused(call(**kw), who + "R=%d rows with rpm=%d" % (kw.get("R", 6), kw.get("rpm", 3))), kw
    for L in (0, -1, 1048577):
        assert _refused(call(L=L), who + "L=%d must be in [1, 1048576]" % L)
    for T in (0, -1, 9):
        assert _refused(call(T=T, levels=table(*[0.1 * i for i in range(9)])), who + "T=%d levels (1 to 8)" % T)
    for relative in (-1, 2):
        assert _refused(call(relative=relative), who + "relative=%d must be 0 or 1" % relative)
    assert _refused(call(levels=table(0.5, float("inf"))), who + "level 1 is not finite")
    assert _refused(call(levels=table(float("nan"), 0.5)), who + "level 0 is not finite")
    assert _refused(call(levels=table(0.5, 0.5)), who + "levels must be strictly ascending (level 1)")
    assert _refused(call(levels=table(0.5, 1.0)), who + "relative level 1 outside [0, 1)")
    assert _refused(call(levels=table(-0.5, 0.5)), who + "relative level 0 outside [0, 1)")
    for smooth in (0, 2, 67, -3):
        assert _refused(call(smooth=smooth), who + "smooth=%d must be odd and in [1, 65]" % smooth)
    for gap in (-1, 64):
        assert _refused(call(gap=gap), who + "gap=%d must be in [0, 63]" % gap)
    for min_len in (0, -1):
        assert _refused(call(min_len=min_len), who + "min_len=%d must be >= 1" % min_len)
    assert _refused(call(max_len=-1), who + "max_len=-1 must be 0 (no limit) or >= min_len=1")
    assert _refused(call(min_len=5, max_len=4), who + "max_len=4 must be 0 (no limit) or >= min_len=5")
    for N in (0, -1, 2049):
        assert _refused(call(N=N), who + "N=%d spans per row (1 to 2048)" % N)
    for skip in (-1, 2, 255):
        assert _refused(call(skip_nan=skip), who + "skip_nan=%d must be 0 or 1" % skip)


def test_python_side_refusals_come_before_the_device_is_looked_for():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import similarity as S
    s, sp, m = torch.zeros(2, 3, 40), torch.zeros(2, 3, 5, 2), torch.ones(2, 40)
    bad_valid = [dict(valid=torch.ones(2, 41)), dict(valid=torch.ones(40)), dict(valid=torch.ones(2, 3, 40)), dict(valid=torch.ones(2, 40, dtype=torch.int64)),
                 dict(valid=torch.ones(2, 40, dtype=torch.complex64)), dict(valid=[[1] * 40] * 2), dict(valid=np.ones((2, 40), np.float32)),
                 dict(skip_nan=2), dict(skip_nan=None), dict(skip_nan="yes"), dict(skip_nan=1.0)]
    score_kw = bad_valid + [dict(pooling="mean"), dict(k=0), dict(k=65), dict(k=1.5), dict(k=True), dict(pooling="attention", temperature=0.0),
                            dict(pooling="attention", temperature=float("inf")), dict(pooling="attention", temperature="hot")]
    for kw in score_kw:
        with pytest.raises(ValueError, match="span_scores_masked"):
            ops.span_scores_masked(s, sp, m, **kw)
    for a in (dict(sims=torch.zeros(40)), dict(sims=torch.zeros(2, 3, 4, 40)), dict(spans=torch.zeros(2, 3, 5, 3)), dict(spans=torch.zeros(2, 5, 2)),
              dict(mask=torch.ones(3, 40)), dict(mask=torch.ones(2, 41)), dict(mask=torch.ones(40)), dict(sims=s.half()), dict(sims=s.long()),
              dict(spans=sp.long()), dict(mask=torch.ones(2, 40, dtype=torch.complex64)), dict(sims=[[0.0] * 40]), dict(sims=torch.zeros(2, 0, 40), spans=torch.zeros(2, 0, 5, 2)),
              dict(sims=torch.zeros(65536, 1), spans=torch.zeros(65536, 1, 2), mask=torch.ones(65536, 1))):
        b = {**dict(sims=s, spans=sp, mask=m), **a}
        with pytest.raises(ValueError, match="span_scores_masked"):
            ops.span_scores_masked(b["sims"], b["spans"], b["mask"])
    with pytest.raises(TypeError):
        ops.span_scores_masked(s, sp, m, torch.ones(2, 40))                           # keyword-only
    out = ops.span_scores_masked_checks("x", s, sp, m, torch.ones(2, 40, dtype=torch.bool), True, 5, "topk", 0.01)
    assert out == ((2, 3), 6, 3, 40, 5, 0, 5, 0.01, 1)
    assert ops.span_scores_masked_checks("x", s[0], sp[0], torch.ones(3, 40), None, 0, 3, "attention", 1)[1:] == (3, 1, 40, 5, 1, 1, 1.0, 0)
    propose_kw = bad_valid + [dict(levels=()), dict(levels=(0.5, 0.5)), dict(levels=(0.5, 1.0)), dict(relative=2), dict(smooth=2), dict(smooth=67), dict(gap=64),
                              dict(gap=-1), dict(min_len=0), dict(max_len=0), dict(min_len=5, max_len=4), dict(max_spans=0), dict(max_spans=2049)]
    for kw in propose_kw:
        with pytest.raises(ValueError, match="span_propose_masked"):
            ops.span_propose_masked(s, m, **kw)
        with pytest.raises(ValueError, match="propose_spans_masked"):
            S.propose_spans_masked(s, m, **kw)
    for a in (dict(sims=torch.zeros(40)), dict(mask=torch.ones(2, 41)), dict(mask=torch.ones(4, 40)), dict(sims=s.long()), dict(sims=[[0.0] * 40]),
              dict(mask=torch.ones(2, 40, dtype=torch.complex64)), dict(sims=torch.zeros(2, 0, 40))):
        b = {**dict(sims=s, mask=m), **a}
        with pytest.raises(ValueError, match="span_propose_masked"):
            ops.span_propose_masked(b["sims"], b["mask"])
    with pytest.raises(ValueError, match="span_propose_masked: sims must be float32"):
        ops.span_propose_masked(s.half(), m)
    with pytest.raises(TypeError):
        ops.span_propose_masked(s, m, torch.ones(2, 40))                              # keyword-only
    text, video, prop = torch.zeros(2, 3, 8), torch.zeros(2, 40, 8), torch.zeros(2, 3, 5, 2)
    for kw in score_kw:
        with pytest.raises(ValueError, match="forward_clip_matching_masked"):
            S.forward_clip_matching_masked(text, video, m, prop, **kw)
        with pytest.raises(ValueError, match="forward_clip_matching_masked"):
            S.forward_clip_matching_masked(text[:, 0], video, m, prop[:, 0], **kw)
    for a in (dict(text=torch.zeros(2, 3, 9)), dict(text=torch.zeros(3, 8)), dict(video=torch.zeros(2, 40)), dict(mask=torch.ones(2, 39)), dict(text=text.long()),
              dict(proposal=torch.zeros(2, 5, 2)), dict(proposal=torch.zeros(2, 3, 5, 3)), dict(mask=torch.ones(2, 40, dtype=torch.complex64)), dict(video=[0.0])):
        b = {**dict(text=text, video=video, mask=m, proposal=prop), **a}
        with pytest.raises(ValueError, match="forward_clip_matching_masked"):
            S.forward_clip_matching_masked(b["text"], b["video"], b["mask"], b["proposal"])
    with pytest.raises(TypeError, match="forward_clip_matching_masked"):
        S.forward_clip_matching_masked(text, video, m, None)
    for kw in bad_valid + [dict(top=0), dict(nms_iou=-1.0), dict(pooling="mean"), dict(k=0), dict(pooling="attention", temperature=0.0), dict(smooth=2),
                           dict(gap=64), dict(max_spans=0), dict(gt=torch.zeros(2, 2)), dict(hit_iou=(0.5,) * 17)]:
        with pytest.raises(ValueError, match="ground_queries_masked"):
            S.ground_queries_masked(text, video, m, **kw)
    with pytest.raises(TypeError, match="ground_queries_masked"):
        S.ground_queries_masked(text, video, m, window=3)
    for a in (dict(text=torch.zeros(2, 3, 9)), dict(video=torch.zeros(2, 40)), dict(mask=torch.ones(2, 39)), dict(text=text.long()), dict(text=None)):
        b = {**dict(text=text, video=video, mask=m), **a}
        with pytest.raises(ValueError, match="ground_queries_masked"):
            S.ground_queries_masked(b["text"], b["video"], b["mask"])
    if not torch.cuda.is_available():                                                  # past the refusals there is the device path only
        for call in (lambda: S.ground_queries_masked(text, video, m, valid=torch.ones(2, 40), skip_nan=True),
                     lambda: S.forward_clip_matching_masked(text, video, m, prop, skip_nan=True), lambda: S.propose_spans_masked(s, m, valid=m.bool())):
            with pytest.raises(hip.HipLibraryError, match="HIP device path only"):
                call()


# ------------------------------------------------------------------ the oracle ------------------------------------------------------------------
VALUES = np.array([0.0, -0.0, 0.25, 0.5, 0.5, 1.0, -1.0, np.nan, np.inf, -0.75, 0.75], dtype=F)


def _random_row(rng, case):
    L = int(rng.integers(1, 40))
    D = int(rng.integers(0, L + 1))
    row = rng.choice(VALUES, size=L) if case % 3 else rng.normal(size=L).astype(F)
    mask = (np.arange(L) < D).astype(F)
    valid = None if case % 4 == 0 else (rng.random(L) < (0.3 if case % 4 == 1 else 0.75)).astype(F)
    return row.astype(F), mask, valid, L, D


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=F).view(np.uint32), np.ascontiguousarray(b, dtype=F).view(np.uint32))


def test_oracle_proposals_against_brute_force():
    rng = np.random.default_rng(23)
    hidden_rows = 0
    for case in range(240):
        row, mask, valid, L, D = _random_row(rng, case)
        skip = case % 2
        relative = (case // 2) % 2
        levels = (0.3, 0.5, 0.8) if relative else (0.2, 0.5)
        smooth, gap = int(rng.choice([1, 3, 5, 9])), int(rng.choice([0, 1, 2, 5]))
        min_len = int(rng.choice([1, 2, 4]))
        max_len = int(rng.choice([0, min_len, 12]))
        max_len = max_len if max_len == 0 or max_len >= min_len else 0
        runs, sp, _, D2 = MO.row_runs(row, mask, valid, skip, levels, relative, smooth, gap, min_len, max_len)
        assert D2 == D and runs == MO.brute(row, mask, valid, skip, levels, relative, smooth, gap, min_len, max_len), (case, L, D, smooth, gap)
        u = MO.usable(row[:D], None if valid is None else valid[:D], skip)
        assert np.array_equal(np.isnan(sp), ~u | np.isnan(sp)) and np.isnan(sp[~u]).all()             # a hidden frame's s' is NaN
        assert all(u[lo] and u[hi - 1] for lo, hi in runs)                                              # a run starts and ends on a usable frame
        hidden_rows += bool(D and not u.all())
    assert hidden_rows > 100


def test_oracle_identities_of_the_proposal_rule():
    rng = np.random.default_rng(29)
    for case in range(120):
        row, mask, valid, L, D = _random_row(rng, case)
        relative = case % 2
        levels = LEVELS if relative else (0.1, 0.4, 0.6)
        gap, smooth = int(rng.choice([0, 1, 3])), int(rng.choice([1, 3, 7]))
        kw = dict(relative=relative, gap=gap, min_len=1, max_len=0, N=8)
        plain = PO.propose(row[None], mask[None], levels, smooth=smooth, **kw)

        def same(a, b):
            assert _same_bits(a["spans"], b["spans"]) and np.array_equal(a["windows"], b["windows"]), case
            assert np.array_equal(a["n_spans"], b["n_spans"]) and np.array_equal(a["n_found"], b["n_found"]) and a["D"] == b["D"], case
            assert all(_same_bits(x, y) for x, y in zip(a["smoothed"], b["smoothed"])), case
        # valid = None, skip_nan = 0 is the unmasked rule; valid of ones is valid = None
        same(MO.propose(row[None], mask[None], levels, smooth=smooth, **kw), plain)
        same(MO.propose(row[None], mask[None], levels, valid=np.ones((1, L), F), smooth=smooth, **kw), plain)
        same(MO.propose(row[None], mask[None], levels, valid=np.full((1, L), np.nan, F), smooth=smooth, **kw), plain)       # a NaN in valid hides nothing
        # smooth = 1: the unmasked rule on sims with NaN over the hidden frames, in every output
        if valid is not None:
            over = row.copy()
            over[valid == 0] = np.nan
            for skip in (0, 1):
                same(MO.propose(row[None], mask[None], levels, valid=valid[None], skip_nan=skip, smooth=1, **kw), PO.propose(over[None], mask[None], levels, smooth=1, **kw))
        # smooth = 1: skip_nan alone changes nothing
        same(MO.propose(row[None], mask[None], levels, skip_nan=1, smooth=1, **kw), PO.propose(row[None], mask[None], levels, smooth=1, **kw))
    # -0 hides a frame
    out = MO.propose(np.array([[0.9, 0.9, 0.9, 0.1]], F), np.ones((1, 4), F), (0.5,), valid=np.array([[1, -0.0, 1, 1]], F), relative=0)
    assert out["windows"][0, :2].tolist() == [[0, 1], [2, 3]] and out["n_found"].tolist() == [2]
    # gap closes a hidden frame; the run's length counts it
    out = MO.propose(np.array([[0.9, 0.9, 0.9, 0.1]], F), np.ones((1, 4), F), (0.5,), valid=np.array([[1, 0, 1, 1]], F), relative=0, gap=1, min_len=3)
    assert out["windows"][0, 0].tolist() == [0, 3] and out["n_found"].tolist() == [1]
    # smoothing: the divisor is the usable count, the sum starts at the first usable frame (-0 stays -0)
    sp = MO.smooth_row(np.array([1.0, 100.0, 4.0, -0.0, 7.0], F), np.array([1, 0, 1, 1, 0], bool), 5, 3)
    assert _same_bits(sp[[0, 2, 3]], np.array([1.0, 2.0, 2.0], F)) and np.isnan(sp[[1, 4]]).all()
    assert _same_bits(MO.smooth_row(np.array([5.0, -0.0, 5.0], F), np.array([0, 1, 0], bool), 3, 3)[1:2], np.array([-0.0], F))
    # no usable frame: no span
    out = MO.propose(np.array([[0.9, 0.8]], F), np.ones((1, 2), F), LEVELS, valid=np.zeros((1, 2), F))
    assert out["n_found"].tolist() == [0] and out["n_spans"].tolist() == [0] and np.isnan(out["smoothed"][0]).all()


def test_oracle_scores_against_the_unmasked_oracle_on_masked_fill():
    """A window with at least k usable frames: the k best usable frames are the k best of the row with -inf over the hidden ones, so the masked top-k sum
    is similarity_oracle's on ``masked_fill(-inf)`` (float64 there: exact for these dyadic values).  With fewer than k the -inf shows, which is why
    ``masked_fill`` is no substitute."""
    rng = np.random.default_rng(31)
    dyadic = np.array([0.0, 0.25, 0.5, 0.75, 1.0, -0.5, 0.125, 0.625], dtype=F)
    seen = short = 0
    for case in range(60):
        L = int(rng.integers(4, 60))
        D = int(rng.integers(1, L + 1))
        sims = rng.choice(dyadic, size=(2, L)).astype(F)
        mask = np.repeat((np.arange(L) < D).astype(F)[None], 2, 0)
        valid = (rng.random((2, L)) < 0.6).astype(F)
        spans = MO.fixed_spans(2, 12, case)
        for k in (1, 3):
            got = MO.span_scores(sims, spans, mask, valid=valid, mode=MO.TOPK, k=k)
            filled = torch.from_numpy(sims).masked_fill(torch.from_numpy(valid) == 0, float("-inf"))
            ref = SO.span_scores64(filled, torch.from_numpy(got["windows"]), "topk", k=k).numpy()
            assert np.array_equal(got["windows"], SO.windows(torch.from_numpy(spans), torch.from_numpy(mask)).numpy())
            enough = got["n_usable"] >= k
            assert np.array_equal(got["scores"][enough].astype(np.float64), ref[enough]), (case, k)
            few = (got["n_usable"] < k) & (got["windows"][..., 1] - got["windows"][..., 0] >= k) & (got["windows"][..., 0] >= 0)
            assert np.isinf(ref[few]).all() and np.isfinite(got["scores"][few & (got["n_usable"] > 0)]).all()
            assert np.isnan(got["scores"][few & (got["n_usable"] == 0)]).all()
            seen += int(enough.sum())
            short += int(few.sum())
    assert seen > 500 and short > 50
    # the unmasked identity, both modes; skip_nan; the void and the empty span
    sims = MO.bumpy(3, 50, 1)
    sims[:, 7] = np.nan
    mask, spans = MO.durations(50, [50, 49, 1]), MO.fixed_spans(3, 12, 7)
    win = SO.windows(torch.from_numpy(spans), torch.from_numpy(mask))
    for mode, pooling in ((MO.TOPK, "topk"), (MO.ATTENTION, "attention")):
        got = MO.span_scores(sims, spans, mask, mode=mode, k=3, temperature=1.0)
        ref = SO.span_scores64(torch.from_numpy(sims), win, pooling, k=3, temperature=1.0).numpy()
        assert np.array_equal(np.isnan(got["scores"]), np.isnan(ref)) and MO.rel_err(got["scores"], ref) < 1e-6
        skipped = MO.span_scores(sims, spans, mask, skip_nan=1, mode=mode, k=3, temperature=1.0)
        inside = (win[..., 0] <= 7) & (win[..., 1] > 7)
        assert np.isnan(got["scores"][inside.numpy()]).all() and not np.isnan(skipped["scores"][inside.numpy()]).any()
        assert np.array_equal(skipped["n_usable"][inside.numpy()], (win[..., 1] - win[..., 0]).numpy()[inside.numpy()] - 1)
    assert np.isnan(got["scores"][:, 4]).all() and (got["windows"][:, 4] == -1).all() and (got["n_usable"][:, 4] == 0).all()          # (nan, 0.1)
    assert got["windows"][0, 3].tolist() == [25, 25] and got["scores"][0, 3] == 0 and got["n_usable"][0, 3] == 0                     # (0.5, 0.0) at D = 50: empty


def test_the_f32_attention_statement_against_float64(capsys):
    """The float32 statement's own distance from float64 on the inputs the GPU module uses, per temperature: the GPU bound is 4 times it (the factor pays
    for another summation order over the lanes).  Printed, and logged when RV_LOG_ERR names a file."""
    worst = {}
    for tau in (0.01, 1.0):
        for name, sims, spans, mask, valid, skip in MO.attention_cases():
            a = MO.span_scores(sims, spans, mask, valid=valid, skip_nan=skip, mode=MO.ATTENTION, temperature=tau)["scores"]
            b = MO.span_scores(sims, spans, mask, valid=valid, skip_nan=skip, mode=MO.ATTENTION, temperature=tau, f64=True)["scores"]
            assert np.array_equal(np.isnan(a), np.isnan(b)), (name, tau)
            worst[tau] = max(worst.get(tau, 0.0), MO.rel_err(a, b))
    with capsys.disabled():
        for tau, e in worst.items():
            line = f"  spans_masked attention tau{tau} float32 statement vs float64 rel {e:.3e} (GPU bound {4 * e:.3e})"
            print(line)
            if os.environ.get("RV_LOG_ERR"):
                with open(os.environ["RV_LOG_ERR"], "a") as fh:
                    fh.write(line + "\n")
    assert all(0 < e < 1e-5 for e in worst.values()), worst                           # float32 arithmetic: a few units of 2^-24 per operation
