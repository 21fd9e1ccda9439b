"""The stage-1 driver's device route on the host: the package surface of ``rv_window_gather_rule`` and ``rv_proposal_cosine`` (names under both module
names, signatures, header, ctypes table, exports.map, both libraries, every refusal of the two C entries before a launch, every Python-side refusal
before a device is looked for), ``stage1.proposal_cosines``' way back to the per-proposal route and the driver's ``--device_features`` flag with the
device stages stubbed - these fail without the feature.  The rest guards the oracle of tests/stage1_oracle.py, which the GPU tests compare the kernels
with: its windows and frames are held to ``stage1.cut_windows`` and its slice rule to Python's.  No GPU."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import stage1_oracle as SO
from revisionllm_amd import hip
from revisionllm_amd.eval import stage1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_ERR_ARG = -1              # include/revision_hip.h: rv_status


# ------------------------------------------------------------------ surface ------------------------------------------------------------------
def test_the_names_import_from_both_module_names():
    from revisionllm_amd import grounding, ops
    from revisionllm_amd.data import feature_store
    for name in ("window_gather_clipped", "proposal_cosine", "proposal_slice", "clipped_window_count", "clipped_window_void"):
        assert getattr(ops, name) is getattr(grounding, name) and getattr(grounding, name).__module__ == "revisionllm_amd.grounding", name
    assert (hip.RV_WINDOWS_SHIFTED, hip.RV_WINDOWS_CLIPPED) == (0, 1)
    for name in ("gather_windows", "proposal_cosines", "score_query_device", "run_query_device", "score_query", "run_query"):
        assert callable(getattr(stage1, name)), name
    assert callable(feature_store.WindowStager.stage_resident_clipped)
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
import revisionllm_amd.ops as real_ops
import revisionllm_amd.eval.stage1 as real_stage1
import revisionllm_amd.data.feature_store as real_store
from revisionllm.ops import window_gather_clipped, proposal_cosine
from revisionllm.eval.stage1 import gather_windows, proposal_cosines, score_query_device
from revisionllm.data.feature_store import WindowStager
import vtimellm.ops as old_ops
import vtimellm.eval.stage1 as old_stage1
assert window_gather_clipped is real_ops.window_gather_clipped is old_ops.window_gather_clipped
assert proposal_cosine is real_ops.proposal_cosine is old_ops.proposal_cosine
assert gather_windows is real_stage1.gather_windows is old_stage1.gather_windows
assert proposal_cosines is real_stage1.proposal_cosines and score_query_device is old_stage1.score_query_device
assert WindowStager.stage_resident_clipped is real_store.WindowStager.stage_resident_clipped
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_signatures():
    from revisionllm_amd import ops
    from revisionllm_amd.data import feature_store
    from revisionllm_amd.eval import eval_nlq_negative as drv
    p = inspect.signature(ops.window_gather_clipped).parameters
    optional = dict(select=None, mask=None, out_dtype=None, return_index=False)
    assert list(p) == ["video", "win", "num_frames"] + list(optional)
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(p)[1:])
    assert all(p[n].default is inspect.Parameter.empty for n in ("win", "num_frames")) and {n: p[n].default for n in optional} == optional
    c = inspect.signature(ops.proposal_cosine).parameters
    assert list(c) == ["windows", "text", "proposals", "k"] and c["k"].kind is inspect.Parameter.KEYWORD_ONLY and c["k"].default is inspect.Parameter.empty
    g = inspect.signature(stage1.gather_windows).parameters
    geometry = dict(debug_window=125, feature_fps=5, num_frames=250, dtype=None)
    assert list(g) == ["features_dev"] + list(geometry) and {n: g[n].default for n in geometry} == geometry
    assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for q in list(g.values())[1:])
    assert list(inspect.signature(stage1.proposal_cosines).parameters) == ["features", "frames", "query_cls", "topk_pool"]
    assert str(inspect.signature(stage1.score_query_device)) == str(inspect.signature(stage1.score_query))
    assert str(inspect.signature(stage1.run_query_device)) == str(inspect.signature(stage1.run_query))
    s = inspect.signature(feature_store.WindowStager.stage_resident_clipped).parameters
    assert list(s)[:2] == ["self", "features_dev"] and list(s.values())[2].kind is inspect.Parameter.VAR_KEYWORD
    args = drv.parse_args([])
    assert args.device_features is False and args.device_features_mb == 2048
    args = drv.parse_args(["--device_features", "--device_features_mb", "64"])
    assert args.device_features is True and args.device_features_mb == 64


def test_entries_in_header_ctypes_table_exports_and_both_libraries():
    from revisionllm_amd import build
    header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    declared = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", header))
    assert "#define RV_ABI_VERSION 5" in header and "#define RV_WINDOWS_SHIFTED 0" in header and "#define RV_WINDOWS_CLIPPED 1" in header
    if not all(os.path.exists(p) for p in hip.LIB_PATHS.values()):
        build.build_library()
    assert declared == set(hip.SIGNATURES) and len(hip.SIGNATURES) == 64
    exports = open(os.path.join(ROOT, "revisionllm_amd", "csrc", "exports.map")).read()
    for name, n_args in (("rv_window_gather_rule", 18), ("rv_proposal_cosine", 11)):
        assert name in declared and name in exports
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, header).group(1)
        assert len(params.split(",")) == len(hip.SIGNATURES[name][1]) == n_args, name
        for flavour, path in hip.LIB_PATHS.items():
            assert hasattr(ctypes.CDLL(path), name), (flavour, name)
    assert "global: rv_*;" in exports
    for flavour in hip.LIB_PATHS:
        assert hip.lib(flavour).rv_abi_version() == 5
    comment = re.search(r"/\* ---- the stage-1 driver on the device.*?\*/", header, re.S).group(0)
    for word in ("word for word", "NOT shifted back", "0, 312, 625, 937", "VOID", "D = 15 for win = 5", "195625", "NULL", "stride must be 2"):
        assert word in comment, word
    comment = re.search(r"/\* The cosine score of P ragged proposals.*?\*/", header, re.S).group(0)
    for word in ("0x7fc00000", "BIT FOR BIT", "min(b + 1, T)", "T <= 7936", "torch.topk", "DEVICE memory", "nothing of feat is read"):
        assert word in comment, word
    gather = open(os.path.join(ROOT, "revisionllm_amd", "csrc", "gather.hip")).read()
    shared = open(os.path.join(ROOT, "revisionllm_amd", "csrc", "grounding.h")).read()
    sample = open(os.path.join(ROOT, "revisionllm_amd", "csrc", "sample.hip")).read()
    assert "ws_bounds_clipped(" in gather and "ws_bounds_clipped(" in shared and "ws_count(a.win, a.stride, D)" in gather
    for body in ("topk_cosine_vector<T>(", "topk_cosine_generic<T>("):                             # one body, called by both entries' kernels
        assert sample.count(body) >= 2, body


# ------------------------------------------------------------------ refusals ------------------------------------------------------------------
def _refused(rc, message):
    return rc == RV_ERR_ARG and message in hip.last_error()


def test_every_refusal_of_rv_window_gather_rule_comes_before_any_launch():
    """Dummy device pointers: a call that got as far as a launch would fault, so a clean RV_ERR_ARG with its message shows the check came first."""
    one = ctypes.c_void_p(64)
    for flavour in hip.LIB_PATHS:
        f = hip.lib(flavour).rv_window_gather_rule
        own, other = (hip.RV_F16, hip.RV_BF16) if flavour == "f16" else (hip.RV_BF16, hip.RV_F16)
        name16 = "fp16" if flavour == "f16" else "bf16"
        good = dict(video=one, video_dtype=hip.RV_F32, ldv=16, mask=one, select=one, R=6, rpm=3, L=100, d=16, win=10, stride=2, keep=4, F=7, out=one,
                    out_dtype=own, frame_idx=one, rule=1)

        def call(**kw):
            a = {**good, **kw}
            return f(a["video"], a["video_dtype"], a["ldv"], a["mask"], a["select"], a["R"], a["rpm"], a["L"], a["d"], a["win"], a["stride"], a["keep"],
                     a["F"], a["out"], a["out_dtype"], a["frame_idx"], a["rule"], None)
        for name in ("video", "out"):
            assert _refused(call(**{name: None}), "rv_window_gather_rule: bad arguments"), (flavour, name)
        for rule in (2, -1, 7):
            assert _refused(call(rule=rule), "rv_window_gather_rule: rule=%d" % rule)
        for stride in (1, 3, 5, 10):
            assert _refused(call(stride=stride), "rv_window_gather_rule: stride=%d with the clipped rule" % stride)
        for kw in (dict(R=0), dict(R=-3), dict(rpm=0), dict(rpm=-1), dict(R=7), dict(R=2, rpm=3)):
            assert _refused(call(**kw), "rv_window_gather_rule: R=%d rows with rpm=%d" % (kw.get("R", 6), kw.get("rpm", 3))), kw
        for L in (0, -1, 1048577):
            assert _refused(call(L=L), "rv_window_gather_rule: L=%d must be in [1, 1048576]" % L)
        for kw in (dict(d=0), dict(d=-1), dict(ldv=15), dict(ldv=0), dict(ldv=-16)):
            assert _refused(call(**kw), "rv_window_gather_rule: d=%d columns with a frame stride of ldv=%d" % (kw.get("d", 16), kw.get("ldv", 16))), kw
        for kw in (dict(stride=0), dict(stride=-1), dict(win=1), dict(win=0), dict(win=101), dict(win=4, stride=5, rule=0), dict(win=200, stride=100, rule=0)):
            assert _refused(call(**kw), "rv_window_gather_rule: win=%d frames with stride=%d" % (kw.get("win", 10), kw.get("stride", 2))), kw
        for keep in (0, -1):
            assert _refused(call(keep=keep), "rv_window_gather_rule: keep=%d must be at least 1" % keep)
        for F in (0, -1, 65537):
            assert _refused(call(F=F), "rv_window_gather_rule: F=%d must be in [1, 65536]" % F)
        for dt in (other, hip.RV_I32, hip.RV_U8, -1, 6):
            assert _refused(call(video_dtype=dt), "rv_window_gather_rule: video_dtype must be f32 or " + name16), dt
            assert _refused(call(out_dtype=dt), "rv_window_gather_rule: out_dtype must be f32 or " + name16), dt
        assert _refused(call(R=2 ** 24, rpm=1, keep=1), "rv_window_gather_rule: R=16777216 rows of keep=1 entries")
        assert _refused(call(R=4096, rpm=1, keep=4096, rule=0, stride=5), "rv_window_gather_rule: R=4096 rows of keep=4096 entries")
        # rv_window_gather keeps its own texts, the null select among them
        g = hip.lib(flavour).rv_window_gather
        assert _refused(g(one, hip.RV_F32, 16, one, None, 6, 3, 100, 16, 10, 5, 4, 7, one, own, one, None), "rv_window_gather: bad arguments (a null video, select")


def test_every_refusal_of_rv_proposal_cosine_comes_before_any_launch():
    one = ctypes.c_void_p(64)
    for flavour in hip.LIB_PATHS:
        f = hip.lib(flavour).rv_proposal_cosine
        own, other = (hip.RV_F16, hip.RV_BF16) if flavour == "f16" else (hip.RV_BF16, hip.RV_F16)
        good = dict(feat=one, dtype=own, q=one, props=one, P=3, W=5, T=12, d=16, k=3, out=one)

        def call(**kw):
            a = {**good, **kw}
            return f(a["feat"], a["dtype"], a["q"], a["props"], a["P"], a["W"], a["T"], a["d"], a["k"], a["out"], None)
        for name in ("feat", "q", "props", "out"):
            assert _refused(call(**{name: None}), "rv_proposal_cosine: bad arguments"), (flavour, name)
        for kw in (dict(P=0), dict(P=-1), dict(W=0), dict(W=-2), dict(T=0), dict(T=-1), dict(d=0), dict(d=-8)):
            a = {**good, **kw}
            assert _refused(call(**kw), "rv_proposal_cosine: P=%d proposals in W=%d windows of T=%d frames and d=%d columns" % (a["P"], a["W"], a["T"], a["d"])), kw
        for dt in (other, hip.RV_I32, hip.RV_U8, -1, 6):
            assert _refused(call(dtype=dt), "rv_proposal_cosine: dtype must be f32 or " + ("fp16" if flavour == "f16" else "bf16")), dt
        # rv_topk_cosine's LDS bound at T: d = 770 has no 16-byte form for 16-bit features, 5 * 770 + T floats must fit 64 KB
        assert _refused(call(d=770, T=16384 - 5 * 770 + 1), "rv_proposal_cosine: 5*d + T too large for LDS")
        assert _refused(call(d=768, T=16384 - 5 * 768 + 1), "rv_proposal_cosine: 5*d + T too large for LDS")
        assert _refused(call(dtype=hip.RV_F32, d=3, T=16384), "rv_proposal_cosine: 5*d + T too large for LDS")


def test_python_side_refusals_come_before_the_device_is_looked_for():
    from revisionllm_amd import ops
    v, s = torch.zeros(2, 40, 8), torch.zeros(2, 3, 4, dtype=torch.int32)
    good = dict(win=10, num_frames=7)
    keywords = [dict(win=0), dict(win=1), dict(win=-5), dict(win=10.0), dict(win=None), dict(win=True), dict(win=41), dict(num_frames=0), dict(num_frames=-1),
                dict(num_frames=2.5), dict(num_frames=None), dict(num_frames=65537), dict(win=2 ** 31), dict(out_dtype=torch.int32), dict(out_dtype="f16"),
                dict(out_dtype=torch.float64), dict(mask=torch.ones(2, 41)), dict(mask=torch.ones(40)), dict(mask=torch.ones(2, 40, dtype=torch.complex64)),
                dict(mask=[[1.0] * 40] * 2), dict(select=torch.zeros((), dtype=torch.int32)), dict(select=torch.zeros(1, 2, 3, 4, dtype=torch.int32)),
                dict(select=torch.zeros(2, 3, 0, dtype=torch.int32)), dict(select=torch.zeros(3, 4, dtype=torch.int32)),
                dict(select=torch.zeros(2, 3, 4, dtype=torch.int64)), dict(select=torch.zeros(2, 3, 4)), dict(select=[[0, 1]])]
    for kw in keywords:
        with pytest.raises(ValueError, match="window_gather_clipped"):
            ops.window_gather_clipped(v, **{**good, "select": s, **kw})
    for video in (torch.zeros(40), torch.zeros(2, 2, 40, 8), torch.zeros(2, 40, 8, dtype=torch.int64), torch.zeros(2, 40, 8, dtype=torch.float64),
                  torch.zeros(2, 0, 8), np.zeros((2, 40, 8), np.float32)):
        with pytest.raises(ValueError, match="window_gather_clipped"):
            ops.window_gather_clipped(video, **good)
    with pytest.raises(ValueError, match="no cross-type 16-bit conversion"):
        ops.window_gather_clipped(v.half(), out_dtype=torch.bfloat16, **good)
    with pytest.raises(ValueError, match="at most 1048576"):
        ops.window_gather_clipped(torch.zeros(1048577, 1), **good)
    with pytest.raises(TypeError):
        ops.window_gather_clipped(v, 10, 7)                                        # keyword-only
    with pytest.raises(TypeError):
        ops.window_gather_clipped(v, win=10)                                       # num_frames has no default
    assert [ops.clipped_window_count(D, 10) for D in (0, 1, 5, 6, 10, 11, 100)] == [0, 0, 0, 1, 1, 2, 19]
    assert ops.clipped_window_void(15, 5) and not ops.clipped_window_void(14, 5) and not ops.clipped_window_void(15, 4)
    assert ops.clipped_window_void(195625, 625) and not any(ops.clipped_window_void(D, 625) for D in range(1, 40000))
    w, t = torch.zeros(5, 12, 16), torch.zeros(16)
    props = torch.zeros(3, 3, dtype=torch.int32)
    for kw in (dict(k=1.0), dict(k=None), dict(k=True), dict(k=2 ** 31), dict(windows=torch.zeros(12, 16)), dict(windows=torch.zeros(5, 0, 16)),
               dict(windows=np.zeros((5, 12, 16), np.float32)), dict(windows=torch.zeros(5, 12, 16, dtype=torch.float64)), dict(windows=torch.zeros(5, 12, 16, dtype=torch.int32)),
               dict(text=torch.zeros(15)), dict(text=torch.zeros(1, 16)), dict(text=np.zeros(16, np.float32)), dict(text=torch.zeros(16, dtype=torch.int64)),
               dict(proposals=torch.zeros(3, 2, dtype=torch.int32)), dict(proposals=torch.zeros(3, 3, dtype=torch.int64)), dict(proposals=torch.zeros(9, dtype=torch.int32)),
               dict(proposals=[(0, 1)]), dict(proposals=[(0, 1, 2.0)]), dict(proposals=[(0, 1, 2 ** 31)]), dict(proposals=[(0, 1, True)]), dict(proposals=7),
               dict(proposals=[3, 4, 5])):
        a = {**dict(windows=w, text=t, proposals=props, k=3), **kw}
        with pytest.raises(ValueError, match="proposal_cosine"):
            ops.proposal_cosine(a["windows"], a["text"], a["proposals"], k=a["k"])
    with pytest.raises(TypeError):
        ops.proposal_cosine(w, t, props, 3)                                        # keyword-only
    with pytest.raises(TypeError):
        ops.proposal_cosine(w, t, props)                                           # k has no default
    assert ops.proposal_cosine(w, t, [], k=3).shape == (0,)                        # nothing to score: no launch, no device
    f = torch.zeros(700, 8)
    for kw in (dict(debug_window=125, feature_fps=4.5), dict(debug_window=0.5, feature_fps=5), dict(debug_window=0), dict(debug_window=-1), dict(debug_window=1, feature_fps=1),
               dict(feature_fps=float("nan")), dict(debug_window="a", feature_fps=1)):
        with pytest.raises(ValueError, match="stage1.gather_windows"):
            stage1.gather_windows(f, **kw)
    for a in (np.zeros((700, 8), np.float32), torch.zeros(700), torch.zeros(700, 8, dtype=torch.int64), torch.zeros(0, 8)):
        with pytest.raises(ValueError, match="stage1.gather_windows"):
            stage1.gather_windows(a)
    for a, kw in ((torch.zeros(624, 8), {}), (torch.zeros(15, 8), dict(debug_window=1, feature_fps=5))):     # shorter than a window; a void last window
        with pytest.raises(ValueError, match="take the host route"):
            stage1.gather_windows(a, **kw)
    with pytest.raises(TypeError):
        stage1.gather_windows(f, 125)                                              # keyword-only


# ------------------------------------------------------------------ the oracle ------------------------------------------------------------------
def test_oracle_windows_are_cut_windows():
    """Every ctx_l from 1 to 2999 at the driver's geometry and F = 250, and five small windows at five frame counts: the oracle's [W, F] table is
    ``stage1.cut_windows``' (which builds a row for a void window from a descending linspace: those rows are left out, the oracle marks them -1)."""
    for ctx_l in range(1, 3000):
        idx = stage1.cut_windows(ctx_l, 125, 5, 250)
        got = SO.frame_indices(ctx_l, 625, 250)
        assert got.shape == idx.shape and np.array_equal(got, idx), ctx_l
        assert got.shape[0] == SO.window_count(ctx_l, 625) and (got.size == 0 or (0 <= got.min() and got.max() < ctx_l))
    voids = 0
    for win in (2, 3, 4, 5, 61):
        for F in (1, 2, 3, 31, 251):
            for ctx_l in range(1, 4 * win + 40):
                idx = stage1.cut_windows(ctx_l, win, 1, F)
                got = SO.frame_indices(ctx_l, win, F)
                assert got.shape == idx.shape, (win, F, ctx_l)
                for i, (s, e) in enumerate(SO.windows(ctx_l, win)):
                    if SO.void(s, e):
                        voids += 1
                        assert (got[i] == -1).all() and win % 2 == 1
                    else:
                        assert np.array_equal(got[i], idx[i]) and 0 <= got[i].min() and got[i].max() < ctx_l, (win, F, ctx_l, i)
    assert voids > 0
    assert [s for s, _ in SO.windows(3000, 625)][:4] == [0, 312, 625, 937]                          # (i * win) // 2, not i * (win // 2)
    assert SO.windows(12, 10) == [(0, 10), (5, 11)] and SO.windows(11, 10)[-1] == (5, 10) and SO.windows(6, 10) == [(0, 5)] and SO.windows(5, 10) == []


def test_void_windows():
    assert SO.windows(15, 5)[-1] == (15, 14) and SO.void(15, 14) and not any(SO.void(s, e) for s, e in SO.windows(14, 5))
    assert not any(SO.void(s, e) for D in range(1, 15) for s, e in SO.windows(D, 5))               # 15 is the first
    for win in range(2, 64, 2):
        for D in range(1, 4001):
            W = SO.window_count(D, win)
            assert W == 0 or ((W - 1) * win) // 2 <= D - 1, (win, D)                               # the last start is the largest
    for win in (624, 626, 1000):
        assert not any(SO.void(*SO.windows(D, win)[-1]) for D in range(win, 4001) if SO.windows(D, win))
    from revisionllm_amd import ops
    for win in (3, 5, 7, 61):
        for D in range(1, 500):
            assert ops.clipped_window_void(D, win) == any(SO.void(s, e) for s, e in SO.windows(D, win)), (win, D)
            assert ops.clipped_window_count(D, win) == SO.window_count(D, win)


def test_slice_rule_is_pythons():
    from revisionllm_amd import ops
    for T in (1, 2, 5, 12):
        for a in range(0, T + 4):
            for b in range(0, T + 4):
                lo, hi = SO.slice_bounds(a, b, T)
                assert (lo, hi) == ops.proposal_slice(a, b, T)
                assert list(range(T)[a:b + 1]) == list(range(lo, max(lo, hi))), (a, b, T)
                assert SO.is_void(0, a, b, 1, T) == (len(range(T)[a:b + 1]) == 0)
    assert SO.is_void(-1, 0, 3, 5, 12) and SO.is_void(5, 0, 3, 5, 12) and SO.is_void(0, -1, 3, 5, 12) and not SO.is_void(4, 11, 11, 5, 12)
    f = torch.arange(24, dtype=torch.float32).view(1, 6, 4) + 1
    q = torch.tensor([1.0, -2.0, 0.5, 3.0])
    n = f[0, 1:4].double()
    sims = (n / n.pow(2).sum(0).sqrt()) @ q.double()
    assert abs(SO.proposal_score(f, q, 0, 1, 3, 2) - float(sims.topk(2).values.sum())) < 1e-12
    assert abs(SO.proposal_score(f, q, 0, 1, 3, 0) - float(sims.mean())) < 1e-12 and np.isnan(SO.proposal_score(f, q, 0, 4, 3, 2))
    assert SO.topk_order(np.array([1.0, np.nan, 3.0, 3.0, np.nan])) == [1, 4, 2, 3, 0]


# ------------------------------------------------------------------ the epilogue ------------------------------------------------------------------
def _host_topk_cosine(feat, q, k=3):
    """``ops.topk_cosine``'s definition in float32 torch on the CPU."""
    out = []
    for f in feat.float():
        sims = f @ (q.float() / f.pow(2).sum(0).sqrt())
        out.append(sims.mean() if k <= 0 else sims.topk(min(k, len(sims))).values.sum())
    return torch.stack(out)


def test_proposal_cosines_takes_one_call_and_goes_back_to_the_loop_on_an_empty_slice(monkeypatch):
    from revisionllm_amd import ops
    calls = []
    feats, q = torch.randn(4, 12, 8, generator=torch.Generator().manual_seed(1)), torch.randn(8, generator=torch.Generator().manual_seed(2))

    def fake_topk_cosine(feat, q_cls, k=3):
        calls.append(("each", tuple(feat.shape), k))
        if feat.shape[1] == 0:
            raise hip.HipLibraryError("rv_topk_cosine failed (status -1): rv_topk_cosine: bad arguments")
        return _host_topk_cosine(feat, q_cls, k)

    def fake_proposal_cosine(windows, text, proposals, *, k):
        calls.append(("one", list(proposals), k))
        return torch.stack([_host_topk_cosine(windows[w][a:b + 1][None], text, k)[0] for w, a, b in proposals])
    monkeypatch.setattr(ops, "topk_cosine", fake_topk_cosine)
    monkeypatch.setattr(ops, "proposal_cosine", fake_proposal_cosine)
    frames = {0: (3, 9), 2: (0, 0), 3: (10, 40)}
    for pool in (True, False):
        del calls[:]
        got = stage1.proposal_cosines(feats, frames, q, pool)
        assert calls == [("one", [(0, 3, 9), (2, 0, 0), (3, 10, 40)], 3 if pool else 0)] and all(isinstance(c, float) for c in got)
        assert got == stage1._proposal_cosines_each(feats, frames, q, pool)
    assert stage1.proposal_cosines(feats, {}, q, True) == []
    for bad in ({0: (3, 9), 1: (12, 14)}, {0: (3, 9), 1: (5, 3)}):                             # a >= T; b < a: Python's slice is empty
        del calls[:]
        with pytest.raises(hip.HipLibraryError, match="rv_topk_cosine"):
            stage1.proposal_cosines(feats, bad, q, True)
        assert [c[0] for c in calls] == ["each", "each"] and calls[1][1][1] == 0                   # the host route, proposal by proposal
    del calls[:]
    with pytest.raises(IndexError):
        stage1.proposal_cosines(feats, {0: (3, 9), 4: (1, 2)}, q, True)                            # a window past W: the host's own IndexError
    assert [c[0] for c in calls] == ["each"]
    answers = ["From 3 to 9.", "Not Present", "From 5 to 5.", "From 23 to 23.", "Between 2 and 30"]
    for kw in (dict(score="mean_entropy", score_merge="multiply"), dict(score="max_entropy", score_merge="add", normalize=False), dict(score="cosine_sim", topk_pool=True)):
        ent = [] if kw["score"] == "cosine_sim" else [0.5, 0.7, 0.2, 0.9, 0.4]
        want = stage1.score_query(feats.repeat(2, 2, 1), answers, ent, q, (10.0, 30.0), 300.0, num_frames=24, **kw)
        got = stage1.score_query_device(feats.repeat(2, 2, 1), answers, ent, q, (10.0, 30.0), 300.0, num_frames=24, **kw)
        assert got == want and len(got[1]["scores"]) == 3


# ------------------------------------------------------------------ the driver's flag ------------------------------------------------------------------
def test_the_driver_writes_the_same_records_with_device_features(tmp_path, monkeypatch):
    """``--device_features`` with the device stages stubbed by host arithmetic: the sequential loop and ``--in_flight 3`` hand the LLM the same window
    tensor and write the same records as the host route; the movie goes through ``ResidentFeatures`` once for its three queries; ``--baseline``,
    ``--plus_baseline`` and a short video keep the host route; with the flag off none of the new calls is made."""
    from revisionllm_amd import ops, sched, serve
    from revisionllm_amd.data import feature_store
    from revisionllm_amd.eval import eval_nlq_negative as drv
    rs = np.random.RandomState(5)
    feat_dir, q_dir = tmp_path / "feats", tmp_path / "qfeats"
    os.makedirs(feat_dir), os.makedirs(q_dir)
    np.save(feat_dir / "movieA.npy", rs.randn(730, 16).astype(np.float16))             # 14 half-overlapping windows of 100 frames
    np.save(feat_dir / "short.npy", rs.randn(300, 16).astype(np.float32))              # a short video: subsampled to num_frames rows, one window
    ann = {}
    for i in range(4):
        ann[f"q{i}"] = {"movie": "short" if i == 3 else "movieA", "sentence": f"Someone opens door number {i}.", "timestamps": [10.0 * i, 10.0 * i + 40],
                        "movie_duration": 15.0 if i == 3 else 146.0}
        np.savez_compressed(q_dir / f"q{i}.npz", token_features=rs.randn(6, 16).astype(np.float32), cls_features=rs.randn(16).astype(np.float32))
    with open(tmp_path / "ann.json", "w") as f:
        json.dump(ann, f)
    routes, scored, uploads = [], [], []

    def host_windows(features, frame_idx):
        return torch.from_numpy(np.asarray(features, dtype=np.float32))[torch.from_numpy(frame_idx.astype(np.int64))]

    class FakeStager:
        op_dtype = torch.float16

        def __init__(self, device, op_dtype=None):
            pass

        def stage_windows(self, features, frame_idx):
            routes.append(("host", len(features)))
            t = host_windows(features, frame_idx)
            return types.SimpleNamespace(wait=lambda: t)

        def stage_resident_clipped(self, features_dev, **geometry):
            assert torch.is_tensor(features_dev) and sorted(geometry) == ["debug_window", "feature_fps", "num_frames"]
            routes.append(("resident", features_dev.shape[0]))
            t = host_windows(features_dev.float().numpy(), stage1.cut_windows(features_dev.shape[0], **geometry))
            return types.SimpleNamespace(wait=lambda: t)

    def crafted(windows):
        """One answer and one entropy statistic per window, made from the tensor itself: another tensor gives another record."""
        texts = ["From 3 to 9.", "Not Present", "From 17 to 17.", "From 0 to 59.", "From 59 to 59.", "Between 30 and 90"]
        digest = [float(w.double().abs().sum()) for w in windows]
        return [texts[(i + int(d)) % len(texts)] for i, d in enumerate(digest)], [1.0 + d % 7.0 for d in digest]

    def fake_topk_cosine(feat, q_cls, k=3):
        scored.append("each")
        return _host_topk_cosine(feat, q_cls, k)

    def fake_proposal_cosine(windows, text, proposals, *, k):
        scored.append("one")
        return torch.stack([_host_topk_cosine(windows[w][a:b + 1][None], text, k)[0] for w, a, b in proposals])

    class FakeInterleaver:
        def __init__(self, servers):
            self.tasks = []

        def add(self, task):
            self.tasks.append(task)
            return task

        def finish(self, task):
            self.tasks.remove(task)
            return task.gen(task)

    class FakeStream:
        def __init__(self, device=None):
            pass

        def wait_stream(self, other):
            pass
    real_upload = feature_store.ResidentFeatures._upload
    monkeypatch.setattr(feature_store.ResidentFeatures, "_upload", lambda self, array: (uploads.append(array.shape), real_upload(self, array))[1])
    monkeypatch.setattr(feature_store, "WindowStager", FakeStager)
    monkeypatch.setattr(stage1, "answer_windows", lambda model, tokenizer, features, *a, **kw: crafted(features))
    monkeypatch.setattr(stage1, "launch_query_steps", lambda model, tokenizer, features, *a, **kw: features)
    monkeypatch.setattr(stage1, "collect_query", lambda model, tokenizer, launched, score: crafted(launched))
    monkeypatch.setattr(ops, "topk_cosine", fake_topk_cosine)
    monkeypatch.setattr(ops, "proposal_cosine", fake_proposal_cosine)
    monkeypatch.setattr(serve, "DecodeServer", lambda *a, **kw: None)
    monkeypatch.setattr(sched, "Interleaver", FakeInterleaver)
    monkeypatch.setattr(sched, "Task", lambda gen, stream, engine, slot: types.SimpleNamespace(gen=gen, cancel=lambda: None))
    monkeypatch.setattr(torch.cuda, "Stream", FakeStream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    base = ["--data_path", str(tmp_path / "ann.json"), "--feat_folder", str(feat_dir), "--q_feat_dir", str(q_dir), "--batch", "4", "--vis_feat_storage", "npy",
            "--debug", "True", "--skip_small_videos", "", "--debug_window", "20", "--num_frames", "60"]
    model = types.SimpleNamespace(device=torch.device("cpu"), engine=types.SimpleNamespace(slot=0))
    records = {}
    modes = {"seq": [], "flight": ["--in_flight", "3"], "baseline": ["--baseline", "True"], "plus": ["--plus_baseline", "True"],
             "plus flight": ["--plus_baseline", "True", "--in_flight", "3"]}
    for mode, flags in modes.items():
        for on in (False, True):
            name = f"{mode} {'on' if on else 'off'}"
            del routes[:], scored[:], uploads[:]
            args = drv.parse_args(base + flags + ["--log_path", str(tmp_path / name)] + (["--device_features"] if on else []))
            assert drv.eval(args, tokenizer=None, model=model) == (4, []), name
            records[name] = [json.loads(line) for line in open(tmp_path / name / "predictions_streaming_0.txt")]
            device = on and mode in ("seq", "flight")
            assert routes == [("resident", 730) if device else ("host", 730)] * 3 + [("host", 60)], (name, routes)
            assert uploads == ([(730, 16)] if device else []), (name, uploads)                 # one upload for the movie's three queries
            assert scored.count("one") == (3 if device else 0) and ("each" in scored or device), (name, scored)
        assert records[f"{mode} on"] == records[f"{mode} off"], mode
    assert records["seq on"] == records["flight on"] and records["seq off"] != records["plus off"] != records["baseline off"]
    recs = records["seq on"]
    assert [r["query_id"] for r in recs] == ["q0", "q1", "q2", "q3"] and [len(r["answer"]) for r in recs] == [14, 14, 14, 1]
    assert all(len(r["info"]["scores"]) == len(r["info"]["iou"]) for r in recs) and sum(len(r["info"]["scores"]) for r in recs) > 6
