"""The joint between the coarse and the fine half of the grounding chain, on the host: the package surface of ``rvc_windows_valid``,
``rvc_span_scores_masked_rows`` and ``rvc_span_propose_masked_rows`` (names under both module names, signatures, the chain library's header, ctypes
table and exports held to each other with the new names among them, every refusal of the three C entries before a launch, every Python-side refusal
before a device is looked for) - these fail without the feature.  The rest guards the oracle of tests/windows_valid_oracle.py, which the GPU tests
compare the kernel with: it is held to a brute-force set union, and its windows to ``stage2.cut_windows`` / ``stage1.cut_windows``.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import frames_select_oracle as FO
import windows_valid_oracle as VO
from revisionllm_amd import hip
from revisionllm_amd.eval import stage1, stage2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_ERR_ARG = -1              # include/revision_hip.h: rv_status
MINE = {"rvc_windows_valid", "rvc_span_scores_masked_rows", "rvc_span_propose_masked_rows"}
F = np.float32


# ------------------------------------------------------------------ surface ------------------------------------------------------------------
def test_the_names_import_from_both_module_names():
    from revisionllm_amd import grounding, ops
    from revisionllm_amd.eval import similarity
    for name in ("windows_valid", "WindowsValid", "span_scores_masked_rows", "span_propose_masked_rows", "span_rows_valid", "WINDOWS_VALID_MAX_KEEP"):
        assert getattr(ops, name) is getattr(grounding, name), name
    assert ops.windows_valid.__module__ == "revisionllm_amd.grounding" and ops.WindowsValid._fields == ("valid", "n_valid")
    assert similarity.WindowedGrounding._fields == ("grounding", "selection", "valid", "n_valid")
    for name in ("windows_valid", "ground_queries_in_windows"):
        assert callable(getattr(similarity, name)), name
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
import revisionllm_amd.ops as real_ops
import revisionllm_amd.eval.similarity as real_similarity
from revisionllm.ops import windows_valid, span_scores_masked_rows, span_propose_masked_rows, WindowsValid
from revisionllm.eval.similarity import ground_queries_in_windows, WindowedGrounding
import revisionllm.eval.similarity as new_similarity
import vtimellm.ops as old_ops
import vtimellm.eval.similarity as old_similarity
assert windows_valid is real_ops.windows_valid is old_ops.windows_valid and WindowsValid is real_ops.WindowsValid
assert span_scores_masked_rows is real_ops.span_scores_masked_rows is old_ops.span_scores_masked_rows
assert span_propose_masked_rows is real_ops.span_propose_masked_rows is old_ops.span_propose_masked_rows
assert ground_queries_in_windows is real_similarity.ground_queries_in_windows is old_similarity.ground_queries_in_windows
assert new_similarity.windows_valid is real_similarity.windows_valid is old_similarity.windows_valid
assert WindowedGrounding is old_similarity.WindowedGrounding
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
    E = inspect.Parameter.empty
    want = dict(rule=E, win=E, stride=None, frames="all", num_frames=None, valid=None, return_count=False)
    for fn in (ops.windows_valid, similarity.windows_valid):
        p = inspect.signature(fn).parameters
        assert list(p)[:2] == ["select", "mask"] and all(p[n].kind is not K for n in list(p)[:2]) and keywords(fn) == want, fn
    assert keywords(ops.span_scores_masked_rows) == {**keywords(ops.span_scores_masked), "valid": E}
    assert list(inspect.signature(ops.span_scores_masked_rows).parameters) == list(inspect.signature(ops.span_scores_masked).parameters)
    assert keywords(ops.span_propose_masked_rows) == {**keywords(ops.span_propose_masked), "valid": E}
    assert list(inspect.signature(ops.span_propose_masked_rows).parameters) == list(inspect.signature(ops.span_propose_masked).parameters)
    g = inspect.signature(similarity.ground_queries_in_windows).parameters
    assert list(g)[:3] == ["text", "video", "mask"] and g["propose_keywords"].kind is inspect.Parameter.VAR_KEYWORD
    assert keywords(similarity.ground_queries_in_windows) == dict(
        rule=E, win=E, stride=None, select=None, keep=None, frames="all", num_frames=None, select_k=3, min_sep=1, valid=None, skip_nan=False, top=10,
        nms_iou=0.5, k=3, pooling="topk", temperature=0.01, gt=None, hit_iou=ops.HIT_IOU)
    # no existing function gained a keyword
    gm = inspect.signature(similarity.ground_queries_masked).parameters
    assert list(gm) == ["text", "video", "mask", "valid", "skip_nan", "top", "nms_iou", "k", "pooling", "temperature", "gt", "hit_iou", "propose_keywords"]
    for fn in (ops.span_scores_masked, ops.span_propose_masked, ops.window_select_frames, similarity.select_windows_frames, similarity.ground_queries):
        assert not {"rpv", "select", "rows"} & set(inspect.signature(fn).parameters), fn.__name__


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    return {line.split()[-1] for line in nm.stdout.splitlines() if line.split() and line.split()[-2] in "TDBR"}


def test_header_table_and_exports_agree():
    from revisionllm_amd import build
    header = open(os.path.join(ROOT, "include", "revision_hip_chain.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(rvc_[a-z0-9_]+)\s*\(", code))
    if not all(os.path.exists(p) for p in [hip.CHAIN_LIB_PATH, hip.EXT_LIB_PATH] + list(hip.LIB_PATHS.values())):
        build.build_library()
    assert declared == set(hip.CHAIN_SIGNATURES) == _exported(hip.CHAIN_LIB_PATH) and MINE <= declared
    assert f"#define RVC_ABI_VERSION {hip.RVC_ABI_VERSION}" in header and hip.RVC_ABI_VERSION == 1
    params = {}
    for name in declared:
        params[name] = [p.split()[-1].lstrip("*") for p in re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code).group(1).split(",") if p.strip() != "void"]
        assert len(params[name]) == len(hip.CHAIN_SIGNATURES[name][1]), name
    assert params["rvc_windows_valid"] == ["select", "mask", "valid_in", "R", "rpm", "L", "rule", "win", "stride", "frames", "F", "keep", "valid", "n_valid",
                                           "stream"]
    # the _rows entries: the arguments of the entries without _rows, with rpv directly behind valid
    for base in ("rvc_span_scores_masked", "rvc_span_propose_masked"):
        at = params[base].index("valid") + 1
        assert params[base + "_rows"] == params[base][:at] + ["rpv"] + params[base][at:], base
        a, b = hip.CHAIN_SIGNATURES[base][1], hip.CHAIN_SIGNATURES[base + "_rows"][1]
        assert b == a[:at] + [ctypes.c_int32] + a[at:], base
    assert len(hip.SIGNATURES) == 64 and len(hip.EXT_SIGNATURES) == 3                                # no other library gained a symbol
    rule = re.search(r"/\* ---- a window selection becomes a validity row.*?\*/", header, re.S).group(0)
    for word in ("EVERY element", "uninitialised memory", "ws_count", "ws_bounds_clipped", "void windows are no windows", "np.linspace(lo, hi - 1, F, dtype=int32)",
                 "names nothing and is ignored", "Order and duplicates do not matter", "t < D", "-0 hides a frame", "a NaN in valid_in does not",
                 "read only at frames a named window covers", "keep outside [1, 2048]", "vector stores only, no atomics, no scratch"):
        assert word in rule, word
    rows = re.search(r"/\* ---- the two masked span entries with a validity row per ROW.*?\*/", header, re.S).group(0)
    for word in ("valid[(r / rpv) * L + t]", "stays row (r / rpm)", "with rpv = rpm every output equals", "With rpv = 1 on a [B,Q,L] layout", "rpv < 1\n",
                 "rows not a multiple of rpv"):
        assert word in rows, word
    csrc = os.path.join(ROOT, "revisionllm_amd", "csrc")
    src = {n: open(os.path.join(csrc, n)).read() for n in ("span_scores.h", "span_propose.h", "spans_chain.hip", "valid_chain.hip")}
    assert "valid_chain.hip" in build.CHAIN_SOURCES and src["valid_chain.hip"].count("__global__") == 1
    assert src["span_scores.h"].count("mk.rpv") == 1 and src["span_propose.h"].count("a.rpv") == 1                   # one place each
    assert src["span_scores.h"].count("void span_scores_kernel(") == 1 and src["span_propose.h"].count("void span_propose_kernel(") == 1
    assert "template <int RULE, int FRAMES>" in src["valid_chain.hip"] and "atomic" not in src["valid_chain.hip"].split("#include")[1]
    for fn in ("block_mask_sum<WS_TPB>", "duration_frames(", "ws_rule_count<RULE>", "ws_rule_bounds<RULE>", "ws_frame_at<FRAMES>"):
        assert fn in src["valid_chain.hip"], fn                                                       # the selection's own code, not a copy


def _refused(rc, message):
    return rc == RV_ERR_ARG and message in hip.chain_last_error()


def test_every_refusal_of_the_validity_entry_comes_before_any_launch():
    """Dummy device pointers: a call that got as far as a launch would fault, so a clean RV_ERR_ARG with its message shows the check came first."""
    one = ctypes.c_void_p(64)
    f = hip.chain_lib().rvc_windows_valid
    who = "rvc_windows_valid: "
    good = dict(select=one, mask=one, valid_in=one, R=6, rpm=3, L=100, rule=0, win=20, stride=5, frames=0, F=0, keep=4, valid=one, n_valid=one)
    order = list(good)

    def call(**kw):
        a = {**good, **kw}
        return f(*[a[n] for n in order], None)
    for name in ("select", "mask", "valid"):
        assert _refused(call(**{name: None}), who + "bad arguments (a null select, mask or valid)"), name
    for kw in (dict(R=0), dict(R=-3), dict(rpm=0), dict(rpm=-1), dict(R=7), dict(R=2, rpm=3)):
        assert _refused(call(**kw), who + "R=%d rows with rpm=%d" % (kw.get("R", 6), kw.get("rpm", 3))), kw
    for L in (0, -1, 1048577):
        assert _refused(call(L=L), who + "L=%d must be in [1, 1048576]" % L)
    for rule in (-1, 2):
        assert _refused(call(rule=rule), who + "rule=%d" % rule)
    for frames in (-1, 2):
        assert _refused(call(frames=frames), who + "frames=%d" % frames)
    for stride in (1, 3, 5):
        assert _refused(call(rule=1, stride=stride), who + "stride=%d with the clipped rule" % stride)
    for kw in (dict(stride=0), dict(stride=-2), dict(win=4), dict(win=0), dict(win=101), dict(rule=1, stride=2, win=1)):
        a = {**good, **kw}
        assert _refused(call(**kw), who + "win=%d frames with stride=%d" % (a["win"], a["stride"])), kw
    for F_ in (0, -1, 1025):
        assert _refused(call(frames=1, F=F_), who + "F=%d sampled frames per window must be in [1, 1024]" % F_)
    for F_ in (1, -1, 250):
        assert _refused(call(frames=0, F=F_), who + "F=%d with every frame of a window (F = 0)" % F_)
    for keep in (0, -1, 2049):
        assert _refused(call(keep=keep), who + "keep=%d entries per row must be in [1, 2048]" % keep)


def test_every_refusal_of_the_rows_entries_comes_before_any_launch():
    one = ctypes.c_void_p(64)
    lib = hip.chain_lib()
    table = lambda *v: (ctypes.c_float * len(v))(*v)                                            # noqa: E731
    who = "rvc_span_scores_masked_rows: "
    good = dict(sims=one, spans=one, mask=one, valid=one, rpv=1, rows=6, rpm=3, L=100, N=5, mode=0, k=3, temperature=0.01, skip_nan=1, scores=one, windows=one,
                n_usable=one)
    order = list(good)

    def call(**kw):
        a = {**good, **kw}
        return lib.rvc_span_scores_masked_rows(*[a[n] for n in order], None)
    for kw in (dict(rpv=0), dict(rpv=-1), dict(rpv=4), dict(rpv=5), dict(rows=3, rpv=2)):
        a = {**good, **kw}
        assert _refused(call(**kw), who + "rows=%d with rpv=%d rows per validity row" % (a["rows"], a["rpv"])), kw
    for name in ("sims", "spans", "mask", "scores"):
        assert _refused(call(**{name: None}), who + "bad arguments"), name
    for kw in (dict(rows=0), dict(L=0), dict(N=0), dict(N=-2)):
        assert _refused(call(**kw), who + "bad arguments"), kw
    for kw in (dict(rpm=0), dict(rpm=-1), dict(rows=7), dict(rpm=4)):
        a = {**good, **kw}
        assert _refused(call(**kw), who + "rows=%d with rpm=%d rows per mask row" % (a["rows"], a["rpm"])), kw
    assert _refused(call(rows=65536, rpm=1), who + "at most 65535 rows per launch (rows=65536)")
    for mode in (-1, 2):
        assert _refused(call(mode=mode), who + "mode=%d must be 0 (top-k) or 1 (attention)" % mode)
    for skip in (-1, 2):
        assert _refused(call(skip_nan=skip), who + "skip_nan=%d must be 0 or 1" % skip)
    for k in (0, 65):
        assert _refused(call(k=k), who + "k=%d must be in [1, 64]" % k)
    for tau in (0.0, float("inf"), float("nan")):
        assert _refused(call(mode=1, temperature=tau), who + "temperature must be finite and not 0"), tau

    who = "rvc_span_propose_masked_rows: "
    good = dict(sims=one, mask=one, valid=one, rpv=1, R=6, rpm=3, L=100, levels=table(0.5, 0.7), T=2, relative=1, smooth=3, gap=1, min_len=1, max_len=0, N=16,
                skip_nan=1, spans=one, n_spans=one, n_found=one, windows=one, smoothed=one)
    order = list(good)

    def call(**kw):                                                                            # noqa: F811
        a = {**good, **kw}
        return lib.rvc_span_propose_masked_rows(*[a[n] for n in order], None)
    for kw in (dict(rpv=0), dict(rpv=-1), dict(rpv=4), dict(R=3, rpv=2)):
        a = {**good, **kw}
        assert _refused(call(**kw), who + "R=%d rows with rpv=%d rows per validity row" % (a["R"], a["rpv"])), kw
    for name in ("sims", "mask", "levels", "spans", "n_spans"):
        assert _refused(call(**{name: None}), who + "bad arguments (a null sims, mask, levels, spans or n_spans)"), name
    for kw in (dict(R=0), dict(rpm=0), dict(R=7)):
        assert _refused(call(**kw), who + "R=%d rows with rpm=%d" % (kw.get("R", 6), kw.get("rpm", 3))), kw
    assert _refused(call(L=1048577), who + "L=1048577 must be in [1, 1048576]")
    assert _refused(call(T=9), who + "T=9 levels (1 to 8)")
    assert _refused(call(relative=2), who + "relative=2 must be 0 or 1")
    assert _refused(call(levels=table(0.5, 0.5)), who + "levels must be strictly ascending (level 1)")
    assert _refused(call(smooth=2), who + "smooth=2 must be odd and in [1, 65]")
    assert _refused(call(gap=64), who + "gap=64 must be in [0, 63]")
    assert _refused(call(min_len=0), who + "min_len=0 must be >= 1")
    assert _refused(call(min_len=5, max_len=4), who + "max_len=4 must be 0 (no limit) or >= min_len=5")
    assert _refused(call(N=2049), who + "N=2049 spans per row (1 to 2048)")
    assert _refused(call(skip_nan=2), who + "skip_nan=2 must be 0 or 1")
    # the entries without _rows keep their texts
    assert lib.rvc_span_scores_masked(one, one, one, one, 7, 3, 100, 5, 0, 3, 0.01, 1, one, one, one, None) == RV_ERR_ARG
    assert "rvc_span_scores_masked: rows=7 with rpm=3 rows per mask row (rpm >= 1, rows a multiple of rpm)" == hip.chain_last_error()
    assert lib.rvc_span_propose_masked(one, one, one, 6, 3, 100, table(0.5), 1, 1, 3, 1, 1, 0, 16, 2, one, one, one, one, one, None) == RV_ERR_ARG
    assert "rvc_span_propose_masked: skip_nan=2 must be 0 or 1" == hip.chain_last_error()


def test_python_side_refusals_come_before_the_device_is_looked_for():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import similarity as S
    sel, m = torch.zeros(2, 3, 4, dtype=torch.int32), torch.ones(2, 40)
    geometry = dict(rule="shifted", win=10, stride=5)
    bad = [dict(rule="other"), dict(rule=0), dict(win=0), dict(win=41), dict(stride=None), dict(stride=11), dict(rule="clipped", stride=3), dict(frames="some"),
           dict(frames="sampled"), dict(frames="sampled", num_frames=0), dict(frames="sampled", num_frames=1025), dict(num_frames=3),
           dict(valid=torch.ones(2, 41)), dict(valid=torch.ones(2, 3, 40)), dict(valid=torch.ones(2, 40, dtype=torch.int64)), dict(valid=[[1] * 40] * 2)]
    for kw in bad:
        for fn, name in ((ops.windows_valid, "windows_valid"), (S.windows_valid, "windows_valid")):
            with pytest.raises(ValueError, match=name):
                fn(sel, m, **{**geometry, **kw})
    for kw in (dict(return_count=2), dict(return_count="yes")):
        with pytest.raises(ValueError, match="windows_valid"):
            ops.windows_valid(sel, m, **geometry, **kw)
    for a in (dict(select=sel.long()), dict(select=sel.float()), dict(select=torch.zeros(4, dtype=torch.int32)), dict(select=torch.zeros(3, 3, 4, dtype=torch.int32)),
              dict(select=torch.zeros(3, 4, dtype=torch.int32)), dict(select=torch.zeros(2, 3, 0, dtype=torch.int32)), dict(select=torch.zeros(2, 2049, dtype=torch.int32)),
              dict(select=[[0]]), dict(mask=torch.ones(40)), dict(mask=torch.ones(2, 40, dtype=torch.complex64)), dict(mask=None)):
        b = {**dict(select=sel, mask=m), **a}
        with pytest.raises(ValueError, match="windows_valid"):
            ops.windows_valid(b["select"], b["mask"], **geometry)
    with pytest.raises(TypeError):
        ops.windows_valid(sel, m, "shifted", 10, 5)                                   # keyword-only
    s, sp = torch.zeros(2, 3, 40), torch.zeros(2, 3, 5, 2)
    ok = torch.ones(2, 3, 40)
    bad_valid = [torch.ones(2, 40), torch.ones(2, 3, 41), torch.ones(6, 40), torch.ones(2, 3, 40, dtype=torch.int64), [[1] * 40] * 6, None,
                 np.ones((2, 3, 40), np.float32)]
    for v in bad_valid:
        with pytest.raises(ValueError, match="span_scores_masked_rows"):
            ops.span_scores_masked_rows(s, sp, m, valid=v)
        with pytest.raises(ValueError, match="span_propose_masked_rows"):
            ops.span_propose_masked_rows(s, m, valid=v)
    with pytest.raises(TypeError):
        ops.span_scores_masked_rows(s, sp, m)                                          # valid is required
    with pytest.raises(TypeError):
        ops.span_propose_masked_rows(s, m)
    for kw in (dict(skip_nan=2), dict(pooling="mean"), dict(k=0), dict(k=65), dict(pooling="attention", temperature=0.0)):
        with pytest.raises(ValueError, match="span_scores_masked_rows"):
            ops.span_scores_masked_rows(s, sp, m, valid=ok, **kw)
    for a in (dict(sims=s.half()), dict(spans=torch.zeros(2, 3, 5, 3)), dict(mask=torch.ones(3, 40))):
        b = {**dict(sims=s, spans=sp, mask=m), **a}
        with pytest.raises(ValueError, match="span_scores_masked_rows"):
            ops.span_scores_masked_rows(b["sims"], b["spans"], b["mask"], valid=ok)
    for kw in (dict(skip_nan=2), dict(levels=()), dict(smooth=2), dict(gap=64), dict(min_len=0), dict(max_spans=2049)):
        with pytest.raises(ValueError, match="span_propose_masked_rows"):
            ops.span_propose_masked_rows(s, m, valid=ok, **kw)
    with pytest.raises(ValueError, match="span_propose_masked_rows: sims must be float32"):
        ops.span_propose_masked_rows(s.half(), m, valid=ok.half())


def test_ground_queries_in_windows_refusals():
    from revisionllm_amd.eval import similarity as S
    text, video, m = torch.zeros(2, 3, 8), torch.zeros(2, 40, 8), torch.ones(2, 40)
    sel = torch.zeros(2, 3, 4, dtype=torch.int32)
    geometry = dict(rule="shifted", win=10, stride=5)
    with pytest.raises(ValueError, match="ground_queries_in_windows: exactly one of select"):
        S.ground_queries_in_windows(text, video, m, **geometry)
    with pytest.raises(ValueError, match="ground_queries_in_windows: exactly one of select"):
        S.ground_queries_in_windows(text, video, m, select=sel, keep=3, **geometry)
    with pytest.raises(TypeError, match="ground_queries_in_windows"):
        S.ground_queries_in_windows(text, video, m, select=sel, window=3, **geometry)
    with pytest.raises(TypeError, match="ground_queries_in_windows"):
        S.ground_queries_in_windows(text, video, m, keep=3, return_bounds=True, **geometry)
    with pytest.raises(TypeError):
        S.ground_queries_in_windows(text, video, m, select=sel)                        # rule and win are required
    for kw in (dict(select=sel.long()), dict(select=sel[:, 0]), dict(select=sel[:1]), dict(select=[[0]]), dict(select=torch.zeros(2, 3, 0, dtype=torch.int32)),
               dict(select=torch.zeros(2, 3, 2049, dtype=torch.int32)), dict(keep=0), dict(keep=1.5), dict(keep=3, select_k=65), dict(keep=3, min_sep=0),
               dict(keep=3, min_sep=100), dict(select=sel, win=41), dict(keep=3, win=41), dict(select=sel, rule="other"), dict(select=sel, stride=None),
               dict(select=sel, frames="sampled"), dict(select=sel, num_frames=4), dict(select=sel, valid=torch.ones(2, 3, 40)), dict(select=sel, skip_nan=2),
               dict(select=sel, top=0), dict(select=sel, nms_iou=-1.0), dict(select=sel, pooling="mean"), dict(select=sel, k=0), dict(select=sel, smooth=2),
               dict(select=sel, max_spans=0), dict(select=sel, gt=torch.zeros(2, 2)), dict(select=sel, hit_iou=(0.5,) * 17)):
        with pytest.raises(ValueError, match="ground_queries_in_windows"):
            S.ground_queries_in_windows(text, video, m, **{**geometry, **kw})
    for a in (dict(text=torch.zeros(2, 3, 9)), dict(video=torch.zeros(2, 40)), dict(mask=torch.ones(2, 39)), dict(text=text.long())):
        b = {**dict(text=text, video=video, mask=m), **a}
        with pytest.raises(ValueError, match="ground_queries_in_windows"):
            S.ground_queries_in_windows(b["text"], b["video"], b["mask"], select=sel, **geometry)
    if not torch.cuda.is_available():                                                  # past the refusals there is the device path only
        for call in (lambda: S.ground_queries_in_windows(text, video, m, select=sel, **geometry),
                     lambda: S.ground_queries_in_windows(text[:, 0], video, m, keep=3, rule="clipped", win=10, frames="sampled", num_frames=4),
                     lambda: S.windows_valid(sel, m, **geometry)):
            with pytest.raises(hip.HipLibraryError, match="HIP device path only"):
                call()


# ------------------------------------------------------------------ the oracle ------------------------------------------------------------------
def test_oracle_against_brute_force():
    rng = np.random.default_rng(41)
    named = ignored = hidden = 0
    for case in range(300):
        L = int(rng.integers(1, 60))
        rule = case % 2
        stride = 2 if rule else int(rng.choice([1, 2, 3, 5]))
        win = int(rng.integers(stride, max(stride, min(L, 14)) + 1))
        if win > L:
            continue
        frames = (case // 2) % 2
        nf = int(rng.choice([1, 2, 3, 7, 40])) if frames else 0
        R, rpm, keep = 4, 2, int(rng.integers(1, 7))
        Ds = rng.integers(0, L + 1, R // rpm)
        mask = (np.arange(L)[None, :] < Ds[:, None]).astype(F)
        cap = FO.capacity(L, win, stride)
        select = rng.integers(-2, cap + 2, (R, keep)).astype(np.int32)
        valid_in = None if case % 3 == 0 else rng.choice(np.array([0.0, -0.0, 1.0, np.nan, 2.0], F), (R // rpm, L))
        out = VO.windows_valid(select, mask, rule, win, stride, frames, nf, valid_in)
        for r in range(R):
            D = int(Ds[r // rpm])
            assert out["D"][r] == D
            covered = VO.brute_covered(select[r], D, rule, win, stride, frames, nf)
            assert all(0 <= t < D for t in covered)
            want = np.zeros(L, F)
            for t in covered:
                if valid_in is None or not (valid_in[r // rpm, t] == 0):
                    want[t] = 1
                else:
                    hidden += 1
            assert np.array_equal(out["valid"][r].view(np.uint32), want.view(np.uint32)), (case, r)
            assert out["n_valid"][r] == int(want.sum())
            named += int(((select[r] >= 0) & (select[r] < out["W"][r])).sum())
            ignored += int(((select[r] < 0) | (select[r] >= out["W"][r])).sum())
    assert named > 500 and ignored > 500 and hidden > 200
    # -0 hides, NaN does not; a frame behind D stays 0 whatever names it; +0 bits everywhere else
    out = VO.windows_valid([[0, 0, -1]], np.array([[1, 1, 1, 1, 1, 1, 0, 0]], F), 0, 4, 2, 0, 0, np.array([[1, -0.0, np.nan, 0, 2, 1, 1, 1]], F))
    assert out["valid"].tolist() == [[1, 0, 1, 0, 1, 0, 0, 0]] and out["n_valid"].tolist() == [3] and not np.signbit(out["valid"]).any()


def test_oracle_windows_are_cut_windows():
    """The oracle's windows (through tests/frames_select_oracle.py) against both ``cut_windows`` at the drivers' geometry (125 s x 5 fps, 250 frames),
    at a win / stride that does not divide, and at the clipped rule's void case (win 5, D 15): naming every index of ``cut_windows``' range covers
    exactly the frames of its non-void windows."""
    for dw, fps, stride, nf, lengths in ((125, 5, 5, 250, (626, 1873, 3000)), (10, 1, 3, 4, (11, 23, 40)), (7, 1, 2, 3, (8, 15, 29))):
        win = dw * fps
        for ctx_l in lengths:
            times, idx = stage2.cut_windows(ctx_l, dw, fps, stride, nf)
            mask = np.ones((1, ctx_l), F)
            every = np.arange(len(times) + 2, dtype=np.int32)[None] - 1
            for frames, n in ((VO.ALL, 0), (VO.SAMPLED, nf)):
                out = VO.windows_valid(every, mask, VO.SHIFTED, win, stride, frames, n)
                want = set()
                for i, (s, e) in enumerate(times):
                    want |= set(idx[i].tolist()) if frames else set(range(max(s, 0), e + 1))
                assert out["W"] == [len(times)] and set(np.flatnonzero(out["valid"][0]).tolist()) == want, (win, stride, ctx_l, frames)
            for i in (0, len(times) - 1):
                one = VO.windows_valid([[i]], mask, VO.SHIFTED, win, stride, VO.SAMPLED, nf)
                assert set(np.flatnonzero(one["valid"][0]).tolist()) == set(idx[i].tolist())
    for dw, fps, nf, lengths in ((125, 5, 250, (626, 1873, 3000)), (5, 1, 3, (14, 15, 16, 17)), (4, 1, 2, (9, 10))):
        win = dw * fps
        for ctx_l in lengths:
            count = max(0, -(-ctx_l // (win // 2)) - 1)
            bounds = [((i * win) // 2, min((i * win) // 2 + win, ctx_l - 1)) for i in range(count)]
            solid = [(s, e) for s, e in bounds if s <= e]
            if len(solid) == count:
                idx = stage1.cut_windows(ctx_l, dw, fps, nf)                      # (a void window makes the host's linspace run backwards: not compared)
                assert idx.shape[0] == count
            mask = np.ones((1, ctx_l), F)
            every = np.arange(count + 1, dtype=np.int32)[None]
            out = VO.windows_valid(every, mask, VO.CLIPPED, win, 2, VO.ALL, 0)
            want = set()
            for s, e in solid:
                want |= set(range(s, e + 1))
            assert out["W"] == [len(solid)] and set(np.flatnonzero(out["valid"][0]).tolist()) == want, (win, ctx_l)
            if len(solid) == count:
                out = VO.windows_valid(every, mask, VO.CLIPPED, win, 2, VO.SAMPLED, nf)
                assert set(np.flatnonzero(out["valid"][0]).tolist()) == set(idx.ravel().tolist()), (win, ctx_l)
    # win 5, D 15: window 6 would start at frame 15 - void, so naming it names nothing; at D 16 it is the one-frame window [15, 16)
    assert VO.windows_valid([[6]], np.ones((1, 15), F), VO.CLIPPED, 5, 2, VO.ALL, 0)["n_valid"].tolist() == [0]
    assert VO.windows_valid([[6]], np.ones((1, 15), F), VO.CLIPPED, 5, 2, VO.ALL, 0)["W"] == [6]
    assert np.flatnonzero(VO.windows_valid([[6]], np.ones((1, 16), F), VO.CLIPPED, 5, 2, VO.ALL, 0)["valid"][0]).tolist() == [15]
