"""The stage-1 window pre-filter on the host: the package surface of ``rvx_window_select_clipped`` and the companion library (names under both module
names, signatures, its header, ctypes table and exports with the main library's left as they were, every refusal of the C entry before a launch,
every Python-side refusal before a device is looked for), ``windows_from_retrieval`` against ``merge_stage1_stage2``, ``expand_selected`` and the
driver's ``--clip_prefilter_keep`` / ``--retrieval_path`` with the device stages stubbed by host arithmetic - these fail without the feature.  The
rest guards the oracle of tests/stage1_prefilter_oracle.py, which the GPU tests compare the kernel with: its selection is held to a brute-force
statement and its windows to ``stage1.cut_windows``.  No GPU."""
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

import stage1_prefilter_oracle as PO
import window_oracle as WO
from revisionllm_amd import hip
from revisionllm_amd.eval import metrics, stage1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_ERR_ARG = -1              # include/revision_hip.h: rv_status
NEW_STAGE1 = ("clip_stage_windows", "gather_selected", "windows_from_retrieval", "expand_selected", "score_query_selected", "run_query_selected")


# ------------------------------------------------------------------ surface ------------------------------------------------------------------
def test_the_names_import_from_both_module_names():
    from revisionllm_amd import grounding, ops
    from revisionllm_amd.data import feature_store
    from revisionllm_amd.eval import similarity
    for name in ("window_select_clipped", "clipped_window_solid"):
        assert getattr(ops, name) is getattr(grounding, name) and getattr(grounding, name).__module__ == "revisionllm_amd.grounding", name
    assert callable(similarity.select_windows_clipped) and all(callable(getattr(stage1, n)) for n in NEW_STAGE1)
    assert callable(feature_store.WindowStager.stage_resident_selected)
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
import revisionllm_amd.ops as real_ops
import revisionllm_amd.eval.stage1 as real_stage1
import revisionllm_amd.eval.similarity as real_similarity
from revisionllm.ops import window_select_clipped
from revisionllm.eval.similarity import select_windows_clipped
from revisionllm.eval.stage1 import clip_stage_windows, windows_from_retrieval, expand_selected, score_query_selected, run_query_selected
import vtimellm.ops as old_ops
import vtimellm.eval.stage1 as old_stage1
import vtimellm.eval.similarity as old_similarity
assert window_select_clipped is real_ops.window_select_clipped is old_ops.window_select_clipped
assert select_windows_clipped is real_similarity.select_windows_clipped is old_similarity.select_windows_clipped
assert clip_stage_windows is real_stage1.clip_stage_windows is old_stage1.clip_stage_windows
assert windows_from_retrieval is old_stage1.windows_from_retrieval and expand_selected is old_stage1.expand_selected
assert score_query_selected is old_stage1.score_query_selected and run_query_selected is old_stage1.run_query_selected
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_signatures():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import eval_nlq_negative as drv
    from revisionllm_amd.eval import similarity
    required = ["win", "keep"]
    optional = dict(k=3, min_sep=1, gt=None, return_scores=False, return_bounds=False, return_order=False)
    for fn, lead in ((ops.window_select_clipped, ["sims", "mask"]), (similarity.select_windows_clipped, ["text", "video", "mask"])):
        p = inspect.signature(fn).parameters
        assert list(p) == lead + required + list(optional)
        assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in required + list(optional))
        assert all(p[n].default is inspect.Parameter.empty for n in required) and {n: p[n].default for n in optional} == optional
    g = inspect.signature(stage1.clip_stage_windows).parameters
    keywords = dict(debug_window=125, feature_fps=5, keep=inspect.Parameter.empty, num_frames=250, dtype=None, k=3, min_sep=1)
    assert list(g) == ["features_dev", "query_cls"] + list(keywords) and {n: g[n].default for n in keywords} == keywords
    assert all(g[n].kind is inspect.Parameter.KEYWORD_ONLY for n in keywords)
    assert list(inspect.signature(stage1.windows_from_retrieval).parameters) == ["frames", "n_windows", "buffer"]
    assert list(inspect.signature(stage1.expand_selected).parameters) == ["answers", "ent", "windows", "n_windows"]
    s, d = inspect.signature(stage1.score_query_selected).parameters, inspect.signature(stage1.score_query).parameters
    assert list(s)[:8] == ["features_sel", "windows", "n_windows", "answers_sel", "ent_sel", "query_cls", "timestamps", "duration"]
    assert [(n, s[n].default) for n in list(s)[8:]] == [(n, d[n].default) for n in list(d)[6:]]          # score_query's keywords
    r, q = inspect.signature(stage1.run_query_selected).parameters, inspect.signature(stage1.run_query).parameters
    assert list(r)[:5] == ["model", "tokenizer", "features_sel", "windows", "n_windows"] and list(r)[5:] == list(q)[3:]
    # the existing signatures did not move
    assert list(inspect.signature(ops.window_select).parameters)[:5] == ["sims", "mask", "win", "stride", "keep"]
    assert str(inspect.signature(stage1.score_query_device)) == str(inspect.signature(stage1.score_query))
    args = drv.parse_args([])
    assert args.clip_prefilter_keep == 0 and args.retrieval_path is None
    args = drv.parse_args(["--clip_prefilter_keep", "16", "--retrieval_path", "x"])
    assert args.clip_prefilter_keep == 16 and args.retrieval_path == "x"


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    return {line.split()[-1] for line in nm.stdout.splitlines() if line.split() and line.split()[-2] in "TDBR"}


def test_the_companion_library_holds_the_new_entry_and_the_main_one_is_untouched():
    from revisionllm_amd import build
    ext_header = open(os.path.join(ROOT, "include", "revision_hip_ext.h")).read()
    declared = set(re.findall(r"\b(rvx_[a-z0-9_]+)\s*\(", ext_header))
    assert declared == set(hip.EXT_SIGNATURES) == {"rvx_abi_version", "rvx_last_error", "rvx_window_select_clipped"}
    assert "#define RVX_ABI_VERSION 1" in ext_header
    params = re.search(r"\brvx_window_select_clipped\s*\(([^)]*)\)\s*;", ext_header).group(1)
    assert len(params.split(",")) == len(hip.EXT_SIGNATURES["rvx_window_select_clipped"][1]) == 19
    if not (os.path.exists(hip.EXT_LIB_PATH) and all(os.path.exists(p) for p in hip.LIB_PATHS.values())):
        build.build_library()
    assert os.path.basename(hip.EXT_LIB_PATH) == "librevision_hip_ext.so" == os.path.basename(build.EXT_LIB)
    assert _exported(hip.EXT_LIB_PATH) == declared                            # nothing else, the linked-in rv_* names least of all
    assert hip.ext_lib().rvx_abi_version() == 1
    assert open(os.path.join(ROOT, "revisionllm_amd", "csrc", "exports_ext.map")).read().split() == "{ global: rvx_*; local: *; };".split()
    comment = re.search(r"/\* ---- coarse window selection for the stage-1 driver.*?\*/", ext_header, re.S).group(0)
    for word in ("VOID", "suffix", "no back-shift", "win + 1 frames", "ONE frame", "64-bit intermediate", "NaN first", "bit for bit", "kills nothing",
                 "ascending", "0x7fc00000", "1048576", "both strict", "i * win >= 2 D"):
        assert word in comment, word                                          # the definition stands in the header
    # the main library: header, table and exports as they were
    header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    main = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", header))
    assert main == set(hip.SIGNATURES) and len(hip.SIGNATURES) == 64 and "rvx_" not in header and not any(n.startswith("rvx") for n in hip.SIGNATURES)
    assert "#define RV_ABI_VERSION 5" in header
    exports = open(os.path.join(ROOT, "revisionllm_amd", "csrc", "exports.map")).read()
    assert "global: rv_*;" in exports and "rvx" not in exports
    for flavour, path in hip.LIB_PATHS.items():
        assert _exported(path) == main, flavour
    # one definition of the kernel: both translation units instantiate the header's template
    csrc = os.path.join(ROOT, "revisionllm_amd", "csrc")
    shared, old, new = (open(os.path.join(csrc, n)).read() for n in ("window_select.h", "prefilter.hip", "prefilter_ext.hip"))
    assert shared.count("void window_select_kernel(") == 1 and "template <int RULE>" in shared
    assert "window_select_kernel<RV_WINDOWS_SHIFTED>" in old and "window_select_kernel<RV_WINDOWS_CLIPPED>" in new
    assert "__global__" not in old and "__global__" not in new and '#include "window_select.h"' in old and '#include "window_select.h"' in new


def _refused(rc, message):
    return rc == RV_ERR_ARG and message in hip.ext_last_error()


def test_every_refusal_of_the_entry_comes_before_any_launch():
    """Dummy device pointers: a call that got as far as a launch would fault, so a clean RV_ERR_ARG with its message shows the check came first."""
    one = ctypes.c_void_p(64)
    f = hip.ext_lib().rvx_window_select_clipped
    who = "rvx_window_select_clipped: "
    good = dict(sims=one, mask=one, R=6, rpm=3, L=100, win=10, k=3, keep=4, min_sep=2, Wcap=19, gt=one, select=one, n_select=one, n_windows=one,
                win_scores=one, bounds=one, order=one, hit_rank=one)

    def call(**kw):
        a = {**good, **kw}
        return f(a["sims"], a["mask"], a["R"], a["rpm"], a["L"], a["win"], a["k"], a["keep"], a["min_sep"], a["Wcap"], a["gt"], a["select"], a["n_select"],
                 a["n_windows"], a["win_scores"], a["bounds"], a["order"], a["hit_rank"], None)
    for name in ("sims", "mask", "select", "n_select", "n_windows"):
        assert _refused(call(**{name: None}), who + "bad arguments"), name
    for kw in (dict(R=0), dict(R=-3), dict(rpm=0), dict(rpm=-1), dict(R=7), dict(R=2, rpm=3)):
        assert _refused(call(**kw), who + "R=%d rows with rpm=%d" % (kw.get("R", 6), kw.get("rpm", 3))), kw
    for L in (0, -1, 1048577):
        assert _refused(call(L=L), who + "L=%d must be in [1, 1048576]" % L)
    for win in (1, 0, -2, 101):
        assert _refused(call(win=win), who + "win=%d frames (2 <= win <= L=100)" % win)
    for k in (0, -1, 65):
        assert _refused(call(k=k), who + "k=%d must be in [1, 64]" % k)
    for Wcap in (18, 20, 0, -1):
        assert _refused(call(Wcap=Wcap), who + "Wcap=%d must be max(1, ceil(L / (win / 2)) - 1) = 19" % Wcap)
    assert _refused(call(L=2050, win=2, Wcap=2049, keep=1, min_sep=1), who + "L=2050, win=2 give up to 2049 windows (at most 2048)")
    assert _refused(call(L=2050, win=3, Wcap=2049, keep=1, min_sep=1), who + "L=2050, win=3 give up to 2049 windows")
    for keep in (0, -1, 20):
        assert _refused(call(keep=keep), who + "keep=%d must be in [1, Wcap=19]" % keep)
    for min_sep in (0, -1, 20):
        assert _refused(call(min_sep=min_sep), who + "min_sep=%d must be in [1, Wcap=19]" % min_sep)
    assert _refused(call(gt=None), who + "hit_rank needs gt")
    assert _refused(call(L=4, win=4, Wcap=2, keep=1, min_sep=1), who + "Wcap=2 must be max(1, ceil(L / (win / 2)) - 1) = 1")      # one window
    assert _refused(call(L=2, win=2, Wcap=2, keep=1, min_sep=1), who + "Wcap=2 must be max(1, ceil(L / (win / 2)) - 1) = 1")


def test_python_side_refusals_come_before_the_device_is_looked_for():
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import select_windows_clipped
    s, m = torch.zeros(2, 3, 40), torch.ones(2, 40)
    good = dict(win=10, keep=4)
    keywords = [dict(win=0), dict(win=1), dict(win=-5), dict(win=10.0), dict(win=None), dict(win=True), dict(win=41), dict(keep=0), dict(keep=-1),
                dict(keep=2.5), dict(keep=None), dict(k=0), dict(k=65), dict(k=1.5), dict(min_sep=0), dict(min_sep=8), dict(min_sep=1.0), dict(win=2 ** 31),
                dict(gt=torch.zeros(2, 2)), dict(gt=torch.zeros(2, 3, 2, dtype=torch.int32)), dict(gt=[[0.0, 1.0]] * 6)]
    shapes = [dict(sims=torch.zeros(40)), dict(sims=torch.zeros(2, 3, 4, 40)), dict(mask=torch.ones(40)), dict(mask=torch.ones(2, 41)),
              dict(mask=torch.ones(3, 40)), dict(sims=torch.zeros(2, 3, 40, dtype=torch.int64)), dict(mask=torch.ones(2, 40, dtype=torch.complex64)),
              dict(sims=torch.zeros(2, 0, 40)), dict(sims=torch.zeros(5, 40)), dict(sims=[[0.5] * 40])]
    for kw in keywords:
        with pytest.raises(ValueError, match="window_select_clipped"):
            ops.window_select_clipped(s, m, **{**good, **kw})
    for kw in shapes:
        a = {**dict(sims=s, mask=m), **kw}
        with pytest.raises(ValueError, match="window_select_clipped"):
            ops.window_select_clipped(a["sims"], a["mask"], **good)
    with pytest.raises(ValueError, match="window_select_clipped: sims must be float32"):
        ops.window_select_clipped(s.half(), m, **good)
    with pytest.raises(ValueError, match="at most 2048"):
        ops.window_select_clipped(torch.zeros(1, 2050), torch.ones(1, 2050), win=2, keep=1)
    with pytest.raises(TypeError):
        ops.window_select_clipped(s, m, 10, 4)                                     # keyword-only
    with pytest.raises(TypeError):
        ops.window_select_clipped(s, m, win=10)                                    # keep has no default
    with pytest.raises(TypeError):
        ops.window_select_clipped(s, m, win=10, keep=4, stride=2)                  # the rule has no stride
    text, video = torch.zeros(2, 3, 8), torch.zeros(2, 40, 8)
    for kw in keywords:
        with pytest.raises(ValueError, match="select_windows_clipped"):
            select_windows_clipped(text, video, m, **{**good, **kw})
    for a in (dict(text=torch.zeros(2, 3, 9)), dict(text=torch.zeros(3, 8)), dict(text=torch.zeros(8)), dict(video=torch.zeros(2, 40)),
              dict(mask=torch.ones(2, 39)), dict(text=text.long()), dict(video=video.long()), dict(text=None),
              dict(mask=torch.ones(2, 40, dtype=torch.complex64))):
        b = {**dict(text=text, video=video, mask=m), **a}
        with pytest.raises(ValueError, match="select_windows_clipped"):
            select_windows_clipped(b["text"], b["video"], b["mask"], **good)
    assert [ops.clipped_window_solid(D, 3) for D in (0, 1, 5, 6, 600)] == [0, 0, 4, 4, 400]
    assert [ops.clipped_window_solid(D, 5) for D in (13, 14, 15)] == [6, 6, 6] and ops.clipped_window_solid(3000, 625) == 9


def test_clip_stage_windows_and_gather_selected_refusals():
    f, q = torch.zeros(700, 8), torch.zeros(8)
    for kw in (dict(debug_window=125, feature_fps=4.5), dict(debug_window=0.2, feature_fps=5), dict(debug_window=0), dict(feature_fps=float("nan")),
               dict(keep=0), dict(keep=2.5), dict(keep=None), dict(keep=True)):
        with pytest.raises(ValueError, match="stage1.clip_stage_windows"):
            stage1.clip_stage_windows(f, q, **{**dict(keep=4), **kw})
    for a, b in ((torch.zeros(700), q), (f, torch.zeros(9)), (f, torch.zeros(1, 8)), (f.long(), q), (torch.zeros(0, 8), q), (f.numpy(), q), (f, q.long())):
        with pytest.raises(ValueError, match="stage1.clip_stage_windows"):
            stage1.clip_stage_windows(a, b, keep=4)
    with pytest.raises(ValueError, match="ctx_l=600 frames for windows of 625"):
        stage1.clip_stage_windows(torch.zeros(600, 8), q, keep=4)                   # shorter than one window
    with pytest.raises(ValueError, match="ctx_l=15 frames for windows of 5"):
        stage1.clip_stage_windows(torch.zeros(15, 8), q, debug_window=1, keep=4)    # a void window
    with pytest.raises(TypeError):
        stage1.clip_stage_windows(f, q)                                            # keep has no default
    with pytest.raises(TypeError):
        stage1.clip_stage_windows(f, q, 125, keep=4)                               # keyword-only
    for windows in ([], [-1], [2], [0, 1.5], [True]):
        with pytest.raises(ValueError, match="stage1.gather_selected"):
            stage1.gather_selected(f, windows)                                     # 700 frames: windows 0 and 1
    with pytest.raises(ValueError, match="stage1.gather_selected: ctx_l=600"):
        stage1.gather_selected(torch.zeros(600, 8), [0])


# ------------------------------------------------------------------ the oracle ------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [(125, 5), (2, 1), (3, 1), (4, 1), (5, 1), (61, 1)])
def test_oracle_bounds_are_cut_windows(geometry):
    """The first and the last index of every non-void window of ``stage1.cut_windows``, for every ctx_l below 3000; the void ones are a suffix (the
    oracle asserts it) and are what ``ops.clipped_window_void`` / ``clipped_window_solid`` say."""
    from revisionllm_amd import ops
    dw, fps = geometry
    win = dw * fps
    for ctx_l in range(1, 3000):
        idx = stage1.cut_windows(ctx_l, dw, fps, num_frames=2)                     # (first, last) of every index, void ones included
        wins = np.array(PO.windows(ctx_l, win), dtype=np.int64).reshape(-1, 2)
        n, every = len(wins), idx.shape[0]
        assert every == ops.clipped_window_count(ctx_l, win) and n == ops.clipped_window_solid(ctx_l, win) <= every
        assert np.array_equal(idx[:n, 0], wins[:, 0]) and np.array_equal(idx[:n, 1], wins[:, 1] - 1), (win, ctx_l)
        assert bool((idx[n:, 0] > idx[n:, 1]).all()) and bool((idx[:n, 0] <= idx[:n, 1]).all())              # the rest is void, and nothing else is
        assert n == 0 or (wins[0, 0] == 0 and wins[-1, 1] <= ctx_l and int((wins[:, 1] - wins[:, 0]).max()) <= win + 1)
        assert (n < every) == ops.clipped_window_void(ctx_l, win) and (win % 2 == 1 or n == every)
        assert ctx_l < win or every <= PO.capacity(ctx_l, win)


def test_void_suffixes_and_the_one_frame_window():
    assert PO.all_windows(5, 3) == [(0, 3), (1, 4), (3, 4), (4, 4)] and len(PO.windows(5, 3)) == 4                   # no void window yet
    assert PO.all_windows(6, 3) == [(0, 3), (1, 4), (3, 5), (4, 5), (6, 5)] and PO.windows(6, 3) == [(0, 4), (1, 5), (3, 6), (4, 6)]
    assert PO.all_windows(15, 5)[-1] == (15, 14) and len(PO.all_windows(15, 5)) == 7 and PO.windows(15, 5)[-1] == (12, 15) and len(PO.windows(15, 5)) == 6
    assert all(len(PO.windows(D, 5)) == len(PO.all_windows(D, 5)) for D in range(1, 15))                             # 15 is the first for win = 5
    assert all(len(PO.windows(D, 3)) == len(PO.all_windows(D, 3)) for D in range(1, 6))                              # 6 is the first for win = 3
    assert PO.all_windows(13, 5)[-1] == (12, 12) and PO.windows(13, 5)[-1] == (12, 13)                               # one frame: s == e
    assert len(PO.all_windows(600, 3)) == 599 and len(PO.windows(600, 3)) == 400                                     # a long suffix
    assert max(len(PO.all_windows(D, 3)) - len(PO.windows(D, 3)) for D in range(1, 700)) == 232
    out = PO.select(np.arange(12, dtype=np.float32)[None] / 10, np.array([[1] * 6 + [0] * 6], np.float32), win=3, k=2, keep=5, min_sep=1,
                    gt=np.array([[5.5, 9.0]]))
    assert out["D"] == [6] and out["n_windows"].tolist() == [4] and out["select"].tolist() == [[0, 1, 2, 3, -1]]
    assert out["bounds"][0].tolist() == [[0, 4], [1, 5], [3, 6], [4, 6]] + [[-1, -1]] * 7 and out["order"][0, :5].tolist() == [2, 3, 1, 0, -1]
    assert out["hit_rank"].tolist() == [0] and np.isnan(out["win_scores"][0, 4:]).all()


def test_oracle_selection_against_brute_force():
    rng = np.random.default_rng(11)
    values = np.array([0.0, -0.0, 0.25, 0.5, 0.5, 1.0, -1.0, np.nan, np.inf, -0.75], dtype=np.float32)
    for case in range(150):
        win = int(rng.choice([2, 3, 4, 5, 7, 8]))
        L = int(rng.integers(win, 48))
        D = int(rng.integers(0, L + 1))
        row = rng.choice(values, size=L) if case % 3 else rng.normal(size=L).astype(np.float32)
        if case % 3 and case % 2:
            row[row == np.inf] = 2.0
        mask = (np.arange(L) < D).astype(np.float32)[None]
        Wcap = PO.capacity(L, win)
        for k in (1, 3):
            for min_sep in (1, 2, min(3, Wcap)):
                keep = int(rng.integers(1, Wcap + 1))
                out = PO.select(row[None], mask, win, k, keep, min_sep)
                chosen, seq = PO.brute_select([float(v) for v in row], D, win, k, keep, min_sep)
                W = int(out["n_windows"][0])
                assert out["order"][0, :W].tolist() == seq and (out["order"][0, W:] == -1).all(), (win, L, D, k, min_sep)
                assert out["select"][0, :int(out["n_select"][0])].tolist() == chosen and len(chosen) == min(keep, W)


# ------------------------------------------------------------------ retrieval and expansion ------------------------------------------------------------------
def test_windows_from_retrieval_is_the_merge_rule():
    """A full stage-1 log in which every answer parses: the answers that survive ``merge_stage1_stage2`` are exactly those at the returned indices."""
    rng = np.random.default_rng(4)
    for case in range(40):
        n = int(rng.integers(2, 60))
        answers = [f"From {i % 200} to {i % 200 + 7}." for i in range(n)]
        frames = {}
        for j in range(int(rng.integers(1, 5))):
            f = float(rng.integers(0, int(n / .4) + 5))
            frames[str(j)] = (f, f + float(rng.integers(0, 40)))
        for buffer in (0, 2):
            gl = {"query_id": "q", "answer": list(answers), "info": {"iou": [i / 1000 for i in range(n)], "scores": [float(i) for i in range(n)]}}
            rl = {"query_id": "q", "info": {"frames": dict(frames)}}
            merged, _ = metrics.merge_stage1_stage2([gl], [rl], buffer=buffer)
            got = stage1.windows_from_retrieval(frames, n, buffer)
            assert got == sorted(set(got)) and all(0 <= i < n for i in got)
            if got:
                assert merged[0]["answer"] == [answers[i] for i in got] and merged[0]["info"]["iou"] == [i / 1000 for i in got], (case, buffer)
            else:
                assert merged[0]["answer"] == answers                                     # nothing retrieved: the merge filters nothing
            assert stage1.windows_from_retrieval(list(frames.values()), n, buffer) == got
    assert stage1.windows_from_retrieval({"a": (10, 20), "b": (15, 30)}, 57) == list(range(4, 12))
    assert stage1.windows_from_retrieval({"a": (10, 20)}, 57, buffer=2) == list(range(2, 10)) and stage1.windows_from_retrieval({"a": (10, 400)}, 57) == list(range(4, 56))
    assert stage1.windows_from_retrieval({}, 57) == [] and stage1.windows_from_retrieval({"a": (0, 1)}, 57) == []


def test_expand_selected():
    a, e = stage1.expand_selected(["From 1 to 2.", "x"], [0.5, 0.25], [1, 4], 6)
    assert a == ["Not Present", "From 1 to 2.", "Not Present", "Not Present", "x", "Not Present"] and a[0] == metrics.NOT_PRESENT[0]
    assert e[1] == 0.5 and e[4] == 0.25 and all(np.isnan(e[i]) for i in (0, 2, 3, 5))
    assert stage1.expand_selected(["y"], [], [0], 2) == (["y", "Not Present"], [])
    assert stage1.expand_selected([], [], [], 3) == (["Not Present"] * 3, [])
    for bad in ((["a"], [], [0, 1], 3), (["a", "b"], [1.0], [0, 1], 3), (["a", "b"], [], [1, 0], 3), (["a", "b"], [], [1, 1], 3), (["a"], [], [3], 3),
                (["a"], [], [-1], 3)):
        with pytest.raises(ValueError, match="expand_selected"):
            stage1.expand_selected(*bad)
    # iou() never reads a filler: the kept statistics are those of the parsed answers
    _, _, kept = stage1.iou(a, (0.1, 0.2), 60, 1000, e)
    assert kept == [0.5]


# ------------------------------------------------------------------ the driver's flags ------------------------------------------------------------------
def _host_topk_cosine(feat, q, k=3):
    """``ops.topk_cosine``'s definition in float32 torch on the CPU."""
    out = []
    for f in feat.float():
        sims = f @ (q.float() / f.pow(2).sum(0).sqrt())
        out.append(sims.mean() if k <= 0 else sims.topk(min(k, len(sims))).values.sum())
    return torch.stack(out)


TEXTS = ["From 3 to 9.", "Not Present", "From 17 to 17.", "From 0 to 59.", "From 20 to 31.", "Between 30 and 90"]


def _crafted(windows):
    """One answer and one entropy statistic per window, made from the window's own frames: a window answers the same in any tensor that holds it."""
    digest = [float(w.double().abs().sum()) for w in windows]
    return [TEXTS[int(d) % len(TEXTS)] for d in digest], [1.0 + d % 7.0 for d in digest]


def test_the_driver_runs_a_selection_only_when_asked(tmp_path, monkeypatch):
    """``--clip_prefilter_keep`` / ``--retrieval_path`` with the device stages stubbed by host arithmetic, in the sequential loop and ``--in_flight 3``."""
    from revisionllm_amd import ops, sched, serve
    from revisionllm_amd.data import feature_store
    from revisionllm_amd.eval import eval_nlq_negative as drv
    rs = np.random.RandomState(5)
    feat_dir, q_dir, s2_dir = tmp_path / "feats", tmp_path / "qfeats", tmp_path / "stage2"
    for d in (feat_dir, q_dir, s2_dir):
        os.makedirs(d)
    movie = rs.randn(730, 16).astype(np.float16)                                         # 14 half-overlapping windows of 100 frames
    np.save(feat_dir / "movieA.npy", movie)
    np.save(feat_dir / "short.npy", rs.randn(300, 16).astype(np.float32))              # a short video: subsampled, host route, every window
    ann, qcls = {}, {}
    for i in range(4):
        ann[f"q{i}"] = {"movie": "short" if i == 3 else "movieA", "sentence": f"Someone opens door number {i}.", "timestamps": [10.0 * i, 10.0 * i + 40],
                        "movie_duration": 15.0 if i == 3 else 146.0}
        qcls[f"q{i}"] = rs.randn(16).astype(np.float32)
        np.savez_compressed(q_dir / f"q{i}.npz", token_features=rs.randn(6, 16).astype(np.float32), cls_features=qcls[f"q{i}"])
    with open(tmp_path / "ann.json", "w") as f:
        json.dump(ann, f)
    with open(s2_dir / "predictions_streaming_0.txt", "w") as f:                         # q0 and q3 have stage-2 records, q1 an empty one, q2 none
        f.write(json.dumps({"query_id": "q0", "answer": [], "info": {"frames": {"0": [5.0, 16.0], "1": [20.0, 26.0]}}}) + "\n")
        f.write(json.dumps({"query_id": "q1", "answer": [], "info": {"frames": {}}}) + "\n")
        f.write(json.dumps({"query_id": "q3", "answer": [], "info": {"frames": {"0": [0.0, 30.0]}}}) + "\n")
    routes = []

    def host_windows(features, frame_idx):
        return torch.from_numpy(np.asarray(features, dtype=np.float32))[torch.from_numpy(frame_idx.astype(np.int64))]

    def host_pick(features, query_cls, keep, win):
        """The pre-filter's choice in host arithmetic (the oracle on a float32 cosine row)."""
        f = torch.from_numpy(np.asarray(features, dtype=np.float32))
        q = torch.from_numpy(np.asarray(query_cls, dtype=np.float32))
        sims = ((f @ q) / (f.norm(dim=1) * q.norm())).numpy()
        L = len(sims)
        out = PO.select(sims[None], np.ones((1, L), np.float32), win, 3, min(keep, PO.capacity(L, win)), 1)
        return [i for i in out["select"][0].tolist() if i >= 0]

    class FakeStager:
        op_dtype = torch.float16

        def __init__(self, device, op_dtype=None):
            pass

        def stage_windows(self, features, frame_idx):
            routes.append(("host", len(features)))
            t = host_windows(features, frame_idx)
            return types.SimpleNamespace(wait=lambda: t)

        def stage_resident_clipped(self, features_dev, **geometry):
            routes.append(("resident", features_dev.shape[0]))
            t = host_windows(features_dev.float().numpy(), stage1.cut_windows(features_dev.shape[0], **geometry))
            return types.SimpleNamespace(wait=lambda: t)

        def stage_resident_selected(self, features_dev, *, windows=None, query_cls=None, keep=None, **geometry):
            assert sorted(geometry) == ["debug_window", "feature_fps", "num_frames"] and (windows is None) != (query_cls is None)
            feats = features_dev.float().numpy()
            if windows is None:
                windows = host_pick(feats, query_cls, keep, int(geometry["debug_window"] * geometry["feature_fps"]))
            routes.append(("selected", list(windows)))
            t = host_windows(feats, stage1.cut_windows(features_dev.shape[0], **geometry)[list(windows)])
            return list(windows), types.SimpleNamespace(wait=lambda: t)

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
    monkeypatch.setattr(feature_store, "WindowStager", FakeStager)
    monkeypatch.setattr(stage1, "answer_windows", lambda model, tokenizer, features, *a, **kw: _crafted(features))
    monkeypatch.setattr(stage1, "launch_query_steps", lambda model, tokenizer, features, *a, **kw: features)
    monkeypatch.setattr(stage1, "collect_query", lambda model, tokenizer, launched, score: _crafted(launched))
    monkeypatch.setattr(ops, "topk_cosine", _host_topk_cosine)
    monkeypatch.setattr(ops, "proposal_cosine", lambda windows, text, proposals, *, k: torch.stack(
        [_host_topk_cosine(windows[w][a:b + 1][None], text, k)[0] for w, a, b in proposals]))
    monkeypatch.setattr(serve, "DecodeServer", lambda *a, **kw: None)
    monkeypatch.setattr(sched, "Interleaver", FakeInterleaver)
    monkeypatch.setattr(sched, "Task", lambda gen, stream, engine, slot: types.SimpleNamespace(gen=gen, cancel=lambda: None))
    monkeypatch.setattr(torch.cuda, "Stream", FakeStream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    base = ["--data_path", str(tmp_path / "ann.json"), "--feat_folder", str(feat_dir), "--q_feat_dir", str(q_dir), "--batch", "4", "--vis_feat_storage", "npy",
            "--debug", "True", "--skip_small_videos", "", "--debug_window", "20", "--num_frames", "60"]
    model = types.SimpleNamespace(device=torch.device("cpu"), engine=types.SimpleNamespace(slot=0))
    kw = dict(num_frames=60, debug_window=20, score="mean_entropy", score_merge="multiply", normalize=True, topk_pool=True, plus_baseline=False)
    full = host_windows(movie, stage1.cut_windows(730, 20, 5, 60))
    W = full.shape[0]
    assert W == 14

    def run(name, flags):
        del routes[:]
        args = drv.parse_args(base + flags + ["--log_path", str(tmp_path / name)])
        assert drv.eval(args, tokenizer=None, model=model) == (4, []), name
        return [json.loads(line) for line in open(tmp_path / name / "predictions_streaming_0.txt")], list(routes)

    def padded(i, windows):
        """``score_query`` on the full tensor with the answers of the windows that did not run replaced by "Not Present"."""
        answers, ent = _crafted(full)
        answers = [a if j in windows else "Not Present" for j, a in enumerate(answers)]
        got = stage1.score_query(full, answers, ent, torch.from_numpy(qcls[f"q{i}"]), ann[f"q{i}"]["timestamps"], 146.0, **kw)
        return {"answer": got[0], "iou": got[1]["iou"], "scores": got[1]["scores"]}

    def parts(rec):
        return {"answer": rec["answer"], "iou": rec["info"]["iou"], "scores": rec["info"]["scores"]}
    for mode, flight in (("seq", []), ("flight", ["--in_flight", "3"])):
        host, host_routes = run(f"{mode} host", flight)
        off, off_routes = run(f"{mode} off", flight + ["--device_features"])
        assert off == host and off_routes == [("resident", 730)] * 3 + [("host", 60)] and host_routes == [("host", 730)] * 3 + [("host", 60)]
        assert all("windows" not in r["info"] for r in off)
        # keep >= W: every window runs, the record's parts are the flag-off record's
        allw, r_all = run(f"{mode} all", flight + ["--device_features", "--clip_prefilter_keep", "14"])
        assert r_all == [("selected", list(range(14)))] * 3 + [("host", 60)]
        assert [parts(r) for r in allw] == [parts(r) for r in off] and all(r["info"]["windows"] == list(range(14)) for r in allw[:3])
        assert allw[3] == off[3] and "windows" not in allw[3]["info"]
        big, r_big = run(f"{mode} big", flight + ["--device_features", "--clip_prefilter_keep", "500"])
        assert big == allw and r_big == r_all
        # a proper subset
        some, r_some = run(f"{mode} some", flight + ["--device_features", "--clip_prefilter_keep", "5"])
        picks = [host_pick(movie, qcls[f"q{i}"], 5, 100) for i in range(3)]
        assert r_some == [("selected", p) for p in picks] + [("host", 60)] and all(len(p) == 5 and p == sorted(set(p)) for p in picks)
        for i in range(3):
            assert parts(some[i]) == padded(i, picks[i]) and some[i]["info"]["windows"] == picks[i] and len(some[i]["answer"]) == 14
            assert sorted(some[i]["info"]) == ["iou", "scores", "windows"] and len(some[i]["info"]["iou"]) == len(some[i]["info"]["scores"])
        assert some[3] == off[3] and any(parts(a) != parts(b) for a, b in zip(some[:3], off[:3]))
        # --retrieval_path: q0 has a record, q1 an empty retrieval, q2 none, q3 keeps the host route whatever its record says
        ret, r_ret = run(f"{mode} ret", flight + ["--device_features", "--retrieval_path", str(s2_dir)])
        want = stage1.windows_from_retrieval({"0": [5.0, 16.0], "1": [20.0, 26.0]}, 14)
        assert want == [2, 3, 4, 5, 8, 9] and r_ret == [("selected", want), ("resident", 730), ("resident", 730), ("host", 60)]
        assert parts(ret[0]) == padded(0, want) and ret[0]["info"]["windows"] == want and ret[1:] == off[1:]
        buf, r_buf = run(f"{mode} buf", flight + ["--device_features", "--retrieval_path", str(s2_dir), "--retrieval_buffer", "1"])
        assert r_buf[0] == ("selected", stage1.windows_from_retrieval({"0": [5.0, 16.0], "1": [20.0, 26.0]}, 14, 1)) and buf[1:] == off[1:]
        if mode == "seq":
            seq = (off, some, ret)
        else:
            assert (off, some, ret) == seq                                               # both loops write the same records
    for flags, message in ((["--device_features", "--clip_prefilter_keep", "4", "--retrieval_path", str(s2_dir)], "pass one of them"),
                           (["--clip_prefilter_keep", "4"], "--device_features"), (["--retrieval_path", str(s2_dir)], "--device_features"),
                           (["--device_features", "--clip_prefilter_keep", "-1"], "a window count")):
        with pytest.raises(ValueError, match=message):
            drv.eval(drv.parse_args(base + flags + ["--log_path", str(tmp_path / "refused")]), tokenizer=None, model=model)
    no_q = [a for a in base if a not in ("--q_feat_dir", str(q_dir))]
    with pytest.raises(ValueError, match="--q_feat_dir"):
        drv.eval(drv.parse_args(no_q + ["--device_features", "--clip_prefilter_keep", "4", "--log_path", str(tmp_path / "refused")]), tokenizer=None, model=model)
    # a log written with a selection goes through the merge and the metrics unchanged
    logs = metrics.load_predictions(str(tmp_path / "seq some"))
    assert len(logs) == 4 and metrics.grounding_metrics_stream(logs)["mIoU"] >= 0.0
    retrieval = [{"query_id": f"q{i}", "info": {"frames": {"0": [0.0, 40.0]}}} for i in range(4)]
    merged, fraction = metrics.merge_stage1_stage2(logs, retrieval)
    assert len(merged) == 4 and 0.0 < fraction <= 1.0 and metrics.grounding_metrics_stream(merged) is not None
    assert all(len(m["info"]["iou"]) == len(m["info"]["scores"]) for m in merged)
