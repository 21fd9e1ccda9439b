"""The frame-set window selection on the host: the package surface of ``rvc_window_select_frames`` and the chain library (names under both module
names, signatures, its header, ctypes table and exports held to EACH OTHER - the library is open, so no literal list and no count - with the other two
libraries left as they were, every refusal of the C entry before a launch, every Python-side refusal before a device is looked for) and both drivers'
``--clip_prefilter_frames`` with the device stages stubbed - these fail without the feature.  The rest guards the oracle of
tests/frames_select_oracle.py, which the GPU tests compare the kernel with: its selection is held to a brute-force statement and its sampled frames
to ``stage2.cut_windows`` and ``stage1.cut_windows``.  No GPU."""
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

import frames_select_oracle as FO
from revisionllm_amd import hip
from revisionllm_amd.eval import stage1, stage2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_ERR_ARG = -1              # include/revision_hip.h: rv_status
MINE = {"rvc_abi_version", "rvc_last_error", "rvc_window_select_frames"}


# ------------------------------------------------------------------ surface ------------------------------------------------------------------
def test_the_names_import_from_both_module_names():
    from revisionllm_amd import grounding, ops
    from revisionllm_amd.data import feature_store
    from revisionllm_amd.eval import similarity
    for name in ("window_select_frames", "FrameWindowSelection", "window_select_frames_keywords", "window_select_valid"):
        assert getattr(ops, name) is getattr(grounding, name) and getattr(grounding, name).__module__ == "revisionllm_amd.grounding", name
    assert ops.FrameWindowSelection._fields == ops.WindowSelection._fields + ("n_candidates",)
    assert callable(similarity.select_windows_frames) and callable(stage1.clip_stage_windows_frames) and callable(stage2.clip_stage_windows_frames)
    assert callable(feature_store.WindowStager.stage_resident_selected_frames)
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
import revisionllm_amd.ops as real_ops
import revisionllm_amd.eval.stage1 as real_stage1
import revisionllm_amd.eval.stage2 as real_stage2
import revisionllm_amd.eval.similarity as real_similarity
from revisionllm.ops import window_select_frames, FrameWindowSelection
from revisionllm.eval.similarity import select_windows_frames
import vtimellm.ops as old_ops
import vtimellm.eval.stage1 as old_stage1
import vtimellm.eval.stage2 as old_stage2
import vtimellm.eval.similarity as old_similarity
assert window_select_frames is real_ops.window_select_frames is old_ops.window_select_frames
assert FrameWindowSelection is real_ops.FrameWindowSelection
assert select_windows_frames is real_similarity.select_windows_frames is old_similarity.select_windows_frames
assert real_stage1.clip_stage_windows_frames is old_stage1.clip_stage_windows_frames
assert real_stage2.clip_stage_windows_frames is old_stage2.clip_stage_windows_frames
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_signatures():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import eval_nlq_negative as drv1
    from revisionllm_amd.eval import eval_nlq_retrieval_e2e2 as drv2
    from revisionllm_amd.eval import similarity
    E = inspect.Parameter.empty
    keywords = dict(rule=E, win=E, stride=None, keep=E, frames="all", num_frames=None, valid=None, k=3, min_sep=1, gt=None, return_scores=False,
                    return_bounds=False, return_order=False)
    for fn, lead in ((ops.window_select_frames, ["sims", "mask"]), (similarity.select_windows_frames, ["text", "video", "mask"])):
        p = inspect.signature(fn).parameters
        assert list(p) == lead + list(keywords) and {n: p[n].default for n in keywords} == keywords
        assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in keywords)
    for stage in (stage1, stage2):
        old, new = inspect.signature(stage.clip_stage_windows).parameters, inspect.signature(stage.clip_stage_windows_frames).parameters
        assert list(new) == list(old) + ["score_frames", "valid"] and all(new[n].default == old[n].default and new[n].kind == old[n].kind for n in old)
        assert new["score_frames"].default == "sampled" and new["valid"].default is None and new["valid"].kind is inspect.Parameter.KEYWORD_ONLY
    # the existing signatures did not move
    assert list(inspect.signature(ops.window_select).parameters)[:5] == ["sims", "mask", "win", "stride", "keep"]
    assert "frames" not in inspect.signature(ops.window_select).parameters and "valid" not in inspect.signature(ops.window_select_clipped).parameters
    assert ops.WindowSelection._fields == ("select", "n_select", "n_windows", "scores", "bounds", "order", "hit_rank")
    for drv in (drv1, drv2):
        assert drv.parse_args([]).clip_prefilter_frames == "all" and drv.parse_args(["--clip_prefilter_frames", "sampled"]).clip_prefilter_frames == "sampled"
        with pytest.raises(SystemExit):
            drv.parse_args(["--clip_prefilter_frames", "some"])


def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    return {line.split()[-1] for line in nm.stdout.splitlines() if line.split() and line.split()[-2] in "TDBR"}


def test_the_chain_library_is_open_and_the_other_two_are_untouched():
    from revisionllm_amd import build
    header = open(os.path.join(ROOT, "include", "revision_hip_chain.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                             # declarations only: comments name entries of other libraries
    declared = set(re.findall(r"\b(rvc_[a-z0-9_]+)\s*\(", code))
    libs = [hip.CHAIN_LIB_PATH, hip.EXT_LIB_PATH] + list(hip.LIB_PATHS.values())
    if not all(os.path.exists(p) for p in libs):
        build.build_library()
    # header == table == exports, whatever else the library holds by now; this feature's names are among them
    assert declared == set(hip.CHAIN_SIGNATURES) == _exported(hip.CHAIN_LIB_PATH) and MINE <= declared
    assert all(n.startswith("rvc_") for n in declared)
    assert f"#define RVC_ABI_VERSION {hip.RVC_ABI_VERSION}" in header and hip.chain_lib().rvc_abi_version() == hip.RVC_ABI_VERSION == 1
    for name, (_, args) in hip.CHAIN_SIGNATURES.items():                            # every declaration has as many parameters as its table entry
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code).group(1).strip()
        assert (0 if params == "void" else len(params.split(","))) == len(args), name
    assert len(hip.CHAIN_SIGNATURES["rvc_window_select_frames"][1]) == 25
    assert os.path.basename(hip.CHAIN_LIB_PATH) == "librevision_hip_chain.so" == os.path.basename(build.CHAIN_LIB)
    assert open(os.path.join(ROOT, "revisionllm_amd", "csrc", "exports_chain.map")).read().split() == "{ global: rvc_*; local: *; };".split()
    for c, v in (("RV_FRAMES_ALL", hip.RV_FRAMES_ALL), ("RV_FRAMES_SAMPLED", hip.RV_FRAMES_SAMPLED), ("RVC_MAX_SAMPLED", hip.RVC_MAX_SAMPLED),
                 ("RV_WINDOWS_SHIFTED", hip.RV_WINDOWS_SHIFTED), ("RV_WINDOWS_CLIPPED", hip.RV_WINDOWS_CLIPPED)):
        assert re.search(r"#define %s %d\b" % (c, v), header), c
    comment = re.search(r"/\* ---- coarse window selection on a chosen frame set.*?\*/", header, re.S).group(0)
    for word in ("np.linspace", "POSITION", "valid[t_j] != 0", "a NaN in valid does not", "does not change the duration", "0x7fc00000", "no candidate", "AMONG",
                 "min(keep, C_r)", "bit for bit", "1 <= F <= 1024", "F != 0", "stride != 2", "no global", "no scratch"):
        assert word in comment, word                                               # the definition stands in the header
    # the companion library and the main one: header, table and exports as they were
    ext_header = open(os.path.join(ROOT, "include", "revision_hip_ext.h")).read()
    ext = set(re.findall(r"\b(rvx_[a-z0-9_]+)\s*\(", ext_header))
    assert ext == set(hip.EXT_SIGNATURES) == _exported(hip.EXT_LIB_PATH) and len(ext) == 3 and hip.ext_lib().rvx_abi_version() == 1
    main_header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    main = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", main_header))
    assert main == set(hip.SIGNATURES) and len(main) == 64 and "#define RV_ABI_VERSION 5" in main_header and "rvc_" not in main_header + ext_header
    for flavour, path in hip.LIB_PATHS.items():
        assert _exported(path) == main, flavour
    # one definition of the kernel and one of the index rule
    csrc = os.path.join(ROOT, "revisionllm_amd", "csrc")
    src = {n: open(os.path.join(csrc, n)).read() for n in ("window_select.h", "grounding.h", "gather.hip", "prefilter_chain.hip", "prefilter.hip", "prefilter_ext.hip")}
    assert src["window_select.h"].count("void window_select_kernel(") == 1 and "template <int RULE, int FRAMES" in src["window_select.h"]
    assert "__global__" not in src["prefilter_chain.hip"] and '#include "window_select.h"' in src["prefilter_chain.hip"]
    assert sum(s.count("int gw_linspace(") for s in src.values()) == 1 and "int gw_linspace(" in src["grounding.h"] and "gw_linspace(" in src["gather.hip"]
    assert "gw_linspace(" in src["window_select.h"]


def _refused(rc, message):
    return rc == RV_ERR_ARG and message in hip.chain_last_error()


def test_every_refusal_of_the_entry_comes_before_any_launch():
    """Dummy device pointers: a call that got as far as a launch would fault, so a clean RV_ERR_ARG with its message shows the check came first."""
    one = ctypes.c_void_p(64)
    f = hip.chain_lib().rvc_window_select_frames
    who = "rvc_window_select_frames: "
    good = dict(sims=one, mask=one, valid=one, R=6, rpm=3, L=100, rule=0, win=10, stride=2, frames=1, F=7, k=3, keep=4, min_sep=2, Wcap=19, gt=one, select=one,
                n_select=one, n_windows=one, n_candidates=one, win_scores=one, bounds=one, order=one, hit_rank=one)
    order = list(good)

    def call(**kw):
        a = {**good, **kw}
        return f(*[a[n] for n in order], None)
    for name in ("sims", "mask", "select", "n_select", "n_windows", "n_candidates"):
        assert _refused(call(**{name: None}), who + "bad arguments"), name
    for rule in (-1, 2, 7):
        assert _refused(call(rule=rule), who + "rule=%d (0: shifted windows, 1: clipped windows)" % rule)
    for frames in (-1, 2):
        assert _refused(call(frames=frames), who + "frames=%d (0: every frame, 1: the sampled frames)" % frames)
    for kw in (dict(R=0), dict(R=-3), dict(rpm=0), dict(rpm=-1), dict(R=7), dict(R=2, rpm=3)):
        assert _refused(call(**kw), who + "R=%d rows with rpm=%d" % (kw.get("R", 6), kw.get("rpm", 3))), kw
    for L in (0, -1, 1048577):
        assert _refused(call(L=L), who + "L=%d must be in [1, 1048576]" % L)
    for stride in (1, 3, 5, 0):
        assert _refused(call(rule=1, stride=stride), who + "stride=%d with the clipped rule" % stride)
    for kw in (dict(win=1), dict(win=0), dict(win=-2), dict(win=101), dict(stride=0), dict(stride=-1), dict(stride=11), dict(rule=1, win=1), dict(rule=1, win=101)):
        a = {**good, **kw}
        assert _refused(call(**kw), who + "win=%d frames with stride=%d (stride >= 1, stride <= win <= L=100)" % (a["win"], a["stride"])), kw
    for F in (0, -1, 1025, 65536):
        assert _refused(call(F=F), who + "F=%d sampled frames per window must be in [1, 1024]" % F)
    for F in (1, 250, -1):
        assert _refused(call(frames=0, F=F), who + "F=%d with every frame of a window (F = 0)" % F)
    for k in (0, -1, 65):
        assert _refused(call(k=k), who + "k=%d must be in [1, 64]" % k)
    for Wcap in (18, 20, 0, -1):
        assert _refused(call(Wcap=Wcap), who + "Wcap=%d must be max(1, ceil(L / (win / stride)) - 1) = 19" % Wcap)
    assert _refused(call(stride=5, Wcap=19), who + "Wcap=19 must be max(1, ceil(L / (win / stride)) - 1) = 49")
    for rule in (0, 1):
        assert _refused(call(rule=rule, L=2050, win=2, Wcap=2049, keep=1, min_sep=1), who + "L=2050, win=2, stride=2 give up to 2049 windows (at most 2048)")
    for keep in (0, -1, 20):
        assert _refused(call(keep=keep), who + "keep=%d must be in [1, Wcap=19]" % keep)
    for min_sep in (0, -1, 20):
        assert _refused(call(min_sep=min_sep), who + "min_sep=%d must be in [1, Wcap=19]" % min_sep)
    assert _refused(call(gt=None), who + "hit_rank needs gt")


def test_python_side_refusals_come_before_the_device_is_looked_for():
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import select_windows_frames
    s, m = torch.zeros(2, 3, 40), torch.ones(2, 40)
    good = dict(rule="shifted", win=10, stride=2, keep=4)
    keywords = [dict(rule="both"), dict(rule=0), dict(rule=None), dict(stride=None), dict(rule="clipped", stride=5), dict(rule="clipped", stride=2.0),
                dict(frames="some"), dict(frames=1), dict(frames="sampled"), dict(frames="sampled", num_frames=0), dict(frames="sampled", num_frames=1025),
                dict(frames="sampled", num_frames=2.0), dict(frames="sampled", num_frames=True), dict(num_frames=250), dict(frames="all", num_frames=0),
                dict(win=0), dict(win=1, stride=2), dict(win=10.0), dict(win=None), dict(win=True), dict(win=41), dict(keep=0), dict(keep=2.5), dict(keep=None),
                dict(k=0), dict(k=65), dict(k=1.5), dict(min_sep=0), dict(min_sep=8, stride=1), dict(min_sep=1.0), dict(win=2 ** 31), dict(stride=0),
                dict(gt=torch.zeros(2, 2)), dict(gt=torch.zeros(2, 3, 2, dtype=torch.int32)), dict(gt=[[0.0, 1.0]] * 6),
                dict(valid=torch.ones(2, 41)), dict(valid=torch.ones(40)), dict(valid=torch.ones(2, 3, 40)), dict(valid=torch.ones(2, 40, dtype=torch.int64)),
                dict(valid=torch.ones(2, 40, dtype=torch.complex64)), dict(valid=[[1] * 40] * 2), dict(valid=np.ones((2, 40), np.float32))]
    shapes = [dict(sims=torch.zeros(40)), dict(sims=torch.zeros(2, 3, 4, 40)), dict(mask=torch.ones(40)), dict(mask=torch.ones(2, 41)),
              dict(mask=torch.ones(3, 40)), dict(sims=torch.zeros(2, 3, 40, dtype=torch.int64)), dict(mask=torch.ones(2, 40, dtype=torch.complex64)),
              dict(sims=torch.zeros(2, 0, 40)), dict(sims=torch.zeros(5, 40)), dict(sims=[[0.5] * 40])]
    for kw in keywords:
        with pytest.raises(ValueError, match="window_select_frames"):
            ops.window_select_frames(s, m, **{**good, **kw})
    for kw in shapes:
        a = {**dict(sims=s, mask=m), **kw}
        with pytest.raises(ValueError, match="window_select_frames"):
            ops.window_select_frames(a["sims"], a["mask"], **good)
    with pytest.raises(ValueError, match="window_select_frames: sims must be float32"):
        ops.window_select_frames(s.half(), m, **good)
    with pytest.raises(ValueError, match="at most 2048"):
        ops.window_select_frames(torch.zeros(1, 2050), torch.ones(1, 2050), rule="clipped", win=2, keep=1)
    with pytest.raises(TypeError):
        ops.window_select_frames(s, m, "shifted", 10, 2, 4)                         # keyword-only
    with pytest.raises(TypeError):
        ops.window_select_frames(s, m, win=10, keep=4)                              # rule has no default
    text, video = torch.zeros(2, 3, 8), torch.zeros(2, 40, 8)
    for kw in keywords:
        with pytest.raises(ValueError, match="select_windows_frames"):
            select_windows_frames(text, video, m, **{**good, **kw})
    for a in (dict(text=torch.zeros(2, 3, 9)), dict(text=torch.zeros(3, 8)), dict(video=torch.zeros(2, 40)), dict(mask=torch.ones(2, 39)), dict(text=text.long()),
              dict(text=None), dict(mask=torch.ones(2, 40, dtype=torch.complex64))):
        b = {**dict(text=text, video=video, mask=m), **a}
        with pytest.raises(ValueError, match="select_windows_frames"):
            select_windows_frames(b["text"], b["video"], b["mask"], **good)
    # what the keyword checker hands the entry
    assert ops.window_select_frames_keywords("x", "clipped", 10, None, 4) == (1, 10, 2, 4, 0, 0, 3, 1)
    assert ops.window_select_frames_keywords("x", "shifted", 625, 5, 100, "sampled", 250, 3, 2) == (0, 625, 5, 100, 1, 250, 3, 2)
    f, q = torch.zeros(700, 8), torch.zeros(8)
    for stage, pick in ((stage1, dict(keep=4)), (stage2, dict(batch=4))):
        for kw in (dict(score_frames="some"), dict(score_frames=None), dict(valid=torch.ones(699)), dict(valid=torch.ones(1, 700)), dict(valid=np.ones(700, np.int64)),
                   dict(debug_window=125, feature_fps=4.5)):
            with pytest.raises(ValueError, match="clip_stage_windows_frames"):
                stage.clip_stage_windows_frames(f, q, **{**pick, **kw})
        for nf in (1025, 0):                                                            # the selection's F is the gather's num_frames
            with pytest.raises(ValueError, match=f"num_frames={nf} sampled frames per window"):
                stage.clip_stage_windows_frames(f, q, num_frames=nf, **pick)
        with pytest.raises(ValueError, match="clip_stage_windows_frames"):
            stage.clip_stage_windows_frames(torch.zeros(600, 8), q, **pick)             # shorter than one window: the host route
        with pytest.raises(TypeError):
            stage.clip_stage_windows_frames(f, q, 125, **pick)                          # keyword-only


# ------------------------------------------------------------------ the oracle ------------------------------------------------------------------
def test_oracle_sampled_frames_are_cut_windows():
    """The oracle's windows and sample indices against both ``cut_windows`` at the drivers' geometry (125 s x 5 fps, 250 frames) and at win in
    {2, 3, 5, 11, 61} x F in {1, 2, 3, 31, 251}; a void window of the clipped rule is no window of the oracle's."""
    for dw, fps, nfs, lengths in [(125, 5, (250,), (626, 700, 1873, 3000, 9001))] + [(w, 1, (1, 2, 3, 31, 251), range(w + 1, 200, 7)) for w in (2, 3, 5, 11, 61)]:
        win = dw * fps
        for ctx_l in lengths:
            for nf in nfs:
                for stride in (2, 5) if win >= 5 else (2,):
                    _, idx = stage2.cut_windows(ctx_l, dw, fps, stride, nf)
                    wins = FO.windows(ctx_l, FO.SHIFTED, win, stride)
                    assert len(wins) == idx.shape[0] and all(np.array_equal(FO.sample_indices(lo, hi, nf), idx[i]) for i, (lo, hi) in enumerate(wins)), (win, ctx_l, nf)
                    assert all(FO.frame_set(lo, hi, FO.SAMPLED, nf) == idx[i].tolist() for i, (lo, hi) in enumerate(wins))
                idx = stage1.cut_windows(ctx_l, dw, fps, nf)
                wins = FO.windows(ctx_l, FO.CLIPPED, win, 2)
                assert len(wins) <= idx.shape[0] and all(np.array_equal(FO.sample_indices(lo, hi, nf), idx[i]) for i, (lo, hi) in enumerate(wins)), (win, ctx_l, nf)
    assert FO.frame_set(3, 9, FO.ALL, 0) == [3, 4, 5, 6, 7, 8] and FO.frame_set(3, 9, FO.SAMPLED, 6) == [3, 4, 5, 6, 7, 8]
    assert FO.frame_set(10, 12, FO.SAMPLED, 5) == [10, 10, 10, 10, 11] and FO.frame_set(4, 5, FO.SAMPLED, 3) == [4, 4, 4] and FO.frame_set(4, 9, FO.SAMPLED, 1) == [4]


def test_oracle_scores_ties_and_candidates():
    s = np.array([0.5, 0.25, 0.5, np.nan, -0.0, 0.0, 1.0, np.inf], dtype=np.float32)
    assert FO.window_score(s, None, [0, 1, 2], 2) == (np.float32(1.0), 3) and FO.window_score(s, None, [1, 1, 1, 0], 3) == (np.float32(1.0), 4)      # duplicates count
    assert np.isnan(FO.window_score(s, None, [2, 3, 6], 1)[0]) and FO.window_score(s, np.array([1, 1, 1, 0, 1, 1, 1, 1]), [2, 3, 6], 1) == (np.float32(1.0), 2)
    v = np.array([0, -0.0, np.nan, 0, 2.0, 0, 0, 0], dtype=np.float32)
    assert FO.window_score(s, v, list(range(8)), 3) == (np.float32(0.5), 2)                # frames 2 (valid NaN: usable) and 4
    assert FO.window_score(s, v, [0, 1, 3, 5], 3)[1] == 0
    out = FO.select(np.arange(12, dtype=np.float32)[None] / 10, np.ones((1, 12), np.float32), FO.SHIFTED, 4, 2, FO.ALL, 0, 2, 5, 1,
                    valid=np.array([[1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1]], np.float32), gt=np.array([[5.0, 8.0]]))
    # windows [0,5) [2,7) [4,9) [6,11) [7,12): [4,9) has no usable frame
    assert out["bounds"][0].tolist() == [[0, 5], [2, 7], [4, 9], [6, 11], [7, 12]] and out["n_windows"].tolist() == [5] and out["n_candidates"].tolist() == [4]
    assert out["order"][0].tolist() == [4, 3, 0, 1, -1] and out["select"][0].tolist() == [0, 1, 3, 4, -1] and out["n_select"].tolist() == [4]
    assert np.isnan(out["win_scores"][0, 2]) and out["hit_rank"].tolist() == [0]              # [7,12) covers (5, 8); [4,9) is no candidate


def test_oracle_selection_against_brute_force():
    rng = np.random.default_rng(11)
    values = np.array([0.0, -0.0, 0.25, 0.5, 0.5, 1.0, -1.0, np.nan, np.inf, -0.75], dtype=np.float32)
    seen = 0
    for case in range(160):
        win = int(rng.choice([2, 3, 4, 5, 7, 8]))
        rule = case % 2
        stride = 2 if rule == FO.CLIPPED else int(rng.choice([s for s in (1, 2, 3, 5) if s <= win]))
        L = int(rng.integers(win, 48))
        D = int(rng.integers(0, L + 1))
        row = rng.choice(values, size=L) if case % 3 else rng.normal(size=L).astype(np.float32)
        mask = (np.arange(L) < D).astype(np.float32)[None]
        valid = None if case % 4 == 0 else (rng.random((1, L)) < (0.3 if case % 4 == 1 else 0.7)).astype(np.float32)
        frames, nf = (FO.ALL, 0) if case % 5 < 2 else (FO.SAMPLED, int(rng.choice([1, 2, 3, 5, 12])))
        Wcap = FO.capacity(L, win, stride)
        for k in (1, 3):
            for min_sep in (1, 2, min(3, Wcap)):
                keep = int(rng.integers(1, Wcap + 1))
                out = FO.select(row[None], mask, rule, win, stride, frames, nf, k, keep, min_sep, valid=valid)
                chosen, seq, W = FO.brute_select([float(x) for x in row], None if valid is None else valid[0], D, rule, win, stride, frames, nf, k, keep, min_sep)
                C = int(out["n_candidates"][0])
                assert int(out["n_windows"][0]) == W and C == len(seq) <= W, (case, k, min_sep)
                assert out["order"][0, :C].tolist() == seq and (out["order"][0, C:] == -1).all(), (case, rule, win, stride, L, D, frames, nf, k, min_sep)
                assert out["select"][0, :int(out["n_select"][0])].tolist() == chosen and len(chosen) == min(keep, C)
                seen += C < W
    assert seen > 50                                                                   # rows with windows that are no candidates were among them


# ------------------------------------------------------------------ the drivers' flag ------------------------------------------------------------------
def _host_windows(features, frame_idx):
    return torch.from_numpy(np.asarray(features, dtype=np.float32))[torch.from_numpy(frame_idx.astype(np.int64))]


def _fixture(tmp_path, L, duration):
    rs = np.random.RandomState(5)
    feat_dir, q_dir = tmp_path / "feats", tmp_path / "qfeats"
    for d in (feat_dir, q_dir):
        os.makedirs(d)
    np.save(feat_dir / "movieA.npy", rs.randn(L, 16).astype(np.float16))
    ann = {}
    for i in range(2):
        ann[f"q{i}"] = {"movie": "movieA", "sentence": f"Someone opens door number {i}.", "timestamps": [10.0 * i, 10.0 * i + 40], "movie_duration": duration}
        np.savez_compressed(q_dir / f"q{i}.npz", token_features=rs.randn(6, 16).astype(np.float32), cls_features=rs.randn(16).astype(np.float32))
    with open(tmp_path / "ann.json", "w") as f:
        json.dump(ann, f)
    return ["--data_path", str(tmp_path / "ann.json"), "--feat_folder", str(feat_dir), "--q_feat_dir", str(q_dir), "--batch", "4", "--vis_feat_storage", "npy",
            "--debug", "True"]


def test_the_stage2_driver_scores_sampled_frames_only_when_asked(tmp_path, monkeypatch):
    from revisionllm_amd.data import feature_store
    from revisionllm_amd.eval import eval_nlq_retrieval_e2e2 as drv
    base = _fixture(tmp_path, 2600, 520.0)
    routes = []

    class FakeStager:
        op_dtype = torch.float16

        def __init__(self, device, op_dtype=None):
            pass

        def stage_windows(self, features, frame_idx):
            routes.append(("host", len(features)))
            t = _host_windows(features, frame_idx)
            return types.SimpleNamespace(wait=lambda: t)

    def fake_run_query(model, tokenizer, windows, qf, qc, sentence, batch, mode, grounding_windows, single):
        plan = stage2.plan_groups(windows.shape[0], batch)
        return dict(answers=["In video 3."] * len(plan), starts=[p[1] for p in plan], indexes=[list(range(p[2] - p[1])) for p in plan],
                    hierarchy_zooms=[p[0] for p in plan], max_entropy=[1.0] * len(plan), mean_entropy=[2.0] * len(plan),
                    score_cos=[float(windows.double().sum())] * len(plan), grounding_windows=grounding_windows, plan=plan)

    def fake_stage(name, picked):
        def stage(features_dev, query_cls, **kw):
            routes.append((name, kw.get("score_frames")))
            assert kw["batch"] == 4 and kw["num_frames"] == 250 and kw["dtype"] == torch.float16 and (name == "all") == ("score_frames" not in kw)
            geometry = {n: kw[n] for n in ("debug_window", "feature_fps", "stride", "num_frames")}
            return list(picked), _host_windows(features_dev.float().numpy(), stage2.cut_windows(features_dev.shape[0], **geometry)[1][picked])
        return stage
    monkeypatch.setattr(feature_store, "WindowStager", FakeStager)
    monkeypatch.setattr(stage2, "run_query", fake_run_query)
    monkeypatch.setattr(stage2, "clip_grounding_windows", lambda features, query_cls, **kw: [1, 4, 9, 12])
    monkeypatch.setattr(stage2, "clip_stage_windows", fake_stage("all", [1, 4, 9, 12]))
    monkeypatch.setattr(stage2, "clip_stage_windows_frames", fake_stage("frames", [2, 4, 9, 13]))
    model = types.SimpleNamespace(device=torch.device("cpu"))

    def run(name, flags):
        del routes[:]
        assert drv.eval(drv.parse_args(base + ["--log_path", str(tmp_path / name)] + flags), tokenizer=None, model=model) == (2, [])
        return [json.loads(line) for line in open(tmp_path / name / "predictions_streaming_0.txt")], list(routes)
    host, r_host = run("host", ["--clip_prefilter"])
    off, r_off = run("off", ["--clip_prefilter", "--device_features"])
    named, r_named = run("named", ["--clip_prefilter", "--device_features", "--clip_prefilter_frames", "all"])
    assert off == host == named and r_off == r_named == [("all", None)] * 2 and r_host == [("host", 2600)] * 2      # the parent's path, untouched
    sampled, r_sampled = run("sampled", ["--clip_prefilter", "--device_features", "--clip_prefilter_frames", "sampled"])
    assert r_sampled == [("frames", "sampled")] * 2 and sampled != off and len(sampled) == 2
    for flags in (["--clip_prefilter_frames", "sampled"], ["--clip_prefilter", "--clip_prefilter_frames", "sampled"],
                  ["--device_features", "--clip_prefilter_frames", "sampled"]):
        with pytest.raises(ValueError, match="--clip_prefilter_frames sampled"):
            drv.eval(drv.parse_args(base + flags + ["--log_path", str(tmp_path / "refused")]), tokenizer=None, model=model)
    with pytest.raises(ValueError, match="--num_frames 1025 must be in"):
        drv.eval(drv.parse_args(base + ["--clip_prefilter", "--device_features", "--clip_prefilter_frames", "sampled", "--num_frames", "1025", "--log_path",
                                        str(tmp_path / "refused")]), tokenizer=None, model=model)
    assert not os.path.exists(tmp_path / "refused" / "predictions_streaming_0.txt")


def test_the_stage1_driver_scores_sampled_frames_only_when_asked(tmp_path, monkeypatch):
    from revisionllm_amd import ops
    from revisionllm_amd.data import feature_store
    from revisionllm_amd.eval import eval_nlq_negative as drv
    base = _fixture(tmp_path, 730, 146.0) + ["--skip_small_videos", "", "--debug_window", "20", "--num_frames", "60"]
    routes = []

    class FakeStager:
        op_dtype = torch.float16

        def __init__(self, device, op_dtype=None):
            pass

        def stage_windows(self, features, frame_idx):
            routes.append(("host", len(features)))
            t = _host_windows(features, frame_idx)
            return types.SimpleNamespace(wait=lambda: t)

        def stage_resident_clipped(self, features_dev, **geometry):
            routes.append(("resident", features_dev.shape[0]))
            t = _host_windows(features_dev.float().numpy(), stage1.cut_windows(features_dev.shape[0], **geometry))
            return types.SimpleNamespace(wait=lambda: t)

        def _selected(self, name, picked, features_dev, geometry):
            assert sorted(geometry) == ["debug_window", "feature_fps", "num_frames"]
            routes.append((name, list(picked)))
            t = _host_windows(features_dev.float().numpy(), stage1.cut_windows(features_dev.shape[0], **geometry)[picked])
            return list(picked), types.SimpleNamespace(wait=lambda: t)

        def stage_resident_selected(self, features_dev, *, windows=None, query_cls=None, keep=None, **geometry):
            assert windows is None and query_cls is not None and keep == 3
            return self._selected("all", [1, 4, 9], features_dev, geometry)

        def stage_resident_selected_frames(self, features_dev, *, query_cls, keep, score_frames="sampled", valid=None, **geometry):
            assert query_cls is not None and keep == 3 and score_frames == "sampled" and valid is None
            return self._selected("frames", [2, 4, 10], features_dev, geometry)

    def crafted(windows):
        digest = [float(w.double().abs().sum()) for w in windows]
        return [["From 3 to 9.", "Not Present", "From 17 to 17."][int(d) % 3] for d in digest], [1.0 + d % 7.0 for d in digest]

    def host_topk_cosine(feat, q, k=3):
        out = []
        for f in feat.float():
            sims = f @ (q.float() / f.pow(2).sum(0).sqrt())
            out.append(sims.mean() if k <= 0 else sims.topk(min(k, len(sims))).values.sum())
        return torch.stack(out)
    monkeypatch.setattr(feature_store, "WindowStager", FakeStager)
    monkeypatch.setattr(stage1, "answer_windows", lambda model, tokenizer, features, *a, **kw: crafted(features))
    monkeypatch.setattr(ops, "topk_cosine", host_topk_cosine)
    monkeypatch.setattr(ops, "proposal_cosine", lambda windows, text, proposals, *, k: torch.stack(
        [host_topk_cosine(windows[w][a:b + 1][None], text, k)[0] for w, a, b in proposals]))
    model = types.SimpleNamespace(device=torch.device("cpu"), engine=types.SimpleNamespace(slot=0))

    def run(name, flags):
        del routes[:]
        assert drv.eval(drv.parse_args(base + flags + ["--log_path", str(tmp_path / name)]), tokenizer=None, model=model) == (2, [])
        return [json.loads(line) for line in open(tmp_path / name / "predictions_streaming_0.txt")], list(routes)
    off, r_off = run("off", ["--device_features", "--clip_prefilter_keep", "3"])
    named, r_named = run("named", ["--device_features", "--clip_prefilter_keep", "3", "--clip_prefilter_frames", "all"])
    assert off == named and r_off == r_named == [("all", [1, 4, 9])] * 2 and all(r["info"]["windows"] == [1, 4, 9] for r in off)      # the parent's path
    sampled, r_sampled = run("sampled", ["--device_features", "--clip_prefilter_keep", "3", "--clip_prefilter_frames", "sampled"])
    assert r_sampled == [("frames", [2, 4, 10])] * 2 and all(r["info"]["windows"] == [2, 4, 10] and len(r["answer"]) == 14 for r in sampled)
    plain, r_plain = run("plain", ["--device_features"])
    assert r_plain == [("resident", 730)] * 2 and all("windows" not in r["info"] for r in plain)
    for flags in (["--clip_prefilter_frames", "sampled"], ["--device_features", "--clip_prefilter_frames", "sampled"],
                  ["--clip_prefilter_keep", "3", "--clip_prefilter_frames", "sampled"]):
        with pytest.raises(ValueError, match="--clip_prefilter_frames sampled"):
            drv.eval(drv.parse_args(base + flags + ["--log_path", str(tmp_path / "refused")]), tokenizer=None, model=model)
    with pytest.raises(ValueError, match="--num_frames 1025 must be in"):
        drv.eval(drv.parse_args([x for x in base if x != "60"] + ["1025", "--device_features", "--clip_prefilter_keep", "3", "--clip_prefilter_frames", "sampled",
                                                                  "--log_path", str(tmp_path / "refused")]), tokenizer=None, model=model)
