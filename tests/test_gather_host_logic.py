"""The window gather on the host: the package surface of ``rv_window_gather`` (names under both module names, signatures, header, ctypes table, both
libraries, every refusal of the C entry before a launch, every Python-side refusal before a device is looked for), ``ResidentFeatures``' policy on the
CPU and the driver's ``--device_features`` flag with the device stages stubbed - these fail without the feature.  The rest guards the oracle of
tests/gather_oracle.py, which the GPU tests compare the kernel with: its indices are held to ``stage2.cut_windows`` and its linspace rule to
``np.linspace``, at a triple where an integer rule gives other frames among them.  No GPU."""
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

import gather_oracle as GO
import window_oracle as WO
from revisionllm_amd import hip
from revisionllm_amd.eval import stage2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_ERR_ARG = -1              # include/revision_hip.h: rv_status


# ------------------------------------------------------------------ surface ------------------------------------------------------------------
def test_the_names_import_from_both_module_names():
    from revisionllm_amd import grounding, ops
    from revisionllm_amd.data import feature_store
    assert ops.window_gather is grounding.window_gather and grounding.window_gather.__module__ == "revisionllm_amd.grounding"
    assert ops.window_gather_keywords is grounding.window_gather_keywords and ops.window_gather_dtypes is grounding.window_gather_dtypes
    assert ops.WINDOW_GATHER_MAX_FRAMES == grounding.WINDOW_GATHER_MAX_FRAMES == 65536
    assert callable(stage2.gather_windows) and callable(stage2.clip_stage_windows) and callable(feature_store.ResidentFeatures)
    assert callable(feature_store.WindowStager.stage_resident)
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
import revisionllm_amd.ops as real_ops
import revisionllm_amd.eval.stage2 as real_stage2
import revisionllm_amd.data.feature_store as real_store
from revisionllm.ops import window_gather, WINDOW_GATHER_MAX_FRAMES
from revisionllm.eval.stage2 import gather_windows, clip_stage_windows
from revisionllm.data.feature_store import ResidentFeatures, WindowStager
import vtimellm.ops as old_ops
import vtimellm.eval.stage2 as old_stage2
import vtimellm.data.feature_store as old_store
assert window_gather is real_ops.window_gather is old_ops.window_gather and WINDOW_GATHER_MAX_FRAMES == old_ops.WINDOW_GATHER_MAX_FRAMES == 65536
assert gather_windows is real_stage2.gather_windows is old_stage2.gather_windows
assert clip_stage_windows is real_stage2.clip_stage_windows is old_stage2.clip_stage_windows
assert ResidentFeatures is real_store.ResidentFeatures is old_store.ResidentFeatures and WindowStager.stage_resident is old_store.WindowStager.stage_resident
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_signatures():
    from revisionllm_amd import ops
    from revisionllm_amd.data import feature_store
    from revisionllm_amd.eval import eval_nlq_retrieval_e2e2 as drv
    p = inspect.signature(ops.window_gather).parameters
    optional = dict(mask=None, out_dtype=None, return_index=False)
    assert list(p) == ["video", "select", "win", "stride", "num_frames"] + list(optional)
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(p)[2:])
    assert all(p[n].default is inspect.Parameter.empty for n in ("win", "stride", "num_frames")) and {n: p[n].default for n in optional} == optional
    geometry = dict(debug_window=125, feature_fps=5, stride=5)
    g = inspect.signature(stage2.gather_windows).parameters
    assert list(g) == ["features_dev", "windows"] + list(geometry) + ["num_frames", "dtype"] and {n: g[n].default for n in geometry} == geometry
    c = inspect.signature(stage2.clip_stage_windows).parameters
    assert list(c) == ["features_dev", "query_cls"] + list(geometry) + ["batch", "num_frames", "dtype", "k", "min_sep"]
    assert (c["batch"].default, c["num_frames"].default, c["k"].default, c["min_sep"].default) == (100, 250, 3, 1)
    assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for sig in (g, c) for q in list(sig.values())[2:])
    assert "BEFORE" in stage2.clip_stage_windows.__doc__ and "host copy" in stage2.clip_stage_windows.__doc__
    assert list(inspect.signature(feature_store.ResidentFeatures).parameters)[:2] == ["device", "budget_bytes"]
    assert list(inspect.signature(feature_store.ResidentFeatures.get).parameters) == ["self", "movie", "array"]
    s = inspect.signature(feature_store.WindowStager.stage_resident).parameters
    assert list(s)[:3] == ["self", "features_dev", "windows"] and list(s.values())[3].kind is inspect.Parameter.VAR_KEYWORD
    args = drv.parse_args([])
    assert args.device_features is False and args.device_features_mb == 2048
    args = drv.parse_args(["--device_features", "--device_features_mb", "64"])
    assert args.device_features is True and args.device_features_mb == 64
    assert "_stage_on_device" in inspect.getsource(drv._eval_in_flight) and "_stage_on_device" in inspect.getsource(drv.eval)


def test_entry_in_header_ctypes_table_sources_and_both_libraries():
    from revisionllm_amd import build
    header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    declared = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", header))
    assert "#define RV_ABI_VERSION 5" in header and "gather.hip" in build.SOURCES
    if not all(os.path.exists(p) for p in hip.LIB_PATHS.values()):
        build.build_library()
    assert "rv_window_gather" in declared and "rv_window_gather" in hip.SIGNATURES and declared == set(hip.SIGNATURES)
    params = re.search(r"\brv_window_gather\s*\(([^)]*)\)", header).group(1)
    assert len(params.split(",")) == len(hip.SIGNATURES["rv_window_gather"][1]) == 17
    for flavour, path in hip.LIB_PATHS.items():
        assert hasattr(ctypes.CDLL(path), "rv_window_gather"), flavour
        assert hip.lib(flavour).rv_abi_version() == 5
    comment = re.search(r"/\* ---- the recursion's window tensor.*?\*/", header, re.S).group(0)
    for word in ("np.linspace", "float64", "NOT fused", "(0, 130, 31)", "bit for bit", "65504", "all-zero", "1048576", "65536", "the same code", "NULL"):
        assert word in comment, word                                           # the definition stands in the header
    source = open(os.path.join(ROOT, "revisionllm_amd", "csrc", "gather.hip")).read()
    assert '#include "grounding.h"' in source and "duration_frames(block_mask_sum" in source and "ws_bounds(" in source
    for word in ("__ddiv_rn", "__dmul_rn", "__dadd_rn"):
        assert word in source, word


def _refused(rc, message):
    return rc == RV_ERR_ARG and message in hip.last_error()


def test_every_refusal_of_rv_window_gather_comes_before_any_launch():
    """Dummy device pointers: a call that got as far as a launch would fault, so a clean RV_ERR_ARG with its message shows the check came first."""
    one = ctypes.c_void_p(64)
    for flavour in hip.LIB_PATHS:
        f = hip.lib(flavour).rv_window_gather
        own, other = (hip.RV_F16, hip.RV_BF16) if flavour == "f16" else (hip.RV_BF16, hip.RV_F16)
        good = dict(video=one, video_dtype=hip.RV_F32, ldv=16, mask=one, select=one, R=6, rpm=3, L=100, d=16, win=10, stride=5, keep=4, F=7, out=one,
                    out_dtype=own, frame_idx=one)

        def call(**kw):
            a = {**good, **kw}
            return f(a["video"], a["video_dtype"], a["ldv"], a["mask"], a["select"], a["R"], a["rpm"], a["L"], a["d"], a["win"], a["stride"], a["keep"],
                     a["F"], a["out"], a["out_dtype"], a["frame_idx"], None)
        for name in ("video", "select", "out"):
            assert _refused(call(**{name: None}), "rv_window_gather: bad arguments"), (flavour, name)
        for kw in (dict(R=0), dict(R=-3), dict(rpm=0), dict(rpm=-1), dict(R=7), dict(R=2, rpm=3)):
            assert _refused(call(**kw), "rv_window_gather: R=%d rows with rpm=%d" % (kw.get("R", 6), kw.get("rpm", 3))), kw
        for L in (0, -1, 1048577):
            assert _refused(call(L=L), "rv_window_gather: L=%d must be in [1, 1048576]" % L)
        for kw in (dict(d=0), dict(d=-1), dict(ldv=15), dict(ldv=0), dict(ldv=-16)):
            assert _refused(call(**kw), "rv_window_gather: d=%d columns with a frame stride of ldv=%d" % (kw.get("d", 16), kw.get("ldv", 16))), kw
        for kw in (dict(stride=0), dict(stride=-1), dict(win=4), dict(win=0), dict(win=101), dict(win=200, stride=100)):
            assert _refused(call(**kw), "rv_window_gather: win=%d frames with stride=%d" % (kw.get("win", 10), kw.get("stride", 5))), kw
        for keep in (0, -1):
            assert _refused(call(keep=keep), "rv_window_gather: keep=%d must be at least 1" % keep)
        for F in (0, -1, 65537):
            assert _refused(call(F=F), "rv_window_gather: F=%d must be in [1, 65536]" % F)
        for dt in (other, hip.RV_I32, hip.RV_U8, -1, 6):
            assert _refused(call(video_dtype=dt), "rv_window_gather: video_dtype must be f32 or " + ("fp16" if flavour == "f16" else "bf16")), dt
            assert _refused(call(out_dtype=dt), "rv_window_gather: out_dtype must be f32 or " + ("fp16" if flavour == "f16" else "bf16")), dt
        assert _refused(call(R=2 ** 24, rpm=1, keep=1), "rv_window_gather: R=16777216 rows of keep=1 entries")
        assert _refused(call(R=4096, rpm=1, keep=4096), "rv_window_gather: R=4096 rows of keep=4096 entries")


def test_python_side_refusals_come_before_the_device_is_looked_for():
    from revisionllm_amd import ops
    v, s = torch.zeros(2, 40, 8), torch.zeros(2, 3, 4, dtype=torch.int32)
    good = dict(win=10, stride=5, num_frames=7)
    keywords = [dict(win=0), dict(win=-5), dict(win=10.0), dict(win=None), dict(win=True), dict(win=4), dict(win=41), dict(stride=0), dict(stride=2.0),
                dict(stride=11), dict(num_frames=0), dict(num_frames=-1), dict(num_frames=2.5), dict(num_frames=None), dict(num_frames=65537),
                dict(win=2 ** 31), dict(out_dtype=torch.int32), dict(out_dtype="f16"), dict(out_dtype=torch.float64), dict(mask=torch.ones(2, 41)),
                dict(mask=torch.ones(40)), dict(mask=torch.ones(2, 40, dtype=torch.complex64)), dict(mask=[[1.0] * 40] * 2)]
    shapes = [dict(video=torch.zeros(40)), dict(video=torch.zeros(2, 2, 40, 8)), dict(video=torch.zeros(3, 40, 8)), dict(video=torch.zeros(40, 8)),
              dict(video=torch.zeros(2, 40, 8, dtype=torch.int64)), dict(video=torch.zeros(2, 40, 8, dtype=torch.float64)), dict(video=torch.zeros(2, 0, 8)),
              dict(select=torch.zeros((), dtype=torch.int32)), dict(select=torch.zeros(1, 2, 3, 4, dtype=torch.int32)), dict(select=torch.zeros(2, 3, 0, dtype=torch.int32)),
              dict(select=torch.zeros(3, 4, dtype=torch.int32)), dict(select=torch.zeros(2, 3, 4, dtype=torch.int64)), dict(select=torch.zeros(2, 3, 4)),
              dict(select=[[0, 1]]), dict(video=np.zeros((2, 40, 8), np.float32))]
    for kw in keywords:
        with pytest.raises(ValueError, match="window_gather"):
            ops.window_gather(v, s, **{**good, **kw})
    for kw in shapes:
        a = {**dict(video=v, select=s), **kw}
        with pytest.raises(ValueError, match="window_gather"):
            ops.window_gather(a["video"], a["select"], **good)
    with pytest.raises(ValueError, match="no cross-type 16-bit conversion"):
        ops.window_gather(v.half(), s, out_dtype=torch.bfloat16, **good)
    with pytest.raises(ValueError, match="no cross-type 16-bit conversion"):
        ops.window_gather(v.bfloat16(), s, out_dtype=torch.float16, **good)
    with pytest.raises(ValueError, match="at most 1048576"):
        ops.window_gather(torch.zeros(1048577, 1), s[0, 0], **good)
    with pytest.raises(TypeError):
        ops.window_gather(v, s, 10, 5, 7)                                          # keyword-only
    with pytest.raises(TypeError):
        ops.window_gather(v, s, win=10, stride=5)                                  # num_frames has no default
    assert ops.window_gather_keywords("t", np.int64(10), np.int32(5), np.int64(250)) == (10, 5, 250)       # numpy integers are integers
    prev = hip.set_flavour("f16")
    try:
        assert ops.window_gather_dtypes("t", torch.float32, None) == (torch.float16, "f16")
        assert ops.window_gather_dtypes("t", torch.float32, torch.float32) == (torch.float32, "f16")
        assert ops.window_gather_dtypes("t", torch.bfloat16, None) == (torch.bfloat16, "bf16")
        assert ops.window_gather_dtypes("t", torch.bfloat16, torch.float32) == (torch.float32, "bf16")
        assert ops.window_gather_dtypes("t", torch.float32, torch.bfloat16) == (torch.bfloat16, "bf16")
        hip.set_flavour("bf16")
        assert ops.window_gather_dtypes("t", torch.float32, None) == (torch.bfloat16, "bf16")
        assert ops.window_gather_dtypes("t", torch.float16, None) == (torch.float16, "f16")
    finally:
        hip.set_flavour(prev)


def test_stage2_refusals():
    f, q = torch.zeros(700, 8), np.zeros(8, np.float32)
    bad_geometry = (dict(debug_window=125, feature_fps=4.5), dict(debug_window=0.5, feature_fps=5), dict(debug_window=0), dict(debug_window=-1),
                    dict(feature_fps=float("nan")), dict(debug_window="a", feature_fps=1))
    for kw in bad_geometry:
        with pytest.raises(ValueError, match="gather_windows"):
            stage2.gather_windows(f, [0], **kw)
        with pytest.raises(ValueError, match="clip_stage_windows"):
            stage2.clip_stage_windows(f, q, **kw)
    for kw in (dict(batch=0), dict(batch=2.5), dict(batch=None)):
        with pytest.raises(ValueError, match="clip_stage_windows"):
            stage2.clip_stage_windows(f, q, **kw)
    for a in (np.zeros((700, 8), np.float32), torch.zeros(700), torch.zeros(700, 8, dtype=torch.int64), torch.zeros(0, 8)):
        with pytest.raises(ValueError, match="gather_windows"):
            stage2.gather_windows(a, [0])
        with pytest.raises(ValueError, match="clip_stage_windows"):
            stage2.clip_stage_windows(a, q)
    for short in (torch.zeros(600, 8), torch.zeros(625, 8)):                       # no longer than one window: the host route's business
        with pytest.raises(ValueError, match="take the host route"):
            stage2.gather_windows(short, [0])
        with pytest.raises(ValueError, match="take the host route"):
            stage2.clip_stage_windows(short, q)
    for b in (np.zeros(9, np.float32), np.zeros((1, 8), np.float32), np.zeros(8, np.int64)):
        with pytest.raises(ValueError, match="clip_stage_windows"):
            stage2.clip_stage_windows(f, b)
    for windows in ([5], [-6], [0, 1, 7], [1.0], [True]):                          # 700 frames: 5 windows
        with pytest.raises(IndexError, match="gather_windows"):
            stage2.gather_windows(f, windows)
    with pytest.raises(ValueError, match="gather_windows"):
        stage2.gather_windows(f, torch.zeros(2, 2, dtype=torch.int32))
    with pytest.raises(TypeError):
        stage2.gather_windows(f, [0], 125)                                         # keyword-only
    assert stage2.gather_windows(f, [], num_frames=9, dtype=torch.float32).shape == (0, 9, 8)
    for ctx_l in (1, 124, 125, 126, 625, 626, 3000, 36000):
        for g in ((125, 5, 5), (125, 5.0, 5), (2, 5, 4), (26, 5, 1)):
            assert stage2.window_count(ctx_l, *g) == len(stage2.cut_windows(ctx_l, *g, num_frames=2)[0])


# ------------------------------------------------------------------ the oracle ------------------------------------------------------------------
def test_oracle_indices_are_cut_windows():
    """Every ctx_l of the driver's geometry from the first video longer than a window to 2999 at F = 250, and three small geometries at the other
    frame counts: the oracle's [W, F] table is ``cut_windows``' frame_idx."""
    for ctx_l in range(626, 3000):
        _, idx = stage2.cut_windows(ctx_l, 125, 5, 5, 250)
        got = GO.frame_indices(ctx_l, 625, 5, 250)
        assert got.shape == idx.shape and np.array_equal(got, idx), ctx_l
    for (dw, fps, stride), upto in (((2, 5, 4), 120), ((3, 3, 4), 120), ((26, 5, 1), 600)):
        win = dw * fps
        for F in (1, 2, 3, 31, 251):
            for ctx_l in range(win + 1, upto):
                _, idx = stage2.cut_windows(ctx_l, dw, fps, stride, F)
                got = GO.frame_indices(ctx_l, win, stride, F)
                assert got.shape == idx.shape and np.array_equal(got, idx), (dw, fps, stride, F, ctx_l)
                assert idx.shape[0] == len(WO.windows(ctx_l, win, stride)) and (idx.size == 0 or (0 <= idx.min() and idx.max() < ctx_l))


def test_oracle_linspace_is_numpys():
    """The float64 rule against ``np.linspace(..., dtype=int32)``; (0, 130, 31) is a triple where the integer shortcut gives another frame."""
    deltas = list(range(1, 700)) + [1023, 1024, 1100, 2999]
    differ = 0
    for F in (1, 2, 3, 7, 31, 64, 65, 250, 251, 256):
        for s in (0, 1, 125, 1000, 35375):
            for delta in deltas:
                want = np.linspace(s, s + delta, F, dtype=np.int32).tolist()
                got = GO.linspace_index(s, s + delta, F)
                assert list(got) == want, (s, delta, F)
                differ += list(GO.integer_shortcut(s, s + delta, F)) != want
    assert differ > 0
    assert list(GO.linspace_index(0, 130, 31)) == np.linspace(0, 130, 31, dtype=np.int32).tolist() != GO.integer_shortcut(0, 130, 31)
    assert GO.linspace_index(0, 130, 31)[27] == 116 and GO.integer_shortcut(0, 130, 31)[27] == 117
    assert list(GO.linspace_index(0, 61, 8)) == np.linspace(0, 61, 8, dtype=np.int32).tolist() and GO.linspace_index(0, 61, 8)[-1] == 61 \
        and int(7 * (61 / 7)) == 60                                                # the last one is set, not computed
    assert list(GO.linspace_index(7, 7, 5)) == [7] * 5 and list(GO.linspace_index(3, 9, 1)) == [3] and list(GO.linspace_index(3, 9, 2)) == [3, 9]


def test_oracle_gather_on_a_small_case():
    video = torch.arange(2 * 30 * 2, dtype=torch.float32).view(2, 30, 2)
    mask = (np.arange(30)[None, :] < np.array([[30], [12]])).astype(np.float32)
    out, idx, D = GO.gather(video, mask, [[0, 2, -1], [1, 9, 0]], 8, 4, 3, torch.float16)
    assert D == [30, 12] and idx[0, 0].tolist() == [0, 4, 8] and idx[0, 1].tolist() == [4, 8, 12] and idx[0, 2].tolist() == [-1] * 3
    assert idx[1, 0].tolist() == [2, 6, 10] and idx[1, 1].tolist() == [-1] * 3 and idx[1, 2].tolist() == [0, 4, 8]
    assert out.dtype == torch.float16 and out[0, 1, :, 0].tolist() == [8.0, 16.0, 24.0] and out[1, 2, :, 1].tolist() == [61.0, 69.0, 77.0]
    assert not bool(out[0, 2].any()) and not bool(out[1, 1].any())
    big = torch.tensor([7e4, -7e4, float("inf"), 1.0])
    assert GO.convert(big, torch.float16, saturate=True).tolist() == [65504.0, -65504.0, 65504.0, 1.0]
    assert GO.convert(big, torch.float16).tolist()[:2] == [float("inf"), -float("inf")] and GO.convert(big, torch.float32) is big


# ------------------------------------------------------------------ the movie cache ------------------------------------------------------------------
def test_resident_features_on_the_cpu():
    from revisionllm_amd.data.feature_store import ResidentFeatures
    a = np.arange(100 * 8, dtype=np.float32).reshape(100, 8)                       # 3200 bytes
    cache = ResidentFeatures("cpu", 3200 * 3, op_dtype="f16")
    ta = cache.get("a", a)
    assert ta.dtype == torch.float32 and ta.shape == (100, 8) and torch.equal(ta, torch.from_numpy(a)) and (cache.hits, cache.misses) == (0, 1)
    assert cache.get("a", None) is ta and (cache.hits, cache.misses) == (1, 1)     # a hit does not look at the array
    tb, tc = cache.get("b", a + 1), cache.get("c", a + 2)
    assert cache.movies() == ["a", "b", "c"] and cache.bytes == 9600 and len(cache) == 3
    assert cache.get("a", a) is ta and cache.movies() == ["b", "c", "a"]           # used again: the youngest
    td = cache.get("d", a + 3)                                                     # evicts the least recently used: b
    assert cache.movies() == ["c", "a", "d"] and "b" not in cache and cache.evictions == 1 and cache.bytes == 9600
    assert cache.get("b", a + 1) is not tb and cache.movies() == ["a", "d", "b"]   # uploaded again, c goes
    wide = np.zeros((200, 8), np.float32)                                          # 6400 bytes: two entries go
    cache.get("w", wide)
    assert cache.movies() == ["b", "w"] and cache.bytes == 9600
    huge = np.zeros((301, 8), np.float32)                                          # above the whole budget: handed back, not kept, nothing evicted
    th = cache.get("h", huge)
    assert th.shape == (301, 8) and "h" not in cache and cache.movies() == ["b", "w"] and cache.get("h", huge) is not th
    assert torch.equal(tc, torch.from_numpy(a + 2)) and torch.equal(td, torch.from_numpy(a + 3))      # an evicted tensor stays valid for its holder
    # dtype policy: f32 stays; a 16-bit array stays when it is the engine's operand type, else becomes f32 (exact); anything else becomes f32
    h = (np.arange(64, dtype=np.float32).reshape(8, 8) / 7).astype(np.float16)
    for op, kept in (("f16", torch.float16), ("bf16", torch.float32)):
        c = ResidentFeatures("cpu", 1 << 20, op_dtype=op)
        t = c.get("h", h)
        assert t.dtype == kept and torch.equal(t.float(), torch.from_numpy(h).float()) and c.bytes == 64 * (2 if kept == torch.float16 else 4)
        assert c.get("d", h.astype(np.float64)).dtype == torch.float32 and c.get("t", torch.from_numpy(h)).dtype == kept
        b16 = torch.from_numpy(h).bfloat16()
        assert c.get("b", b16).dtype == (torch.bfloat16 if op == "bf16" else torch.float32) and torch.equal(c.get("b", None).float(), b16.float())
        assert c.kept_dtype(torch.float32) == torch.float32
    for bad in (np.zeros(8, np.float32), np.zeros((2, 2, 2), np.float32), np.zeros((4, 4), np.int64)):
        with pytest.raises(ValueError, match="ResidentFeatures"):
            cache.get("bad", bad)
    assert "bad" not in cache


# ------------------------------------------------------------------ the driver's flag ------------------------------------------------------------------
def test_the_driver_writes_the_same_records_with_device_features(tmp_path, monkeypatch):
    """``--device_features`` with the device stages stubbed by host arithmetic: every branch - all windows, ``--clip_prefilter``, a stage-1 record - hands
    ``run_query`` the same window list and the same tensor as the host route and writes the same records; the movie goes through ``ResidentFeatures``
    once; a video no longer than one window takes the host route; with the flag off none of the new calls is made."""
    from revisionllm_amd.data import feature_store
    from revisionllm_amd.eval import eval_nlq_retrieval_e2e2 as drv
    rs = np.random.RandomState(3)
    feat_dir, q_dir, s1_dir = tmp_path / "feats", tmp_path / "qfeats", tmp_path / "stage1"
    for d in (feat_dir, q_dir, s1_dir):
        os.makedirs(d)
    np.save(feat_dir / "movieA.npy", rs.randn(2600, 16).astype(np.float16))
    np.save(feat_dir / "short.npy", rs.randn(625, 16).astype(np.float32))          # ctx_l = clip_length: cut_windows' first start is -1
    ann = {}
    for i in range(4):
        ann[f"q{i}"] = {"movie": "short" if i == 3 else "movieA", "sentence": f"Someone opens door number {i}.", "timestamps": [10.0 * i, 10.0 * i + 4],
                        "movie_duration": 520.0}
        np.savez_compressed(q_dir / f"q{i}.npz", token_features=rs.randn(6, 16).astype(np.float32), cls_features=rs.randn(16).astype(np.float32))
    with open(tmp_path / "ann.json", "w") as f:
        json.dump(ann, f)
    with open(s1_dir / "predictions_streaming_0.txt", "w") as f:                        # q2 has a stage-1 record
        f.write(json.dumps({"query_id": "q2", "answer": ["Not Present", "From 3 to 9.", "Not Present"]}) + "\n")
    runs, routes = [], []
    picked = [1, 4, 5, 9, 12, 13, 17, 18]

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

        def stage_resident(self, features_dev, windows, **geometry):
            assert torch.is_tensor(features_dev) and sorted(geometry) == ["debug_window", "feature_fps", "num_frames", "stride"]
            routes.append(("resident", features_dev.shape[0]))
            t = host_windows(features_dev.float().numpy(), stage2.cut_windows(features_dev.shape[0], **geometry)[1][windows])
            return types.SimpleNamespace(wait=lambda: t)

    def fake_run_query(model, tokenizer, windows, qf, qc, sentence, batch, mode, grounding_windows, single):
        runs.append((sentence[-1], tuple(windows.shape), list(grounding_windows)))
        plan = stage2.plan_groups(windows.shape[0], batch)
        digest = float(windows.double().sum())                                             # the tensor itself goes into the record
        return dict(answers=["In video 3."] * len(plan), starts=[p[1] for p in plan], indexes=[list(range(p[2] - p[1])) for p in plan],
                    hierarchy_zooms=[p[0] for p in plan], max_entropy=[1.0] * len(plan), mean_entropy=[2.0] * len(plan), score_cos=[digest] * len(plan),
                    grounding_windows=grounding_windows, plan=plan)

    def fake_clip_grounding_windows(features, query_cls, **kw):
        routes.append(("clip host", len(features)))
        return [i for i in picked if i < stage2.window_count(len(features))]

    def fake_clip_stage_windows(features_dev, query_cls, **kw):
        assert torch.is_tensor(features_dev) and kw["batch"] == 8 and kw["num_frames"] == 250 and kw["dtype"] == torch.float16
        routes.append(("clip resident", features_dev.shape[0]))
        geometry = {n: kw[n] for n in ("debug_window", "feature_fps", "stride", "num_frames")}
        return list(picked), host_windows(features_dev.float().numpy(), stage2.cut_windows(features_dev.shape[0], **geometry)[1][picked])

    uploads = []
    real_upload = feature_store.ResidentFeatures._upload
    monkeypatch.setattr(feature_store.ResidentFeatures, "_upload", lambda self, array: (uploads.append(array.shape), real_upload(self, array))[1])
    monkeypatch.setattr(feature_store, "WindowStager", FakeStager)
    monkeypatch.setattr(stage2, "run_query", fake_run_query)
    monkeypatch.setattr(stage2, "clip_grounding_windows", fake_clip_grounding_windows)
    monkeypatch.setattr(stage2, "clip_stage_windows", fake_clip_stage_windows)
    base = ["--data_path", str(tmp_path / "ann.json"), "--feat_folder", str(feat_dir), "--q_feat_dir", str(q_dir), "--batch", "8", "--vis_feat_storage", "npy",
            "--grounding_path", str(s1_dir), "--debug", "True"]
    model = types.SimpleNamespace(device=torch.device("cpu"))
    W = len(stage2.cut_windows(2600)[0])
    records = {}
    for name, flags in (("off", []), ("on", ["--device_features"]), ("clip off", ["--clip_prefilter"]), ("clip on", ["--clip_prefilter", "--device_features"])):
        del runs[:], routes[:], uploads[:]
        assert drv.eval(drv.parse_args(base + ["--log_path", str(tmp_path / name)] + flags), tokenizer=None, model=model) == (4, [])
        records[name] = [json.loads(line) for line in open(tmp_path / name / "predictions_streaming_0.txt")]
        clip, on = "clip" in name, "on" in name
        n = 8 if clip else W
        assert [r[:2] for r in runs] == [("0", (n, 250, 16)), ("1", (n, 250, 16)), ("2", (8, 250, 16)), ("3", (1 if clip else 4, 250, 16))], name
        first = [("clip resident", 2600)] if clip and on else [("clip host", 2600), ("host", 2600)] if clip else [("resident" if on else "host", 2600)]
        short = [("clip host", 625)] * clip + [("host", 625)]                                  # the short video: the host route, flag or not
        assert routes == first * 2 + [("resident" if on else "host", 2600)] + short, (name, routes)
        assert uploads == ([(2600, 16)] if on else []), name                                   # one upload for the movie's three queries
    assert records["on"] == records["off"] and records["clip on"] == records["clip off"] and records["off"] != records["clip off"]
    assert len(records["on"]) == 4 and records["on"][0]["info"]["score_cos"][0] != 0.0
