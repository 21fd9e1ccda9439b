"""Window selection on the host: the package surface of ``rv_window_select`` (names under both module names, signatures, header, ctypes table, both
libraries, every refusal of the C entry before a launch, every Python-side refusal before a device is looked for, ``window_recall``,
``clip_grounding_windows``' refusals) - these fail without the feature.  The rest guards the oracle of tests/window_oracle.py, which the GPU tests
compare the kernel with: its selection is held to an independently written brute-force statement, its window bounds to ``stage2.cut_windows``, and
its sequence to the greedy-prefix property that lets the kernel stop early.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import window_oracle as WO
from revisionllm_amd import hip
from revisionllm_amd.eval import stage2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_ERR_ARG = -1              # include/revision_hip.h: rv_status
GEOMETRIES = (((125, 5, 5), 3000), ((125, 5.0, 5), 3000), ((2, 5, 4), 400), ((3, 3, 4), 400), ((1, 7, 3), 400), ((4, 2.0, 3), 400))


# ------------------------------------------------------------------ surface ------------------------------------------------------------------
def test_the_names_import_from_both_module_names():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import metrics, similarity
    assert callable(ops.window_select) and ops.WINDOW_SELECT_MAX == 2048
    assert callable(similarity.select_windows) and callable(stage2.clip_grounding_windows) and callable(metrics.window_recall)
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
import revisionllm_amd.eval.similarity as real
import revisionllm_amd.eval.stage2 as real_stage2
import revisionllm_amd.eval.metrics as real_metrics
import revisionllm_amd.ops as real_ops
from revisionllm.eval.similarity import select_windows
from revisionllm.eval.stage2 import clip_grounding_windows
from revisionllm.eval.metrics import window_recall
from revisionllm.ops import window_select, WindowSelection, WINDOW_SELECT_MAX
import vtimellm.eval.similarity as old
import vtimellm.eval.stage2 as old_stage2
import vtimellm.eval.metrics as old_metrics
import vtimellm.ops as old_ops
assert select_windows is real.select_windows and old.select_windows is real.select_windows
assert clip_grounding_windows is real_stage2.clip_grounding_windows is old_stage2.clip_grounding_windows
assert window_recall is real_metrics.window_recall is old_metrics.window_recall
assert window_select is real_ops.window_select is old_ops.window_select and WindowSelection is real_ops.WindowSelection is old_ops.WindowSelection
assert WINDOW_SELECT_MAX == old_ops.WINDOW_SELECT_MAX == 2048
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_signatures_and_fields():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import eval_nlq_retrieval_e2e2 as drv
    from revisionllm_amd.eval import metrics, similarity
    required = ["win", "stride", "keep"]
    optional = dict(k=3, min_sep=1, gt=None, return_scores=False, return_bounds=False, return_order=False)
    for fn, lead in ((ops.window_select, ["sims", "mask"]), (similarity.select_windows, ["text", "video", "mask"])):
        p = inspect.signature(fn).parameters
        assert list(p) == lead + required + list(optional)
        assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in required + list(optional))
        assert all(p[n].default is inspect.Parameter.empty for n in required) and {n: p[n].default for n in optional} == optional
    g = inspect.signature(stage2.clip_grounding_windows).parameters
    keywords = dict(debug_window=125, feature_fps=5, stride=5, batch=100, k=3, min_sep=1)
    assert list(g) == ["features", "query_cls"] + list(keywords) and {n: g[n].default for n in keywords} == keywords
    assert all(g[n].kind is inspect.Parameter.KEYWORD_ONLY for n in keywords)
    assert "host copy" in stage2.clip_grounding_windows.__doc__
    w = inspect.signature(metrics.window_recall).parameters
    assert list(w) == ["hit_rank", "topk"] and w["topk"].default == (1, 5, 10, 50, 100)
    assert ops.WindowSelection._fields == ("select", "n_select", "n_windows", "scores", "bounds", "order", "hit_rank")
    assert "rv_window_select" in similarity.__doc__ and "select_windows" in similarity.__doc__
    assert drv.parse_args([]).clip_prefilter is False and drv.parse_args(["--clip_prefilter"]).clip_prefilter is True


def test_entry_in_header_ctypes_table_and_both_libraries():
    header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    declared = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", header))
    assert "#define RV_ABI_VERSION 5" in header
    if not all(os.path.exists(p) for p in hip.LIB_PATHS.values()):
        from revisionllm_amd import build
        build.build_library()
    assert "rv_window_select" in declared and "rv_window_select" in hip.SIGNATURES
    assert declared == set(hip.SIGNATURES)                                     # the table is the header, no more and no less
    params = re.search(r"\brv_window_select\s*\(([^)]*)\)", header).group(1)
    assert len(params.split(",")) == len(hip.SIGNATURES["rv_window_select"][1]) == 20
    for flavour, path in hip.LIB_PATHS.items():
        assert hasattr(ctypes.CDLL(path), "rv_window_select"), flavour
        assert hip.lib(flavour).rv_abi_version() == 5
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
        if nm.returncode == 0:                                                 # the library exports the header's symbols and nothing else
            exported = {line.split()[-1] for line in nm.stdout.splitlines() if line.split() and line.split()[-2] in "TDBR"}
            assert exported == declared, (flavour, sorted(exported ^ declared))
    comment = re.search(r"/\* ---- coarse window selection.*?\*/", header, re.S).group(0)
    for word in ("build-defined", "64-bit intermediate", "NaN first", "bit for bit", "kills nothing", "ascending", "0x7fc00000", "1048576", "both strict"):
        assert word in comment, word                                           # the definition stands in the header


def _refused(rc, message):
    return rc == RV_ERR_ARG and message in hip.last_error()


def test_every_refusal_of_rv_window_select_comes_before_any_launch():
    """Dummy device pointers: a call that got as far as a launch would fault, so a clean RV_ERR_ARG with its message shows the check came first."""
    one = ctypes.c_void_p(64)
    for flavour in hip.LIB_PATHS:
        f = hip.lib(flavour).rv_window_select
        good = dict(sims=one, mask=one, R=6, rpm=3, L=100, win=10, stride=5, k=3, keep=4, min_sep=2, Wcap=49, gt=one, select=one, n_select=one,
                    n_windows=one, win_scores=one, bounds=one, order=one, hit_rank=one)

        def call(**kw):
            a = {**good, **kw}
            return f(a["sims"], a["mask"], a["R"], a["rpm"], a["L"], a["win"], a["stride"], a["k"], a["keep"], a["min_sep"], a["Wcap"], a["gt"],
                     a["select"], a["n_select"], a["n_windows"], a["win_scores"], a["bounds"], a["order"], a["hit_rank"], None)
        for name in ("sims", "mask", "select", "n_select", "n_windows"):
            assert _refused(call(**{name: None}), "rv_window_select: bad arguments"), (flavour, name)
        for kw in (dict(R=0), dict(R=-3), dict(rpm=0), dict(rpm=-1), dict(R=7), dict(R=2, rpm=3)):
            assert _refused(call(**kw), "rv_window_select: R=%d rows with rpm=%d" % (kw.get("R", 6), kw.get("rpm", 3))), kw
        for L in (0, -1, 1048577):
            assert _refused(call(L=L), "rv_window_select: L=%d must be in [1, 1048576]" % L)
        for kw in (dict(stride=0), dict(stride=-1), dict(win=4), dict(win=0), dict(win=101), dict(win=200, stride=100)):
            assert _refused(call(**kw), "rv_window_select: win=%d frames with stride=%d" % (kw.get("win", 10), kw.get("stride", 5))), kw
        for k in (0, -1, 65):
            assert _refused(call(k=k), "rv_window_select: k=%d must be in [1, 64]" % k)
        for Wcap in (48, 50, 0, -1):
            assert _refused(call(Wcap=Wcap), "rv_window_select: Wcap=%d must be max(1, ceil(L / (win / stride)) - 1) = 49" % Wcap)
        assert _refused(call(L=2050, win=2, stride=2, Wcap=2049, keep=1, min_sep=1), "rv_window_select: L=2050, win=2, stride=2 give up to 2049 windows")
        for keep in (0, -1, 50):
            assert _refused(call(keep=keep), "rv_window_select: keep=%d must be in [1, Wcap=49]" % keep)
        for min_sep in (0, -1, 50):
            assert _refused(call(min_sep=min_sep), "rv_window_select: min_sep=%d must be in [1, Wcap=49]" % min_sep)
        assert _refused(call(gt=None), "rv_window_select: hit_rank needs gt")
        assert _refused(call(L=10, win=10, stride=1, Wcap=9, keep=1, min_sep=1), "rv_window_select: Wcap=9 must be")   # one hop: no window, capacity 1


def test_python_side_refusals_come_before_the_device_is_looked_for():
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import select_windows
    s, m = torch.zeros(2, 3, 40), torch.ones(2, 40)
    good = dict(win=10, stride=5, keep=4)
    keywords = [dict(win=0), dict(win=-5), dict(win=10.0), dict(win=None), dict(win=True), dict(win=4), dict(win=41), dict(stride=0), dict(stride=2.0),
                dict(stride=11), dict(keep=0), dict(keep=-1), dict(keep=2.5), dict(keep=None), dict(k=0), dict(k=65), dict(k=1.5), dict(min_sep=0),
                dict(min_sep=20), dict(min_sep=1.0), dict(win=2 ** 31), dict(gt=torch.zeros(2, 2)), dict(gt=torch.zeros(2, 3, 2, dtype=torch.int32)),
                dict(gt=[[0.0, 1.0]] * 6)]
    shapes = [dict(sims=torch.zeros(40)), dict(sims=torch.zeros(2, 3, 4, 40)), dict(mask=torch.ones(40)), dict(mask=torch.ones(2, 41)),
              dict(mask=torch.ones(3, 40)), dict(sims=torch.zeros(2, 3, 40, dtype=torch.int64)), dict(mask=torch.ones(2, 40, dtype=torch.complex64)),
              dict(sims=torch.zeros(2, 0, 40)), dict(sims=torch.zeros(5, 40)), dict(sims=[[0.5] * 40])]
    for kw in keywords:
        with pytest.raises(ValueError, match="window_select"):
            ops.window_select(s, m, **{**good, **kw})
    for kw in shapes:
        a = {**dict(sims=s, mask=m), **kw}
        with pytest.raises(ValueError, match="window_select"):
            ops.window_select(a["sims"], a["mask"], **good)
    with pytest.raises(ValueError, match="window_select: sims must be float32"):
        ops.window_select(s.half(), m, **good)
    with pytest.raises(ValueError, match="at most 2048"):
        ops.window_select(torch.zeros(1, 2050), torch.ones(1, 2050), win=2, stride=2, keep=1)
    with pytest.raises(TypeError):
        ops.window_select(s, m, 10, 5, 4)                                          # keyword-only
    with pytest.raises(TypeError):
        ops.window_select(s, m, win=10, stride=5)                                  # keep has no default
    assert ops.window_select_keywords("t", np.int64(10), np.int32(5), 7, np.int64(3), 2) == (10, 5, 7, 3, 2)       # numpy integers are integers
    assert ops.window_select_capacity("t", 40, 10, 5) == 19 and ops.window_select_capacity("t", 10, 10, 1) == 1
    text, video = torch.zeros(2, 3, 8), torch.zeros(2, 40, 8)
    for kw in keywords:
        with pytest.raises(ValueError, match="select_windows"):
            select_windows(text, video, m, **{**good, **kw})
    for a in (dict(text=torch.zeros(2, 3, 9)), dict(text=torch.zeros(3, 8)), dict(text=torch.zeros(8)), dict(video=torch.zeros(2, 40)),
              dict(mask=torch.ones(2, 39)), dict(text=text.long()), dict(video=video.long()), dict(text=None),
              dict(mask=torch.ones(2, 40, dtype=torch.complex64))):
        b = {**dict(text=text, video=video, mask=m), **a}
        with pytest.raises(ValueError, match="select_windows"):
            select_windows(b["text"], b["video"], b["mask"], **good)


def test_clip_grounding_windows_refusals():
    f, q = np.zeros((700, 8), np.float32), np.zeros(8, np.float32)
    for kw in (dict(debug_window=125, feature_fps=4.5), dict(debug_window=0.5, feature_fps=5), dict(debug_window=0), dict(debug_window=-1),
               dict(feature_fps=float("nan")), dict(debug_window="a", feature_fps=1), dict(batch=0), dict(batch=2.5), dict(batch=None),
               dict(stride=0), dict(stride=626), dict(k=0), dict(k=65), dict(min_sep=0), dict(min_sep=6, debug_window=125)):
        with pytest.raises(ValueError, match="clip_grounding_windows|select_windows"):
            stage2.clip_grounding_windows(f, q, **kw)
    for a, b in ((np.zeros(700, np.float32), q), (f, np.zeros(9, np.float32)), (f, np.zeros((1, 8), np.float32)), (np.zeros((700, 8), np.int64), q),
                 (np.zeros((0, 8), np.float32), q)):
        with pytest.raises(ValueError, match="clip_grounding_windows"):
            stage2.clip_grounding_windows(a, b)
    with pytest.raises(ValueError, match="win=625 frames for rows of L=600"):
        stage2.clip_grounding_windows(np.zeros((600, 8), np.float32), q)           # a video shorter than one window (the driver skips those)
    with pytest.raises(TypeError):
        stage2.clip_grounding_windows(f, q, 125)                                   # keyword-only


# ------------------------------------------------------------------ the metric ------------------------------------------------------------------
def test_window_recall_against_a_direct_count():
    from revisionllm_amd.eval.metrics import window_recall
    rng = np.random.default_rng(0)
    hr = rng.integers(-1, 120, size=(7, 13)).astype(np.int32)
    hr[0, :4] = [-1, 0, 1, 100]
    topk = (1, 5, 10, 50, 100)
    want = [sum(1 for v in hr.reshape(-1) if 0 <= v < kk) / hr.size for kk in topk]
    for given in (hr, torch.from_numpy(hr), hr.reshape(-1), hr.astype(np.int64)):
        got = window_recall(given)
        assert isinstance(got, list) and got == want
    assert window_recall(hr, topk=(3,)) == [sum(1 for v in hr.reshape(-1) if 0 <= v < 3) / hr.size]
    assert window_recall(np.array([-1, -1])) == [0.0] * 5 and window_recall(np.array([0])) == [1.0] * 5
    assert window_recall(np.zeros(0, np.int32)) is None
    for bad in ((), (0,), (1, -2), 5, ("a",)):
        with pytest.raises(ValueError, match="window_recall"):
            window_recall(hr, topk=bad)
    # the reference's count (evaluate_pre_filtered_window.py:56-73) on the same selections: any of the first K windows is a true window
    seqs = [list(rng.permutation(30)) for _ in range(40)]
    truths = [set(rng.choice(30, size=int(rng.integers(1, 4)), replace=False).tolist()) for _ in range(40)]
    ranks = np.array([next(p for p, i in enumerate(sq) if i in tr) for sq, tr in zip(seqs, truths)])
    ref = [sum(any(i in tr for i in sq[:kk]) for sq, tr in zip(seqs, truths)) / 40 for kk in topk]
    assert window_recall(ranks) == ref


# ------------------------------------------------------------------ the oracle ------------------------------------------------------------------
def test_oracle_bounds_are_cut_windows():
    for (dw, fps, stride), upto in GEOMETRIES:
        win = int(dw * fps)
        for ctx_l in range(1, upto):
            times, idx = stage2.cut_windows(ctx_l, dw, fps, stride, num_frames=2)
            wins = WO.windows(ctx_l, win, stride)
            assert len(wins) == len(times) == idx.shape[0] and (ctx_l < win or len(wins) <= WO.capacity(ctx_l, win, stride))
            assert [(s, e) for s, e, _, _ in wins] == [(int(s), int(e)) for s, e in times], (dw, fps, stride, ctx_l)
            assert all(0 <= lo < hi <= ctx_l and lo == max(s, 0) and hi == e + 1 for s, e, lo, hi in wins)
            assert all(a[2] <= b[2] for a, b in zip(wins, wins[1:]))
        assert WO.capacity(upto, win, stride) == max(1, len(WO.windows(upto, win, stride)))


def test_oracle_selection_against_brute_force():
    rng = np.random.default_rng(1)
    for case in range(300):
        W = int(rng.integers(0, 24))
        scores = rng.choice(np.array([0.0, -0.0, 0.25, 0.5, 0.5, 1.0, -1.0, np.nan, np.inf, -np.inf], dtype=np.float32), size=W) if case % 3 else \
            rng.normal(size=W).astype(np.float32)
        for min_sep in (1, 2, 3, 5, max(1, W)):
            seq = WO.sequence(scores, min_sep)
            assert seq == WO.brute(scores, min_sep), (scores.tolist(), min_sep)
            assert sorted(seq) == list(range(W))
            if min_sep == 1:
                assert seq == WO.rank_order(scores)
    assert WO.rank_order(np.array([0.0, -0.0, np.nan, 1.0, np.nan, -np.inf, 1.0], np.float32)) == [3, 6, 0, 1, 5, 2, 4]
    # a plateau: the best three are neighbours, pass 1 takes one of them, then the far ones, and pass 2 fills in rank order
    assert WO.sequence(np.array([0.9, 1.0, 0.8, 0.1, 0.2, 0.3], np.float32), 3) == [1, 5, 0, 2, 4, 3]


def test_oracle_greedy_prefix_and_scores():
    """What lets the kernel stop at ``keep`` taken: the first n entries of the sequence are the same however far the walk goes."""
    rng = np.random.default_rng(2)
    for _ in range(60):
        W = int(rng.integers(1, 30))
        scores = np.round(rng.normal(size=W), 1).astype(np.float32)
        for min_sep in (1, 2, 4):
            full = WO.sequence(scores, min_sep)
            order = WO.rank_order(scores)
            for keep in range(1, W + 1):                 # the walk cut off after `keep` taken, pass 2 filling only up to keep
                alive, seq = [True] * W, []
                for i in order:
                    if len(seq) == keep:
                        break
                    if alive[i]:
                        seq.append(i)
                        for j in range(W):
                            if abs(i - j) < min_sep:
                                alive[j] = False
                seq += [i for i in order if i not in seq][:keep - len(seq)]
                assert seq == full[:keep]
    s = np.array([0.5, np.nan, 0.25, 1.0, 1.0, -0.0, 3.0], np.float32)
    assert np.isnan(WO.window_score(s, 0, 4, 2)) and WO.window_score(s, 2, 7, 3) == np.float32(5.0) and WO.window_score(s, 2, 4, 64) == np.float32(1.25)
    assert WO.window_score(s, 5, 6, 3).tobytes() == np.float32(0.0).tobytes()      # 0 + -0 = +0, as the kernel's add gives it
    out = WO.select(np.stack([s, s]), np.array([[1, 1, 1, 1, 1, 1, 0]], np.float32), win=2, stride=1, k=1, keep=3, min_sep=2, gt=np.array([[2.0, 3.0], [6.0, 9.0]]))
    assert out["D"] == [6, 6] and out["n_windows"].tolist() == [2, 2] and out["bounds"][0, :2].tolist() == [[0, 3], [2, 5]]
    assert out["select"].tolist() == [[0, 1, -1]] * 2 and out["order"][0, :2].tolist() == [1, 0] and out["hit_rank"].tolist() == [0, -1]


# ------------------------------------------------------------------ the driver's flag ------------------------------------------------------------------
def test_the_driver_uses_the_clip_prefilter_only_when_asked(tmp_path, monkeypatch):
    """``--clip_prefilter`` with the device stages stubbed out: a query without a stage-1 record gets its windows from ``clip_grounding_windows`` (the
    driver's geometry and ``--batch`` handed over, ``frame_idx`` indexed by the result, the list passed on to ``run_query``); a query with a stage-1
    record keeps ``prefilter_windows``; with the flag off the new call is never made and every window runs."""
    import json
    import types
    from revisionllm_amd.data import feature_store
    from revisionllm_amd.eval import eval_nlq_retrieval_e2e2 as drv
    rs = np.random.RandomState(3)
    feat_dir, q_dir, s1_dir = tmp_path / "feats", tmp_path / "qfeats", tmp_path / "stage1"
    for d in (feat_dir, q_dir, s1_dir):
        os.makedirs(d)
    np.save(feat_dir / "movieA.npy", rs.randn(2600, 16).astype(np.float16))
    ann = {}
    for i in range(3):
        ann[f"q{i}"] = {"movie": "movieA", "sentence": f"Someone opens door number {i}.", "timestamps": [10.0 * i, 10.0 * i + 4], "movie_duration": 520.0}
        np.savez_compressed(q_dir / f"q{i}.npz", token_features=rs.randn(6, 16).astype(np.float32), cls_features=rs.randn(16).astype(np.float32))
    with open(tmp_path / "ann.json", "w") as f:
        json.dump(ann, f)
    with open(s1_dir / "predictions_streaming_0.txt", "w") as f:                        # q2 has a stage-1 record
        f.write(json.dumps({"query_id": "q2", "answer": ["Not Present", "From 3 to 9.", "Not Present"]}) + "\n")
    runs, asked = [], []

    class FakeStager:
        def __init__(self, device, op_dtype=None):
            pass

        def stage_windows(self, features, frame_idx):
            t = torch.zeros(frame_idx.shape[0], 1, 1)
            return types.SimpleNamespace(wait=lambda: t)

    def fake_run_query(model, tokenizer, windows, qf, qc, sentence, batch, mode, grounding_windows, single):
        runs.append((sentence[-1], windows.shape[0], list(grounding_windows)))
        plan = stage2.plan_groups(windows.shape[0], batch)
        return dict(answers=["In video 3."] * len(plan), starts=[p[1] for p in plan], indexes=[list(range(p[2] - p[1])) for p in plan],
                    hierarchy_zooms=[p[0] for p in plan], max_entropy=[1.0] * len(plan), mean_entropy=[2.0] * len(plan), score_cos=[0.5] * len(plan),
                    grounding_windows=grounding_windows, plan=plan)

    def fake_clip_grounding_windows(features, query_cls, **kw):
        asked.append((features.shape, np.asarray(query_cls).shape, kw))
        return [1, 4, 5, 9, 12, 13, 17, 18]

    monkeypatch.setattr(feature_store, "WindowStager", FakeStager)
    monkeypatch.setattr(stage2, "run_query", fake_run_query)
    monkeypatch.setattr(stage2, "clip_grounding_windows", fake_clip_grounding_windows)
    base = ["--data_path", str(tmp_path / "ann.json"), "--feat_folder", str(feat_dir), "--q_feat_dir", str(q_dir), "--batch", "8", "--vis_feat_storage", "npy",
            "--grounding_path", str(s1_dir), "--debug", "True"]
    model = types.SimpleNamespace(device=torch.device("cpu"))
    W = len(stage2.cut_windows(2600)[0])
    assert drv.eval(drv.parse_args(base + ["--log_path", str(tmp_path / "off")]), tokenizer=None, model=model) == (3, [])
    assert asked == [] and [r[:2] for r in runs] == [("0", W), ("1", W), ("2", 8)] and runs[0][2] == list(range(W))
    with_record = runs[2][2]
    del runs[:]
    assert drv.eval(drv.parse_args(base + ["--log_path", str(tmp_path / "on"), "--clip_prefilter"]), tokenizer=None, model=model) == (3, [])
    assert [r[:2] for r in runs] == [("0", 8), ("1", 8), ("2", 8)] and runs[0][2] == runs[1][2] == [1, 4, 5, 9, 12, 13, 17, 18] and runs[2][2] == with_record
    assert len(asked) == 2 and asked[0][0] == (2600, 16) and asked[0][1] == (16,)
    assert asked[0][2] == dict(debug_window=125, feature_fps=5.0, stride=5, batch=8)
