"""Span proposals on the host: the package surface of ``rv_span_propose`` (names under both module names, signatures, header, ctypes table, both
libraries, every refusal of the C entry before a launch, every Python-side refusal before a device is looked for) - these fail without the feature.
The rest guards the oracle of tests/propose_oracle.py, which the GPU tests compare the kernel with: it is held to an independently written brute-force
statement of the rule, the span encoding is held to the f32 window rule of tests/similarity_oracle.py, and the degenerate rows give nothing.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import propose_oracle as P
import similarity_oracle as S
from revisionllm_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_ERR_ARG = -1              # include/revision_hip.h: rv_status
LEVELS = (0.5, 0.6, 0.7, 0.8, 0.9)


# ------------------------------------------------------------------ surface ------------------------------------------------------------------
def test_the_names_import_from_both_module_names():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import similarity
    assert callable(ops.span_propose) and callable(ops.span_propose_keywords) and ops.SPAN_PROPOSE_MAX_LEVELS == 8
    assert callable(similarity.propose_spans) and callable(similarity.ground_queries)
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
import revisionllm_amd.eval.similarity as real
import revisionllm_amd.ops as real_ops
from revisionllm.eval.similarity import propose_spans, ground_queries, Grounding
from revisionllm.ops import span_propose, span_propose_keywords, SpanProposals, SPAN_PROPOSE_MAX_LEVELS
import vtimellm.eval.similarity as old
import vtimellm.ops as old_ops
assert propose_spans is real.propose_spans and old.propose_spans is real.propose_spans
assert ground_queries is real.ground_queries and old.ground_queries is real.ground_queries and Grounding is real.Grounding is old.Grounding
assert span_propose is real_ops.span_propose is old_ops.span_propose and SpanProposals is real_ops.SpanProposals is old_ops.SpanProposals
assert span_propose_keywords is old_ops.span_propose_keywords and SPAN_PROPOSE_MAX_LEVELS == old_ops.SPAN_PROPOSE_MAX_LEVELS == 8
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_signatures_and_fields():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import similarity
    keywords = dict(levels=LEVELS, relative=True, smooth=1, gap=0, min_len=1, max_len=None, max_spans=256, return_windows=False, return_smoothed=False)
    for fn in (ops.span_propose, similarity.propose_spans):
        p = inspect.signature(fn).parameters
        assert list(p) == ["sims", "mask"] + list(keywords)
        assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in keywords)
        assert {n: p[n].default for n in keywords} == keywords
    g = inspect.signature(similarity.ground_queries).parameters
    assert list(g) == ["text", "video", "mask", "top", "nms_iou", "k", "pooling", "temperature", "gt", "hit_iou", "propose_keywords"]
    assert all(g[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(g)[3:-1]) and g["propose_keywords"].kind is inspect.Parameter.VAR_KEYWORD
    assert {n: g[n].default for n in list(g)[3:-1]} == dict(top=10, nms_iou=0.5, k=3, pooling="topk", temperature=0.01, gt=None, hit_iou=ops.HIT_IOU)
    assert ops.SpanProposals._fields == ("spans", "n_spans", "n_found", "windows", "smoothed")
    assert similarity.Grounding._fields == ("spans", "scores", "n_keep", "proposals", "rank")
    assert "rv_span_propose" in similarity.__doc__ and "ground_queries" in similarity.__doc__


def test_entry_in_header_ctypes_table_and_both_libraries():
    header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    declared = set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", header))
    assert "#define RV_ABI_VERSION 5" in header
    if not all(os.path.exists(p) for p in hip.LIB_PATHS.values()):
        from revisionllm_amd import build
        build.build_library()
    assert "rv_span_propose" in declared and "rv_span_propose" in hip.SIGNATURES
    assert declared == set(hip.SIGNATURES)                                     # the table is the header, no more and no less
    params = re.search(r"\brv_span_propose\s*\(([^)]*)\)", header).group(1)
    assert len(params.split(",")) == len(hip.SIGNATURES["rv_span_propose"][1]) == 19
    for flavour, path in hip.LIB_PATHS.items():
        assert hasattr(ctypes.CDLL(path), "rv_span_propose"), flavour
        assert hip.lib(flavour).rv_abi_version() == 5
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
        if nm.returncode == 0:                                                 # the library exports the header's symbols and nothing else
            exported = {line.split()[-1] for line in nm.stdout.splitlines() if line.split() and line.split()[-2] in "TDBR"}
            assert exported == declared, (flavour, sorted(exported ^ declared))
    comment = re.search(r"/\* ---- span proposals from a similarity row.*?\*/", header, re.S).group(0)
    for word in ("build-defined", "ascending order", "strict", "l + 1", "0x7fc00000", "1048576"):     # the definition stands in the header
        assert word in comment, word


def _refused(rc, message):
    return rc == RV_ERR_ARG and message in hip.last_error()


def test_every_refusal_of_rv_span_propose_comes_before_any_launch():
    """Dummy device pointers: a call that got as far as a launch would fault, so a clean RV_ERR_ARG with its message shows the check came first."""
    one = ctypes.c_void_p(64)
    table = lambda *v: (ctypes.c_float * len(v))(*v)                          # noqa: E731
    for flavour in hip.LIB_PATHS:
        f = hip.lib(flavour).rv_span_propose
        good = dict(sims=one, mask=one, R=6, rpm=3, L=100, levels=table(*LEVELS), T=5, relative=1, smooth=5, gap=2, min_len=2, max_len=50, N=64, spans=one,
                    n_spans=one, n_found=one, windows=one, smoothed=one)

        def call(**kw):
            a = {**good, **kw}
            return f(a["sims"], a["mask"], a["R"], a["rpm"], a["L"], a["levels"], a["T"], a["relative"], a["smooth"], a["gap"], a["min_len"], a["max_len"],
                     a["N"], a["spans"], a["n_spans"], a["n_found"], a["windows"], a["smoothed"], None)
        for name in ("sims", "mask", "levels", "spans", "n_spans"):
            assert _refused(call(**{name: None}), "rv_span_propose: bad arguments"), (flavour, name)
        for kw in (dict(R=0), dict(R=-3), dict(rpm=0), dict(rpm=-1), dict(R=7), dict(R=2, rpm=3)):
            assert _refused(call(**kw), "rv_span_propose: R=%d rows with rpm=%d" % (kw.get("R", 6), kw.get("rpm", 3))), kw
        for L in (0, -1, 1048577):
            assert _refused(call(L=L), "rv_span_propose: L=%d must be in [1, 1048576]" % L)
        for T in (0, -1, 9):
            assert _refused(call(T=T), "rv_span_propose: T=%d levels (1 to 8)" % T)
        for rel in (2, -1):
            assert _refused(call(relative=rel), "rv_span_propose: relative=%d must be 0 or 1" % rel)
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert _refused(call(levels=table(0.1, bad, 0.9), T=3, relative=0), "rv_span_propose: level 1 is not finite"), bad
        assert _refused(call(levels=table(0.1, 0.5, 0.5), T=3), "rv_span_propose: levels must be strictly ascending (level 2)")
        assert _refused(call(levels=table(0.5, 0.1), T=2, relative=0), "rv_span_propose: levels must be strictly ascending (level 1)")
        assert _refused(call(levels=table(0.5, 1.0), T=2), "rv_span_propose: relative level 1 outside [0, 1)")
        assert _refused(call(levels=table(-0.25, 0.5), T=2), "rv_span_propose: relative level 0 outside [0, 1)")
        for smooth in (0, -1, 2, 64, 67):
            assert _refused(call(smooth=smooth), "rv_span_propose: smooth=%d must be odd and in [1, 65]" % smooth)
        for gap in (-1, 64):
            assert _refused(call(gap=gap), "rv_span_propose: gap=%d must be in [0, 63]" % gap)
        for min_len in (0, -2):
            assert _refused(call(min_len=min_len), "rv_span_propose: min_len=%d must be >= 1" % min_len)
        for max_len in (-1, 1):
            assert _refused(call(max_len=max_len), "rv_span_propose: max_len=%d must be 0 (no limit) or >= min_len=2" % max_len)
        for N in (0, -1, 2049):
            assert _refused(call(N=N), "rv_span_propose: N=%d spans per row (1 to 2048)" % N)


def test_python_side_refusals_come_before_the_device_is_looked_for():
    from revisionllm_amd import ops
    from revisionllm_amd.eval.similarity import ground_queries, propose_spans
    s, m = torch.zeros(2, 3, 40), torch.ones(2, 40)
    keywords = [dict(levels=()), dict(levels=tuple(i / 10 for i in range(9))), dict(levels=(0.5, 0.5)), dict(levels=(0.6, 0.5)), dict(levels=(0.5, 1.0)),
                dict(levels=(-0.1, 0.5)), dict(levels=(0.5, float("nan"))), dict(levels=(float("inf"),), relative=False), dict(levels=0.5), dict(levels=("a",)),
                dict(levels=(0.5, 0.5 + 1e-12)),                                        # equal once rounded to float32
                dict(levels=(1e39,), relative=False), dict(relative=2), dict(relative=None), dict(relative="yes"),
                dict(smooth=0), dict(smooth=2), dict(smooth=67), dict(smooth=3.0), dict(smooth=True), dict(gap=-1), dict(gap=64), dict(gap=1.5),
                dict(min_len=0), dict(min_len=1.0), dict(max_len=0), dict(min_len=5, max_len=4), dict(max_len=2.5), dict(max_spans=0), dict(max_spans=2049),
                dict(max_spans=None), dict(max_spans=8.0)]
    shapes = [dict(sims=torch.zeros(40)), dict(sims=torch.zeros(2, 3, 4, 40)), dict(mask=torch.ones(40)), dict(mask=torch.ones(2, 41)),
              dict(mask=torch.ones(3, 40)), dict(mask=torch.ones(6, 40)), dict(sims=torch.zeros(2, 3, 40, dtype=torch.int64)),
              dict(mask=torch.ones(2, 40, dtype=torch.complex64)), dict(sims=torch.zeros(2, 0, 40)), dict(sims=torch.zeros(5, 40)), dict(sims=[[0.5] * 40])]
    for fn, who in ((ops.span_propose, "span_propose"), (propose_spans, "propose_spans")):
        for kw in keywords:
            with pytest.raises(ValueError, match=who):
                fn(s, m, **kw)
        for kw in shapes:
            a = {**dict(sims=s, mask=m), **kw}
            with pytest.raises(ValueError, match=who):
                fn(a["sims"], a["mask"])
    with pytest.raises(ValueError, match="span_propose: sims must be float32"):
        ops.span_propose(s.half(), m)
    got = ops.span_propose_keywords("t", np.array([0.25, 0.5]), 1, np.int64(5), np.int32(2), 2, None, np.int64(17))
    assert got == ((0.25, 0.5), 1, 5, 2, 2, 0, 17)                                   # numpy numbers are numbers; None is "no limit" = 0
    assert ops.span_propose_keywords("t", (0.1,))[0] == (float(np.float32(0.1)),)   # the levels come back as the float32 values the kernel compares
    text, video = torch.zeros(2, 3, 8), torch.zeros(2, 40, 8)
    for kw in keywords:
        with pytest.raises(ValueError, match="ground_queries"):
            ground_queries(text, video, m, **kw)
    for kw in (dict(top=0), dict(top=2.5), dict(nms_iou=-1.0), dict(nms_iou=float("nan")), dict(k=0), dict(k=65), dict(pooling="max"),
               dict(pooling="attention", temperature=0.0), dict(hit_iou=tuple(range(17))), dict(gt=torch.zeros(2, 2)), dict(gt=torch.zeros(2, 3, 2, dtype=torch.int32))):
        with pytest.raises(ValueError, match="ground_queries"):
            ground_queries(text, video, m, **kw)
    for a in (dict(text=torch.zeros(2, 3, 9)), dict(text=torch.zeros(3, 8)), dict(text=torch.zeros(8)), dict(video=torch.zeros(2, 40)), dict(mask=torch.ones(2, 39)),
              dict(text=text.long()), dict(video=video.long()), dict(text=None)):
        b = {**dict(text=text, video=video, mask=m), **a}
        with pytest.raises(ValueError, match="ground_queries"):
            ground_queries(b["text"], b["video"], b["mask"])
    with pytest.raises(TypeError, match="ground_queries"):
        ground_queries(text, video, m, proposal=torch.zeros(2, 3, 4, 2))
    if not torch.cuda.is_available():                          # device code: a valid call raises instead of falling back to torch on the CPU
        with pytest.raises(hip.HipLibraryError):
            propose_spans(s, m)
        with pytest.raises(hip.HipLibraryError):
            ground_queries(text, video, m)


# ------------------------------------------------------------------ the oracle ------------------------------------------------------------------
def test_oracle_equals_a_brute_force_statement_of_the_rule():
    """Short random rows (D <= 40), every gap 0 .. 3, smooth 1 / 3 / 5, T 1 .. 4, both threshold forms, values on a coarse grid (ties, plateaus, equal
    thresholds) and continuous ones, a NaN now and then: the scan must give what judging every frame pair from the definition gives, with the duplicate
    test made against ALL higher levels (the oracle, like the kernel, looks at level l + 1 only)."""
    rng = np.random.default_rng(5)
    cases = runs = dupes = 0
    for gap in range(4):
        for smooth in (1, 3, 5):
            for T in range(1, 5):
                for it in range(9):
                    D = int(rng.integers(0, 41))
                    L = max(1, D + int(rng.integers(0, 3)))
                    s = (rng.integers(0, 6, L) / 4).astype(np.float32) if it % 3 else rng.normal(size=L).astype(np.float32)
                    if it % 4 == 0 and L > 2:
                        s[rng.integers(0, L, 2)] = np.nan
                    mask = (np.arange(L) < D).astype(np.float32)
                    relative = int(rng.integers(0, 2))
                    levels = sorted(rng.choice([0.0, 0.2, 0.25, 0.4, 0.5, 0.75, 0.9], T, replace=False).tolist())
                    min_len = int(rng.integers(1, 4))
                    max_len = int(rng.choice([0, min_len + 4]))
                    got, _, _, _ = P.row_runs(s, mask, levels, relative, smooth, gap, min_len, max_len)
                    assert got == P.brute(s, mask, levels, relative, smooth, gap, min_len, max_len), (gap, smooth, T, it, s.tolist(), levels)
                    loose, _, _, _ = P.row_runs(s, mask, levels, relative, smooth, gap, 1, 0)
                    per = sum(len(P.row_runs(s, mask, [lv], 0, smooth, gap, 1, 0)[0]) for lv in
                              (P.thresholds(P.smooth_row(s, D, smooth), levels, relative) or [])) if D else 0
                    cases, runs, dupes = cases + 1, runs + len(got), dupes + per - len(loose)
    assert cases == 432 and runs > 800 and dupes > 50                                   # the cases are not degenerate: runs, and duplicates dropped


def _round_trip(D, lo, hi):
    """(lo, hi) -> encode -> the f32 window rule of rv_span_scores over an array of D frames whose mask is all ones -> (lo', hi')."""
    dur = np.float32(D)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    c = ((lo32 + hi32) * np.float32(0.5)) / dur
    w = ((hi32 - lo32) - np.float32(0.5)) / dur
    assert c.dtype == np.float32 and w.dtype == np.float32
    start, end, finite = S.start_end_f32(c, w, dur)
    a, b = S.slice_lo_hi(start, end, D)
    return a, b, finite


def test_encoding_matches_the_oracle_s_and_round_trips_exhaustively_below_600_frames():
    for D in range(1, 600):
        lo, hi = np.triu_indices(D + 1, k=1)                  # every 0 <= lo < hi <= D
        a, b, finite = _round_trip(D, lo, hi)
        assert finite.all() and np.array_equal(a, lo) and np.array_equal(b, hi), D
    c, w = P.encode(3, 17, 40)                                # the oracle's scalar form is the same arithmetic
    assert (c, w) == (np.float32(np.float32(10.0) / np.float32(40)), np.float32(np.float32(13.5) / np.float32(40)))


@pytest.mark.parametrize("D", [1000, 4095, 4096, 4097, 20000, 65535, 65536, 10 ** 5, 262143, 5 * 10 ** 5, 10 ** 6, 1048576, 2 * 10 ** 6, 4 * 10 ** 6])
def test_encoding_round_trips_on_sampled_and_edge_pairs_up_to_the_frame_limit(D):
    """6 10^5 pairs: uniform ones, short spans everywhere, and spans at both ends of the row.  1048576 is the limit rv_span_propose accepts; the two sizes beyond it show the margin (at 4 10^6 the
    scaled bounds come within a rounding of the integers, which is why the limit stands where it does)."""
    rng = np.random.default_rng(D)
    n = 150000
    u = np.sort(rng.integers(0, D + 1, (n, 2)), axis=1)
    short_lo = rng.integers(0, D, n)
    short = np.stack([short_lo, np.minimum(short_lo + rng.integers(1, 9, n), D)], 1)
    head = np.stack([rng.integers(0, 4, n), rng.integers(4, D + 1, n)], 1)
    tail = np.stack([rng.integers(0, D - 3, n), D - rng.integers(0, 4, n)], 1)
    pairs = np.concatenate([u, short, head, tail])
    pairs = pairs[pairs[:, 0] < pairs[:, 1]]
    assert len(pairs) > 5 * 10 ** 5
    a, b, finite = _round_trip(D, pairs[:, 0], pairs[:, 1])
    assert finite.all() and np.array_equal(a, pairs[:, 0]) and np.array_equal(b, pairs[:, 1])


def test_padded_spans_give_the_void_window():
    out = P.propose(np.zeros((1, 12), dtype=np.float32), np.ones((1, 12)), LEVELS, N=4)
    assert out["n_spans"].tolist() == [0] and (out["spans"].view(np.uint32) == P.NAN_BITS).all() and (out["windows"] == -1).all()
    win = S.windows(torch.from_numpy(out["spans"]), torch.ones(1, 12))
    assert win.tolist() == [[list(S.NAN_WINDOW)] * 4]


def test_flat_all_nan_and_empty_rows_give_nothing():
    L = 30
    rows = np.stack([np.full(L, 0.75, dtype=np.float32), np.full(L, np.nan, dtype=np.float32), np.linspace(0, 1, L, dtype=np.float32)])
    for relative, levels in ((1, (0.0, 0.5)), (0, (0.8, 0.9))):
        out = P.propose(rows[:2], np.ones((2, L)), levels, relative=relative, smooth=3, gap=1)
        assert out["n_found"].tolist() == [0, 0]
    out = P.propose(rows[2:], np.zeros((1, L)), (0.0, 0.5), N=8)                        # D = 0
    assert out["n_found"].tolist() == [0] and out["D"] == [0] and len(out["smoothed"][0]) == 0
    out = P.propose(rows[2:], np.ones((1, L)), (0.0, 0.5), N=8)                         # the same row with its frames: levels 1 then 0, both to the end
    assert out["windows"][0, :2].tolist() == [[15, 30], [1, 30]] and out["n_found"].tolist() == [2]


def test_hand_made_rows():
    s = np.array([[0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0]], dtype=np.float32)
    m = np.ones((1, 12))
    assert P.propose(s, m, (0.5,), gap=0)["windows"][0, :3].tolist() == [[1, 3], [4, 5], [7, 10]]
    assert P.propose(s, m, (0.5,), gap=1)["windows"][0, :2].tolist() == [[1, 5], [7, 10]]                    # the gap of 2 stays open
    assert P.propose(s, m, (0.5,), gap=2)["windows"][0, :2].tolist() == [[1, 10], [-1, -1]]
    assert P.propose(s, m, (0.5,), min_len=2, max_len=2)["windows"][0, :2].tolist() == [[1, 3], [-1, -1]]
    assert P.propose(s, m, (0.25, 0.5, 0.75))["n_found"].tolist() == [3]                                     # the same runs at three levels: kept once
    stair = np.array([[0, 1, 2, 3, 2, 1, 0, 3, 0]], dtype=np.float32)
    out = P.propose(stair, np.ones((1, 9)), (0.0, 0.5, 0.9), N=8)
    assert out["windows"][0, :5].tolist() == [[3, 4], [7, 8], [2, 5], [1, 6], [-1, -1]]                      # (7, 8) is a run of all three levels
    assert P.propose(stair, np.ones((1, 9)), (1.0, 2.0, 3.0), relative=0)["windows"][0, :4].tolist() == [[3, 4], [7, 8], [2, 5], [-1, -1]]   # strict: 3 > 3 is false
