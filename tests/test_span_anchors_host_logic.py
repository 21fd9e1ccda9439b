"""Multi-scale sliding-window proposals on the host: what the GPU items of tests/test_gpu_span_anchors.py rely on, and the package surface of
``rvc_span_anchors``.  First the oracle of tests/span_anchors_oracle.py itself: it equals an independently written brute-force statement on seeded
random and quantised rows with hidden frames (where ties are common), its anchor enumeration for every D in 1 .. 300, the encoding round trip of
anchors through the f32 window rule - the refine oracle's copy AND ``rv_span_scores``' own oracle (tests/similarity_oracle.py) - and the planted rows:
one outlier frame and a modest plateau, which the threshold generator (tests/propose_oracle.py) never proposes and this one ranks first.  Then the
surface: names under both module names, signatures, header == ctypes table == exports with the new names among them, every refusal of the C entries
before a launch, every Python-side refusal before a device is looked for - these fail without the feature.  No GPU."""
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
import similarity_oracle as SO
import span_anchors_oracle as AO
import span_refine_oracle as RO
from helpers import assert_grounding_rule_is_shared
from revisionllm_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_ERR_ARG = -1              # include/revision_hip.h: rv_status
F = np.float32
NAN, INF = float("nan"), float("inf")


def same(a, b, what):
    for name in a:
        x, y = a[name], b[name]
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) if x.dtype == F else np.array_equal(x, y), (what, name)


# ------------------------------------------------------------------ the oracle ------------------------------------------------------------------
def test_oracle_against_brute_force():
    rng = np.random.default_rng(26)
    peaks = cut = tied_cut = inadmissible = 0
    for case in range(160):
        L = int(rng.integers(1, 91))
        R = 2
        Ds = rng.integers(0, L + 1, R)
        if case % 5 == 0:
            Ds[0] = L
        mask = (np.arange(L)[None, :] < Ds[:, None]).astype(F)
        kind = case % 4
        sims = rng.uniform(-1.2, 1.2, (R, L)).astype(F) if kind == 1 else np.round(rng.uniform(-1, 1, (R, L)) * 2).astype(F) / 2     # (mostly: many ties)
        if kind == 3:
            sims[:] = F(0.25)
        sims[rng.random((R, L)) < 0.08] = NAN
        valid = None if case % 3 == 0 else rng.choice(np.array([1.0, 1.0, 1.0, 0.0, -0.0, NAN, 2.0], dtype=F), (R, L))
        S = int(rng.integers(1, 5))
        scales = []
        for _ in range(S):
            length = int(rng.integers(1, 14))
            scales.append((length, int(rng.integers(1, length + 1)), int(rng.integers(1, 9))))
        mode, peak, min_usable = case % 2, int(rng.choice([0, 1, 2, 5, 64])), int(rng.choice([1, 1, 2, 4]))
        full = AO.anchors(sims, mask, valid, 1, scales, mode, peak, min_usable, 2048)
        same(full, AO.anchors(sims, mask, valid, 1, scales, mode, peak, min_usable, 2048, brute=True), (case, "uncut"))
        assert (full["n_spans"] == full["n_found"]).all()
        peaks += int(full["n_found"].sum())
        inadmissible += int(sum(len(AO.anchor_starts(Ds[r], ln, st)) for r in range(R) for ln, st, _ in scales) > 0 and full["n_found"].sum() == 0)
        for N in sorted({1, max(1, int(full["n_found"].max()) - 1), max(1, int(full["n_found"].max() // 2))}):
            a = AO.anchors(sims, mask, valid, 1, scales, mode, peak, min_usable, N)
            same(a, AO.anchors(sims, mask, valid, 1, scales, mode, peak, min_usable, N, brute=True), (case, N))
            for r in range(R):
                n, nf = a["n_spans"][r], a["n_found"][r]
                assert nf == full["n_found"][r] and n == min(nf, N)
                assert (a["windows"][r, n:] == -1).all() and np.isnan(a["spans"][r, n:]).all() and np.isnan(a["scores"][r, n:]).all() and (a["scale"][r, n:] == -1).all()
                order = [(a["scale"][r, i], a["windows"][r, i, 0]) for i in range(n)]
                assert order == sorted(order)
                if nf > N:
                    cut += 1
                    # the kept scores are the N largest of the uncut call, and a dropped peak never beats a kept one
                    allsc = np.sort(full["scores"][r, :nf].astype(np.float64))[::-1]
                    assert np.array_equal(np.sort(a["scores"][r, :n].astype(np.float64))[::-1], allsc[:N])
                    tied_cut += int(allsc[N - 1] == allsc[N])
    assert peaks > 2000 and cut > 150 and tied_cut > 40 and inadmissible > 3, (peaks, cut, tied_cut, inadmissible)


def test_anchor_enumeration_for_every_duration():
    for length, stride in ((1, 1), (7, 1), (7, 3), (7, 7), (16, 4), (40, 10), (25, 6), (300, 75), (299, 2)):
        for D in range(1, 301):
            starts = AO.anchor_starts(D, length, stride)
            if length > D:
                assert starts == []
                continue
            regular = [i * stride for i in range(D) if i * stride + length <= D]
            flush = (D - length) % stride != 0
            assert starts == regular + ([D - length] if flush else []), (length, stride, D)
            assert starts[0] == 0 and starts[-1] == D - length and len(set(starts)) == len(starts) and starts == sorted(starts)
            # the count the kernel and its workspace use, and its monotonicity in D (a row of D <= L frames fits a workspace sized for L)
            room = D - length
            assert len(starts) == room // stride + 1 + (room % stride != 0)
            assert len(starts) >= len(AO.anchor_starts(D - 1, length, stride))
            # anchor i of the kernel starts at min(i * stride, D - length)
            assert starts == [min(i * stride, D - length) for i in range(len(starts))]


def test_the_encoding_round_trip_through_the_window_rule():
    """[a, b) -> (centre, width) -> ``rv_span_scores``' window is [a, b) again, by the refine oracle's copy of the rule and by tests/similarity_oracle.py's."""
    for L, D, scales in ((1, 1, ((1, 1, 1),)), (300, 291, ((1, 1, 1), (7, 3, 2), (291, 1, 5), (100, 100, 9))), (36000, 35999, ((25, 6, 12), (400, 100, 200), (3000, 750, 1))),
                         (2 ** 20, 2 ** 20 - 3, ((1, 50000, 1), (625, 99991, 1), (2 ** 19, 2 ** 17, 1)))):
        mask = (np.arange(L) < D).astype(F)[None]
        pairs = np.array([(a, a + ln) for ln, st, _ in scales for a in AO.anchor_starts(D, ln, st)])
        spans = np.array([RO.encode(a, b, F(D)) for a, b in pairs], dtype=F)
        for (a, b), (c, w) in zip(pairs[:: max(1, len(pairs) // 2000)], spans[:: max(1, len(pairs) // 2000)]):
            assert RO.window(c, w, RO.CXW, F(D), L) == (a, b), (L, D, a, b)
        got = SO.windows(torch.from_numpy(spans[None]), torch.from_numpy(mask)).numpy()[0]
        assert np.array_equal(got, pairs), (L, D)


def _iou(lo, hi, a, b):
    inter = max(0, min(hi, b) - max(lo, a))
    return inter / ((hi - lo) + (b - a) - inter)


def test_planted_rows_the_threshold_generator_misses_and_this_one_ranks_first():
    sims, los = AO.planted_rows()
    mask = np.ones(sims.shape, dtype=F)
    con = AO.anchors(sims, mask, None, 1, AO.PLANTED_SCALES, AO.CONTRAST, 2, 1, 256)
    mean = AO.anchors(sims, mask, None, 1, AO.PLANTED_SCALES, AO.MEAN, 2, 1, 256)
    thr = PO.propose(sims, mask, (0.5, 0.6, 0.7, 0.8, 0.9))
    for r, lo in enumerate(los):
        n = con["n_spans"][r]
        assert con["n_found"][r] == n and 40 <= n < 256                                        # max_spans = 256 never truncates
        assert tuple(con["windows"][r, np.argmax(con["scores"][r, :n])]) == (lo, lo + 40)      # contrast: exactly the plateau, in 50 of 50
        m = mean["n_spans"][r]
        a, b = mean["windows"][r, np.argmax(mean["scores"][r, :m])]
        assert lo <= a and b <= lo + 40 and (a, b) != (lo, lo + 40)                            # mean: a 20-frame anchor INSIDE it wins, in 50 of 50
        assert all(_iou(lo, lo + 40, a, b) < 0.1 for a, b in thr["windows"][r, :thr["n_spans"][r]])       # default levels: nothing near it, in 50 of 50


def test_flat_and_staircase_rows():
    L = 100
    mask = np.ones((1, L), dtype=F)
    flat = np.full((1, L), 0.25, dtype=F)
    for mode in (AO.MEAN, AO.CONTRAST):
        for peak in (1, 2, 64):
            out = AO.anchors(flat, mask, None, 1, ((10, 5, 5), (7, 7, 3)), mode, peak, 1, 64)
            assert out["n_found"][0] == 2 and out["windows"][0, :2].tolist() == [[0, 10], [0, 7]]        # a flat stretch yields only its first anchor
        out = AO.anchors(flat, mask, None, 1, ((10, 5, 5),), mode, 0, 1, 64)
        assert out["n_found"][0] == 19                                                                   # peak = 0: every admissible anchor
    up = (np.arange(L) // 10 / 16).astype(F)[None]
    out = AO.anchors(up, mask, None, 1, ((10, 10, 5),), AO.MEAN, 2, 1, 64)
    assert out["windows"][0, :out["n_spans"][0]].tolist() == [[90, 100]]                                 # a rising staircase: the last step
    out = AO.anchors(up[:, ::-1].copy(), mask, None, 1, ((10, 10, 5),), AO.MEAN, 2, 1, 64)
    assert out["windows"][0, :out["n_spans"][0]].tolist() == [[0, 10]]


# ------------------------------------------------------------------ surface ------------------------------------------------------------------
def test_the_names_import_from_both_module_names():
    from revisionllm_amd import grounding, ops
    from revisionllm_amd.eval import similarity
    for name in ("span_anchors", "SpanAnchors", "span_anchors_keywords", "span_anchors_checks", "SPAN_ANCHORS_MAX_SCALES", "SPAN_ANCHORS_MAX_PEAK", "SPAN_ANCHOR_SCORES"):
        assert getattr(ops, name) is getattr(grounding, name), name
    assert ops.span_anchors.__module__ == "revisionllm_amd.grounding"
    assert ops.SpanAnchors._fields == ("spans", "scores", "n_spans", "n_found", "windows", "scale")
    assert (ops.SPAN_ANCHORS_MAX_SCALES, ops.SPAN_ANCHORS_MAX_PEAK, ops.SPAN_ANCHOR_SCORES) == (8, 64, {"mean": 0, "contrast": 1})
    for name in ("propose_anchors", "ground_queries_anchored"):
        assert callable(getattr(similarity, name)), name
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
import revisionllm_amd.ops as real_ops
import revisionllm_amd.eval.similarity as real_similarity
from revisionllm.ops import span_anchors, SpanAnchors
from revisionllm.eval.similarity import ground_queries_anchored, propose_anchors
import vtimellm.ops as old_ops
import vtimellm.eval.similarity as old_similarity
assert span_anchors is real_ops.span_anchors is old_ops.span_anchors and SpanAnchors is real_ops.SpanAnchors is old_ops.SpanAnchors
assert ground_queries_anchored is real_similarity.ground_queries_anchored is old_similarity.ground_queries_anchored
assert propose_anchors is real_similarity.propose_anchors is old_similarity.propose_anchors
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr + r.stdout


def test_signatures():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import similarity
    K, E = inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty

    def keywords(fn):
        return {n: p.default for n, p in inspect.signature(fn).parameters.items() if p.kind is K}
    want = dict(scales=E, score="contrast", peak=2, min_usable=1, valid=None, max_spans=256, return_windows=False, return_scale=False)
    for fn in (ops.span_anchors, similarity.propose_anchors):
        p = inspect.signature(fn).parameters
        assert list(p)[:2] == ["sims", "mask"] and all(p[n].kind is not K for n in list(p)[:2]) and keywords(fn) == want and list(keywords(fn)) == list(want), fn
    g = inspect.signature(similarity.ground_queries_anchored).parameters
    assert list(g)[:3] == ["text", "video", "mask"]
    want = dict(scales=E, score="contrast", peak=2, min_usable=1, valid=None, max_spans=256, top=10, nms_iou=0.5, gt=None, hit_iou=ops.HIT_IOU, radius=None,
                margin=None, min_len=1)
    assert keywords(similarity.ground_queries_anchored) == want and list(keywords(similarity.ground_queries_anchored)) == list(want)
    # no existing function gained a keyword
    assert list(inspect.signature(similarity.ground_queries_refined).parameters) == ["text", "video", "mask", "radius", "margin", "min_len", "form", "valid", "skip_nan", "top",
                                                                                     "nms_iou", "k", "pooling", "temperature", "gt", "hit_iou", "propose_keywords"]
    assert list(inspect.signature(similarity.ground_queries).parameters) == ["text", "video", "mask", "top", "nms_iou", "k", "pooling", "temperature", "gt", "hit_iou",
                                                                             "propose_keywords"]
    for fn in (ops.span_propose, ops.span_propose_masked, ops.span_refine, ops.span_rank, ops.span_scores, ops.window_select, similarity.ground_queries_masked,
               similarity.ground_queries_in_windows, similarity.propose_spans):
        assert not {"scales", "score", "peak", "min_usable", "anchors"} & set(inspect.signature(fn).parameters), fn.__name__


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
    assert declared == set(hip.CHAIN_SIGNATURES) == _exported(hip.CHAIN_LIB_PATH) and {"rvc_span_anchors", "rvc_span_anchors_workspace"} <= declared
    assert f"#define RVC_ABI_VERSION {hip.RVC_ABI_VERSION}" in header and hip.RVC_ABI_VERSION == 1
    assert "#define RVC_ANCHORS_MEAN 0" in header and "#define RVC_ANCHORS_CONTRAST 1" in header and (hip.RVC_ANCHORS_MEAN, hip.RVC_ANCHORS_CONTRAST) == (0, 1)
    params = [p.split()[-1].lstrip("*") for p in re.search(r"\brvc_span_anchors\s*\(([^)]*)\)\s*;", code).group(1).split(",")]
    assert params == ["sims", "mask", "valid", "rpv", "rows", "rpm", "L", "scales", "S", "mode", "peak", "min_usable", "max_spans", "out_spans", "scores", "n_spans",
                      "n_found", "windows", "scale", "workspace", "workspace_bytes", "stream"]
    params = [p.split()[-1].lstrip("*") for p in re.search(r"\brvc_span_anchors_workspace\s*\(([^)]*)\)\s*;", code).group(1).split(",")]
    assert params == ["L", "scales", "S", "rows"]
    P, I, T = ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)
    assert hip.CHAIN_SIGNATURES["rvc_span_anchors"] == (ctypes.c_int, [P, P, P, I, I, I, I, T, I, I, I, I, I, P, P, P, P, P, P, P, ctypes.c_int64, P])
    assert hip.CHAIN_SIGNATURES["rvc_span_anchors_workspace"] == (ctypes.c_int64, [I, T, I, I])
    # the other two libraries: no symbol more
    assert len(hip.SIGNATURES) == 64 and len(hip.EXT_SIGNATURES) == 3
    for path in hip.LIB_PATHS.values():
        assert _exported(path) == set(hip.SIGNATURES), path
    assert _exported(hip.EXT_LIB_PATH) == set(hip.EXT_SIGNATURES)
    rule = re.search(r"/\* ---- multi-scale sliding-window proposals.*?\*/", header, re.S).group(0)
    for word in ("0x7fc00000", "(-1, -1)", "-0 hides a frame", "16777216.f", "ties-to-even", "+-inf clamps to +-1", "NO RESULT DEPENDS ON THE ORDER OF ANY SUM",
                 "a_i = i * stride_s", "(D - len_s) % stride_s != 0", "flush with the end: a = D - len_s", "A scale with len_s > D has no anchors",
                 "J = (double)Sin / (double)Cin.", "(double)Sin / (double)Cin - (double)Sout / (double)Cout", "S(max(0, a - margin_s), a) + S(b, min(D, b + margin_s))",
                 "Cin >= min_usable", "Cout > 0", "(J descending as float64 VALUES, index ascending)", "|j - i| <= peak", "peak = 0 makes every admissible anchor a peak",
                 "A FLAT STRETCH THEREFORE YIELDS ONLY ITS FIRST ANCHOR", "(J descending,\n * scale index ascending, anchor index ascending)",
                 "truncation is by score, not by position", "(scale index, anchor index) order", "c = ((a + b) * 0.5) / dur", "w = ((b - a) - 0.5) / dur",
                 "S outside [1, 8]", "L outside [1, 1048576]", "stride outside [1, len]", "margin < 1 in contrast mode", "peak outside [0, 64]", "min_usable < 1",
                 "max_spans outside [1, 2048]", "no 65535 limit", "no global atomics", "no scratch"):
        assert word in rule, word
    src = open(os.path.join(ROOT, "revisionllm_amd", "csrc", "anchors_chain.hip")).read()
    assert "anchors_chain.hip" in build.CHAIN_SOURCES and src.count("__global__") == 1
    body = src[src.index("namespace {"):]
    atomics = re.findall(r"\batomic\w*\s*\(\s*&?(\w+)", body)
    assert atomics == ["hist"] and "__shared__ int hist[256]" in body                     # the one atomic counts into LDS: no global atomic
    for fn in ("duration_frames(", "__ddiv_rn", "contrast_f64(", "sim_quantise(", "sim_usable(", "span_mask_sum<AN_TPB>(", "span_encode(", "blockIdx.x"):
        assert fn in src, fn
    for helper in ("span_mask_sum", "span_encode", "sim_quantise", "sim_usable", "contrast_f64"):       # the rules it shares with the other stages: one definition each
        assert_grounding_rule_is_shared(helper, os.path.join(ROOT, "revisionllm_amd", "csrc"))
    assert "blockIdx.y" not in src


def _refused(rc, message):
    return rc == RV_ERR_ARG and message in hip.chain_last_error()


def _table(*triples):
    flat = [v for t in triples for v in t]
    return (ctypes.c_int32 * len(flat))(*flat)


def test_every_refusal_of_the_c_entries_comes_before_any_launch():
    """Dummy device pointers: a call that got as far as a launch would fault, so a clean RV_ERR_ARG with its message shows the check came first."""
    one = ctypes.c_void_p(64)
    lib = hip.chain_lib()
    f, w = lib.rvc_span_anchors, lib.rvc_span_anchors_workspace
    who = "rvc_span_anchors: "
    table = _table((20, 5, 10), (40, 10, 20))
    good = dict(sims=one, mask=one, valid=one, rpv=1, rows=6, rpm=3, L=100, scales=table, S=2, mode=1, peak=2, min_usable=1, max_spans=16, out_spans=one, scores=one,
                n_spans=one, n_found=one, windows=one, scale=one, workspace=one, workspace_bytes=1 << 40)
    order = list(good)

    def call(**kw):
        a = {**good, **kw}
        return f(*[a[n] for n in order], None)
    for name in ("sims", "mask", "out_spans", "scores", "n_spans", "n_found"):
        assert _refused(call(**{name: None}), who + "bad arguments (a null sims, mask, out_spans, scores, n_spans or n_found)"), name
    assert _refused(call(scales=None), who + "bad arguments (a null scales)")
    for mode in (-1, 2):
        assert _refused(call(mode=mode), who + "mode=%d (0: mean, 1: contrast)" % mode)
    for S in (0, -1, 9):
        assert _refused(call(S=S), who + "S=%d scales must be in [1, 8]" % S)
    for L in (0, -1, 1048577):
        assert _refused(call(L=L), who + "L=%d must be in [1, 1048576]" % L)
    for rows in (0, -3):
        assert _refused(call(rows=rows), who + "rows=%d must be at least 1" % rows)
    for bad, msg in (((0, 1, 1), "scale 1 has len=0, stride=1"), ((-4, 1, 1), "scale 1 has len=-4, stride=1"), ((5, 0, 1), "scale 1 has len=5, stride=0"),
                     ((5, 6, 1), "scale 1 has len=5, stride=6"), ((5, -1, 1), "scale 1 has len=5, stride=-1")):
        for mode in (0, 1):
            assert _refused(call(scales=_table((20, 5, 10), bad), mode=mode), who + msg), bad
    for margin in (0, -2):
        assert _refused(call(scales=_table((20, 5, margin), (40, 10, 20))), who + "scale 0 has margin=%d (at least 1 in contrast mode)" % margin)
    for kw in (dict(rpm=0), dict(rpm=-1), dict(rows=7), dict(rpm=4)):
        a = {**good, **kw}
        assert _refused(call(**kw), who + "rows=%d with rpm=%d rows per mask row" % (a["rows"], a["rpm"])), kw
    for kw in (dict(rpv=0), dict(rpv=-1), dict(rpv=4), dict(rpv=5)):
        a = {**good, **kw}
        assert _refused(call(**kw), who + "rows=%d with rpv=%d rows per validity row" % (a["rows"], a["rpv"])), kw
    for peak in (-1, 65):
        assert _refused(call(peak=peak), who + "peak=%d must be in [0, 64]" % peak)
    for mu in (0, -5):
        assert _refused(call(min_usable=mu), who + "min_usable=%d must be >= 1" % mu)
    for N in (0, -1, 2049):
        assert _refused(call(max_spans=N), who + "max_spans=%d must be in [1, 2048]" % N)
    # the workspace: per row L + 1 prefix points of 16 bytes and two 8-byte keys per anchor of a row of D = L frames
    per_row = 101 * 16 + 16 * (len(AO.anchor_starts(100, 20, 5)) + len(AO.anchor_starts(100, 40, 10)))
    assert w(100, table, 2, 6) == 6 * per_row and w(100, table, 2, 1) == per_row
    assert w(1 << 20, _table((1, 1, 1)) , 1, 70000) == 70000 * (((1 << 20) + 1) * 16 + 16 * (1 << 20))           # beyond 2^31 bytes, beyond 65535 rows
    assert w(100, _table((101, 101, 0)), 1, 1) == 101 * 16                                                     # no anchors; the margin is not this function's
    for kw, msg in ((dict(workspace=None), "workspace of"), (dict(workspace=ctypes.c_void_p(72)), "workspace of"), (dict(workspace_bytes=6 * per_row - 1), "workspace of"),
                    (dict(workspace_bytes=0), "workspace of"), (dict(workspace_bytes=-1), "workspace of")):
        assert _refused(call(**kw), who + msg), kw
    assert str(6 * per_row) in hip.chain_last_error()
    who = "rvc_span_anchors_workspace: "
    for args, msg in (((100, None, 2, 6), "bad arguments (a null scales)"), ((100, table, 0, 6), "S=0 scales must be in [1, 8]"), ((100, table, 9, 6), "S=9 scales"),
                      ((0, table, 2, 6), "L=0 must be in"), ((1048577, table, 2, 6), "L=1048577 must be in"), ((100, table, 2, 0), "rows=0 must be at least 1"),
                      ((100, _table((20, 21, 1)), 1, 6), "scale 0 has len=20, stride=21")):
        assert _refused(w(*args), who + msg), args


def test_python_side_refusals_come_before_the_device_is_looked_for():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import similarity as S
    s, m = torch.zeros(2, 3, 40), torch.ones(2, 40)
    good = dict(scales=(8, (12, 3), (20, 5, 4)))
    assert ops.span_anchors_keywords("x", **good)[0] == ((8, 2, 4), (12, 3, 6), (20, 5, 4))                     # stride = max(1, len // 4), margin = max(1, len // 2)
    assert ops.span_anchors_keywords("x", scales=[1, 3])[0] == ((1, 1, 1), (3, 1, 1))
    for fn, name in ((ops.span_anchors, "span_anchors"), (S.propose_anchors, "propose_anchors")):
        for kw in (dict(scales=()), dict(scales=[4] * 9), dict(scales=8), dict(scales="8"), dict(scales=None), dict(scales=[0]), dict(scales=[-3]), dict(scales=[2.0]),
                   dict(scales=[True]), dict(scales=[(8, 0)]), dict(scales=[(8, 9)]), dict(scales=[(8, 2, 0)]), dict(scales=[(8, 2, 1, 1)]), dict(scales=[()]),
                   dict(scales=[(8, 2.0)]), dict(scales=[2 ** 31]), dict(score="max"), dict(score=1), dict(score=None), dict(peak=-1), dict(peak=65), dict(peak=1.0),
                   dict(peak=True), dict(min_usable=0), dict(min_usable=1.5), dict(max_spans=0), dict(max_spans=2049), dict(max_spans=None), dict(return_windows=2),
                   dict(return_scale="yes"), dict(valid=torch.ones(2, 41)), dict(valid=torch.ones(3, 40)), dict(valid=torch.ones(2, 3, 40, dtype=torch.int64)),
                   dict(valid=[[1] * 40] * 2), dict(valid=np.ones((2, 40), np.float32))):
            with pytest.raises(ValueError, match=name):
                fn(s, m, **{**good, **kw})
        for a in (dict(mask=torch.ones(3, 40)), dict(mask=torch.ones(2, 41)), dict(mask=torch.ones(40)), dict(mask=torch.ones(2, 40, dtype=torch.complex64)),
                  dict(sims=torch.zeros(40)), dict(sims=torch.zeros(2, 3, 0)), dict(sims=s.long()), dict(sims=None)):
            b = {**dict(sims=s, mask=m), **a}
            with pytest.raises(ValueError, match=name):
                fn(b["sims"], b["mask"], **good)
        with pytest.raises(TypeError):
            fn(s, m, (8,))                                                             # keyword-only
        with pytest.raises(TypeError):
            fn(s, m)                                                                   # scales is required
    with pytest.raises(ValueError, match="span_anchors: sims must be float32"):
        ops.span_anchors(s.half(), m, **good)
    with pytest.raises(ValueError, match="span_anchors: L=1048577"):
        ops.span_anchors(torch.zeros(1, 1048577), torch.ones(1, 1048577), **good)
    text, video = torch.zeros(2, 3, 8), torch.zeros(2, 40, 8)
    for kw in (dict(scales=[0]), dict(score="median"), dict(peak=65), dict(min_usable=0), dict(max_spans=0), dict(valid=torch.ones(2, 41)), dict(valid=torch.ones(2, 2, 40)),
               dict(top=0), dict(nms_iou=-1.0), dict(gt=torch.zeros(2, 2)), dict(hit_iou=(0.5,) * 17), dict(radius=4), dict(margin=8), dict(radius=0, margin=8),
               dict(radius=4, margin=129), dict(radius=4, margin=8, min_len=0), dict(min_len=0)):
        with pytest.raises(ValueError, match="ground_queries_anchored"):
            S.ground_queries_anchored(text, video, m, **{**good, **kw})
    with pytest.raises(TypeError):
        S.ground_queries_anchored(text, video, m, levels=(0.5,), **good)
    with pytest.raises(TypeError):
        S.ground_queries_anchored(text, video, m)
    for a in (dict(text=torch.zeros(2, 3, 9)), dict(video=torch.zeros(2, 40)), dict(mask=torch.ones(2, 39)), dict(text=text.long())):
        b = {**dict(text=text, video=video, mask=m), **a}
        with pytest.raises(ValueError, match="ground_queries_anchored"):
            S.ground_queries_anchored(b["text"], b["video"], b["mask"], **good)
    if not torch.cuda.is_available():
        # both shapes of valid are taken: past the refusals there is the device path only
        for call in (lambda: S.ground_queries_anchored(text, video, m, **good), lambda: S.ground_queries_anchored(text[:, 0], video, m, valid=m.bool(), radius=4, margin=8, **good),
                     lambda: S.ground_queries_anchored(text, video, m, valid=torch.ones(2, 3, 40), score="mean", **good),
                     lambda: S.propose_anchors(s, m, valid=torch.ones(2, 3, 40), **good), lambda: S.propose_anchors(s.half(), m, valid=m, score="mean", **good)):
            with pytest.raises(hip.HipLibraryError, match="HIP device path only"):
                call()
