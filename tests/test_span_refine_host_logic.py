"""Boundary refinement on the host: what the GPU items of tests/test_gpu_span_refine.py rely on, and the package surface of ``rvc_span_refine``.
First the oracle of tests/span_refine_oracle.py itself: on a step row it returns exactly the plateau from every starting pair (the planted-plateau GPU
items rest on this), a flat row keeps every original pair, the oracle equals an independently written brute-force statement on some hundreds of seeded
short rows, the quantiser at ties and beyond +-1, and the encoding round trip of refined windows through the f32 window rule - the oracle's copy AND
``rv_span_scores``' own oracle (tests/similarity_oracle.py), which holds the kernel's second statement of that rule to the first.  Then the surface:
names under both module names, signatures, header == ctypes table == exports with the new name among them and the other two libraries unchanged, every
refusal of the C entry before a launch, every Python-side refusal before a device is looked for - these fail without the feature.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import similarity_oracle as SO
import span_refine_oracle as RO
from helpers import GROUNDING_RULES, assert_grounding_rule_is_shared
from revisionllm_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RV_ERR_ARG = -1              # include/revision_hip.h: rv_status
F = np.float32
NAN, INF = float("nan"), float("inf")


def step_row(L, p0, p1):
    s = np.zeros(L, dtype=F)
    s[p0:p1] = 1
    return s


def xx(lo, hi, D):
    """(start, end) fractions whose window is exactly [lo, hi) under a duration of D frames: a quarter frame inside either bound."""
    return [F((lo + 0.25) / D), F((hi - 0.25) / D)]


# ------------------------------------------------------------------ the oracle ------------------------------------------------------------------
def test_on_a_step_row_the_oracle_returns_the_plateau_from_every_starting_pair():
    for L, D, p0, p1, radius, margin in ((60, 60, 20, 33, 5, 3), (60, 55, 8, 9, 2, 8), (200, 200, 70, 140, 64, 5), (40, 40, 3, 37, 3, 3), (100, 100, 40, 52, 1, 40)):
        assert p0 >= margin and D - p1 >= margin
        s = step_row(L, p0, p1)
        mask = (np.arange(L) < D).astype(F)[None]
        starts = [(lo, hi) for lo in range(max(0, p0 - radius), p0 + radius + 1) for hi in range(p1 - radius, min(D, p1 + radius) + 1) if hi > lo]
        assert len(starts) > radius * radius
        if radius > 5:                                            # (16641 starting pairs of 16641 candidates each: the corners, the plateau and every 1201st)
            starts = sorted(set(starts[::1201] + [starts[0], starts[-1], (p0, p1), (p0 - radius, p1 - radius), (p0 + radius, min(D, p1 + radius))]))
        spans = np.array([xx(lo, hi, D) for lo, hi in starts], dtype=F)[None]
        for brute in (False, True) if radius <= 5 else (False,):
            out = RO.refine(s[None], spans, RO.XX, mask, None, 1, radius, margin, 1, brute=brute)
            assert (out["windows"][0] == (p0, p1)).all(), (L, p0, p1, radius, margin)
            assert (out["contrast"][0] == F(2 ** 24)).all() and not (out["contrast0"][0] > F(2 ** 24)).any()
        # (the starting windows are what was meant)
        assert [RO.window(a, b, RO.XX, F(D), L) for a, b in spans[0]] == starts
        # the same from (centre, width) spans
        cxw = np.array([RO.encode(lo, hi, F(D)) for lo, hi in starts], dtype=F)[None]
        assert (RO.refine(s[None], cxw, RO.CXW, mask, None, 1, radius, margin, 1)["windows"][0] == (p0, p1)).all()


def test_a_flat_row_keeps_every_original_pair():
    L, D = 50, 47
    mask = (np.arange(L) < D).astype(F)[None]
    pairs = [(0, 1), (1, 47), (46, 47), (10, 20), (3, 4), (0, 5), (40, 47), (20, 21)]
    spans = np.array([xx(lo, hi, D) for lo, hi in pairs], dtype=F)[None]
    for value in (0.0, 0.37, -1.0, 5.0):
        s = np.full((1, L), value, dtype=F)
        for radius, margin in ((1, 1), (5, 3), (64, 128)):
            out = RO.refine(s, spans, RO.XX, mask, None, 1, radius, margin, 1)
            assert out["windows"][0].tolist() == [list(p) for p in pairs], (value, radius, margin)
            assert not out["contrast"][0].any() and not out["contrast0"][0].any()               # every J is 0: the distance decides
    # the whole row has no context and is not admissible: a shorter candidate that has some is taken, at contrast 0
    out = RO.refine(np.full((1, L), 0.37, dtype=F), np.array([[xx(0, 47, D)]], dtype=F), RO.XX, mask, None, 1, 2, 3, 1)
    assert out["windows"][0].tolist() == [[0, 46]] and out["contrast"][0, 0] == 0 and np.isnan(out["contrast0"][0, 0])


def test_oracle_against_brute_force():
    rng = np.random.default_rng(25)
    moved = kept = void = inadmissible = 0
    cases = 0
    for case in range(180):
        L = int(rng.integers(1, 81))
        radius, margin = (1, 2, 5)[case % 3], (1, 3, 40)[(case // 3) % 3]
        R, rpm, N = 2, 1, 4
        Ds = rng.integers(0, L + 1, R)
        if case % 7 == 0:
            Ds[0] = L
        mask = (np.arange(L)[None, :] < Ds[:, None]).astype(F)
        kind = case % 4
        sims = rng.uniform(-1.2, 1.2, (R, L)).astype(F) if kind else np.round(rng.uniform(-1, 1, (R, L)) * 2).astype(F) / 2       # (kind 0: many ties)
        sims[rng.random((R, L)) < 0.08] = NAN
        valid = None if case % 3 == 0 else rng.choice(np.array([1.0, 1.0, 1.0, 0.0, -0.0, NAN, 2.0], dtype=F), (R, L))
        form = case % 2
        lo = rng.integers(-3, L + 3, (R, N))
        ln = rng.integers(-1, 12, (R, N))
        dd = np.maximum(Ds, 1)[:, None].astype(np.float64)
        xx_ = np.stack([(lo + 0.25) / dd, (lo + ln - 0.25) / dd], -1)
        spans = xx_.astype(F) if form == RO.XX else np.stack([(xx_[..., 0] + xx_[..., 1]) / 2, xx_[..., 1] - xx_[..., 0]], -1).astype(F)
        spans[0, 0] = NAN
        min_len = int(rng.choice([1, 1, 2, 9]))
        a = RO.refine(sims, spans, form, mask, valid, 1, radius, margin, min_len)
        b = RO.refine(sims, spans, form, mask, valid, 1, radius, margin, min_len, brute=True)
        for name in a:
            x, y = a[name], b[name]
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) if x.dtype == F else np.array_equal(x, y), (case, name)
        cases += 1
        for r in range(R):
            for n in range(N):
                w = RO.window(spans[r, n, 0], spans[r, n, 1], form, F(Ds[r]), L)
                got = tuple(a["windows"][r, n])
                if got == (-1, -1):
                    void += 1
                    assert np.isnan(a["spans"][r, n]).all() and np.isnan(a["contrast"][r, n]) and np.isnan(a["contrast0"][r, n])
                    continue
                orig = (min(w[0], Ds[r]), min(w[1], Ds[r]))
                assert abs(got[0] - orig[0]) <= radius and abs(got[1] - orig[1]) <= radius and 0 <= got[0] < got[1] <= Ds[r]
                assert got == orig or got[1] - got[0] >= min_len
                if np.isnan(a["contrast"][r, n]):
                    inadmissible += 1
                    assert got == orig
                else:
                    assert np.isnan(a["contrast0"][r, n]) or a["contrast"][r, n] >= a["contrast0"][r, n]
                    moved += got != orig
                    kept += got == orig
    assert cases == 180 and moved > 300 and kept > 30 and void > 100 and inadmissible > 5, (moved, kept, void, inadmissible)


def test_the_quantiser_at_ties_and_beyond_one():
    q = RO.quantise(np.array([2.0 ** -25, 3 * 2.0 ** -25, -(2.0 ** -25), -3 * 2.0 ** -25, 5 * 2.0 ** -25, 1.0, -1.0, 1.5, -7.0, INF, -INF, NAN, 0.0, -0.0,
                              2.0 ** -24, 1 - 2.0 ** -24, 0.5], dtype=F))
    assert q.tolist() == [0, 2, 0, -2, 2, 2 ** 24, -2 ** 24, 2 ** 24, -2 ** 24, 2 ** 24, -2 ** 24, 0, 0, 0, 1, 2 ** 24 - 1, 2 ** 23]
    # the product is exact in f32: a power of two times an f32 in [-1, 1] (no overflow, no underflow to a subnormal that loses bits above 2^-24 steps)
    rng = np.random.default_rng(3)
    s = rng.uniform(-1, 1, 4000).astype(F)
    assert np.array_equal((s * F(16777216.0)).astype(np.float64), s.astype(np.float64) * 16777216.0)
    # NaN is never usable, whatever valid says; -0 in valid hides, NaN in valid does not
    u = RO.usable(np.array([0.1, NAN, 0.2, 0.3, 0.4, 0.5], dtype=F), np.array([1, 1, -0.0, NAN, 1e-45, 1], dtype=F), 5)
    assert u.tolist() == [True, False, False, True, True, False]
    # sums of 2^20 frames at full scale stay far inside int64 and convert to float64 exactly
    assert (2 ** 20) * (2 ** 24) == 2 ** 44 and float(np.float64(2 ** 44 - 1)) == 2 ** 44 - 1


def test_the_encoding_round_trip_through_the_window_rule():
    """[a, b) -> (centre, width) -> ``rv_span_scores``' window is [a, b) again, by the oracle's copy of the rule and by tests/similarity_oracle.py's."""
    rng = np.random.default_rng(11)
    for L in (1, 2, 63, 300, 20000, 2 ** 20):
        for D in sorted({L, max(1, L - 1), max(1, L // 3), 1}):
            hi = rng.integers(1, D + 1, 300)
            lo = (rng.random(300) * hi).astype(np.int64)
            pairs = np.concatenate([np.stack([lo, hi], 1), [[0, D], [D - 1, D], [0, 1]]])
            spans = np.array([RO.encode(a, b, F(D)) for a, b in pairs], dtype=F)
            for (a, b), (c, w) in zip(pairs, spans):
                assert RO.window(c, w, RO.CXW, F(D), L) == (a, b), (L, D, a, b)
            mask = (np.arange(L) < D).astype(F)[None]
            got = SO.windows(torch.from_numpy(spans[None]), torch.from_numpy(mask)).numpy()[0]
            assert np.array_equal(got, pairs), (L, D)
    # the two statements of the rule agree on spans of every kind, void ones included
    L, D = 50, 37
    mask = (np.arange(L) < D).astype(F)[None]
    spans = np.concatenate([rng.uniform(-0.5, 1.5, (400, 2)), [[NAN, 0.1], [0.5, INF], [0.5, -0.2], [3e38, 3e38], [-2.0, 0.1], [0.5, 0.0]]]).astype(F)
    got = SO.windows(torch.from_numpy(spans[None]), torch.from_numpy(mask)).numpy()[0]
    for (c, w), g in zip(spans, got):
        mine = RO.window(c, w, RO.CXW, F(D), L)
        assert (mine or SO.NAN_WINDOW) == tuple(g), (c, w)
    assert RO.window(NAN, 0.1, RO.XX, F(D), L) is None and RO.window(0.25, 0.5, RO.XX, F(D), L) == (9, 19)
    assert RO.duration_frames(F(0.5), 9) == 0 and RO.duration_frames(F(NAN), 9) == 0 and RO.duration_frames(F(12.0), 9) == 9 and RO.duration_frames(F(3.7), 9) == 3


# ------------------------------------------------------------------ surface ------------------------------------------------------------------
def test_the_names_import_from_both_module_names():
    from revisionllm_amd import grounding, ops
    from revisionllm_amd.eval import similarity
    for name in ("span_refine", "RefinedSpans", "span_refine_keywords", "span_refine_checks", "SPAN_REFINE_MAX_RADIUS", "SPAN_REFINE_MAX_MARGIN"):
        assert getattr(ops, name) is getattr(grounding, name), name
    assert ops.span_refine.__module__ == "revisionllm_amd.grounding" and ops.RefinedSpans._fields == ("spans", "windows", "contrast", "contrast0")
    assert (ops.SPAN_REFINE_MAX_RADIUS, ops.SPAN_REFINE_MAX_MARGIN) == (64, 128)
    assert similarity.RefinedGrounding._fields == ("grounding", "refined", "scores")
    for name in ("refine_spans", "ground_queries_refined"):
        assert callable(getattr(similarity, name)), name
    code = f"""
import sys
sys.path.insert(0, {ROOT!r})
import revisionllm_amd
revisionllm_amd.install_as_revisionllm()
import revisionllm_amd.ops as real_ops
import revisionllm_amd.eval.similarity as real_similarity
from revisionllm.ops import span_refine, RefinedSpans
from revisionllm.eval.similarity import ground_queries_refined, refine_spans, RefinedGrounding
import vtimellm.ops as old_ops
import vtimellm.eval.similarity as old_similarity
assert span_refine is real_ops.span_refine is old_ops.span_refine and RefinedSpans is real_ops.RefinedSpans is old_ops.RefinedSpans
assert ground_queries_refined is real_similarity.ground_queries_refined is old_similarity.ground_queries_refined
assert refine_spans is real_similarity.refine_spans is old_similarity.refine_spans
assert RefinedGrounding is old_similarity.RefinedGrounding
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
    want = dict(form="cxw", radius=E, margin=E, min_len=1, valid=None, return_windows=False, return_contrast=False)
    for fn in (ops.span_refine, similarity.refine_spans):
        p = inspect.signature(fn).parameters
        assert list(p)[:3] == ["sims", "spans", "mask"] and all(p[n].kind is not K for n in list(p)[:3]) and keywords(fn) == want, fn
    g = inspect.signature(similarity.ground_queries_refined).parameters
    assert list(g)[:3] == ["text", "video", "mask"] and g["propose_keywords"].kind is inspect.Parameter.VAR_KEYWORD
    assert keywords(similarity.ground_queries_refined) == {**dict(radius=E, margin=E, min_len=1, form="cxw"), **keywords(similarity.ground_queries_masked)}
    # no existing function gained a keyword
    gm = inspect.signature(similarity.ground_queries_masked).parameters
    assert list(gm) == ["text", "video", "mask", "valid", "skip_nan", "top", "nms_iou", "k", "pooling", "temperature", "gt", "hit_iou", "propose_keywords"]
    for fn in (ops.span_scores_masked, ops.span_scores_masked_rows, ops.span_propose_masked, ops.span_rank, ops.span_scores, similarity.ground_queries,
               similarity.ground_queries_in_windows, similarity.propose_spans_masked):
        assert not {"radius", "margin", "refine"} & set(inspect.signature(fn).parameters), fn.__name__


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
    assert declared == set(hip.CHAIN_SIGNATURES) == _exported(hip.CHAIN_LIB_PATH) and "rvc_span_refine" in declared
    assert f"#define RVC_ABI_VERSION {hip.RVC_ABI_VERSION}" in header and hip.RVC_ABI_VERSION == 1
    params = [p.split()[-1].lstrip("*") for p in re.search(r"\brvc_span_refine\s*\(([^)]*)\)\s*;", code).group(1).split(",")]
    assert params == ["sims", "spans", "form", "mask", "valid", "rpv", "rows", "rpm", "L", "N", "radius", "margin", "min_len", "out_spans", "windows", "contrast",
                      "contrast0", "stream"]
    P, I = ctypes.c_void_p, ctypes.c_int32
    assert hip.CHAIN_SIGNATURES["rvc_span_refine"] == (ctypes.c_int, [P, P, I, P, P, I, I, I, I, I, I, I, I, P, P, P, P, P])
    # the other two libraries: no symbol more
    assert len(hip.SIGNATURES) == 64 and len(hip.EXT_SIGNATURES) == 3
    for path in hip.LIB_PATHS.values():
        assert _exported(path) == set(hip.SIGNATURES), path
    assert _exported(hip.EXT_LIB_PATH) == set(hip.EXT_SIGNATURES)
    rule = re.search(r"/\* ---- boundary refinement.*?\*/", header, re.S).group(0)
    for word in ("ALWAYS (centre, width)", "0x7fc00000", "(-1, -1)", "lo0 = min(lo, D)", "hi0 <= lo0", "-0 hides a frame", "16777216.f", "ties-to-even",
                 "+-inf clamps to +-1", "NO RESULT DEPENDS ON THE ORDER OF ANY SUM", "valid is read only where sims is read", "min(lo0 + radius, D - 1)",
                 "max(1, hi0 - radius)", "the original pair (lo0, hi0) is always a candidate", "Cin = C(a, b) > 0", "(double)Sin / (double)Cin - (double)Sout / (double)Cout",
                 "then the smallest |a - lo0| + |b - hi0|; then the smaller a; then the smaller b", "contrast is NaN", "c = ((a + b) * 0.5) / dur",
                 "w = ((b - a) - 0.5) / dur", "radius outside [1, 64]", "margin outside [1, 128]", "min_len < 1", "rows > 65535", "no atomics, no scratch"):
        assert word in rule, word
    src = open(os.path.join(ROOT, "revisionllm_amd", "csrc", "refine_chain.hip")).read()
    assert "refine_chain.hip" in build.CHAIN_SOURCES and src.count("__global__") == 1 and "atomic" not in src.split("#include")[1].lower().replace("__atomic_", "")
    for fn in ("duration_frames(", "span_mask_sum<256>(", "SPAN_NOT_FINITE(", "span_slice(", "span_encode(", "sim_usable(", "sim_quantise(", "contrast_f64("):
        assert fn in src, fn
    for helper in GROUNDING_RULES:                                                          # every rule it shares with the other stages: one definition each
        assert_grounding_rule_is_shared(helper, os.path.join(ROOT, "revisionllm_amd", "csrc"))


def _refused(rc, message):
    return rc == RV_ERR_ARG and message in hip.chain_last_error()


def test_every_refusal_of_the_c_entry_comes_before_any_launch():
    """Dummy device pointers: a call that got as far as a launch would fault, so a clean RV_ERR_ARG with its message shows the check came first."""
    one = ctypes.c_void_p(64)
    f = hip.chain_lib().rvc_span_refine
    who = "rvc_span_refine: "
    good = dict(sims=one, spans=one, form=1, mask=one, valid=one, rpv=1, rows=6, rpm=3, L=100, N=5, radius=8, margin=16, min_len=1, out_spans=one, windows=one,
                contrast=one, contrast0=one)
    order = list(good)

    def call(**kw):
        a = {**good, **kw}
        return f(*[a[n] for n in order], None)
    for name in ("sims", "spans", "mask", "out_spans"):
        assert _refused(call(**{name: None}), who + "bad arguments (a null sims, spans, mask or out_spans)"), name
    for form in (-1, 2):
        assert _refused(call(form=form), who + "form=%d must be 0 (start, end) or 1 (centre, width)" % form)
    for kw in (dict(rows=0), dict(rows=-3), dict(N=0), dict(N=-1)):
        a = {**good, **kw}
        assert _refused(call(**kw), who + "rows=%d, N=%d (both at least 1)" % (a["rows"], a["N"])), kw
    for L in (0, -1, 1048577):
        assert _refused(call(L=L), who + "L=%d must be in [1, 1048576]" % L)
    for kw in (dict(rpm=0), dict(rpm=-1), dict(rows=7), dict(rpm=4)):
        a = {**good, **kw}
        assert _refused(call(**kw), who + "rows=%d with rpm=%d rows per mask row" % (a["rows"], a["rpm"])), kw
    for kw in (dict(rpv=0), dict(rpv=-1), dict(rpv=4), dict(rpv=5)):
        a = {**good, **kw}
        assert _refused(call(**kw), who + "rows=%d with rpv=%d rows per validity row" % (a["rows"], a["rpv"])), kw
    assert _refused(call(rows=65536, rpm=1), who + "at most 65535 rows per launch (rows=65536)")
    for radius in (0, -1, 65):
        assert _refused(call(radius=radius), who + "radius=%d must be in [1, 64]" % radius)
    for margin in (0, -1, 129):
        assert _refused(call(margin=margin), who + "margin=%d must be in [1, 128]" % margin)
    for min_len in (0, -5):
        assert _refused(call(min_len=min_len), who + "min_len=%d must be >= 1" % min_len)


def test_python_side_refusals_come_before_the_device_is_looked_for():
    from revisionllm_amd import ops
    from revisionllm_amd.eval import similarity as S
    s, sp, m = torch.zeros(2, 3, 40), torch.zeros(2, 3, 5, 2), torch.ones(2, 40)
    good = dict(radius=4, margin=8)
    for fn, name in ((ops.span_refine, "span_refine"), (S.refine_spans, "refine_spans")):
        for kw in (dict(radius=0), dict(radius=65), dict(radius=2.0), dict(radius=True), dict(margin=0), dict(margin=129), dict(margin=None), dict(min_len=0),
                   dict(min_len=1.5), dict(form="xxw"), dict(form=1), dict(return_windows=2), dict(return_contrast="yes"),
                   dict(valid=torch.ones(2, 41)), dict(valid=torch.ones(3, 40)), dict(valid=torch.ones(2, 3, 40, dtype=torch.int64)), dict(valid=[[1] * 40] * 2),
                   dict(valid=np.ones((2, 40), np.float32))):
            with pytest.raises(ValueError, match=name):
                fn(s, sp, m, **{**good, **kw})
        for a in (dict(spans=torch.zeros(2, 3, 5, 3)), dict(spans=torch.zeros(2, 5, 2)), dict(spans=torch.zeros(2, 4, 5, 2)), dict(spans=sp.long()), dict(spans=[[0, 1]]),
                  dict(mask=torch.ones(3, 40)), dict(mask=torch.ones(2, 41)), dict(mask=torch.ones(40)), dict(mask=torch.ones(2, 40, dtype=torch.complex64)),
                  dict(sims=torch.zeros(40)), dict(sims=torch.zeros(2, 3, 0)), dict(sims=s.long()), dict(sims=None)):
            b = {**dict(sims=s, spans=sp, mask=m), **a}
            with pytest.raises(ValueError, match=name):
                fn(b["sims"], b["spans"], b["mask"], **good)
        with pytest.raises(TypeError):
            fn(s, sp, m, "cxw", 4, 8)                                                  # keyword-only
        with pytest.raises(TypeError):
            fn(s, sp, m, radius=4)                                                     # margin is required
    with pytest.raises(ValueError, match="span_refine: sims must be float32"):
        ops.span_refine(s.half(), sp, m, **good)
    with pytest.raises(ValueError, match="span_refine: 65536 rows"):
        ops.span_refine(torch.zeros(65536, 4), torch.zeros(65536, 1, 2), torch.ones(65536, 4), **good)
    # both shapes of valid are taken: past the refusals there is the device path only
    text, video = torch.zeros(2, 3, 8), torch.zeros(2, 40, 8)
    for kw in (dict(radius=0), dict(margin=129), dict(min_len=0), dict(form="wc"), dict(valid=torch.ones(2, 3, 40)), dict(skip_nan=2), dict(top=0), dict(nms_iou=-1.0),
               dict(pooling="mean"), dict(k=0), dict(smooth=2), dict(max_spans=0), dict(gt=torch.zeros(2, 2)), dict(hit_iou=(0.5,) * 17)):
        with pytest.raises(ValueError, match="ground_queries_refined"):
            S.ground_queries_refined(text, video, m, **{**good, **kw})
    with pytest.raises(TypeError, match="ground_queries_refined"):
        S.ground_queries_refined(text, video, m, window=3, **good)
    with pytest.raises(TypeError):
        S.ground_queries_refined(text, video, m, radius=4)
    for a in (dict(text=torch.zeros(2, 3, 9)), dict(video=torch.zeros(2, 40)), dict(mask=torch.ones(2, 39)), dict(text=text.long())):
        b = {**dict(text=text, video=video, mask=m), **a}
        with pytest.raises(ValueError, match="ground_queries_refined"):
            S.ground_queries_refined(b["text"], b["video"], b["mask"], **good)
    if not torch.cuda.is_available():
        for call in (lambda: S.ground_queries_refined(text, video, m, **good), lambda: S.ground_queries_refined(text[:, 0], video, m, form="xx", valid=m.bool(), **good),
                     lambda: S.refine_spans(s, sp, m, valid=torch.ones(2, 3, 40), **good), lambda: S.refine_spans(s.half(), sp, m, valid=m, form="xx", **good)):
            with pytest.raises(hip.HipLibraryError, match="HIP device path only"):
                call()
