"""The grounding chain's wrappers and checkers (revisionllm_amd/grounding.py, reached through ``ops``) against the call records of commit c9da171, on the
CPU: every wrapper is driven on small CPU tensors with stand-ins - a recorder each for ``hip.lib`` / ``hip.ext_lib`` / ``hip.chain_lib``, ``hip.ptr`` ->
``data_ptr()``, ``hip.stream`` -> None - and each call becomes a plain record: the library ("lib:<its flavour argument>", "ext", "chain"), the entry's name and
the arguments in order - scalars as they are, a ctypes table as a list, every pointer as [n-th distinct storage of the inputs, byte offset], [name of the
returned field, byte offset], "copy" when it falls in neither (a cast, a contiguous copy, a workspace) or null.  The returned tensors' shapes and dtypes are
recorded with them, what a checker returns is recorded as plain values, and a refusal becomes (exception class name, message).

tests/golden/grounding_call_records.json holds, in the order of the sorted case keys, the first 6 hex digits of the SHA-256 of each record's canonical JSON
(a refusal: the first letter of the class name - CLASSES -, then the digest of the message): digests, because the records themselves are larger than a golden
file may be.  The file was written by THIS module run as a script against a checkout of commit c9da171 - the parent of the change that folded the wrappers'
pasted bodies - and must never be regenerated from the code under test.  To regenerate it (a new case, a new axis), check out the commit whose behaviour is
the reference into another directory and run

    python tests/test_grounding_call_records.py --root <that checkout> [--full records.json]

``--full`` also writes the whole records; run it against both trees and diff the two files to see HOW a case that fails here differs.
"""
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "grounding_call_records.json")
F32, F64, F16, BF16, I32, I64, U8, BOOL = (torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int32, torch.int64, torch.uint8, torch.bool)
L = 12

#: case key -> the refusal's new text (the class is still the golden file's), with the reason.  None: one body serves each family without a reworded refusal.
REWORDED = {}


def z(*shape, dt=F32):
    return torch.zeros(*shape, dtype=dt)


def layouts():
    """name -> (sims, mask): [R,L] with a mask row per row, [R,L] with rpm = 2, [B,Q,L] with rpm = 3."""
    return {"rl": (z(4, L), z(4, L)), "rl-rpm2": (z(4, L), z(2, L)), "bql": (z(2, 3, L), z(2, L))}


def strided(shape):
    """zeros of ``shape`` whose last axis has stride 2"""
    return z(*shape[:-1], 2 * shape[-1])[..., ::2]


# ---- the cases: key -> (function name in ops, args, kwargs) ----
def keyword_checker_cases():
    c = {}
    f = "span_propose_keywords"
    for k, kw in (("default", {}), ("levels-int", dict(levels=5)), ("levels-text", dict(levels=("a",))), ("levels-none", dict(levels=())),
                  ("levels-nine", dict(levels=tuple(i / 10 for i in range(9)))), ("relative-2", dict(relative=2)), ("relative-text", dict(relative="no")),
                  ("relative-1", dict(relative=1)), ("level-huge", dict(levels=(1e300,), relative=False)), ("level-nan", dict(levels=(float("nan"),))),
                  ("descending", dict(levels=(0.5, 0.4))), ("equal-as-f32", dict(levels=(0.5, 0.5 + 1e-12))), ("relative-level-1", dict(levels=(0.5, 1.0))),
                  ("relative-level-negative", dict(levels=(-0.1,))), ("absolute", dict(levels=(-3.0, 7.5), relative=False)), ("smooth-even", dict(smooth=4)),
                  ("smooth-0", dict(smooth=0)), ("smooth-67", dict(smooth=67)), ("smooth-true", dict(smooth=True)), ("smooth-65", dict(smooth=65)),
                  ("gap-negative", dict(gap=-1)), ("gap-64", dict(gap=64)), ("gap-float", dict(gap=1.0)), ("min_len-0", dict(min_len=0)),
                  ("min_len-big", dict(min_len=2 ** 31)), ("max_len-below", dict(min_len=3, max_len=2)), ("max_len-float", dict(max_len=4.0)),
                  ("max_len", dict(min_len=2, max_len=9)), ("max_spans-0", dict(max_spans=0)), ("max_spans-2049", dict(max_spans=2049)),
                  ("max_spans-true", dict(max_spans=True))):
        c["kw/propose/" + k] = (f, ("w",), kw)
    f = "window_select_keywords"
    for k, a in (("ok", (8, 2, 3)), ("k-min_sep", (8, 2, 3, 64, 2)), ("win-0", (0, 2, 3)), ("win-true", (True, 1, 3)), ("stride-float", (8, 2.0, 3)),
                 ("keep-0", (8, 2, 0)), ("k-0", (8, 2, 3, 0)), ("min_sep-0", (8, 2, 3, 3, 0)), ("keep-big", (8, 2, 2 ** 31)), ("win-below-stride", (2, 3, 1)),
                 ("k-65", (8, 2, 3, 65))):
        c["kw/select/" + k] = (f, ("w",) + a, {})
    f = "window_select_capacity"
    for k, a in (("ok", (12, 4, 2)), ("win-above-L", (12, 13, 2)), ("too-many", (4100, 2, 2)), ("min_sep-above", (12, 4, 2, 6)), ("min_sep-at", (12, 4, 2, 5)),
                 ("one-window", (4, 4, 1, 1))):
        c["kw/capacity/" + k] = (f, ("w",) + a, {})
    f = "window_select_frames_keywords"
    for k, a, kw in (("shifted", ("shifted", 8, 2, 3), {}), ("clipped", ("clipped", 8, None, 3), {}), ("clipped-2", ("clipped", 8, 2, 3), {}),
                     ("clipped-3", ("clipped", 8, 3, 3), {}), ("clipped-true", ("clipped", 8, True, 3), {}), ("shifted-none", ("shifted", 8, None, 3), {}),
                     ("rule-unknown", ("both", 8, 2, 3), {}), ("rule-code", (0, 8, 2, 3), {}), ("frames-unknown", ("shifted", 8, 2, 3), dict(frames="some")),
                     ("frames-code", ("shifted", 8, 2, 3), dict(frames=1)), ("sampled", ("shifted", 8, 2, 3), dict(frames="sampled", num_frames=5)),
                     ("sampled-1024", ("clipped", 8, None, 3), dict(frames="sampled", num_frames=1024, k=4, min_sep=2)),
                     ("sampled-none", ("shifted", 8, 2, 3), dict(frames="sampled")), ("sampled-0", ("shifted", 8, 2, 3), dict(frames="sampled", num_frames=0)),
                     ("sampled-1025", ("shifted", 8, 2, 3), dict(frames="sampled", num_frames=1025)),
                     ("sampled-true", ("shifted", 8, 2, 3), dict(frames="sampled", num_frames=True)), ("all-num_frames", ("shifted", 8, 2, 3), dict(num_frames=5)),
                     ("win-0", ("shifted", 0, 2, 3), {}), ("k-65", ("clipped", 8, None, 3), dict(k=65))):
        c["kw/frames/" + k] = (f, ("w",) + a, kw)
    f = "window_gather_keywords"
    for k, a in (("ok", (8, 2, 5)), ("win-0", (0, 2, 5)), ("stride-true", (8, True, 5)), ("num_frames-0", (8, 2, 0)), ("win-below-stride", (2, 3, 5)),
                 ("num_frames-big", (8, 2, 65537)), ("num_frames-max", (8, 2, 65536))):
        c["kw/gather/" + k] = (f, ("w",) + a, {})
    f = "window_gather_dtypes"
    for k, a in (("f32-none", (F32, None)), ("f16-none", (F16, None)), ("bf16-none", (BF16, None)), ("f32-f32", (F32, F32)), ("f32-bf16", (F32, BF16)),
                 ("f16-f32", (F16, F32)), ("bf16-bf16", (BF16, BF16)), ("f16-bf16", (F16, BF16)), ("bf16-f16", (BF16, F16)), ("video-i32", (I32, None)),
                 ("video-f64", (F64, F32)), ("out-i32", (F32, I32)), ("out-text", (F16, "float16"))):
        c["kw/gather-dtypes/" + k] = (f, ("w",) + a, {})
    f = "span_rank_keywords"
    for k, a in (("ok", (5, 0.5, (0.3, 0.5))), ("top-none", (None, 1, ())), ("top-0", (0, 0.5, ())), ("top-true", (True, 0.5, ())), ("top-float", (2.0, 0.5, ())),
                 ("nms-text", (5, "x", ())), ("hit-text", (5, 0.5, ("a",))), ("hit-number", (5, 0.5, 0.5)), ("nms-negative", (5, -0.1, ())), ("nms-nan", (5, float("nan"), ())),
                 ("hit-17", (5, 0.5, tuple(i / 20 for i in range(17))))):
        c["kw/rank/" + k] = (f, ("w",) + a, {})
    f = "skip_nan_flag"
    for k, v in (("true", True), ("false", False), ("1", 1), ("0", 0), ("2", 2), ("text", "yes"), ("none", None), ("float", 1.0)):
        c["kw/skip_nan/" + k] = (f, ("w", v), {})
    f = "span_refine_keywords"
    for k, a, kw in (("ok", (3, 5), {}), ("xx", (64, 128, 4, "xx", True, 1), {}), ("form-unknown", (3, 5), dict(form="wc")), ("form-code", (3, 5), dict(form=1)),
                     ("radius-0", (0, 5), {}), ("radius-65", (65, 5), {}), ("radius-true", (True, 5), {}), ("margin-0", (3, 0), {}), ("margin-129", (3, 129), {}),
                     ("margin-float", (3, 5.0), {}), ("min_len-0", (3, 5, 0), {}), ("min_len-big", (3, 5, 2 ** 31), {}), ("windows-2", (3, 5), dict(return_windows=2)),
                     ("contrast-text", (3, 5), dict(return_contrast="yes")), ("contrast-none", (3, 5), dict(return_contrast=None))):
        c["kw/refine/" + k] = (f, ("w",) + a, kw)
    f = "span_anchors_keywords"
    for k, a, kw in (("ints", ((8, 16, 33),), {}), ("pairs", ([(8, 2), (16, 4)],), dict(score="mean", peak=0, min_usable=3, max_spans=7)),
                     ("triples", (((8, 2, 3), [16, 4, 100], 5),), dict(return_windows=True, return_scale=1)), ("len-1", ((1,),), {}),
                     ("margin-big", (((8, 2, 2 ** 31 - 1),),), {}), ("text", ("8,16",), {}), ("bytes", (b"816",), {}), ("set", ({8, 16},), {}), ("int", (8,), {}),
                     ("none", ((),), {}), ("nine", (tuple(range(1, 10)),), {}), ("score-unknown", ((8,),), dict(score="max")), ("score-code", ((8,),), dict(score=1)),
                     ("scale-float", ((8.0,),), {}), ("scale-four", (((8, 2, 3, 4),),), {}), ("scale-empty", (((),),), {}), ("scale-true", ((True,),), {}),
                     ("scale-mixed", (((8, 2.0),),), {}), ("len-0", ((0,),), {}), ("len-big", ((2 ** 31,),), {}), ("stride-0", (((8, 0),),), {}),
                     ("stride-above", (((8, 9),),), {}), ("margin-0", (((8, 2, 0),),), {}), ("margin-over", (((8, 2, 2 ** 31),),), {}),
                     ("peak-negative", ((8,),), dict(peak=-1)), ("peak-65", ((8,),), dict(peak=65)), ("peak-true", ((8,),), dict(peak=True)),
                     ("min_usable-0", ((8,),), dict(min_usable=0)), ("max_spans-0", ((8,),), dict(max_spans=0)), ("max_spans-2049", ((8,),), dict(max_spans=2049)),
                     ("windows-2", ((8,),), dict(return_windows=2)), ("scale-text", ((8,),), dict(return_scale="no"))):
        c["kw/anchors/" + k] = (f, ("w",) + a, kw)
    return c


def tensor_checker_cases():
    c = {}
    f = "span_propose_shapes"
    for k, (s, m) in layouts().items():
        c["sh/propose/" + k] = (f, ("w", s, m), {})
    for k, a in (("sims-list", ([[0.0]], z(1, 1))), ("mask-none", (z(4, L), None)), ("sims-1d", (z(L), z(1, L))), ("sims-4d", (z(1, 2, 2, L), z(1, L))),
                 ("mask-1d", (z(4, L), z(L))), ("mask-3d", (z(2, 3, L), z(2, 3, L))), ("L-differs", (z(4, L), z(4, L + 1))), ("no-rows", (z(0, L), z(1, L))),
                 ("no-frames", (z(4, 0), z(4, 0))), ("no-mask-rows", (z(4, L), z(0, L))), ("bql-mask-rows", (z(2, 3, L), z(3, L))), ("uneven", (z(4, L), z(3, L))),
                 ("more-mask-rows", (z(2, L), z(4, L))), ("L-max", (torch.empty(1, 1 << 20), torch.empty(1, 1 << 20))),
                 ("L-too-long", (torch.empty(1, (1 << 20) + 1), torch.empty(1, (1 << 20) + 1))), ("sims-i32", (z(4, L, dt=I32), z(4, L))),
                 ("sims-f16", (z(4, L, dt=F16), z(4, L))), ("mask-complex", (z(4, L), z(4, L, dt=torch.complex64))), ("mask-bool", (z(4, L), z(4, L, dt=BOOL))),
                 ("mask-i64", (z(4, L), z(4, L, dt=I64)))):
        c["sh/propose/" + k] = (f, ("w",) + a, {})
    f = "window_select_gt"
    for k, a in (("none", (None, (4,))), ("ok", (z(4, 2), (4,))), ("ok-bq", (z(2, 3, 2, dt=F64), (2, 3))), ("list", ([[0.0, 1.0]], (1,))), ("shape", (z(4, 3), (4,))),
                 ("lead", (z(6, 2), (2, 3))), ("i32", (z(4, 2, dt=I32), (4,)))):
        c["sh/gt/" + k] = (f, ("w",) + a, {})
    m = z(2, L)
    f = "window_select_valid"
    for k, a in (("none", (None, m)), ("f32", (z(2, L), m)), ("bool", (z(2, L, dt=BOOL), m)), ("u8", (z(2, L, dt=U8), m)), ("f16", (z(2, L, dt=F16), m)),
                 ("list", ([[1.0] * L] * 2, m)), ("mask-list", (z(2, L), [[1.0] * L] * 2)), ("both-lists", ([1.0], [1.0])), ("shape", (z(3, L), m)),
                 ("sims-shape", (z(2, 3, L), m)), ("i32", (z(2, L, dt=I32), m)), ("i64", (z(2, L, dt=I64), m))):
        c["sh/valid/" + k] = (f, ("w",) + a, {})
    s = z(2, 3, L)
    f = "span_rows_valid"
    for k, a in (("f32", (z(2, 3, L), s)), ("bool", (z(2, 3, L, dt=BOOL), s)), ("u8", (z(2, 3, L, dt=U8), s)), ("none", (None, s)), ("list", ([1.0], s)),
                 ("sims-list", (z(2, 3, L), [1.0])), ("mask-shape", (z(2, L), s)), ("flat", (z(6, L), s)), ("i32", (z(2, 3, L, dt=I32), s))):
        c["sh/rows-valid/" + k] = (f, ("w",) + a, {})
    f = "span_scores_masked_checks"
    for k, (s, m) in layouts().items():
        if k != "rl-rpm2":                                                                   # (the scores take a mask row per video: [R,L] or [B,L])
            c["sh/scores/" + k] = (f, ("w", s, z(*s.shape[:-1], 5, 2), m), {})
    s, sp, m = z(4, L), z(4, 5, 2), z(4, L)
    for k, a, kw in (("attention", (s, sp, m), dict(pooling="attention", temperature=2, k="unused", skip_nan=True)), ("valid", (s, sp, m, z(4, L, dt=U8)), {}),
                     ("k-64", (s, sp, m), dict(k=64)), ("n0", (s, z(4, 0, 2), m), {}), ("spans-f64", (s, z(4, 5, 2, dt=F64), m), {}),
                     ("pooling-unknown", (s, sp, m), dict(pooling="mean")), ("skip_nan-2", (s, sp, m), dict(skip_nan=2)), ("sims-list", ([0.0], sp, m), {}),
                     ("spans-none", (s, None, m), {}), ("mask-list", (s, sp, [1.0]), {}), ("sims-1d", (z(L), z(5, 2), z(1, L)), {}), ("spans-3", (s, z(4, 5, 3), m), {}),
                     ("spans-rows", (s, z(3, 5, 2), m), {}), ("spans-dim", (s, z(4, 10), m), {}), ("mask-rows", (s, sp, z(2, L)), {}), ("mask-L", (s, sp, z(4, L - 1)), {}),
                     ("bql-mask-per-row", (z(2, 3, L), z(2, 3, 5, 2), z(6, L)), {}), ("sims-f64", (z(4, L, dt=F64), sp, m), {}), ("spans-i32", (s, z(4, 5, 2, dt=I32), m), {}),
                     ("mask-complex", (s, sp, z(4, L, dt=torch.complex64)), {}), ("valid-shape", (s, sp, m, z(2, L)), {}), ("valid-i32", (s, sp, m, z(4, L, dt=I32)), {}),
                     ("valid-list", (s, sp, m, [1.0]), {}), ("no-rows", (z(0, L), z(0, 5, 2), z(0, L)), {}), ("no-frames", (z(4, 0), sp, z(4, 0)), {}),
                     ("rows-65536", (torch.empty(65536, 1), torch.empty(65536, 1, 2), torch.empty(65536, 1)), {}), ("k-0", (s, sp, m), dict(k=0)), ("k-65", (s, sp, m), dict(k=65)),
                     ("k-true", (s, sp, m), dict(k=True)), ("k-float", (s, sp, m), dict(k=3.0)), ("temperature-text", (s, sp, m), dict(temperature="hot")),
                     ("temperature-none", (s, sp, m), dict(temperature=None)), ("temperature-0-topk", (s, sp, m), dict(temperature=0)),
                     ("temperature-0", (s, sp, m), dict(pooling="attention", temperature=0)), ("temperature-inf", (s, sp, m), dict(pooling="attention", temperature=float("inf"))),
                     ("temperature-nan", (s, sp, m), dict(pooling="attention", temperature=float("nan")))):
        c["sh/scores/" + k] = (f, ("w",) + a, kw)
    f = "windows_valid_checks"
    sel, sel3 = z(4, 3, dt=I32), z(2, 3, 3, dt=I32)
    for k, a, kw in (("rl", (sel, z(4, L), "shifted", 4, 2), {}), ("rl-rpm2", (sel, z(2, L), "clipped", 4), {}), ("bql", (sel3, z(2, L), "clipped", 4, None, "sampled", 3), {}),
                     ("valid-count", (sel, z(4, L), "shifted", 4, 2), dict(valid=z(4, L, dt=BOOL), return_count=True)), ("rule-unknown", (sel, z(4, L), "both", 4, 2), {}),
                     ("shifted-none", (sel, z(4, L), "shifted", 4), {}), ("all-num_frames", (sel, z(4, L), "shifted", 4, 2, "all", 3), {}), ("select-list", ([[0]], z(4, L), "shifted", 4, 2), {}),
                     ("mask-none", (sel, None, "shifted", 4, 2), {}), ("select-1d", (z(3, dt=I32), z(1, L), "shifted", 4, 2), {}), ("mask-1d", (sel, z(L), "shifted", 4, 2), {}),
                     ("select-i64", (z(4, 3, dt=I64), z(4, L), "shifted", 4, 2), {}), ("no-rows", (z(0, 3, dt=I32), z(1, L), "shifted", 4, 2), {}),
                     ("no-keep", (z(4, 0, dt=I32), z(4, L), "shifted", 4, 2), {}), ("no-frames", (sel, z(4, 0), "shifted", 4, 2), {}), ("bql-mask-rows", (sel3, z(3, L), "shifted", 4, 2), {}),
                     ("uneven", (sel, z(3, L), "shifted", 4, 2), {}), ("keep-2049", (z(1, 2049, dt=I32), z(1, L), "shifted", 4, 2), {}),
                     ("L-too-long", (z(1, 3, dt=I32), torch.empty(1, (1 << 20) + 1), "shifted", 4, 2), {}), ("win-above-L", (sel, z(4, L), "shifted", 13, 2), {}),
                     ("mask-complex", (sel, z(4, L, dt=torch.complex64), "shifted", 4, 2), {}), ("valid-shape", (sel, z(2, L), "shifted", 4, 2), dict(valid=z(4, L))),
                     ("valid-i32", (sel, z(4, L), "shifted", 4, 2), dict(valid=z(4, L, dt=I32))), ("count-2", (sel, z(4, L), "shifted", 4, 2), dict(return_count=2)),
                     ("count-text", (sel, z(4, L), "shifted", 4, 2), dict(return_count="yes"))):
        c["sh/windows-valid/" + k] = (f, ("w",) + a, kw)
    f = "span_refine_checks"
    for k, (s, m) in layouts().items():
        sp = z(*s.shape[:-1], 5, 2)
        c["sh/refine/" + k] = (f, ("w", s, sp, m), {})
        c["sh/refine/" + k + "/valid-mask"] = (f, ("w", s, sp, m, z(*m.shape, dt=BOOL)), {})
        c["sh/refine/" + k + "/valid-rows"] = (f, ("w", s, sp, m, z(*s.shape, dt=U8)), {})
    s, sp, m = z(4, L), z(4, 5, 2), z(2, L)
    for k, a in (("spans-list", (s, [[0.0, 1.0]], m)), ("sims-list", ([0.0], sp, m)), ("mask-1d", (s, sp, z(L))), ("spans-dim", (s, z(4, 10), m)), ("spans-rows", (s, z(3, 5, 2), m)),
                 ("spans-3", (s, z(4, 5, 3), m)), ("n0", (s, z(4, 0, 2), m)), ("sims-f64", (z(4, L, dt=F64), sp, m)), ("spans-i64", (s, z(4, 5, 2, dt=I64), m)),
                 ("rows-65536", (torch.empty(65536, 1), torch.empty(65536, 1, 2), torch.empty(1, 1))), ("valid-list", (s, sp, m, [1.0])), ("valid-shape", (s, sp, m, z(3, L))),
                 ("valid-i32", (s, sp, m, z(4, L, dt=I32))), ("valid-f16", (s, sp, m, z(2, L, dt=F16)))):
        c["sh/refine/" + k] = (f, ("w",) + a, {})
    f = "span_anchors_checks"
    for k, (s, m) in layouts().items():
        c["sh/anchors/" + k] = (f, ("w", s, m), {})
        c["sh/anchors/" + k + "/valid-mask"] = (f, ("w", s, m, z(*m.shape)), {})
        c["sh/anchors/" + k + "/valid-rows"] = (f, ("w", s, m, z(*s.shape, dt=BOOL)), {})
    s, m = z(4, L), z(2, L)
    for k, a in (("sims-list", ([0.0], m)), ("uneven", (s, z(3, L))), ("sims-f64", (z(4, L, dt=F64), m)), ("valid-list", (s, m, [1.0])), ("valid-shape", (s, m, z(4, L + 1))),
                 ("valid-i64", (s, m, z(2, L, dt=I64)))):
        c["sh/anchors/" + k] = (f, ("w",) + a, {})
    return c


def mask_kinds(shape):
    return {"f32": z(*shape), "bool": z(*shape, dt=BOOL), "u8": z(*shape, dt=U8), "f64": z(*shape, dt=F64)}


def propose_cases():
    c = {}
    for lk, (s, m) in layouts().items():
        for f, valids in (("span_propose", {"": None}), ("span_propose_masked", {"/valid-none": {}, "/valid-mask": dict(valid=z(*m.shape, dt=BOOL))}),
                          ("span_propose_masked_rows", {"/valid-rows": dict(valid=z(*s.shape, dt=U8))})):
            for vk, vkw in valids.items():
                vkw = vkw or {}
                c[f"{f}/{lk}{vk}"] = (f, (s, m), dict(vkw))
                c[f"{f}/{lk}{vk}/all-outputs"] = (f, (s, m), dict(vkw, return_windows=True, return_smoothed=True, max_spans=7, levels=(0.25, 0.5), smooth=3, gap=2, min_len=2,
                                                                 max_len=9, relative=False))
    s, m = z(4, L), z(2, L)
    for f, vkw in (("span_propose", {}), ("span_propose_masked", dict(valid=z(2, L), skip_nan=True)), ("span_propose_masked_rows", dict(valid=z(4, L), skip_nan=1))):
        for mk, mm in mask_kinds((2, L)).items():
            c[f"{f}/mask-{mk}"] = (f, (s, mm), dict(vkw, return_windows=True))
        c[f"{f}/sims-strided"] = (f, (strided((4, L)), m), dict(vkw, return_smoothed=True))
        c[f"{f}/mask-strided"] = (f, (s, strided((2, L))), dict(vkw))
        c[f"{f}/sims-f64"] = (f, (z(4, L, dt=F64), m), dict(vkw))
        c[f"{f}/sims-f16"] = (f, (z(4, L, dt=F16), m), dict(vkw))
        c[f"{f}/smooth-even"] = (f, (s, m), dict(vkw, smooth=2))
        c[f"{f}/uneven"] = (f, (s, z(3, L)), dict(vkw))
        c[f"{f}/sims-list"] = (f, ([0.0], m), dict(vkw))
    for f, good in (("span_propose_masked", z(2, L)), ("span_propose_masked_rows", z(4, L))):
        c[f"{f}/skip_nan-2"] = (f, (s, m), dict(valid=good, skip_nan=2))
        c[f"{f}/valid-i32"] = (f, (s, m), dict(valid=good.to(I32)))
        c[f"{f}/valid-shape"] = (f, (s, m), dict(valid=z(3, L)))
        c[f"{f}/valid-strided"] = (f, (s, m), dict(valid=strided(tuple(good.shape))))
        c[f"{f}/valid-f16"] = (f, (s, m), dict(valid=good.to(F16)))
    c["span_propose_masked/valid-rows-shaped"] = ("span_propose_masked", (s, m), dict(valid=z(4, L)))
    c["span_propose_masked_rows/valid-mask-shaped"] = ("span_propose_masked_rows", (s, m), dict(valid=z(2, L)))
    c["span_propose_masked_rows/valid-none"] = ("span_propose_masked_rows", (s, m), dict(valid=None))
    return c


def select_cases():
    c = {}
    fams = (("window_select", dict(win=4, stride=2, keep=3)), ("window_select_clipped", dict(win=4, keep=3)),
            ("window_select_frames", dict(rule="shifted", win=4, stride=2, keep=3)), ("window_select_frames", dict(rule="clipped", win=4, keep=3)),
            ("window_select_frames", dict(rule="shifted", win=4, stride=1, keep=3, frames="sampled", num_frames=3)),
            ("window_select_frames", dict(rule="clipped", win=5, stride=2, keep=3, frames="sampled", num_frames=2)))
    for f, base in fams:
        tag = f + "".join("/" + str(base[k]) for k in ("rule", "frames") if k in base)
        valids = {"": {}} if f != "window_select_frames" else {"": {}, "/valid": None}
        for lk, (s, m) in layouts().items():
            for vk, vkw in valids.items():
                vkw = dict(valid=z(*m.shape, dt=BOOL)) if vkw is None else vkw
                c[f"{tag}/{lk}{vk}"] = (f, (s, m), dict(base, **vkw))
                c[f"{tag}/{lk}{vk}/all-outputs"] = (f, (s, m), dict(base, **vkw, k=2, min_sep=2, gt=z(*s.shape[:-1], 2), return_scores=True, return_bounds=True, return_order=True))
        s, m = z(4, L), z(2, L)
        for flag in ("return_scores", "return_bounds", "return_order"):
            c[f"{tag}/{flag}"] = (f, (s, m), dict(base, **{flag: True}))
        c[f"{tag}/gt-f64"] = (f, (s, m), dict(base, gt=z(4, 2, dt=F64)))
        c[f"{tag}/gt-strided"] = (f, (s, m), dict(base, gt=strided((4, 2))))
        c[f"{tag}/keep-above-capacity"] = (f, (s, m), dict(base, keep=99))
        for mk, mm in mask_kinds((2, L)).items():
            c[f"{tag}/mask-{mk}"] = (f, (s, mm), dict(base))
        c[f"{tag}/sims-strided"] = (f, (strided((4, L)), m), dict(base))
        c[f"{tag}/sims-f64"] = (f, (z(4, L, dt=F64), m), dict(base))
        c[f"{tag}/keep-0"] = (f, (s, m), dict(base, keep=0))
        c[f"{tag}/win-above-L"] = (f, (s, m), dict(base, win=L + 1))
        c[f"{tag}/min_sep-above"] = (f, (s, m), dict(base, min_sep=50))
        c[f"{tag}/gt-shape"] = (f, (s, m), dict(base, gt=z(4, 3)))
        c[f"{tag}/gt-i32"] = (f, (s, m), dict(base, gt=z(4, 2, dt=I32)))
        c[f"{tag}/uneven"] = (f, (s, z(3, L)), dict(base))
        c[f"{tag}/mask-complex"] = (f, (s, z(2, L, dt=torch.complex64)), dict(base))
    s, m = z(4, L), z(2, L)
    f, base = "window_select_frames", dict(rule="shifted", win=4, stride=2, keep=3)
    for vk, v in (("u8", z(2, L, dt=U8)), ("f32", z(2, L)), ("f64-strided", strided((2, L)).to(F64)), ("strided", strided((2, L)))):
        c[f"{f}/valid-{vk}"] = (f, (s, m), dict(base, valid=v))
    c[f"{f}/valid-i32"] = (f, (s, m), dict(base, valid=z(2, L, dt=I32)))
    c[f"{f}/valid-sims-shaped"] = (f, (s, m), dict(base, valid=z(4, L)))
    c[f"{f}/rule-unknown"] = (f, (s, m), dict(base, rule="both"))
    c[f"{f}/all-num_frames"] = (f, (s, m), dict(base, num_frames=3))
    c[f"{f}/sampled-none"] = (f, (s, m), dict(base, frames="sampled"))
    c[f"{f}/clipped-stride-3"] = (f, (s, m), dict(base, rule="clipped", stride=3))
    c[f"{f}/shifted-no-stride"] = (f, (s, m), dict(rule="shifted", win=4, keep=3))
    c["window_select/stride-above-win"] = ("window_select", (s, m), dict(win=2, stride=3, keep=1))
    c["window_select/too-many"] = ("window_select", (z(1, 4100), z(1, 4100)), dict(win=2, stride=2, keep=1))
    return c


def gather_cases():
    c = {}
    d = 8
    for f, base in (("window_gather", dict(win=4, stride=2, num_frames=3)), ("window_gather_clipped", dict(win=4, num_frames=3))):
        def case(key, video, select, **kw):
            if f == "window_gather":
                c[f"{f}/{key}"] = (f, (video, select), dict(base, **kw))
            else:
                c[f"{f}/{key}"] = (f, (video,), dict(base, select=select, **kw))
        v2, v3 = z(L, d), z(2, L, d)
        s1, s2, s3 = z(3, dt=I32), z(4, 3, dt=I32), z(2, 2, 3, dt=I32)
        for vk, v in (("ld", v2), ("bld", v3)):
            for sk, s in (("select-1d", s1), ("select-2d", s2), ("select-3d", s3)):
                case(f"{vk}/{sk}", v, s)
            case(f"{vk}/mask-index", v, s2, mask=z(*v.shape[:-1]), return_index=True)
            case(f"{vk}/mask-bool", v, s2, mask=z(*v.shape[:-1], dt=BOOL))
            case(f"{vk}/mask-shape", v, s2, mask=z(*v.shape[:-1], 1))
            case(f"{vk}/mask-complex", v, s2, mask=z(*v.shape[:-1], dt=torch.complex64))
        if f == "window_gather_clipped":
            for vk, v in (("ld", v2), ("bld", v3), ("ld-frame-stride", z(L, 2 * d)[:, :d]), ("bld-frame-stride", z(2, L, d + 3)[:, :, :d]), ("bld-f16", z(2, L, d, dt=F16))):
                case(f"{vk}/select-none", v, None)
                case(f"{vk}/select-none/mask-index", v, None, mask=z(*v.shape[:-1], dt=U8), return_index=True)
            case("odd-win/select-none", z(15, d), None, win=5)
            case("select-none/win-above-L", v2, None, win=L + 1)
            case("select-none/L-too-long", torch.empty((1 << 20) + 1, 1), None)
        case("ld/frame-stride", z(L, 2 * d)[:, :d], s2)
        case("bld/frame-stride", z(2, L, d + 3)[:, :, :d], s3, return_index=True)
        case("bld/video-stride", z(2, L + 2, d)[:, :L], s2)
        case("bld/one-video-stride", z(1, L + 2, d)[:, :L], s2)
        case("ld/element-stride", strided((L, d)), s2)
        case("ld/transposed", z(d, L).t(), s2)
        case("select-strided", v2, z(4, 6, dt=I32)[:, ::2])
        for vt in (F32, F16, BF16):
            for ot in (None, F32, F16, BF16):
                case(f"dtypes/{vt}-{ot}".replace("torch.", ""), z(L, d, dt=vt), s2, out_dtype=ot)
        case("video-i32", z(L, d, dt=I32), s2)
        case("out-i32", v2, s2, out_dtype=I32)
        case("video-list", [[0.0]], s2)
        case("select-list", v2, [0, 1])
        case("mask-list", v2, s2, mask=[1.0])
        case("video-1d", z(L), s2)
        case("video-4d", z(1, 2, L, d), s2)
        case("video-empty", z(L, 0), s2)
        case("select-4d", v3, z(2, 1, 2, 3, dt=I32))
        case("select-empty", v2, z(4, 0, dt=I32))
        case("select-i64", v2, z(4, 3, dt=I64))
        case("select-3d-for-ld", v2, s3)
        case("select-3d-videos", v3, z(3, 2, 3, dt=I32))
        case("select-uneven", v3, z(3, 3, dt=I32))
        case("L-too-long", torch.empty((1 << 20) + 1, 1), s2)
        case("win-above-L", v2, s2, win=L + 1)
        case("win-0", v2, s2, win=0)
        case("num_frames-big", v2, s2, num_frames=65537)
    c["window_gather/stride-above-win"] = ("window_gather", (z(L, 8), z(3, dt=I32)), dict(win=2, stride=3, num_frames=3))
    return c


def scores_cases():
    c = {}
    for f in ("span_scores_masked", "span_scores_masked_rows"):
        rows = f.endswith("_rows")
        for lk, (s, m) in (("rl", (z(4, L), z(4, L))), ("bql", (z(2, 3, L), z(2, L)))):
            sp = z(*s.shape[:-1], 5, 2)
            valids = {"/valid-rows": z(*s.shape, dt=BOOL)} if rows else {"/valid-none": None, "/valid-mask": z(*m.shape, dt=U8)}
            for vk, v in valids.items():
                c[f"{f}/{lk}{vk}"] = (f, (s, sp, m), dict(valid=v))
                c[f"{f}/{lk}{vk}/all-outputs"] = (f, (s, sp, m), dict(valid=v, skip_nan=True, k=5, return_windows=True, return_usable=True))
                c[f"{f}/{lk}{vk}/attention"] = (f, (s, sp, m), dict(valid=v, pooling="attention", temperature=0.5, return_usable=True))
                c[f"{f}/{lk}{vk}/n0"] = (f, (s, z(*s.shape[:-1], 0, 2), m), dict(valid=v, return_windows=True, return_usable=True))
        s, sp, m = z(4, L), z(4, 5, 2), z(4, L)
        good = z(4, L)
        c[f"{f}/return_windows"] = (f, (s, sp, m), dict(valid=good, return_windows=True))
        for mk, mm in mask_kinds((4, L)).items():
            c[f"{f}/mask-{mk}"] = (f, (s, sp, mm), dict(valid=good))
            c[f"{f}/valid-{mk}"] = (f, (s, sp, m), dict(valid=mm))
        c[f"{f}/sims-strided"] = (f, (strided((4, L)), sp, m), dict(valid=good))
        c[f"{f}/spans-f64-strided"] = (f, (s, strided((4, 5, 2)).to(F64), m), dict(valid=good))
        c[f"{f}/valid-strided"] = (f, (s, sp, m), dict(valid=strided((4, L))))
        c[f"{f}/sims-f64"] = (f, (z(4, L, dt=F64), sp, m), dict(valid=good))
        c[f"{f}/valid-i32"] = (f, (s, sp, m), dict(valid=z(4, L, dt=I32)))
        c[f"{f}/valid-shape"] = (f, (s, sp, m), dict(valid=z(2, L)))
        c[f"{f}/valid-list"] = (f, (s, sp, m), dict(valid=[1.0]))
        c[f"{f}/skip_nan-text"] = (f, (s, sp, m), dict(valid=good, skip_nan="yes"))
        c[f"{f}/k-65"] = (f, (s, sp, m), dict(valid=good, k=65))
        c[f"{f}/pooling-unknown"] = (f, (s, sp, m), dict(valid=good, pooling="max"))
        c[f"{f}/temperature-0"] = (f, (s, sp, m), dict(valid=good, pooling="attention", temperature=0.0))
        c[f"{f}/mask-rows"] = (f, (s, sp, z(2, L)), dict(valid=good))
    c["span_scores_masked_rows/valid-none"] = ("span_scores_masked_rows", (z(4, L), z(4, 5, 2), z(4, L)), dict(valid=None))
    c["span_scores_masked_rows/bql/valid-mask-shaped"] = ("span_scores_masked_rows", (z(2, 3, L), z(2, 3, 5, 2), z(2, L)), dict(valid=z(2, L)))
    c["span_scores_masked/bql/valid-rows-shaped"] = ("span_scores_masked", (z(2, 3, L), z(2, 3, 5, 2), z(2, L)), dict(valid=z(2, 3, L)))
    for lk, f, (s, m) in (("rl", "span_scores", (z(4, L), z(4, L))), ("bql", "span_scores_multi", (z(2, 3, L), z(2, L)))):
        c[f"{f}/{lk}"] = (f, (s, z(*s.shape[:-1], 5, 2), m), {})
        c[f"{f}/{lk}/windows"] = (f, (s, z(*s.shape[:-1], 5, 2), m.to(BOOL)), dict(pooling="attention", return_windows=True))
    return c


def later_stage_cases():
    c = {}
    f = "windows_valid"
    for lk, (sel, m) in (("rl", (z(4, 3, dt=I32), z(4, L))), ("rl-rpm2", (z(4, 3, dt=I32), z(2, L))), ("bql", (z(2, 3, 3, dt=I32), z(2, L)))):
        for rk, kw in (("shifted", dict(rule="shifted", win=4, stride=2)), ("clipped", dict(rule="clipped", win=4)),
                       ("shifted/sampled", dict(rule="shifted", win=4, stride=1, frames="sampled", num_frames=3)),
                       ("clipped/sampled", dict(rule="clipped", win=5, frames="sampled", num_frames=2))):
            c[f"{f}/{rk}/{lk}"] = (f, (sel, m), kw)
            c[f"{f}/{rk}/{lk}/valid-count"] = (f, (sel, m), dict(kw, valid=z(*m.shape, dt=BOOL), return_count=True))
    sel, m, kw = z(4, 3, dt=I32), z(2, L), dict(rule="shifted", win=4, stride=2)
    for mk, mm in mask_kinds((2, L)).items():
        c[f"{f}/mask-{mk}"] = (f, (sel, mm), kw)
        c[f"{f}/valid-{mk}"] = (f, (sel, m), dict(kw, valid=mm))
    c[f"{f}/select-strided"] = (f, (z(4, 6, dt=I32)[:, ::2], m), dict(kw, valid=strided((2, L))))
    c[f"{f}/select-i64"] = (f, (z(4, 3, dt=I64), m), kw)
    c[f"{f}/valid-i32"] = (f, (sel, m), dict(kw, valid=z(2, L, dt=I32)))
    c[f"{f}/count-2"] = (f, (sel, m), dict(kw, return_count=2))
    c[f"{f}/win-above-L"] = (f, (sel, m), dict(kw, win=L + 1))

    f = "span_refine"
    base = dict(radius=3, margin=5)
    for lk, (s, m) in layouts().items():
        sp = z(*s.shape[:-1], 5, 2)
        for vk, v in (("valid-none", None), ("valid-mask", z(*m.shape, dt=BOOL)), ("valid-rows", z(*s.shape, dt=U8))):
            c[f"{f}/{lk}/{vk}"] = (f, (s, sp, m), dict(base, valid=v))
            c[f"{f}/{lk}/{vk}/xx-all-outputs"] = (f, (s, sp, m), dict(base, valid=v, form="xx", min_len=2, return_windows=True, return_contrast=True))
            c[f"{f}/{lk}/{vk}/n0"] = (f, (s, z(*s.shape[:-1], 0, 2), m), dict(base, valid=v, return_windows=True, return_contrast=True))
    s, sp, m = z(4, L), z(4, 5, 2), z(2, L)
    c[f"{f}/return_windows"] = (f, (s, sp, m), dict(base, return_windows=True))
    c[f"{f}/return_contrast"] = (f, (s, sp, m), dict(base, return_contrast=True))
    for mk, mm in mask_kinds((2, L)).items():
        c[f"{f}/mask-{mk}"] = (f, (s, sp, mm), base)
        c[f"{f}/valid-{mk}"] = (f, (s, sp, m), dict(base, valid=mm))
    c[f"{f}/all-strided"] = (f, (strided((4, L)), strided((4, 5, 2)).to(F64), strided((2, L))), dict(base, valid=strided((4, L))))
    c[f"{f}/radius-65"] = (f, (s, sp, m), dict(radius=65, margin=5))
    c[f"{f}/form-unknown"] = (f, (s, sp, m), dict(base, form="wc"))
    c[f"{f}/sims-f64"] = (f, (z(4, L, dt=F64), sp, m), base)
    c[f"{f}/spans-list"] = (f, (s, [[0.0, 1.0]], m), base)
    c[f"{f}/valid-shape"] = (f, (s, sp, m), dict(base, valid=z(3, L)))
    c[f"{f}/valid-i32"] = (f, (s, sp, m), dict(base, valid=z(2, L, dt=I32)))
    c[f"{f}/valid-list"] = (f, (s, sp, m), dict(base, valid=[1.0]))

    f = "span_anchors"
    base = dict(scales=(4, (6, 2), (8, 2, 3)))
    for lk, (s, m) in layouts().items():
        for vk, v in (("valid-none", None), ("valid-mask", z(*m.shape, dt=U8)), ("valid-rows", z(*s.shape, dt=BOOL))):
            for sk in ("contrast", "mean"):
                c[f"{f}/{lk}/{vk}/{sk}"] = (f, (s, m), dict(base, valid=v, score=sk))
            c[f"{f}/{lk}/{vk}/all-outputs"] = (f, (s, m), dict(base, valid=v, peak=0, min_usable=2, max_spans=9, return_windows=True, return_scale=True))
    s, m = z(4, L), z(2, L)
    c[f"{f}/return_windows"] = (f, (s, m), dict(base, return_windows=True))
    c[f"{f}/return_scale"] = (f, (s, m), dict(base, return_scale=True))
    c[f"{f}/one-scale"] = (f, (s, m), dict(scales=[5]))
    c[f"{f}/margin-max"] = (f, (s, m), dict(scales=[(5, 1, 2 ** 31 - 1)]))
    for mk, mm in mask_kinds((2, L)).items():
        c[f"{f}/mask-{mk}"] = (f, (s, mm), base)
        c[f"{f}/valid-{mk}"] = (f, (s, m), dict(base, valid=mm))
    c[f"{f}/all-strided"] = (f, (strided((4, L)), strided((2, L))), dict(base, valid=strided((2, L))))
    c[f"{f}/scales-text"] = (f, (s, m), dict(scales="4"))
    c[f"{f}/score-unknown"] = (f, (s, m), dict(base, score="max"))
    c[f"{f}/sims-f64"] = (f, (z(4, L, dt=F64), m), base)
    c[f"{f}/uneven"] = (f, (s, z(3, L)), base)
    c[f"{f}/valid-shape"] = (f, (s, m), dict(base, valid=z(3, L)))
    c[f"{f}/valid-i32"] = (f, (s, m), dict(base, valid=z(4, L, dt=I32)))
    c[f"{f}/valid-list"] = (f, (s, m), dict(base, valid=[1.0]))

    f = "span_rank"
    for lk, sc in (("rl", z(4, 5)), ("bql", z(2, 3, 5))):
        c[f"{f}/{lk}"] = (f, (sc, z(*sc.shape, 2)), {})
        c[f"{f}/{lk}/top-order"] = (f, (sc, z(*sc.shape, 2, dt=F64)), dict(top=3, nms_iou=0.5, form="xx", return_order=True))
    c[f"{f}/n0"] = (f, (z(4, 0), z(4, 0, 2)), {})
    c[f"{f}/top-0"] = (f, (z(4, 5), z(4, 5, 2)), dict(top=0))
    return c


def all_cases():
    c = {}
    for part in (keyword_checker_cases, tensor_checker_cases, propose_cases, select_cases, gather_cases, scores_cases, later_stage_cases):
        for k, v in part().items():
            assert k not in c, k
            c[k] = v
    return c


# ---- running a case with the stand-ins, and the record it leaves ----
class Ptr(int):
    """What the stand-in for hip.ptr returns: the address, known to be one."""


class Recorder:
    """A library: every entry is recorded and answers 0 (a workspace query: 4096 bytes)."""

    def __init__(self, calls, tag):
        self.calls, self.tag = calls, tag

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((self.tag, name, args))
            return 4096 if name.endswith("_workspace") else 0
        return fn


@contextlib.contextmanager
def patched(pairs):
    old = [(o, n, getattr(o, n)) for o, n, _ in pairs]
    for o, n, v in pairs:
        setattr(o, n, v)
    try:
        yield
    finally:
        for o, n, v in old:
            setattr(o, n, v)


def tensors_in(x):
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, (list, tuple)):
        for e in x:
            yield from tensors_in(e)
    elif isinstance(x, dict):
        for e in x.values():
            yield from tensors_in(e)


class Resolver:
    """Addresses -> where they point: into the n-th distinct storage of the inputs, into a returned tensor, or into a copy."""

    def __init__(self, inputs):
        self.storages, self.outputs = [], {}
        for t in tensors_in(inputs):
            s = t.untyped_storage()
            if s.nbytes() and all(s.data_ptr() != p for p, _ in self.storages):
                self.storages.append((s.data_ptr(), s.nbytes()))

    def __call__(self, p):
        if not p:
            return None
        for name, t in self.outputs.items():
            if t.numel() and t.data_ptr() <= p < t.data_ptr() + t.numel() * t.element_size():
                return [name, p - t.data_ptr()]
        for i, (base, size) in enumerate(self.storages):
            if base <= p < base + size:
                return [i, p - base]
        return "copy"


def plain(v, resolve):
    """One argument of an entry, or one returned value -> JSON."""
    if isinstance(v, ctypes.Array):
        return [plain(e, resolve) for e in v]
    if isinstance(v, Ptr):
        return dict(ptr=resolve(int(v)))
    if torch.is_tensor(v):
        return dict(shape=list(v.shape), dtype=str(v.dtype))
    if isinstance(v, torch.dtype):
        return str(v)
    if isinstance(v, (list, tuple)):
        return [plain(e, resolve) for e in v]
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, float):
        return v if v == v and abs(v) != float("inf") else repr(v)
    return repr(v)


def lib_tag(f):
    return "lib:" + (str(f.dtype) if torch.is_tensor(f) else str(f))


def run_case(case):
    """-> the record of one case: {"calls": [...], "returns": ...} or {"refused": [class name, message]}."""
    from revisionllm_amd import hip, ops
    fn, args, kwargs = case
    calls = []
    pairs = [(hip, "lib", lambda f=None: Recorder(calls, lib_tag(f))), (hip, "ext_lib", lambda: Recorder(calls, "ext")),
             (hip, "chain_lib", lambda: Recorder(calls, "chain")), (hip, "ptr", lambda t: None if t is None else Ptr(t.data_ptr())), (hip, "stream", lambda: None)]
    resolve = Resolver((args, kwargs))
    prev = hip.set_flavour("f16")                                                             # (the records name the default flavour's 16-bit type: the fp16 build's)
    with patched(pairs):
        try:
            out = getattr(ops, fn)(*args, **kwargs)
        except Exception as e:                                                               # noqa: BLE001 (whatever is raised is the record)
            assert calls == [], "refused after a library was touched"
            return dict(refused=[type(e).__name__, str(e)])
        finally:
            hip.set_flavour(prev)
    if hasattr(out, "_asdict"):
        fields = out._asdict()
    elif torch.is_tensor(out):
        fields = {"out": out}
    elif isinstance(out, tuple) and any(torch.is_tensor(t) for t in out):
        fields = {"out%d" % i: t for i, t in enumerate(out)}
    else:
        fields = None
    if fields is None:
        returns = plain(out, resolve)                                                         # a checker's plain values
    else:
        resolve.outputs = {k: t for k, t in fields.items() if torch.is_tensor(t)}
        returns = {k: plain(t, resolve) for k, t in fields.items()}
    return dict(calls=[dict(lib=tag, entry=name, args=[plain(a, resolve) for a in a_]) for tag, name, a_ in calls], returns=returns)


CLASSES = {"V": "ValueError", "H": "HipLibraryError", "T": "TypeError", "A": "AttributeError"}


def digest(x):
    return hashlib.sha256(json.dumps(x, sort_keys=True).encode()).hexdigest()[:6]


def short(record):
    """What the golden file keeps of a record."""
    if "refused" in record:
        return record["refused"][0][0] + digest(record["refused"][1])
    return digest(record)


@pytest.fixture(scope="module")
def records():
    return {k: run_case(c) for k, c in all_cases().items()}


@pytest.fixture(scope="module")
def golden_records():
    with open(GOLDEN) as f:
        g = json.load(f)
    return dict(keys=g["keys"], records=g["records"].split())


def test_the_golden_file_is_small_and_names_these_cases(records, golden_records):
    assert os.path.getsize(GOLDEN) < 16384
    assert golden_records["keys"] == digest(sorted(records)), "the case list has changed: regenerate the golden file from the REFERENCE commit (module docstring)"
    assert len(golden_records["records"]) == len(records)
    assert set(REWORDED) <= set(records)


def test_every_entry_every_library_and_every_axis_are_covered(records):
    entries = {}
    for k, r in records.items():
        for call in r.get("calls", []):
            entries.setdefault((call["lib"].split(":")[0], call["entry"]), []).append(k)
    assert sorted(entries) == sorted([("lib", "rv_span_scores"), ("lib", "rv_span_scores_multi"), ("lib", "rv_span_rank"), ("lib", "rv_span_propose"),
                                      ("lib", "rv_window_select"), ("lib", "rv_window_gather"), ("lib", "rv_window_gather_rule"), ("ext", "rvx_window_select_clipped"),
                                      ("chain", "rvc_window_select_frames"), ("chain", "rvc_span_scores_masked"), ("chain", "rvc_span_scores_masked_rows"),
                                      ("chain", "rvc_span_propose_masked"), ("chain", "rvc_span_propose_masked_rows"), ("chain", "rvc_windows_valid"),
                                      ("chain", "rvc_span_refine"), ("chain", "rvc_span_anchors_workspace"), ("chain", "rvc_span_anchors")])
    cases = all_cases()
    for f in {c[0] for c in cases.values()}:                                                 # every function: accepted and refused
        mine = [records[k] for k, c in cases.items() if c[0] == f]
        assert any("refused" in r for r in mine) or f in ("span_scores", "span_scores_multi"), f
        assert any("refused" not in r for r in mine), f
    launches = [r for r in records.values() if r.get("calls")]
    assert all(len(r["calls"]) == (2 if r["calls"][0]["entry"].endswith("_workspace") else 1) for r in launches)
    text = json.dumps(launches)
    assert '"copy"' in text and "null" in text
    assert {c["lib"] for r in launches for c in r["calls"] if "gather" in c["entry"]} == {"lib:f16", "lib:bf16"}
    assert any(r["calls"] == [] for r in records.values() if "calls" in r and isinstance(r["returns"], dict))      # N = 0: no launch
    assert {r["refused"][0] for r in records.values() if "refused" in r} <= set(CLASSES.values())


def test_the_records_are_the_reference_commits(records, golden_records):
    """Every case: the same entries with the same arguments and the same returned shapes, or the same refusal - class always, text unless the key is in REWORDED
    (then the text given there)."""
    wrong = []
    for i, k in enumerate(sorted(records)):
        want, r = golden_records["records"][i], records[k]
        if k in REWORDED:
            assert "refused" in r and want[0] in CLASSES, k
            if r["refused"] != [CLASSES[want[0]], REWORDED[k]]:
                wrong.append((k, "reworded refusal: expected " + repr([CLASSES[want[0]], REWORDED[k]]), r))
        elif short(r) != want:
            wrong.append((k, "expected " + want, r))
    assert not wrong, "%d case(s) differ from the reference commit (the module docstring says how to see the reference's records):\n" % len(wrong) + \
        "\n".join(f"{k}: {why}, got {short(r)}: {json.dumps(r, sort_keys=True)}" for k, why, r in wrong[:20])


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="write tests/golden/grounding_call_records.json from the checkout at --root (the reference commit)")
    ap.add_argument("--root", required=True)
    ap.add_argument("--full", help="also write the whole records to this file")
    a = ap.parse_args()
    if os.path.realpath(a.root) == os.path.realpath(os.path.dirname(HERE)):
        sys.exit("--root is the tree this module sits in: the golden file comes from the REFERENCE commit, never from the code under test")
    sys.path.insert(0, os.path.abspath(a.root))
    recs = {k: run_case(c) for k, c in all_cases().items()}
    with open(GOLDEN, "w") as f:
        json.dump(dict(keys=digest(sorted(recs)), records=" ".join(short(recs[k]) for k in sorted(recs))), f, separators=(",", ":"))
        f.write("\n")
    if a.full:
        with open(a.full, "w") as f:
            json.dump(recs, f, sort_keys=True, indent=1)
    print(f"{len(recs)} cases, {sum('refused' in r for r in recs.values())} refusals -> {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
