"""SHA-256 digests of what the CLIP grounding chain's entries write, for a fixed, seeded case list: the check that a change of csrc/grounding.h,
csrc/similarity.hip, csrc/rank.hip, csrc/propose.hip, csrc/prefilter.hip or the stage-2 scores of csrc/sample.hip leaves every output bit where it was.

    REVISION_HIP_LIB=... REVISION_HIP_LIB_BF16=... python tools/grounding_digest.py [--out FILE]     (default: profiles/grounding_digest.json)

Run it once on a build of the parent commit (the two variables name its libraries) and once on this tree's build, in a fresh process each on the same
machine; the two files must hold the same digests.  Both operand flavours run.  Every entry is called through ``ops``; while a case runs, ``torch.empty``
hands out tensors pre-filled with NaN (floating point) or -1 (integers), so a missing store shows as well as a stray one.  The cases that differ
only in the keywords behind the colon of their name form a group; a group's digest is the SHA-256 over its cases in turn, each with its name and all
its outputs in the order the wrapper returns them.

The shapes are the smallest that reach every kernel form and edge:
  frame_cosine        B = 2, L = 70; d = 768 (16-byte loads) and d = 100 on a view one element off 16-byte alignment (element loads); 16-bit and f32
  frame_cosine_multi  Q = 1, 17, 129 (1, 2 and 8 + 1 query tiles), L = 130 (two blocks, a ragged one), d = 768 and d = 6; 16-bit and f32
  span_scores(_multi) L = 200, N = 9: windows of 0, 1, 65 and L frames and two non-finite spans, a NaN inside the 65-frame window; k = 1, 3, 64; both poolings
  span_rank           N = 5, 64 (wave kernel), 65, 300, 2048 (block kernel); R = 5; top 1 / 5 / N; nms_iou 0, 0.5, 1; ties, a NaN and a -inf score, a void
                      span; both forms; with gt (five thresholds) and without; the order
  span_propose        L = 63, 300, 700; T = 1, 5, 8; smooth 1 / 5 / 65; gap 0 / 2 / 63; relative on and off; max_spans 4 and 256; windows and smoothed
  window_select       L = 700, win 64, stride 4 and L = 2300, win 1101, stride 3 (windows of more than 1024 frames); keep 3 and Wcap; min_sep 1 and 3; k 3
                      and 64; gt; scores, bounds and order
  topk_cosine         n = 3, T = 70; d = 768 (fast kernel) and d = 100 (generic); k = 0, 3, 64; one NaN similarity; 16-bit and f32
  topk_pool, attn_pool  Nv = 2, Nt = 3, T = 70; d = 768 and 100; 16-bit and f32
The chain library's entries (f32 rows only: one build for both flavours, so they run once, under "chain"; REVISION_HIP_LIB_EXT and REVISION_HIP_LIB_CHAIN
name the parent's builds), on [3, 3, L] rows with L = 63, 257 and 700, one NaN frame a row, N = 9 spans with an empty, two non-finite and a span past the row:
  window_select_clipped   win 16 (L = 63) or 64; keep 3 and Wcap; min_sep 1 and 3; k 3 and 64; gt; scores, bounds and order
  window_select_frames    both rules, both frame sets (5 sampled frames), with a validity row per mask row and without; gt; scores, bounds and order
  span_scores_masked(_rows)    both poolings, k 1 / 3 / 64, skip_nan on and off; valid None and per mask row (per row for _rows); windows and usable counts
  span_propose_masked(_rows)   T = 5; smooth 1 / 5; gap 0 / 2; relative on and off; skip_nan on and off; valid as above; windows and smoothed
  windows_valid           both rules, both frame sets; a select with -1 padding, a duplicate and an index past the windows; valid on and off; the counts
  span_refine             both forms; radius / margin 3 / 5 and 64 / 128; min_len 1 and 4; valid None, per mask row and per row; windows and contrasts
  span_anchors            both scores; three scales (8, (16, 4), (33, 5, 7)); peak 0 and 2; max_spans 4 and 256; valid as span_refine; windows and scales
The stages that take a mask run on [B = 3, Q = 3, L] rows with one mask row per three rows: all ones (D = L), 0 / 1 with min(130, L - 10) ones, and
fractional values (which hold the order of the duration sum).
"""
import argparse
import hashlib
import itertools
import json
import math
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from revisionllm_amd import hip, ops  # noqa: E402

NAN, INF = float("nan"), float("inf")
_empty = torch.empty


def sentinel_empty(*size, **kw):
    t = _empty(*size, **kw)
    return t.fill_(NAN if t.dtype.is_floating_point else -1)


def rnd(name, *shape, uniform=False):
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    return (torch.rand if uniform else torch.randn)(*shape, generator=g)


def output_bytes(out):
    torch.cuda.synchronize()
    parts = out if isinstance(out, tuple) else (out,)
    return b"".join(t.cpu().contiguous().view(torch.uint8).numpy().tobytes() for t in parts if t is not None)


def off_by_one(t):
    """The same values in a contiguous view that starts one element behind a 16-byte boundary."""
    buf = _empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


def masks(L):
    m = torch.ones(3, L)
    m[1] = 0
    m[1, torch.randperm(L, generator=torch.Generator().manual_seed(L))[:min(130, L - 10)]] = 1
    m[2] = 0.05 + 0.9 * rnd("mask%d" % L, L, uniform=True)
    return m.cuda()


def rows(name, L):
    """[3, 3, L] similarity-like rows: slow waves plus noise, one NaN frame."""
    t = torch.arange(L, dtype=torch.float32)
    phase = rnd(name + "phase", 3, 3, 1, uniform=True) * 6.28
    s = 0.5 + 0.35 * torch.sin(t / (7.0 + 9.0 * rnd(name + "per", 3, 3, 1, uniform=True)) + phase) + 0.08 * rnd(name, 3, 3, L)
    s[0, 1, L // 3] = NAN
    return s.cuda()


def cases(dt):
    """("group:case", thunk) of every case, the cases of a group in a row; dt: the flavour's 16-bit dtype."""
    feats = (("op16", dt), ("f32", torch.float32))
    for (fn, fd), d in itertools.product(feats, (768, 100)):
        video, text = rnd("fc_v%d" % d, 2, 70, d).to(fd).cuda(), rnd("fc_t%d" % d, 2, d).cuda()
        video = off_by_one(video) if d == 100 else video
        yield "frame_cosine/%s/d%d" % (fn, d), lambda v=video, t=text: ops.frame_cosine(t, v)
    for (fn, fd), d, Q in itertools.product(feats, (768, 6), (1, 17, 129)):
        video, text = rnd("fcm_v%d" % d, 2, 130, d).to(fd).cuda(), rnd("fcm_t%d_%d" % (d, Q), 2, Q, d).cuda()
        yield "frame_cosine_multi/%s/d%d:Q%d" % (fn, d, Q), lambda v=video, t=text: ops.frame_cosine_multi(t, v)

    L, D = 200, 130.0
    spans = rnd("ss_spans", 2, 3, 9, 2, uniform=True) * torch.tensor([1.0, 0.4])
    fixed = torch.tensor([[0.5, -0.01], [10.5 / D, 0.5 / D], [72.5 / D, 64.5 / D], [1.0, 4.0], [NAN, 0.1], [0.5, INF]])   # 0, 1, 65, L frames; non-finite
    spans[:, :, :6] = fixed
    sims = rnd("ss_sims", 2, 3, L)
    sims[0, :, 50] = NAN
    m = masks(L)[1:]                                                      # duration 130 and a fractional row
    spans, sims = spans.cuda(), sims.cuda()
    for k, (pooling, tau) in itertools.product((1, 3, 64), (("topk", 0.01), ("attention", 0.01), ("attention", 1.0))):
        kw = dict(k=k, pooling=pooling, temperature=tau, return_windows=True)
        yield "span_scores/%s%g:k%d" % (pooling, tau, k), lambda kw=kw: ops.span_scores(sims[:, 0].contiguous(), spans[:, 0].contiguous(), m, **kw)
        yield "span_scores_multi/%s%g:k%d" % (pooling, tau, k), lambda kw=kw: ops.span_scores_multi(sims, spans, m, **kw)

    for N in (5, 64, 65, 300, 2048):
        scores = (rnd("sr_s%d" % N, 5, N) * 4).round() / 4                # ties
        scores[0, 1], scores[1, 2] = NAN, -INF
        cxw = torch.stack([rnd("sr_c%d" % N, 5, N, uniform=True), 0.02 + 0.3 * rnd("sr_w%d" % N, 5, N, uniform=True)], -1)
        cxw[2, 3, 1] = 0.0                                                  # a void span
        xx = torch.stack([cxw[..., 0] - 0.5 * cxw[..., 1], cxw[..., 0] + 0.5 * cxw[..., 1]], -1)
        gt = torch.tensor([[0.2, 0.5], [0.0, 1.0], [0.6, 0.61], [0.4, 0.4], [0.1, 0.9]]).cuda()
        scores, cxw, xx = scores.cuda(), cxw.cuda(), xx.cuda()
        for top, nms, form in itertools.product(sorted({1, 5, N}), (0.0, 0.5, 1.0), ("cxw", "xx")):
            sp = cxw if form == "cxw" else xx
            yield ("span_rank/N%d/%s:top%d/nms%g" % (N, form, top, nms),
                   lambda a=(scores, sp), kw=dict(top=top, nms_iou=nms, form=form): tuple(ops.span_rank(*a, gt=gt, return_order=True, **kw)))
        yield "span_rank/N%d/cxw:nogt" % N, lambda a=(scores, cxw): tuple(ops.span_rank(*a, top=5, nms_iou=0.5))

    for L in (63, 300, 700):
        s, m = rows("sp%d" % L, L), masks(L)
        for T, smooth, gap, relative, cap in itertools.product((1, 5, 8), (1, 5, 65), (0, 2, 63), (True, False), (4, 256)):
            levels = [0.2 + 0.7 * i / max(T - 1, 1) for i in range(T)] if T > 1 else [0.55]
            kw = dict(levels=levels, relative=relative, smooth=smooth, gap=gap, max_spans=cap, return_windows=True, return_smoothed=True)
            yield "span_propose/L%d/T%d:smooth%d/gap%d/rel%d/cap%d" % (L, T, smooth, gap, relative, cap), lambda s=s, m=m, kw=kw: tuple(ops.span_propose(s, m, **kw))

    for L, win, stride in ((700, 64, 4), (2300, 1101, 3)):
        s, m = rows("ws%d" % L, L), masks(L)
        wcap = max(1, math.ceil(L / (win // stride)) - 1)
        gt = (rnd("ws_gt%d" % L, 3, 3, 1, uniform=True) * 0.8 * L + torch.tensor([0.0, 0.15 * L])).cuda()
        gt[2, 2, 1] = gt[2, 2, 0]                                           # a void ground truth
        for keep, sep, k in itertools.product((3, wcap), (1, 3), (3, 64)):
            kw = dict(win=win, stride=stride, keep=keep, k=k, min_sep=sep, gt=gt, return_scores=True, return_bounds=True, return_order=True)
            yield "window_select/L%d/sep%d:keep%d/k%d" % (L, sep, keep, k), lambda s=s, m=m, kw=kw: tuple(ops.window_select(s, m, **kw))

    for (fn, fd), d in itertools.product(feats, (768, 100)):
        feat, q = rnd("tc_f%d" % d, 3, 70, d), rnd("tc_q%d" % d, d).cuda()
        feat[0, 5, 0] = INF                                                 # its column norm is inf: frame 5 of segment 0 scores inf * 0 = NaN, the others 0
        feat = feat.to(fd).cuda()
        for k in (0, 3, 64):
            yield "topk_cosine/%s/d%d:k%d" % (fn, d, k), lambda f=feat, q=q, k=k: ops.topk_cosine(f, q, k=k)
        video, text = rnd("tp_v%d" % d, 2, 70, d).to(fd).cuda(), rnd("tp_t%d" % d, 3, d).cuda()
        for k in (3, 64):
            yield "topk_pool/%s/d%d:k%d" % (fn, d, k), lambda v=video, t=text, k=k: ops.topk_pool(t, v, k, return_index=True)
        for tau in (0.01, 1.0):
            yield "attn_pool/%s/d%d:tau%g" % (fn, d, tau), lambda v=video, t=text, tau=tau: ops.attn_pool(t, v, tau)


def chain_cases():
    """The cases of the companion and the chain library (f32 rows only: no flavour)."""
    for L in (63, 257, 700):
        s, m = rows("ch%d" % L, L), masks(L)
        valid_m = (rnd("ch_vm%d" % L, 3, L, uniform=True) > 0.2).cuda()                # a validity row per mask row
        valid_r = (rnd("ch_vr%d" % L, 3, 3, L, uniform=True) > 0.2).cuda()             # a validity row per row
        win, stride = (16, 2) if L == 63 else (64, 4)
        gt = (rnd("ch_gt%d" % L, 3, 3, 1, uniform=True) * 0.8 * L + torch.tensor([0.0, 0.15 * L])).cuda()
        gt[2, 2, 1] = gt[2, 2, 0]                                           # a void ground truth
        outs = dict(gt=gt, return_scores=True, return_bounds=True, return_order=True)
        for keep, sep, k in itertools.product((3, 10 ** 6), (1, 3), (3, 64)):
            kw = dict(win=win, keep=keep, k=k, min_sep=sep, **outs)
            yield "window_select_clipped/L%d/sep%d:keep%d/k%d" % (L, sep, keep, k), lambda s=s, m=m, kw=kw: tuple(ops.window_select_clipped(s, m, **kw))
        for rule, frames, (vn, v) in itertools.product(("shifted", "clipped"), ("all", "sampled"), (("none", None), ("mask", valid_m))):
            kw = dict(rule=rule, win=win, stride=stride if rule == "shifted" else None, keep=3, frames=frames, num_frames=5 if frames == "sampled" else None, valid=v, **outs)
            yield "window_select_frames/L%d/%s:%s/valid-%s" % (L, rule, frames, vn), lambda s=s, m=m, kw=kw: tuple(ops.window_select_frames(s, m, **kw))

        spans = rnd("ch_spans%d" % L, 3, 3, 9, 2, uniform=True) * torch.tensor([1.0, 0.4])
        spans[:, :, :4] = torch.tensor([[0.5, -0.01], [NAN, 0.1], [0.5, INF], [1.5, 2.0]])      # empty, two non-finite, past the row
        spans = spans.cuda()
        xx = torch.stack([spans[..., 0] - 0.5 * spans[..., 1], spans[..., 0] + 0.5 * spans[..., 1]], -1)
        for (pooling, tau), k, skip in itertools.product((("topk", 0.01), ("attention", 0.01), ("attention", 1.0)), (1, 3, 64), (False, True)):
            kw = dict(k=k, pooling=pooling, temperature=tau, skip_nan=skip, return_windows=True, return_usable=True)
            for vn, v in (("none", None), ("mask", valid_m)):
                yield ("span_scores_masked/L%d/%s%g:k%d/skip%d/valid-%s" % (L, pooling, tau, k, skip, vn),
                       lambda s=s, m=m, v=v, kw=kw: tuple(ops.span_scores_masked(s, spans, m, valid=v, **kw)))
            yield ("span_scores_masked_rows/L%d/%s%g:k%d/skip%d" % (L, pooling, tau, k, skip),
                   lambda s=s, m=m, kw=kw: tuple(ops.span_scores_masked_rows(s, spans, m, valid=valid_r, **kw)))
        for smooth, gap, relative, skip in itertools.product((1, 5), (0, 2), (True, False), (False, True)):
            kw = dict(levels=[0.2 + 0.7 * i / 4 for i in range(5)], relative=relative, smooth=smooth, gap=gap, skip_nan=skip, max_spans=9, return_windows=True,
                      return_smoothed=True)
            tag = "smooth%d/gap%d/rel%d/skip%d" % (smooth, gap, relative, skip)
            for vn, v in (("none", None), ("mask", valid_m)):
                yield "span_propose_masked/L%d:%s/valid-%s" % (L, tag, vn), lambda s=s, m=m, v=v, kw=kw: tuple(ops.span_propose_masked(s, m, valid=v, **kw))
            yield "span_propose_masked_rows/L%d:%s" % (L, tag), lambda s=s, m=m, kw=kw: tuple(ops.span_propose_masked_rows(s, m, valid=valid_r, **kw))

        select = torch.tensor([0, 2, 2, -1, 5, 999], dtype=torch.int32).repeat(3, 3, 1)
        select[1, :, 0], select[2, 1] = 1, -1
        select = select.cuda()
        for rule, frames, (vn, v) in itertools.product(("shifted", "clipped"), ("all", "sampled"), (("none", None), ("mask", valid_m))):
            kw = dict(rule=rule, win=win, stride=stride if rule == "shifted" else None, frames=frames, num_frames=5 if frames == "sampled" else None, valid=v,
                      return_count=True)
            yield "windows_valid/L%d/%s:%s/valid-%s" % (L, rule, frames, vn), lambda m=m, kw=kw: tuple(ops.windows_valid(select, m, **kw))

        for form, (radius, margin), min_len, (vn, v) in itertools.product(("cxw", "xx"), ((3, 5), (64, 128)), (1, 4), (("none", None), ("mask", valid_m), ("rows", valid_r))):
            kw = dict(form=form, radius=radius, margin=margin, min_len=min_len, valid=v, return_windows=True, return_contrast=True)
            yield ("span_refine/L%d/%s:r%d/m%d/min%d/valid-%s" % (L, form, radius, margin, min_len, vn),
                   lambda s=s, m=m, sp=spans if form == "cxw" else xx, kw=kw: tuple(ops.span_refine(s, sp, m, **kw)))
        for score, peak, cap, (vn, v) in itertools.product(("mean", "contrast"), (0, 2), (4, 256), (("none", None), ("mask", valid_m), ("rows", valid_r))):
            kw = dict(scales=(8, (16, 4), (33, 5, 7)), score=score, peak=peak, max_spans=cap, valid=v, return_windows=True, return_scale=True)
            yield "span_anchors/L%d/%s:peak%d/cap%d/valid-%s" % (L, score, peak, cap, vn), lambda s=s, m=m, kw=kw: tuple(ops.span_anchors(s, m, **kw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grounding_digest.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "grounding_digest needs the GPU"
    res, calls = {}, 0
    for fl in ("f16", "bf16", "chain"):
        if fl != "chain":
            hip.set_flavour(fl)
        groups = {}
        for name, call in (chain_cases() if fl == "chain" else cases(hip.op_dtype(fl))):
            torch.empty = sentinel_empty
            try:
                out = call()
            finally:
                torch.empty = _empty
            h = groups.setdefault(name.split(":")[0], hashlib.sha256())
            h.update(name.encode() + b"\0" + output_bytes(out))
            calls += fl != "bf16"
        res[fl] = {g: h.hexdigest() for g, h in groups.items()}
    out = dict(abi=hip.lib("f16").rv_abi_version(), cases=calls, groups=len(res["f16"]) + len(res["chain"]), digests=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(dict(out=a.out, cases=out["cases"], groups=out["groups"], sha256_of_digests=hashlib.sha256(json.dumps(res, sort_keys=True).encode()).hexdigest())))


if __name__ == "__main__":
    main()
