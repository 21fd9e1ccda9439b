"""The stage-1 window pre-filter on the device (``ops.window_select_clipped`` -> rvx_window_select_clipped of the companion library: duration, every
non-void window of stage1.cut_windows' geometry scored by its top-k cosines, rank order, selection, the first ``keep`` ascending - one launch) against
the same selection composed from the entries that were there before it, against ``rv_window_select`` at stride 2 on the same rows (the same kernel
source under the other window rule) and inside ``stage1.clip_stage_windows``.

8 videos x Q queries (--queries) x L frames (--frames), cosine rows of random features with a stretch raised towards each query's text, win = 625,
keep = 8 / 16 / 32 (--keeps), min_sep = 1, a ground truth per row.  All forms of a case run in one process, alternating, between device events;
warm-up + timed rounds per form; medians with min .. max.  Per case:

  kernel_ms             rvx_window_select_clipped alone through the C entry into preallocated outputs (select, counts, hit_rank), per call over --reps
                        back-to-back calls
  shifted_kernel_ms     rv_window_select at stride = 2 on the same rows and outputs, the same way (the shifted rule: its last windows are full ones)
  select_ms             one ``ops.window_select_clipped`` call with gt, synchronised: enqueue + one kernel + the wait (a latency, host overhead included)
  composed_ms           the same selection from the existing entries, synchronised once: the clipped windows encoded as (centre, width) spans in torch,
                        ``ops.span_scores_multi``, ``ops.span_rank`` (top = keep, no NMS), a torch sort of the kept indices; its select is compared with
                        the kernel's
  clip_stage_ms         one ``stage1.clip_stage_windows`` call on the first video and its first query (cosine row, selection, gather of ``keep`` windows
                        of 250 frames, the ``.tolist()``), between host clocks; once per (L, keep), repeated under every Q
No ratio is fixed in advance: the file holds what was measured, ``not_ahead`` lists every case in which select_ms is not below composed_ms or
kernel_ms not below shifted_kernel_ms.  The driver end to end on real features is not measured here.

Writes one JSON object to --out (default profiles/stage1_prefilter.json) and prints it.

    python tools/stage1_prefilter_prof.py [--queries 1,16,64] [--frames 18000,36000] [--keeps 8,16,32] [--warmup 2] [--iters 5] [--reps 32] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, reps=1):
    """Seconds per call over ``reps`` back-to-back calls between two device events; the second event is waited for."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def spread(v):
    return dict(median=statistics.median(v) * 1e3, min=min(v) * 1e3, max=max(v) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--queries", default="1,16,64")
    ap.add_argument("--frames", default="18000,36000")
    ap.add_argument("--keeps", default="8,16,32")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--win", type=int, default=625)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=32, help="back-to-back calls per timed window of the kernel forms")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage1_prefilter.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval import stage1
    assert torch.cuda.is_available(), "stage1_prefilter_prof needs the GPU: a CPU run says nothing about time"
    B, d, win, k = a.videos, a.dim, a.win, a.k
    lib, ext = hip.lib(), hip.ext_lib()
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), videos=B, dim=d, win=win, k=k, min_sep=1, warmup=a.warmup, iters=a.iters,
               reps=a.reps, cases={}, not_ahead=[])
    g = torch.Generator(device=dev).manual_seed(0)

    for L in (int(x) for x in a.frames.split(",")):
        video = torch.randn(B, L, d, generator=g, device=dev)
        mask = torch.ones(B, L, device=dev)
        Wcap = ops.window_select_capacity("prof", L, win, 2)
        W = ops.clipped_window_solid(L, win)
        for Q in (int(q) for q in a.queries.split(",")):
            R = B * Q
            text = torch.randn(B, Q, d, generator=g, device=dev)
            v = video.clone()
            for b in range(B):
                for q in range(min(Q, 8)):                                        # a raised stretch for the first queries of each video
                    lo = (997 * (q + 1) + 131 * b) % (L - 400)
                    v[b, lo:lo + 120 + 30 * q] += 0.6 * text[b, q]
            v16 = v.to(hip.op_dtype())
            del v
            sims = ops.frame_cosine_multi(text, v16)
            flat = sims.view(R, L)
            gt = torch.stack([torch.arange(R, device=dev) * 37.0 % (L - 300), torch.arange(R, device=dev) * 37.0 % (L - 300) + 250.0], dim=1).contiguous()
            i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)                    # noqa: E731
            for keep in (int(x) for x in a.keeps.split(",")):
                outs = dict(select=i32(R, keep), n_select=i32(R), n_windows=i32(R), hit_rank=i32(R))

                def kernel(_):
                    hip.ext_check(ext.rvx_window_select_clipped(hip.ptr(flat), hip.ptr(mask), R, Q, L, win, k, keep, 1, Wcap, hip.ptr(gt), hip.ptr(outs["select"]),
                                                                hip.ptr(outs["n_select"]), hip.ptr(outs["n_windows"]), None, None, None, hip.ptr(outs["hit_rank"]),
                                                                hip.stream()), "rvx_window_select_clipped")

                def shifted(_):
                    hip.check(lib.rv_window_select(hip.ptr(flat), hip.ptr(mask), R, Q, L, win, 2, k, keep, 1, Wcap, hip.ptr(gt), hip.ptr(outs["select"]),
                                                   hip.ptr(outs["n_select"]), hip.ptr(outs["n_windows"]), None, None, None, hip.ptr(outs["hit_rank"]),
                                                   hip.stream()), "rv_window_select")

                def select(_):
                    return ops.window_select_clipped(sims, mask, win=win, keep=keep, k=k, gt=gt.view(B, Q, 2))

                def composed(_):
                    i = torch.arange(W, device=dev, dtype=torch.int64)
                    s = i * win // 2
                    e = torch.clamp(s + win, max=L - 1)
                    lo, hi = s.float(), (e + 1).float()
                    spans = torch.stack([((lo + hi) * 0.5) / L, ((hi - lo) - 0.5) / L], dim=-1).expand(B, Q, W, 2).contiguous()
                    scores = ops.span_scores_multi(sims, spans, mask, k=k)
                    return torch.sort(ops.span_rank(scores, spans, top=keep, nms_iou=1.0).keep, dim=-1).values

                def clip_stage():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    windows, tensor = stage1.clip_stage_windows(v16[0], text[0, 0], debug_window=win // 5, feature_fps=5, keep=keep, k=k)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0

                t = dict(kernel=[], shifted_kernel=[], select=[], composed=[], clip_stage=[])
                for it in range(a.warmup + a.iters):
                    s = dict(kernel=timed(kernel, a.reps), shifted_kernel=timed(shifted, a.reps), select=timed(select), composed=timed(composed),
                             clip_stage=clip_stage())
                    if it >= a.warmup:
                        for name in t:
                            t[name].append(s[name])
                out = select(0)
                med = {name: statistics.median(x) for name, x in t.items()}
                r = {name + "_ms": spread(x) for name, x in t.items()}
                r.update(rows=R, queries=Q, frames=L, keep=keep, windows=int(out.n_windows.max()), composed_agrees=bool(torch.equal(composed(0), out.select)),
                         composed_over_select=med["composed"] / med["select"], shifted_over_clipped_kernel=med["shifted_kernel"] / med["kernel"],
                         kernel_us_per_row=med["kernel"] * 1e6 / R, kernel_gb_per_s=(R + B) * L * 4 / med["kernel"] / 1e9)
                name = f"L{L}_Q{Q}_keep{keep}"
                res["cases"][name] = r
                if not med["select"] < med["composed"]:
                    res["not_ahead"].append(name + ": select_ms >= composed_ms")
                if not med["kernel"] < med["shifted_kernel"]:
                    res["not_ahead"].append(name + ": kernel_ms >= shifted_kernel_ms")
        del video
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
