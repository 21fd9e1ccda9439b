"""Window selection on the device (``ops.window_select`` -> rv_window_select: duration, every window of cut_windows' geometry scored by its top-k
cosines, rank order, greedy selection with a minimum separation, top up, the first ``keep`` ascending, the ground truth's first place - one launch)
against the route composed from the entries that were there before it and against the host route.

8 videos x Q queries (--queries) x L frames (--frames), cosine rows of random features with a stretch raised towards each query's text, win = 625,
stride = 5, keep = 100, min_sep = 1 and 3, a ground truth per row.  All forms of a case run in one process, alternating, between device events (the
host route between host clocks, its copy included); warm-up + timed rounds per form; medians with min .. max.  Per case:

  kernel_ms             rv_window_select alone through the C entry into preallocated outputs (select, counts, hit_rank), per call over --reps back-to-back
                        calls; kernel_sep3_ms the same with min_sep = 3 (the greedy walk runs over every window, since hit_rank wants the whole sequence)
  select_ms             one ``ops.window_select`` call with gt, synchronised: enqueue + one kernel + the wait (a latency, host overhead included)
  composed_ms           the same selection at min_sep = 1 from the existing entries, synchronised once: the windows encoded as (centre, width) spans in
                        torch, ``ops.span_scores_multi``, ``ops.span_rank`` (top = keep, no NMS), a torch sort of the kept indices; no hit_rank (span_rank's
                        hits are IoU thresholds, another quantity); its select is compared with the kernel's
  host_copy_ms          ``.cpu()`` of the cosine rows (waits for the device)
  host_select_ms        tests/window_oracle.py (numpy float32, Python loops) over the first --host-rows rows, scaled to all rows
  kernel_gb_per_s       (rows + mask rows) * L * 4 bytes over kernel_ms: the bytes that come from memory once (each frame is then read again from cache
                        by the `stride` windows that hold it, k times)
and one line for the longest greedy walk: 8 rows, L = 2049, win = stride = 2 (2048 windows), keep = 2048, min_sep = 2.

Writes one JSON object to --out (default profiles/similarity_windows.json) and prints it.

    python tools/similarity_window_prof.py [--queries 1,16,64] [--frames 18000,36000] [--warmup 2] [--iters 5] [--reps 32] [--host-rows 2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
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
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--win", type=int, default=625)
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--keep", type=int, default=100)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=32, help="back-to-back calls per timed window of the kernel forms")
    ap.add_argument("--host-rows", type=int, default=2, help="rows the host oracle runs over per round (scaled to all rows)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_windows.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import window_oracle as WO
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval.metrics import window_recall
    assert torch.cuda.is_available(), "similarity_window_prof needs the GPU: a CPU run says nothing about time"
    B, d, win, stride, keep, k = a.videos, a.dim, a.win, a.stride, a.keep, a.k
    lib = hip.lib()
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), videos=B, dim=d, win=win, stride=stride, keep=keep, k=k, warmup=a.warmup,
               iters=a.iters, reps=a.reps, cases={})
    g = torch.Generator(device=dev).manual_seed(0)

    def entry(flat, mask, R, rpm, L, win_, stride_, k_, keep_, min_sep, Wcap, gt, out):
        hip.check(lib.rv_window_select(hip.ptr(flat), hip.ptr(mask), R, rpm, L, win_, stride_, k_, keep_, min_sep, Wcap, hip.ptr(gt), hip.ptr(out["select"]),
                                       hip.ptr(out["n_select"]), hip.ptr(out["n_windows"]), None, None, hip.ptr(out.get("order")),
                                       hip.ptr(out.get("hit_rank")), hip.stream()), "rv_window_select")

    for L in (int(x) for x in a.frames.split(",")):
        video = torch.randn(B, L, d, generator=g, device=dev)
        mask = torch.ones(B, L, device=dev)
        Wcap = WO.capacity(L, win, stride)
        for Q in (int(q) for q in a.queries.split(",")):
            R = B * Q
            text = torch.randn(B, Q, d, generator=g, device=dev)
            v = video.clone()
            for b in range(B):
                for q in range(min(Q, 8)):                                        # a raised stretch for the first queries of each video
                    lo = (997 * (q + 1) + 131 * b) % (L - 400)
                    v[b, lo:lo + 120 + 30 * q] += 0.6 * text[b, q]
            sims = ops.frame_cosine_multi(text, v.to(hip.op_dtype()))
            del v
            flat = sims.view(R, L)
            gt = torch.stack([torch.arange(R, device=dev) * 37.0 % (L - 300), torch.arange(R, device=dev) * 37.0 % (L - 300) + 250.0], dim=1).contiguous()
            i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)                    # noqa: E731
            outs = dict(select=i32(R, keep), n_select=i32(R), n_windows=i32(R), hit_rank=i32(R))

            def kernel(_, sep=1):
                entry(flat, mask, R, Q, L, win, stride, k, keep, sep, Wcap, gt, outs)

            def select(_, sep=1):
                return ops.window_select(sims, mask, win=win, stride=stride, keep=keep, k=k, min_sep=sep, gt=gt.view(B, Q, 2))

            def composed(_):
                i = torch.arange(Wcap, device=dev, dtype=torch.int64)
                s = i * win // stride
                e = torch.clamp(s + win, max=L - 1)
                s = torch.where(e - s < win, e - win, s).clamp(min=0)
                lo, hi = s.float(), (e + 1).float()
                spans = torch.stack([((lo + hi) * 0.5) / L, ((hi - lo) - 0.5) / L], dim=-1).expand(B, Q, Wcap, 2).contiguous()
                scores = ops.span_scores_multi(sims, spans, mask, k=k)
                return torch.sort(ops.span_rank(scores, spans, top=keep, nms_iou=1.0).keep, dim=-1).values

            rows = min(a.host_rows, R)
            t = dict(kernel=[], kernel_sep3=[], select=[], select_sep3=[], composed=[], host_copy=[], host_select=[])
            for it in range(a.warmup + a.iters):
                s = dict(kernel=timed(kernel, a.reps), kernel_sep3=timed(lambda j: kernel(j, 3), a.reps), select=timed(select),
                         select_sep3=timed(lambda j: select(j, 3)), composed=timed(composed))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hs = flat.cpu()
                t1 = time.perf_counter()
                ref = WO.select(hs[:rows].numpy(), np.ones((rows, L), dtype=np.float32), win, stride, k, keep, 1, gt=gt[:rows].cpu().numpy())
                t2 = time.perf_counter()
                s.update(host_copy=t1 - t0, host_select=(t2 - t1) * R / rows)
                if it >= a.warmup:
                    for name in t:
                        t[name].append(s[name])
            out = select(0)
            med = {name: statistics.median(x) for name, x in t.items()}
            r = {name + "_ms": spread(x) for name, x in t.items()}
            r.update(rows=R, queries=Q, frames=L, windows=int(out.n_windows.max()), host_rows_timed=rows,
                     host_agrees_on_timed_rows=bool(np.array_equal(out.select.view(R, keep)[:rows].cpu().numpy(), ref["select"])
                                                    and np.array_equal(out.hit_rank.view(R)[:rows].cpu().numpy(), ref["hit_rank"])),
                     composed_agrees=bool(torch.equal(composed(0), out.select)),
                     recall=dict(zip(("R@1", "R@5", "R@10", "R@50", "R@100"), window_recall(out.hit_rank))),
                     composed_over_select=med["composed"] / med["select"], host_over_select=(med["host_copy"] + med["host_select"]) / med["select"],
                     kernel_us_per_row=med["kernel"] * 1e6 / R, memory_mb=(R + B) * L * 4 / 1e6, kernel_gb_per_s=(R + B) * L * 4 / med["kernel"] / 1e9)
            res["cases"][f"L{L}_Q{Q}_R{R}"] = r
        del video
    # the longest greedy walk: every second window is taken in pass 1, one barrier each, then pass 2
    L, R = 2049, 8
    flat = torch.randn(R, L, generator=g, device=dev)
    mask = torch.ones(R, L, device=dev)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)                            # noqa: E731
    outs = dict(select=i32(R, 2048), n_select=i32(R), n_windows=i32(R), order=i32(R, 2048))
    walk = [timed(lambda j: entry(flat, mask, R, 1, L, 2, 2, 2, 2048, 2, 2048, None, outs), 8) for _ in range(a.warmup + a.iters)][a.warmup:]
    rank = [timed(lambda j: entry(flat, mask, R, 1, L, 2, 2, 2, 2048, 1, 2048, None, outs), 8) for _ in range(a.warmup + a.iters)][a.warmup:]
    res["longest_walk"] = dict(rows=R, frames=L, windows=2048, keep=2048, min_sep2_ms=spread(walk), min_sep1_ms=spread(rank))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
