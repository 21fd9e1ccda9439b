"""Span proposals on the device (``eval.similarity.propose_spans`` -> rv_span_propose: duration, smoothing, thresholds at T levels, runs with gaps closed,
filter, duplicates, (centre, width) spans in one launch) and the grounder built on it (``ground_queries``: cosine rows, proposals, span scores, ranking)
against the host route the proposal stage replaces: the cosine rows copied to the host and a Python loop per row.

8 videos x Q queries (--queries) x L = 8192 frames of 768 features in the build's 16-bit type, T = 5 levels, smooth = 5, gap = 2, at most 256 spans per
row.  All forms of a case run in one process, alternating, between device events (the host route between host clocks, its copy included); warm-up + timed
rounds per form; medians with min .. max.  Per case:

  kernel_ms             rv_span_propose alone through the C entry into preallocated outputs, per call over --reps back-to-back calls
  propose_ms            one ``propose_spans`` call, synchronised: enqueue + one kernel + the wait (a latency, host overhead included)
  ground_ms             one ``ground_queries`` call, synchronised (four stages and the gather of the kept spans)
  stages_ms             the same four stages called one by one through ``ops`` and synchronised once at the end, no gather
  host_copy_ms          ``.cpu()`` of the cosine rows (waits for the device)
  host_propose_ms       tests/propose_oracle.py (numpy float32, a Python loop per row) over the first --host-rows rows, scaled to all rows; its windows are
                        compared with the device's on those rows
  host_over_propose     (host_copy + host_propose) / propose: an END-TO-END ratio that is mostly interpreter overhead, not a kernel comparison
Inputs: random features with a stretch raised towards each query's text, so the rows look like cosine rows with a peak.

Writes one JSON object to --out (default profiles/similarity_propose.json) and prints it.

    python tools/similarity_propose_prof.py [--queries 1,16,64] [--frames 8192] [--warmup 2] [--iters 5] [--reps 64] [--host-rows 4] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (0.5, 0.6, 0.7, 0.8, 0.9)


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
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--smooth", type=int, default=5)
    ap.add_argument("--gap", type=int, default=2)
    ap.add_argument("--max-spans", type=int, default=256)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=64, help="back-to-back calls per timed window of the kernel form")
    ap.add_argument("--host-rows", type=int, default=4, help="rows the host oracle runs over per round (scaled to all rows)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_propose.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import propose_oracle as P
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval import similarity as S
    assert torch.cuda.is_available(), "similarity_propose_prof needs the GPU: a CPU run says nothing about time"
    B, L, d, N = a.videos, a.frames, a.dim, a.max_spans
    lib = hip.lib()
    kw = dict(levels=LEVELS, smooth=a.smooth, gap=a.gap, max_spans=N)
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), videos=B, frames=L, dim=d, levels=list(LEVELS), smooth=a.smooth, gap=a.gap,
               max_spans=N, top=a.top, warmup=a.warmup, iters=a.iters, reps=a.reps, cases={})
    g = torch.Generator().manual_seed(0)
    video = torch.randn(B, L, d, generator=g)
    mask = torch.ones(B, L).cuda()
    table = (ctypes.c_float * len(LEVELS))(*LEVELS)
    for Q in (int(q) for q in a.queries.split(",")):
        R = B * Q
        text = torch.randn(B, Q, d, generator=g)
        v = video.clone()
        for b in range(B):
            for q in range(min(Q, 8)):                                            # a raised stretch for the first queries of each video
                lo = (997 * (q + 1) + 131 * b) % (L - 400)
                v[b, lo:lo + 120 + 30 * q] += 0.6 * text[b, q]
        v = v.to(hip.op_dtype()).cuda()
        text = text.cuda()
        sims = ops.frame_cosine_multi(text, v)
        flat = sims.view(R, L)
        spans, n_spans, n_found = torch.empty(R, N, 2, device="cuda"), torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, dtype=torch.int32, device="cuda")

        def kernel(_):
            hip.check(lib.rv_span_propose(hip.ptr(flat), hip.ptr(mask), R, Q, L, table, len(LEVELS), 1, a.smooth, a.gap, 1, 0, N, hip.ptr(spans), hip.ptr(n_spans),
                                          hip.ptr(n_found), None, None, hip.stream()), "rv_span_propose")

        def propose(_):
            return S.propose_spans(sims, mask, return_windows=True, **kw)

        def ground(_):
            return S.ground_queries(text, v, mask, top=a.top, **kw)

        def stages(_):
            s = ops.frame_cosine_multi(text, v)
            p = ops.span_propose(s, mask, **kw)
            sc = ops.span_scores_multi(s, p.spans, mask)
            return ops.span_rank(sc, p.spans, top=a.top, nms_iou=0.5)

        rows = min(a.host_rows, R)
        t = dict(kernel=[], propose=[], ground=[], stages=[], host_copy=[], host_propose=[])
        for i in range(a.warmup + a.iters):
            s = dict(kernel=timed(kernel, a.reps), propose=timed(propose), ground=timed(ground), stages=timed(stages))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hs = flat.cpu()
            t1 = time.perf_counter()
            ref = P.propose(hs[:rows].numpy(), np.ones((rows, L), dtype=np.float32), LEVELS, 1, a.smooth, a.gap, 1, 0, N)
            t2 = time.perf_counter()
            s.update(host_copy=t1 - t0, host_propose=(t2 - t1) * R / rows)
            if i >= a.warmup:
                for k in t:
                    t[k].append(s[k])
        out = propose(0)
        med = {k: statistics.median(x) for k, x in t.items()}
        r = {k + "_ms": spread(x) for k, x in t.items()}
        r.update(rows=R, queries=Q, found_per_row_mean=float(out.n_found.float().mean()), found_per_row_max=int(out.n_found.max()), host_rows_timed=rows,
                 host_agrees_on_timed_rows=bool(np.array_equal(out.windows.view(R, N, 2)[:rows].cpu().numpy(), ref["windows"])),
                 host_over_propose=(med["host_copy"] + med["host_propose"]) / med["propose"], ground_over_stages=med["ground"] / med["stages"],
                 kernel_us_per_row=med["kernel"] * 1e6 / R, row_bytes_mb=R * L * 4 / 1e6, kernel_gb_per_s=R * L * 4 / med["kernel"] / 1e9)
        res["cases"][f"Q{Q}_R{R}"] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
