"""The sliding-window generator (``rvc_span_anchors`` behind ``ops.span_anchors`` and ``ground_queries_anchored``) timed at the sizes the drivers run:
there is no parent kernel to compare with, so what is written down is what the kernel and the calls around it take, what bounds that, and the only
route a user had before - the cosine rows copied to the host and a Python loop.

8 videos x Q queries (--queries) x L frames (--frames) of 768 features in the build's 16-bit type; five scales of 25 to 400 frames with the default
strides (len // 4) and margins (len // 2), contrast scores, peak = 2, at most 256 spans per row.  The forms of a case alternate in one process between
device events; warm-up + timed rounds per form; medians with min .. max.  Per case:

  anchors_kernel_ms    rvc_span_anchors alone through the C entry into preallocated outputs and workspace, per call over --reps back-to-back calls
  span_anchors_ms      one ``ops.span_anchors`` call on resident cosine rows, synchronised (a latency, host overhead and allocations included)
  anchored_ms          one ``ground_queries_anchored`` call, synchronised: cosine rows, anchors, ranking
  thresholds_ms        one ``ground_queries`` call on the same tensors, synchronised: cosine rows, threshold proposals, span scores, ranking
  host_route_ms        ``sims.cpu()`` once plus the numpy statement of the rule (tests/span_anchors_oracle.py) on --host-rows rows, scaled to all rows
  host_over_span_anchors   the END-TO-END ratio of host_route_ms and span_anchors_ms as it comes out: a Python loop against a device call, not a
                       kernel comparison; nothing is gated on it
  bytes_compulsory     sims and mask read once, the outputs written once
  bytes_workspace      the prefix pairs and the two key arrays written once and read once (the least the three passes move through L2 / HBM)
  kernel_GBps          (bytes_compulsory + bytes_workspace) over anchors_kernel_ms
  same_as_host         the device call's windows, scores and counts equal the numpy statement's on the host rows, bit for bit (outside the timed rounds)
Inputs: random features with a stretch raised towards each query's text, so the rows look like cosine rows with a peak.

Writes one JSON object to --out (default profiles/similarity_anchors.json) and prints it.

    python tools/similarity_anchor_prof.py [--queries 1,16,64] [--frames 18000,36000] [--warmup 2] [--iters 5] [--reps 32] [--out FILE]"""
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
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--scales", default="25,50,100,200,400")
    ap.add_argument("--peak", type=int, default=2)
    ap.add_argument("--max-spans", type=int, default=256)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=32, help="back-to-back calls per timed window of the kernel form")
    ap.add_argument("--host-rows", type=int, default=2, help="rows the host route is run on (its time is scaled to all rows)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_anchors.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import span_anchors_oracle as AO
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval import similarity as S
    assert torch.cuda.is_available(), "similarity_anchor_prof needs the GPU: a CPU run says nothing about time"
    B, d, N = a.videos, a.dim, a.max_spans
    scales = tuple(int(x) for x in a.scales.split(","))
    table = ops.span_anchors_keywords("similarity_anchor_prof", scales)[0]
    flat = (ctypes.c_int32 * (3 * len(table)))(*(v for t in table for v in t))
    chain = hip.chain_lib()
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), videos=B, dim=d, scales=[list(t) for t in table], score="contrast", peak=a.peak,
               max_spans=N, top=a.top, warmup=a.warmup, iters=a.iters, reps=a.reps, host_rows=a.host_rows, cases={})
    g = torch.Generator().manual_seed(0)
    for L in (int(x) for x in a.frames.split(",")):
        video = torch.randn(B, L, d, generator=g)
        mask = torch.ones(B, L).cuda()
        anchors_per_row = sum(len(AO.anchor_starts(L, ln, st)) for ln, st, _ in table)
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
            nbytes = chain.rvc_span_anchors_workspace(L, flat, len(table), R)
            work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            o_spans, o_scores = torch.empty(R, N, 2, device="cuda"), torch.empty(R, N, device="cuda")
            o_n, o_found = torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, dtype=torch.int32, device="cuda")

            def kernel(_):
                hip.chain_check(chain.rvc_span_anchors(hip.ptr(sims), hip.ptr(mask), None, Q, R, Q, L, flat, len(table), hip.RVC_ANCHORS_CONTRAST, a.peak, 1, N,
                                                       hip.ptr(o_spans), hip.ptr(o_scores), hip.ptr(o_n), hip.ptr(o_found), None, None, hip.ptr(work), nbytes,
                                                       hip.stream()), "rvc_span_anchors")

            def span_anchors(_):
                return ops.span_anchors(sims, mask, scales=scales, peak=a.peak, max_spans=N)

            def anchored(_):
                return S.ground_queries_anchored(text, v, mask, scales=scales, peak=a.peak, max_spans=N, top=a.top)

            def thresholds(_):
                return S.ground_queries(text, v, mask, max_spans=N, top=a.top)

            def host_route():
                t0 = time.perf_counter()
                rows = sims.cpu().numpy().reshape(R, L)
                t1 = time.perf_counter()
                out = AO.anchors(rows[:a.host_rows], np.ones((a.host_rows, L), dtype=np.float32), None, 1, table, AO.CONTRAST, a.peak, 1, N)
                t2 = time.perf_counter()
                return (t1 - t0) + (t2 - t1) * R / a.host_rows, out

            dev = ops.span_anchors(sims, mask, scales=scales, peak=a.peak, max_spans=N, return_windows=True)
            _, host = host_route()
            n = a.host_rows
            same = (np.array_equal(dev.windows.view(R, N, 2)[:n].cpu().numpy(), host["windows"]) and np.array_equal(dev.n_found.view(R)[:n].cpu().numpy(), host["n_found"])
                    and np.array_equal(dev.scores.view(R, N)[:n].cpu().numpy().view(np.uint32), host["scores"].view(np.uint32)))
            assert same, f"L={L} Q={Q}: the device call and the numpy statement differ"
            forms = dict(anchors_kernel=(kernel, a.reps), span_anchors=(span_anchors, 1), anchored=(anchored, 1), thresholds=(thresholds, 1))
            t = {k: [] for k in forms}
            t["host_route"] = []
            for i in range(a.warmup + a.iters):
                s = {k: timed(fn, reps) for k, (fn, reps) in forms.items()}            # the forms alternate inside every round
                s["host_route"] = host_route()[0]
                if i >= a.warmup:
                    for k in t:
                        t[k].append(s[k])
            med = {k: statistics.median(x) for k, x in t.items()}
            r = {k + "_ms": spread(x) for k, x in t.items()}
            compulsory = R * L * 4 + B * L * 4 + R * N * 12 + R * 8
            workspace = R * ((L + 1) * 16 + anchors_per_row * 16) * 2
            r.update(rows=R, queries=Q, frames=L, anchors_per_row=anchors_per_row, peaks_mean=float(dev.n_found.float().mean()), peaks_max=int(dev.n_found.max()),
                     rows_cut=int((dev.n_found > N).sum()), same_as_host=same, bytes_compulsory=compulsory, bytes_workspace=workspace,
                     kernel_GBps=(compulsory + workspace) / med["anchors_kernel"] * 1e-9, host_over_span_anchors=med["host_route"] / med["span_anchors"],
                     anchored_over_thresholds=med["anchored"] / med["thresholds"])
            res["cases"][f"L{L}_Q{Q}_R{R}"] = r
            del v, work
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
