"""Ranking scored proposals on the device (``eval.similarity.rank_proposals`` -> rv_span_rank: sort, greedy temporal NMS, top-M, IoU and first hits against a
ground truth in one launch) against the host route it replaces: the scores and proposals copied to the host, a torch-CPU sort and a per-row NMS loop.

R = 8 videos x Q queries rows (--queries), N proposals per row (--spans: 64 takes the one-wave-per-row form, 1024 the one-block-per-row form), top = 50,
nms_iou = 0.5, five thresholds.  All forms of a case run in one process, alternating, between device events (the host route between host clocks, its copies
included); warm-up + timed rounds per form; medians with min .. max.  Per case:

  rank_ms               one ``rank_proposals`` call, synchronised: enqueue + one kernel + the wait (a latency, host overhead included)
  rank_back_to_back_ms  per call over --reps un-synchronised calls: a throughput, bounded below by the host's enqueue cost per call (five output allocations)
  kernel_ms             rv_span_rank alone through the C entry into preallocated outputs, per call over --reps back-to-back calls (bounded below by the
                        launch rate when the kernel is shorter than a launch)
  host_copy_ms          ``.cpu()`` of the scores, the proposals and the ground truth (each waits for the device)
  host_rank_ms          torch-CPU stable sort of all rows + the NMS / IoU / first-hit loop (numpy float32, vectorised per pivot) over the first --host-rows
                        rows, scaled to R rows (``host_rows_timed`` says how many ran); its result is compared with the device's on those rows
  host_over_rank        (host_copy + host_rank) / rank: an END-TO-END ratio of host overheads, not a kernel comparison
Inputs: rows of (centre, width) proposals clustered as a proposal head makes them, random scores.

Writes one JSON object to --out (default profiles/similarity_rank.json) and prints it.

    python tools/similarity_rank_prof.py [--queries 16,64,256] [--spans 64,1024] [--top 50] [--warmup 2] [--iters 5] [--reps 128] [--host-rows 64] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HITS = (0.1, 0.3, 0.5, 0.7, 0.9)


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


def host_loop(order, spans, gt, top, nms, rows):
    """The host route behind its sort (``order``: the stable descending argsort of every row), on CPU tensors: per row (the first ``rows``) greedy NMS with
    the later proposals tested in one numpy float32 expression per pivot, IoU with the ground truth and first hits.
    -> (keep [rows, top], first_hit [rows, T]).  A timing stand-in for what a caller would write, not another statement of the rule: it has no notion
    of void spans and NaN scores (tests/rank_oracle.py is the definition) and refuses inputs that hold any."""
    order, sp, g = order.numpy(), spans.numpy(), gt.numpy()
    half = np.float32(0.5) * sp[..., 1]
    s_all, e_all = sp[..., 0] - half, sp[..., 0] + half
    assert np.isfinite(s_all).all() and np.isfinite(e_all).all() and (e_all > s_all).all() and np.isfinite(g).all() and (g[:, 1] > g[:, 0]).all(), \
        "host_loop: void spans are not handled"
    keep = np.full((rows, top), -1, dtype=np.int32)
    first = np.full((rows, len(HITS)), -1, dtype=np.int32)
    nms = np.float32(nms)
    for r in range(rows):
        o = order[r]
        s, e = s_all[r][o], e_all[r][o]
        live = np.ones(len(o), dtype=bool)
        kept = []
        for p in range(len(o)):
            if not live[p]:
                continue
            kept.append(p)
            if len(kept) == top:
                break
            inter = np.maximum(np.minimum(e[p], e[p + 1:]) - np.maximum(s[p], s[p + 1:]), np.float32(0))
            union = ((e[p] - s[p]) + (e[p + 1:] - s[p + 1:])) - inter
            live[p + 1:] &= ~(inter > nms * union)
        k = np.array(kept)
        keep[r, :len(k)] = o[k]
        inter = np.maximum(np.minimum(e[k], g[r, 1]) - np.maximum(s[k], g[r, 0]), np.float32(0))
        union = ((e[k] - s[k]) + (g[r, 1] - g[r, 0])) - inter
        iou = np.where(union > 0, inter / union, np.float32(0))
        for t, m in enumerate(HITS):
            hit = np.nonzero(iou > np.float32(m))[0]
            if len(hit):
                first[r, t] = hit[0]
    return keep, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--queries", default="16,64,256")
    ap.add_argument("--spans", default="64,1024")
    ap.add_argument("--top", type=int, default=50)
    ap.add_argument("--nms-iou", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=128, help="back-to-back calls per timed window of the back-to-back forms")
    ap.add_argument("--host-rows", type=int, default=64, help="rows the host loop runs over per round (scaled to all rows)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_rank.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from revisionllm_amd import hip
    from revisionllm_amd.eval import similarity as S
    assert torch.cuda.is_available(), "similarity_rank_prof needs the GPU: a CPU run says nothing about time"
    B, top, nms = a.videos, a.top, a.nms_iou
    lib = hip.lib()
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), videos=B, top=top, nms_iou=nms, thresholds=list(HITS), warmup=a.warmup,
               iters=a.iters, reps=a.reps, cases={})
    g = torch.Generator().manual_seed(0)
    hit = torch.tensor(HITS).cuda()
    for N in (int(n) for n in a.spans.split(",")):
        for Q in (int(q) for q in a.queries.split(",")):
            R = B * Q
            scores = torch.randn(B, Q, N, generator=g).cuda()
            width = torch.tensor([0.03, 0.06, 0.12, 0.25, 0.5])[torch.randint(0, 5, (B, Q, N), generator=g)] * (0.9 + 0.2 * torch.rand(B, Q, N, generator=g))
            spans = torch.stack([0.05 + 0.9 * torch.rand(B, Q, N, generator=g), width], dim=-1).cuda()
            gt = torch.sort(torch.rand(B, Q, 2, generator=g), dim=-1).values.cuda()
            m = min(top, N)
            keep, n_keep = torch.empty(R, m, dtype=torch.int32, device="cuda"), torch.empty(R, dtype=torch.int32, device="cuda")
            keep_iou, first = torch.empty(R, m, device="cuda"), torch.empty(R, len(HITS), dtype=torch.int32, device="cuda")

            def kernel(_):
                hip.check(lib.rv_span_rank(hip.ptr(scores), hip.ptr(spans), 1, R, N, m, nms, hip.ptr(gt), hip.ptr(hit), len(HITS), None, hip.ptr(keep),
                                           hip.ptr(n_keep), hip.ptr(keep_iou), hip.ptr(first), hip.stream()), "rv_span_rank")

            def rank(_):
                return S.rank_proposals(scores, spans, top=top, nms_iou=nms, gt=gt)

            rows = min(a.host_rows, R)
            t = dict(rank=[], rank_back_to_back=[], kernel=[], host_copy=[], host_rank=[])
            for i in range(a.warmup + a.iters):
                s = dict(rank=timed(rank), rank_back_to_back=timed(rank, a.reps), kernel=timed(kernel, a.reps))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hs, hp, hg = scores.cpu(), spans.cpu(), gt.cpu()
                t1 = time.perf_counter()
                order = torch.sort(hs.reshape(R, N), dim=-1, descending=True, stable=True).indices
                t2 = time.perf_counter()
                hk, hf = host_loop(order, hp.reshape(R, N, 2), hg.reshape(R, 2), m, nms, rows)
                t3 = time.perf_counter()
                s.update(host_copy=t1 - t0, host_rank=(t2 - t1) + (t3 - t2) * R / rows)      # (the sort ran over every row; the loop's share scales)
                if i >= a.warmup:
                    for k in t:
                        t[k].append(s[k])
            out = rank(0)
            med = {k: statistics.median(v) for k, v in t.items()}
            r = {k + "_ms": spread(v) for k, v in t.items()}
            r.update(rows=R, proposals=N, kept_per_row_mean=float(out.n_keep.float().mean()), form="wave" if N <= 64 else "block", host_rows_timed=rows,
                     host_agrees_on_timed_rows=bool(np.array_equal(out.keep.reshape(R, m)[:rows].cpu().numpy(), hk)
                                                    and np.array_equal(out.first_hit.reshape(R, -1)[:rows].cpu().numpy(), hf)),
                     host_over_rank=(med["host_copy"] + med["host_rank"]) / med["rank"],
                     host_over_rank_back_to_back=(med["host_copy"] + med["host_rank"]) / med["rank_back_to_back"],
                     kernel_us_per_row=med["kernel"] * 1e6 / R)
            res["cases"][f"N{N}_R{R}"] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
