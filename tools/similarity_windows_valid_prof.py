"""The coarse-to-fine grounder (``ground_queries_in_windows``: one pass over the features, a validity row per query from ``rvc_windows_valid``, the
``_rows`` span entries) next to the only route the parent commit offers to the same spans: ``select_windows_frames`` for all queries, then per query a
torch-built [B, L] validity row and one ``ground_queries_masked`` call - Q calls, each of which reads the features again.

8 videos x Q queries (--queries) x L frames (--frames) of 768 features in the build's 16-bit type; windows of 625 frames at stride 5 (the stage-2
driver's geometry), the best 20 kept per query; T = 5 levels, smooth = 5, gap = 2, at most 256 spans per row.  The forms of a case alternate in one
process between device events; warm-up + timed rounds per form; medians with min .. max.  Per case:

  windows_valid_ms     rvc_windows_valid alone through the C entry into preallocated outputs, per call over --reps back-to-back calls
  in_windows_ms        one ``ground_queries_in_windows(keep=20)`` call, synchronised (a latency, host overhead included)
  per_query_ms         ``select_windows_frames`` + Q x (validity row by torch scatter / cumsum, ``ground_queries_masked``), synchronised
  per_query_over_in_windows   the END-TO-END ratio of those two medians, as it comes out: whole calls with their host overhead, not kernel times;
                       nothing is gated on it
  same_spans           both routes ended in the same spans and scores, bit for bit (checked once per case, outside the timed rounds)
The unmasked entries are not timed again: their code did not change (profiles/windows_valid_isa.txt).
Inputs: random features with a stretch raised towards each query's text, so the rows look like cosine rows with a peak.

Writes one JSON object to --out (default profiles/similarity_windows_valid.json) and prints it.

    python tools/similarity_windows_valid_prof.py [--queries 1,16,64] [--frames 18000,36000] [--warmup 2] [--iters 5] [--reps 64] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

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


def rows_from_bounds(select, bounds, L):
    """select i32 [B, keep] (-1: padding), bounds i32 [B, Wcap, 2] -> f32 [B, L], 1 at the frames of the named windows: +1 / -1 at their ends, a prefix
    sum, a comparison - the torch index arithmetic a caller has to write without ``windows_valid``."""
    named = select >= 0
    at = select.clamp(min=0).long()
    lo = torch.gather(bounds[..., 0], 1, at).long()
    hi = torch.gather(bounds[..., 1], 1, at).long()
    step = torch.zeros(select.shape[0], L + 1, dtype=torch.int32, device=select.device)
    one = named.to(torch.int32)
    step.scatter_add_(1, lo, one)
    step.scatter_add_(1, hi, -one)
    return (step.cumsum(1)[:, :L] > 0).float()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--queries", default="1,16,64")
    ap.add_argument("--frames", default="18000,36000")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--win", type=int, default=625)
    ap.add_argument("--stride", type=int, default=5)
    ap.add_argument("--keep", type=int, default=20)
    ap.add_argument("--smooth", type=int, default=5)
    ap.add_argument("--gap", type=int, default=2)
    ap.add_argument("--max-spans", type=int, default=256)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=64, help="back-to-back calls per timed window of the kernel form")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_windows_valid.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval import similarity as S
    assert torch.cuda.is_available(), "similarity_windows_valid_prof needs the GPU: a CPU run says nothing about time"
    B, d, N = a.videos, a.dim, a.max_spans
    chain = hip.chain_lib()
    geometry = dict(rule="shifted", win=a.win, stride=a.stride)
    kw = dict(levels=LEVELS, smooth=a.smooth, gap=a.gap, max_spans=N, top=a.top)
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), videos=B, dim=d, win=a.win, stride=a.stride, keep=a.keep, levels=list(LEVELS),
               smooth=a.smooth, gap=a.gap, max_spans=N, top=a.top, warmup=a.warmup, iters=a.iters, reps=a.reps, cases={})
    g = torch.Generator().manual_seed(0)
    for L in (int(x) for x in a.frames.split(",")):
        video = torch.randn(B, L, d, generator=g)
        mask = torch.ones(B, L).cuda()
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
            first = S.select_windows_frames(text, v, mask, keep=a.keep, **geometry)
            select = first.select.view(R, -1).contiguous()
            keep = select.shape[1]
            out_valid, n_valid = torch.empty(R, L, device="cuda"), torch.empty(R, dtype=torch.int32, device="cuda")

            def windows_valid(_):
                hip.chain_check(chain.rvc_windows_valid(hip.ptr(select), hip.ptr(mask), None, R, Q, L, hip.RV_WINDOWS_SHIFTED, a.win, a.stride, hip.RV_FRAMES_ALL, 0,
                                                        keep, hip.ptr(out_valid), hip.ptr(n_valid), hip.stream()), "rvc_windows_valid")

            def in_windows(_):
                return S.ground_queries_in_windows(text, v, mask, keep=a.keep, **geometry, **kw)

            def per_query(_):
                sel = S.select_windows_frames(text, v, mask, keep=a.keep, return_bounds=True, **geometry)
                return [S.ground_queries_masked(text[:, q:q + 1], v, mask, valid=rows_from_bounds(sel.select[:, q], sel.bounds, L), **kw) for q in range(Q)]

            new, old = in_windows(0), per_query(0)
            same = all(same_bits(new.grounding.spans[:, q:q + 1], o.spans) and same_bits(new.grounding.scores[:, q:q + 1], o.scores)
                       and torch.equal(new.grounding.n_keep[:, q:q + 1], o.n_keep) for q, o in enumerate(old))
            assert same, f"L={L} Q={Q}: the two routes ended in different spans"
            forms = dict(windows_valid=(windows_valid, a.reps), in_windows=(in_windows, 1), per_query=(per_query, 1))
            t = {k: [] for k in forms}
            for i in range(a.warmup + a.iters):
                s = {k: timed(fn, reps) for k, (fn, reps) in forms.items()}            # the forms alternate inside every round
                if i >= a.warmup:
                    for k in t:
                        t[k].append(s[k])
            med = {k: statistics.median(x) for k, x in t.items()}
            r = {k + "_ms": spread(x) for k, x in t.items()}
            r.update(rows=R, queries=Q, frames=L, windows=int(first.n_windows.max()), valid_frames_mean=float(new.n_valid.float().mean()), same_spans=same,
                     kept_spans_mean=float(new.grounding.n_keep.float().mean()), per_query_over_in_windows=med["per_query"] / med["in_windows"],
                     windows_valid_bytes=R * L * 4 * 2 + B * L * 4)                    # the row written and counted, the mask row read
            res["cases"][f"L{L}_Q{Q}_R{R}"] = r
            del v
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
