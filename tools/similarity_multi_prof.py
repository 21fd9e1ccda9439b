"""Proposal-query matching with Q queries per video at an hour of 5 fps features: ``forward_clip_matching_multi`` (rv_frame_cosine_multi + rv_span_scores_multi,
the features read once for all Q texts) against the route a caller had before it: Q calls of ``forward_clip_matching`` on the same tensors.

B = 8 videos of L = 8192 frames, d = 768 in the build's operand type, N = 64 proposals of mixed length per query.  --sets distinct copies of the features (default
4: 404 MB, more than the 256 MiB infinity cache) are used in turn, so that no call finds its features in a cache.  All forms of a Q run in one process,
alternating, between device events; warm-up + timed rounds per form; medians with min .. max.  Per Q in --queries:

  multi_ms               (a) one ``forward_clip_matching_multi`` call, synchronised: enqueue + three kernels + the wait (a latency)
  multi_back_to_back_ms  (a) per call over --reps un-synchronised calls: a throughput, bounded below by the host's enqueue cost per call
  single_loop_ms         (b) Q calls of ``forward_clip_matching`` (text[:, q], proposal[:, q]), then one synchronise
  single_loop_back_to_back_ms  (b) per round of Q calls over max(1, --reps / Q) un-synchronised rounds
  cosine_multi_ms        (c) rv_frame_cosine_multi alone (with its text-norm launch) per call over back-to-back calls rotating through the copies; its feature
                         bytes over that time as a share of the 8 TB/s HBM figure and its 2 B L d Q FLOPs as a share of the 157.3 TF/s f32-matrix peak; ``bound``
                         names the larger of the two least times
  frame_cosine_ms        the single-text rv_frame_cosine alone, back to back, for the Q = 1 comparison
  span_scores_ms / span_scores_multi_ms   the span kernels alone, back to back

--single-only runs leg (b) at Q = 1 and rv_span_scores alone, and nothing that needs the new entries; with --package-root DIR the package is imported from
DIR (a checkout of the parent commit with its libraries built), so the same job measures the parent's leg.  --parent-json FILE[,FILE] merges the output of
such runs (one before and one after this tree's run: the parent's min .. max is taken over both).

Writes one JSON object to --out (default profiles/similarity_multi.json) and prints it.

    python tools/similarity_multi_prof.py [--queries 1,4,16,64,256] [--spans 64] [--sets 4] [--warmup 2] [--iters 5] [--reps 192] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12
F32_MATRIX_PEAK = 157.3e12


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


def run_forms(forms, warmup, iters):
    t = {name: [] for name, _, _ in forms}
    for i in range(warmup + iters):
        for name, fn, reps in forms:
            s = timed(fn, reps)
            if i >= warmup:
                t[name].append(s)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--spans", type=int, default=64)
    ap.add_argument("--queries", default="1,4,16,64,256")
    ap.add_argument("--sets", type=int, default=4, help="distinct copies of the features used in turn (4 x 101 MB: more than the infinity cache)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=192, help="back-to-back calls per timed window of the back-to-back forms")
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_multi.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval import similarity as S
    assert torch.cuda.is_available(), "similarity_multi_prof needs the GPU: a CPU run says nothing about time"
    dt = hip.op_dtype()
    B, L, d, N = a.videos, a.frames, a.dim, a.spans
    queries = [1] if a.single_only else [int(q) for q in a.queries.split(",")]
    g = torch.Generator().manual_seed(0)
    theme = torch.randn(B, d, generator=g)
    base = torch.randn(B, L, d, generator=g) + 0.3 * theme[:, None, :]
    videos = [base.roll(j, dims=1).to(dt).cuda() for j in range(a.sets)]          # the same frames in another order: distinct memory, no extra host work
    mask = torch.ones(B, L)
    for b in range(B):
        mask[b, L - 61 * b:] = 0
    mask = mask.cuda()
    lo_w, hi_w = torch.log(torch.tensor(0.001)), torch.log(torch.tensor(0.5))
    calls = [0]

    def video():
        calls[0] += 1
        return videos[calls[0] % a.sets]

    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), package_root=os.path.relpath(os.path.abspath(a.package_root), ROOT), videos=B,
               frames=L, dim=d, spans_per_query=N, feature_sets=a.sets, feature_bytes_in_rotation=a.sets * B * L * d * videos[0].element_size(),
               warmup=a.warmup, iters=a.iters, reps=a.reps, per_q={})
    for Q in queries:
        text = (theme[:, None, :] + 0.5 * torch.randn(B, Q, d, generator=g)).cuda()
        spans = torch.stack([torch.rand(B, Q, N, generator=g), torch.exp(lo_w + torch.rand(B, Q, N, generator=g) * (hi_w - lo_w))], dim=-1).cuda()
        singles = [(text[:, q].contiguous(), spans[:, q].contiguous()) for q in range(Q)]
        sims1 = ops.frame_cosine(singles[0][0], videos[0])

        def single_loop(_):
            v = video()
            for t, p in singles:
                S.forward_clip_matching(t, v, mask, p)

        forms = [("single_loop", single_loop, 1), ("single_loop_back_to_back", single_loop, max(1, a.reps // Q)),
                 ("frame_cosine", lambda _: ops.frame_cosine(singles[0][0], video()), a.reps),
                 ("span_scores", lambda _: ops.span_scores(sims1, singles[0][1], mask), a.reps)]
        if not a.single_only:
            simsq = ops.frame_cosine_multi(text, videos[0])
            forms += [("multi", lambda _: S.forward_clip_matching_multi(text, video(), mask, spans), 1),
                      ("multi_back_to_back", lambda _: S.forward_clip_matching_multi(text, video(), mask, spans), a.reps),
                      ("cosine_multi", lambda _: ops.frame_cosine_multi(text, video()), a.reps),
                      ("span_scores_multi", lambda _: ops.span_scores_multi(simsq, spans, mask), a.reps)]
        t = run_forms(forms, a.warmup, a.iters)
        med = {k: statistics.median(v) for k, v in t.items()}
        r = {k + "_ms": spread(v) for k, v in t.items()}
        if not a.single_only:
            feat_bytes, flops = B * L * d * videos[0].element_size(), 2.0 * B * L * d * Q
            least = dict(hbm=feat_bytes / HBM_PEAK, mfma=flops / F32_MATRIX_PEAK)
            r.update(multi_over_single_loop=med["multi"] / med["single_loop"], single_loop_over_multi=med["single_loop"] / med["multi"],
                     back_to_back_multi_over_single_loop=med["multi_back_to_back"] / med["single_loop_back_to_back"],
                     cosine_multi_feature_bytes=feat_bytes, cosine_multi_fraction_of_8TBps=feat_bytes / med["cosine_multi"] / HBM_PEAK,
                     cosine_multi_flops=flops, cosine_multi_fraction_of_f32_matrix_peak=flops / med["cosine_multi"] / F32_MATRIX_PEAK,
                     cosine_multi_bound="mfma" if least["mfma"] > least["hbm"] else "hbm",
                     cosine_multi_share_of_least_time=max(least.values()) / med["cosine_multi"])
            multi = S.forward_clip_matching_multi(text, videos[0], mask, spans).float()
            one = torch.stack([S.forward_clip_matching(t_, videos[0], mask, p_).float() for t_, p_ in singles[:4]], dim=1)
            r["max_abs_diff_multi_vs_single_first_queries"] = float((multi[:, :one.shape[1]] - one).abs().max())
        res["per_q"][str(Q)] = r
    if a.parent_json and "1" in res["per_q"]:
        runs = []
        for path in a.parent_json.split(","):
            with open(path) as f:
                runs.append(json.load(f)["per_q"]["1"])
        mine, out = res["per_q"]["1"], dict(runs=len(runs))
        for key in ("single_loop_back_to_back_ms", "frame_cosine_ms", "span_scores_ms"):
            lo, hi = min(r[key]["min"] for r in runs), max(r[key]["max"] for r in runs)
            out[key] = dict(medians=[r[key]["median"] for r in runs], min=lo, max=hi, this_tree_median=mine[key]["median"],
                            this_tree_median_inside_parents_min_max=lo <= mine[key]["median"] <= hi,
                            this_tree_median_over_parents_max=mine[key]["median"] / hi)
        res["parent_commit_q1"] = out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
