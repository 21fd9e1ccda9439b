"""The masked span kernels (rvc_span_scores_masked, rvc_span_propose_masked of the chain library) next to their unmasked siblings (rv_span_scores_multi,
rv_span_propose), and the masked grounder (``ground_queries_masked``) next to ``ground_queries``.

8 videos x Q queries (--queries) x L = 8192 frames of 768 features in the build's 16-bit type; 64 proposals per row for the score kernels (seeded
(centre, width) spans, centres anywhere in the row, widths of 8 to 408 frames: every one a window with frames in it, none void); ``valid`` hides one
frame in 16; T = 5 levels, smooth = 5, gap = 2, at most 256 spans per row for the proposal kernels.  The forms of a case alternate in one process between device events; warm-up + timed rounds
per form; medians with min .. max.  Per case:

  scores_ms / scores_masked_ms       rv_span_scores_multi / rvc_span_scores_masked (top-k, k = 3) alone through the C entries into preallocated outputs,
                                     per call over --reps back-to-back calls
  attention_ms / attention_masked_ms the same in the attention mode (temperature 0.01)
  propose_ms / propose_masked_ms     rv_span_propose / rvc_span_propose_masked alone, likewise
  ground_ms / ground_masked_ms       one ``ground_queries`` / ``ground_queries_masked(valid=, skip_nan=True)`` call, synchronised (a latency, host overhead
                                     included)
  *_masked_over_*                    the ratios of the medians, as they come out: nothing is gated on them
Inputs: random features with a stretch raised towards each query's text, so the rows look like cosine rows with a peak.

Writes one JSON object to --out (default profiles/similarity_masked.json) and prints it.

    python tools/similarity_masked_prof.py [--queries 1,16,64] [--frames 8192] [--warmup 2] [--iters 5] [--reps 64] [--out FILE]"""
import argparse
import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--queries", default="1,16,64")
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--proposals", type=int, default=64)
    ap.add_argument("--hide-every", type=int, default=16)
    ap.add_argument("--smooth", type=int, default=5)
    ap.add_argument("--gap", type=int, default=2)
    ap.add_argument("--max-spans", type=int, default=256)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=64, help="back-to-back calls per timed window of the kernel forms")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_masked.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from revisionllm_amd import hip, ops
    from revisionllm_amd.eval import similarity as S
    assert torch.cuda.is_available(), "similarity_masked_prof needs the GPU: a CPU run says nothing about time"
    B, L, d, N, P = a.videos, a.frames, a.dim, a.max_spans, a.proposals
    lib, chain = hip.lib(), hip.chain_lib()
    kw = dict(levels=LEVELS, smooth=a.smooth, gap=a.gap, max_spans=N)
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), videos=B, frames=L, dim=d, proposals=P, hide_every=a.hide_every, levels=list(LEVELS),
               smooth=a.smooth, gap=a.gap, max_spans=N, top=a.top, warmup=a.warmup, iters=a.iters, reps=a.reps, cases={})
    g = torch.Generator().manual_seed(0)
    video = torch.randn(B, L, d, generator=g)
    mask = torch.ones(B, L).cuda()
    valid = torch.ones(B, L)
    valid[:, ::a.hide_every] = 0
    valid = valid.cuda()
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
        spans = torch.stack((torch.rand(R, P, generator=g), (8 + 400 * torch.rand(R, P, generator=g)) / L), dim=-1).cuda()
        frames = ops.span_scores_masked(sims, spans.view(B, Q, P, 2), mask, return_usable=True).n_usable
        scores, usable = torch.empty(R, P, device="cuda"), torch.empty(R, P, dtype=torch.int32, device="cuda")
        out_spans, n_spans, n_found = torch.empty(R, N, 2, device="cuda"), torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, dtype=torch.int32, device="cuda")

        def plain_scores(mode):
            def f(_):
                hip.check(lib.rv_span_scores_multi(hip.ptr(flat), hip.ptr(spans), hip.ptr(mask), B, Q, L, P, mode, 3, 0.01, hip.ptr(scores), None, hip.stream()),
                          "rv_span_scores_multi")
            return f

        def masked_scores(mode):
            def f(_):
                hip.chain_check(chain.rvc_span_scores_masked(hip.ptr(flat), hip.ptr(spans), hip.ptr(mask), hip.ptr(valid), R, Q, L, P, mode, 3, 0.01, 1,
                                                             hip.ptr(scores), None, hip.ptr(usable), hip.stream()), "rvc_span_scores_masked")
            return f

        def propose(_):
            hip.check(lib.rv_span_propose(hip.ptr(flat), hip.ptr(mask), R, Q, L, table, len(LEVELS), 1, a.smooth, a.gap, 1, 0, N, hip.ptr(out_spans),
                                          hip.ptr(n_spans), hip.ptr(n_found), None, None, hip.stream()), "rv_span_propose")

        def propose_masked(_):
            hip.chain_check(chain.rvc_span_propose_masked(hip.ptr(flat), hip.ptr(mask), hip.ptr(valid), R, Q, L, table, len(LEVELS), 1, a.smooth, a.gap, 1, 0, N, 1,
                                                          hip.ptr(out_spans), hip.ptr(n_spans), hip.ptr(n_found), None, None, hip.stream()),
                            "rvc_span_propose_masked")

        def ground(_):
            return S.ground_queries(text, v, mask, top=a.top, **kw)

        def ground_masked(_):
            return S.ground_queries_masked(text, v, mask, valid=valid, skip_nan=True, top=a.top, **kw)

        forms = dict(scores=(plain_scores(0), a.reps), scores_masked=(masked_scores(0), a.reps), attention=(plain_scores(1), a.reps),
                     attention_masked=(masked_scores(1), a.reps), propose=(propose, a.reps), propose_masked=(propose_masked, a.reps), ground=(ground, 1),
                     ground_masked=(ground_masked, 1))
        t = {k: [] for k in forms}
        for i in range(a.warmup + a.iters):
            s = {k: timed(fn, reps) for k, (fn, reps) in forms.items()}            # the forms alternate inside every round
            if i >= a.warmup:
                for k in t:
                    t[k].append(s[k])
        med = {k: statistics.median(x) for k, x in t.items()}
        r = {k + "_ms": spread(x) for k, x in t.items()}
        r.update(rows=R, queries=Q, window_frames_mean=float(frames.float().mean()), window_frames_min=int(frames.min()),
                 **{k + "_masked_over_" + k: med[k + "_masked"] / med[k] for k in ("scores", "attention", "propose", "ground")})
        res["cases"][f"Q{Q}_R{R}"] = r
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
