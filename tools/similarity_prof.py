"""Proposal-query matching at an hour of 5 fps features: ``forward_clip_matching`` (rv_frame_cosine + rv_span_scores) against the only route the package offered
before it: one ``ops.topk_pool`` launch per proposal on its slice of the features, with the windows brought to the host first.

B = 8 videos of L = 8192 frames, d = 768, N = 256 proposals of mixed length per video (widths log-uniform in 0.1 % .. 50 % of the video).  --sets distinct copies
of the features (default 4: 404 MB, more than the 256 MiB infinity cache) are used in turn, so that no call finds its features in a cache.  Both forms run in one
process, alternating, between device events; warm-up + timed rounds per form.  What the numbers are:

  fused_ms               one ``forward_clip_matching`` call, synchronised: enqueue + both kernels + the wait (a latency)
  fused_back_to_back_ms  per call over --reps un-synchronised calls: a throughput, bounded below by the host's enqueue cost per call
  loop_ms                the per-proposal loop, synchronised; most of it is the host's launch overhead for B x N x ~6 small kernels - the ratio to fused_ms is an
                         end-to-end comparison of the two routes, not of kernels
  frame_cosine_ms        rv_frame_cosine alone per call over --reps back-to-back calls rotating through the --sets copies, and its bytes over that time as a share
                         of the 8 TB/s HBM figure

Writes one JSON object to --out (default profiles/similarity.json) and prints it.

    python tools/similarity_prof.py [--videos 8] [--frames 8192] [--dim 768] [--spans 256] [--sets 4] [--warmup 2] [--iters 5] [--reps 48] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from revisionllm_amd import hip, ops  # noqa: E402
from revisionllm_amd.eval.similarity import forward_clip_matching  # noqa: E402

HBM_PEAK = 8.0e12


def per_span_loop(text, video, windows):
    """One pooling launch per proposal: its window (``windows``: host list of (lo, hi) per video and proposal) is cut out of the features, its frames and the text
    are scaled to unit length, ``ops.topk_pool`` adds up the (at most) three frames closest to the text and the score is that row's product with the text."""
    unit_text = F.normalize(text, dim=1)
    scores = torch.zeros(len(windows), len(windows[0]), device=video.device)
    for b, row in enumerate(windows):
        for n, (lo, hi) in enumerate(row):
            if hi > lo:
                frames = F.normalize(video[b, lo:hi].float(), dim=1)
                scores[b, n] = ops.topk_pool(unit_text[b:b + 1], frames[None], min(3, hi - lo))[0, 0] @ unit_text[b]
    return scores


def timed(fn, reps=1):
    """Seconds per call over ``reps`` back-to-back calls (call i gets i as its argument) between two device events; the second event is waited for."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        out = fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps, out


def spread(v):
    return dict(median=statistics.median(v) * 1e3, min=min(v) * 1e3, max=max(v) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--spans", type=int, default=256)
    ap.add_argument("--sets", type=int, default=4, help="distinct copies of the features used in turn (4 x 101 MB: more than the infinity cache)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=48, help="back-to-back calls per timed window of the back-to-back forms")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "similarity_prof needs the GPU: a CPU run says nothing about time"
    dt = hip.op_dtype()
    B, L, d, N = a.videos, a.frames, a.dim, a.spans
    g = torch.Generator().manual_seed(0)
    text = torch.randn(B, d, generator=g)
    base = torch.randn(B, L, d, generator=g) + 0.3 * text[:, None, :]
    videos = [base.roll(j, dims=1).to(dt).cuda() for j in range(a.sets)]          # the same frames in another order: distinct memory, no extra host work
    text = text.cuda()
    mask = torch.ones(B, L)
    for b in range(B):
        mask[b, L - 61 * b:] = 0
    mask = mask.cuda()
    lo_w, hi_w = torch.log(torch.tensor(0.001)), torch.log(torch.tensor(0.5))
    spans = torch.stack([torch.rand(B, N, generator=g), torch.exp(lo_w + torch.rand(B, N, generator=g) * (hi_w - lo_w))], dim=-1).cuda()
    calls = [0]

    def video():
        calls[0] += 1
        return videos[calls[0] % a.sets]

    def loop(_):
        v = video()
        _, win = ops.span_scores(ops.frame_cosine(text, v), spans, mask, return_windows=True)
        return per_span_loop(text, v, win.tolist())                               # (.tolist(): the windows come to the host, as that route needs them)

    forms = (("fused", lambda _: forward_clip_matching(text, video(), mask, spans), 1), ("fused_back_to_back", lambda _: forward_clip_matching(text, video(), mask, spans), a.reps),
             ("loop", loop, 1), ("frame_cosine", lambda _: ops.frame_cosine(text, video()), a.reps))
    t = {name: [] for name, _, _ in forms}
    for i in range(a.warmup + a.iters):
        for name, fn, reps in forms:
            s, _ = timed(fn, reps)
            if i >= a.warmup:
                t[name].append(s)
    med = {k: statistics.median(v) for k, v in t.items()}
    cos_bytes = B * L * d * videos[0].element_size() + B * d * 4 + B * L * 4
    exact, win = ops.span_scores(ops.frame_cosine(text, videos[0]), spans, mask, return_windows=True)      # f32, before the rounding to the features' type
    by_loop = per_span_loop(text, videos[0], win.tolist())
    lens = (win[..., 1] - win[..., 0]).clamp_min(0).float()
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), videos=B, frames=L, dim=d, spans=N, feature_sets=a.sets,
               feature_bytes_in_rotation=a.sets * B * L * d * videos[0].element_size(), warmup=a.warmup, iters=a.iters, reps=a.reps,
               window_frames=dict(min=float(lens.min()), median=float(lens.median()), max=float(lens.max())),
               fused_ms=spread(t["fused"]), fused_back_to_back_ms=spread(t["fused_back_to_back"]), loop_ms=spread(t["loop"]),
               loop_over_fused_end_to_end=med["loop"] / med["fused"],
               frame_cosine_ms=spread(t["frame_cosine"]), frame_cosine_bytes=cos_bytes, frame_cosine_bytes_per_s=cos_bytes / med["frame_cosine"],
               frame_cosine_fraction_of_8TBps=cos_bytes / med["frame_cosine"] / HBM_PEAK,
               max_abs_diff_fused_vs_loop=float((exact - by_loop).abs().max()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
