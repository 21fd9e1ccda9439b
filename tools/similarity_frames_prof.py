"""Window selection on a chosen frame set (``ops.window_select_frames`` -> rvc_window_select_frames of the chain library) beside the selection it
generalises (rv_window_select), in one process, alternating.

8 videos x Q queries (--queries) x L frames (--frames), cosine rows of random features with a stretch raised towards each query's text, win = 625,
stride = 5, keep = 100, min_sep = 1, a ground truth per row.  Every form is the C entry into preallocated outputs (select, the counts, hit_rank), per
call over --reps back-to-back calls between two device events; the forms of a case alternate inside every round; warm-up + timed rounds; medians with
min .. max.  Per case:

  window_select_ms      rv_window_select of the loaded main library (the baseline: every frame of a window, no validity)
  parent_select_ms      the same entry of another build of it (--parent-lib: a library built from the parent commit), when given: the two medians'
                        distance against their own min .. max is the margin for "the existing kernel did not move"
  frames_all_ms         rvc_window_select_frames, RV_FRAMES_ALL, valid = NULL (the same code as the baseline plus the n_candidates store)
  frames_sampled_ms     RV_FRAMES_SAMPLED with F = --num-frames (250): 250 of a window's 626 frames, each index from float64 arithmetic
  frames_sampled_valid_ms  the same with a validity row per video that hides one frame in seven and a stretch of 2000 frames
  frames_all_valid_ms   RV_FRAMES_ALL with that validity row
and whether frames_all's outputs equal the baseline's bit for bit, how many windows lost their candidacy under the validity row, and how many rows
choose other windows on the sampled frames than on all.  Nothing here measures recall: the features are random.

Writes one JSON object to --out (default profiles/similarity_frames.json) and prints it.

    python tools/similarity_frames_prof.py [--queries 1,16,64] [--frames 18000,36000] [--warmup 2] [--iters 5] [--reps 32] [--parent-lib FILE] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

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
    ap.add_argument("--num-frames", type=int, default=250)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=32, help="back-to-back calls per timed window")
    ap.add_argument("--parent-lib", default=None, help="another build of the main library (or of its prefilter.hip alone) that exports rv_window_select")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_frames.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from revisionllm_amd import hip, ops
    assert torch.cuda.is_available(), "similarity_frames_prof needs the GPU: a CPU run says nothing about time"
    B, d, win, stride, keep, k, F = a.videos, a.dim, a.win, a.stride, a.keep, a.k, a.num_frames
    lib, chain = hip.lib(), hip.chain_lib()
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        parent.rv_window_select.restype, parent.rv_window_select.argtypes = hip.SIGNATURES["rv_window_select"]
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), videos=B, dim=d, win=win, stride=stride, keep=keep, k=k, num_frames=F,
               warmup=a.warmup, iters=a.iters, reps=a.reps, parent_lib=bool(parent), cases={})
    g = torch.Generator(device=dev).manual_seed(0)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)                            # noqa: E731

    for L in (int(x) for x in a.frames.split(",")):
        video = torch.randn(B, L, d, generator=g, device=dev)
        mask = torch.ones(B, L, device=dev)
        valid = torch.ones(B, L, device=dev)
        valid[:, ::7] = 0
        valid[:, 3000:5000] = 0
        hop = win // stride
        Wcap = max(1, -(-L // hop) - 1)
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
            outs = {name: dict(select=i32(R, keep), n_select=i32(R), n_windows=i32(R), n_candidates=i32(R), hit_rank=i32(R))
                    for name in ("window_select", "parent_select", "frames_all", "frames_sampled", "frames_sampled_valid", "frames_all_valid")}

            def old(which, name):
                o = outs[name]
                hip.check(which.rv_window_select(hip.ptr(flat), hip.ptr(mask), R, Q, L, win, stride, k, keep, 1, Wcap, hip.ptr(gt), hip.ptr(o["select"]),
                                                 hip.ptr(o["n_select"]), hip.ptr(o["n_windows"]), None, None, None, hip.ptr(o["hit_rank"]), hip.stream()),
                          "rv_window_select")

            def new(name, frames, nf, vld):
                o = outs[name]
                hip.chain_check(chain.rvc_window_select_frames(hip.ptr(flat), hip.ptr(mask), hip.ptr(vld), R, Q, L, hip.RV_WINDOWS_SHIFTED, win, stride, frames, nf,
                                                               k, keep, 1, Wcap, hip.ptr(gt), hip.ptr(o["select"]), hip.ptr(o["n_select"]), hip.ptr(o["n_windows"]),
                                                               hip.ptr(o["n_candidates"]), None, None, None, hip.ptr(o["hit_rank"]), hip.stream()),
                                "rvc_window_select_frames")
            forms = dict(window_select=lambda _: old(lib, "window_select"),
                         frames_all=lambda _: new("frames_all", hip.RV_FRAMES_ALL, 0, None),
                         frames_sampled=lambda _: new("frames_sampled", hip.RV_FRAMES_SAMPLED, F, None),
                         frames_sampled_valid=lambda _: new("frames_sampled_valid", hip.RV_FRAMES_SAMPLED, F, valid),
                         frames_all_valid=lambda _: new("frames_all_valid", hip.RV_FRAMES_ALL, 0, valid))
            if parent is not None:
                forms["parent_select"] = lambda _: old(parent, "parent_select")
            t = {name: [] for name in forms}
            for it in range(a.warmup + a.iters):
                for name, fn in forms.items():                                   # the forms alternate inside a round
                    s = timed(fn, a.reps)
                    if it >= a.warmup:
                        t[name].append(s)
            torch.cuda.synchronize()
            med = {name: statistics.median(x) for name, x in t.items()}
            r = {name + "_ms": spread(x) for name, x in t.items()}
            base, every, sampled, hidden = outs["window_select"], outs["frames_all"], outs["frames_sampled"], outs["frames_sampled_valid"]
            r.update(rows=R, queries=Q, frames=L, windows=int(base["n_windows"].max()),
                     frames_all_equals_window_select=bool(all(torch.equal(base[n], every[n]) for n in ("select", "n_select", "n_windows", "hit_rank"))
                                                          and torch.equal(every["n_candidates"], every["n_windows"])),
                     parent_equals_window_select=(bool(all(torch.equal(base[n], outs["parent_select"][n]) for n in ("select", "n_select", "n_windows", "hit_rank")))
                                                  if parent is not None else None),
                     rows_with_another_selection_on_sampled_frames=int((sampled["select"] != base["select"]).any(dim=1).sum()),
                     windows_without_a_usable_frame=int((hidden["n_windows"] - hidden["n_candidates"]).max()),
                     frames_all_over_window_select=med["frames_all"] / med["window_select"],
                     frames_sampled_over_window_select=med["frames_sampled"] / med["window_select"],
                     frames_sampled_valid_over_window_select=med["frames_sampled_valid"] / med["window_select"],
                     parent_over_window_select=med["parent_select"] / med["window_select"] if parent is not None else None)
            res["cases"][f"L{L}_Q{Q}_R{R}"] = r
        del video
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
