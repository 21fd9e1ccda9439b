"""The stage-1 driver's device route against its host route, on one MI355X with the fp16 build -> profiles/stage1_device.json.

Staging (L frames of 768, f32 or fp16 source, every half-overlapping window of 625 frames, 250 frames per window), medians of 5 rounds after warm-up,
the forms alternating inside every round of one process:
  kernel_back_to_back      rv_window_gather_rule (clipped rule, NULL select) alone, REPS launches between two events: time per launch and bytes read +
                           written per launch over that time, as a fraction of the 6.3 TB/s the microarchitecture guide calls achievable
  stage_resident_clipped   one ``WindowStager.stage_resident_clipped(...).wait()`` and a device synchronise, host clock (the driver's call with the flag)
  host_route               ``WindowStager.stage_windows(features, stage1.cut_windows(...)).wait()`` and a synchronise - the driver's call without the flag,
                           whose code this feature does not touch
  movie_upload             the whole movie through ``ResidentFeatures`` (a miss), which the resident route pays once per movie
Epilogue (a [W, 250, 768] fp16 window tensor, P proposals of mixed lengths 1 .. 250 in distinct windows):
  proposal_cosines         one ``stage1.proposal_cosines`` call: one launch, one ``.tolist()``
  per_proposal_loop        ``score_query``'s loop on the same tensors: one ``ops.topk_cosine`` and one ``float()`` per proposal
Both leave the stream idle when they return, so the host clock around them is the end-to-end time.  ``*_over_*`` are END-TO-END ratios."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from revisionllm_amd import hip  # noqa: E402
from revisionllm_amd.data.feature_store import ResidentFeatures, WindowStager  # noqa: E402
from revisionllm_amd.eval import stage1  # noqa: E402

ACHIEVABLE = 6.3e12
GEOMETRY = dict(debug_window=125, feature_fps=5, num_frames=250)


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def rounds_of(forms, rounds, warmup):
    got = {k: [] for k in forms}
    for r in range(warmup + rounds):
        for k, fn in forms.items():
            v = fn()
            if r >= warmup:
                got[k].append(v)
    return got


def staging_case(dev, stager, L, d, src, rounds, warmup, reps):
    rng = np.random.default_rng(L)
    array = rng.standard_normal((L, d), dtype=np.float32).astype(src)
    frame_idx = stage1.cut_windows(L, **GEOMETRY)
    W, F = frame_idx.shape
    cache = ResidentFeatures(dev, 1 << 30, op_dtype="f16", stream=stager.stream)
    resident = cache.get("movie", array)
    torch.cuda.synchronize()
    in_bytes = W * F * d * resident.element_size()                      # every output row reads one source row
    out_bytes = W * F * d * 2
    frames = torch.empty(W, F, d, dtype=torch.float16, device=dev)
    entry, st = hip.lib("f16").rv_window_gather_rule, hip.stream()
    c_args = (hip.ptr(resident), hip.dtype_code(resident), d, None, None, 1, 1, L, d, 625, 2, W, F, hip.ptr(frames), hip.RV_F16, None, hip.RV_WINDOWS_CLIPPED, st)

    def back_to_back():                                                 # the C entry itself: no allocation and no Python wrapper between the launches
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            entry(*c_args)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    def upload():
        fresh = ResidentFeatures(dev, 1 << 30, op_dtype="f16", stream=stager.stream)
        fresh._pinned = cache._pinned                                   # (the pinned buffer is kept across movies: not part of a miss)
        return host_ms(lambda: fresh.get("movie", array))

    forms = {"kernel_back_to_back": back_to_back,
             "stage_resident_clipped": lambda: host_ms(lambda: stager.stage_resident_clipped(resident, **GEOMETRY).wait()),
             "host_route": lambda: host_ms(lambda: stager.stage_windows(array, frame_idx).wait()),
             "movie_upload": upload}
    got = rounds_of(forms, rounds, warmup)
    want = stager.stage_windows(array, frame_idx).wait()
    have = stager.stage_resident_clipped(resident, **GEOMETRY).wait()
    torch.cuda.synchronize()
    out = dict(L=L, d=d, source=str(np.dtype(src)), windows=W, frames=F, bytes_read=in_bytes, bytes_written=out_bytes,
               bit_equal_to_host_route=bool(torch.equal(want.view(torch.int16), have.view(torch.int16))))
    for k in forms:
        out[k + "_ms"] = summary(got[k])
    kernel_s = out["kernel_back_to_back_ms"]["median"] * 1e-3
    out["kernel_bytes_per_s"] = (in_bytes + out_bytes) / kernel_s
    out["kernel_fraction_of_achievable_6.3TBps"] = out["kernel_bytes_per_s"] / ACHIEVABLE
    out["host_over_resident_end_to_end"] = out["host_route_ms"]["median"] / out["stage_resident_clipped_ms"]["median"]
    saved = out["host_route_ms"]["median"] - out["stage_resident_clipped_ms"]["median"]
    out["break_even_queries"] = out["movie_upload_ms"]["median"] / saved if saved > 0 else None
    return out


def epilogue_case(dev, windows, query_cls, P, topk_pool, rounds, warmup):
    W, T, _ = windows.shape
    rng = np.random.default_rng(P)
    frames = {}
    for w in sorted(rng.choice(W, P, replace=False).tolist()):           # iou's dict: one proposal per window that answered
        length = int(rng.choice([1, 3, 10, 40, 120, T]))
        a = int(rng.integers(0, T - length + 1))
        frames[w] = (a, a + length - 1)
    forms = {"proposal_cosines": lambda: host_ms(lambda: stage1.proposal_cosines(windows, frames, query_cls, topk_pool)),
             "per_proposal_loop": lambda: host_ms(lambda: stage1._proposal_cosines_each(windows, frames, query_cls, topk_pool))}
    got = rounds_of(forms, rounds, warmup)
    one, each = stage1.proposal_cosines(windows, frames, query_cls, topk_pool), stage1._proposal_cosines_each(windows, frames, query_cls, topk_pool)
    same = len(one) == len(each) and all(x == y or (x != x and y != y) for x, y in zip(one, each))      # (a one-frame slice with a zero feature is NaN in both)
    out = dict(P=P, windows=W, frames=T, topk_pool=topk_pool, equal_to_the_loop=same, nan_scores=sum(1 for x in one if x != x))
    for k in forms:
        out[k + "_ms"] = summary(got[k])
    out["loop_over_one_call_end_to_end"] = out["per_proposal_loop_ms"]["median"] / out["proposal_cosines_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stage1_device.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--lengths", type=int, nargs="+", default=[18000, 36000])
    ap.add_argument("--proposals", type=int, nargs="+", default=[1, 8, 57, 115])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stage1_device_prof: needs the GPU (no timing is taken on a CPU)")
    hip.set_flavour("f16")
    dev = torch.device("cuda:0")
    stager = WindowStager(dev, op_dtype="f16")
    staging = []
    for L in args.lengths:
        for src in (np.float32, np.float16):
            c = staging_case(dev, stager, L, 768, src, args.rounds, args.warmup, args.reps)
            staging.append(c)
            print(json.dumps({k: c[k] for k in ("L", "source", "windows", "kernel_fraction_of_achievable_6.3TBps", "host_over_resident_end_to_end",
                                                 "break_even_queries", "bit_equal_to_host_route")}), flush=True)
    g = torch.Generator().manual_seed(1)
    movie = torch.randn(max(args.lengths), 768, generator=g).to(dev)
    windows = stage1.gather_windows(movie, dtype=torch.float16, **GEOMETRY)      # 115 windows for 36000 frames
    query_cls = torch.randn(768, generator=g).to(dev)
    epilogue = []
    for P in args.proposals:
        c = epilogue_case(dev, windows, query_cls, min(P, windows.shape[0]), True, args.rounds, args.warmup)
        epilogue.append(c)
        print(json.dumps({k: c[k] for k in ("P", "loop_over_one_call_end_to_end", "equal_to_the_loop")} | {"one_call_ms": c["proposal_cosines_ms"]["median"],
                                                                                                             "loop_ms": c["per_proposal_loop_ms"]["median"]}), flush=True)
    result = dict(device=torch.cuda.get_device_name(0), operand="f16", rounds=args.rounds, warmup=args.warmup, reps=args.reps,
                  host_threads=torch.get_num_threads(), staging=staging, epilogue=epilogue)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
