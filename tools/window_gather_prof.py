"""Staging the recursion's windows from resident features against the host route, on one MI355X with the fp16 build -> profiles/window_gather.json.

Per case (L frames of 768, f32 or fp16 source, 100 selected windows or all of them, 250 frames per window), medians of 5 rounds after warm-up, the forms
alternating inside every round of one process:
  kernel_back_to_back   rv_window_gather alone, REPS launches between two events: time per launch, bytes read + written per launch over that time, and
                        that rate as a fraction of the 6.3 TB/s the microarchitecture guide calls achievable
  call_synchronised     one ``ops.window_gather`` call and a device synchronise, host clock
  stage_resident        one ``WindowStager.stage_resident(...).wait()`` and a synchronise (the driver's call: upload of the list, kernel, event)
  host_route            ``WindowStager.stage_windows(...).wait()`` and a synchronise - the route the driver takes without --device_features - and its two
                        parts: the host gather + cast into the pinned buffer, and the copy
  movie_upload          the whole movie through ``ResidentFeatures`` (a miss), which the resident route pays once per movie
``host_over_resident`` is the END-TO-END ratio of the two synchronised staging calls; ``break_even_queries`` is the number of queries of one movie from
which the resident route, upload included, is the faster one."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from revisionllm_amd import hip, ops  # noqa: E402
from revisionllm_amd.data.feature_store import ResidentFeatures, WindowStager  # noqa: E402
from revisionllm_amd.eval import stage2  # noqa: E402

ACHIEVABLE = 6.3e12
GEOMETRY = dict(debug_window=125, feature_fps=5, stride=5, num_frames=250)


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def case(dev, stager, L, d, src, n_windows, rounds, warmup, reps):
    rng = np.random.default_rng(L + n_windows)
    array = rng.standard_normal((L, d), dtype=np.float32).astype(src)
    _, frame_idx = stage2.cut_windows(L, **GEOMETRY)
    W = frame_idx.shape[0]
    windows = sorted(rng.choice(W, n_windows, replace=False).tolist()) if n_windows < W else list(range(W))
    F = GEOMETRY["num_frames"]
    cache = ResidentFeatures(dev, 1 << 30, op_dtype="f16", stream=stager.stream)
    resident = cache.get("movie", array)
    torch.cuda.synchronize()
    row = torch.tensor(windows, dtype=torch.int32, device=dev)
    in_bytes = len(windows) * F * d * resident.element_size()          # every output row reads one source row (rows shared by windows count each time)
    out_bytes = len(windows) * F * d * 2
    kw = dict(win=625, stride=5, num_frames=F, out_dtype=torch.float16)
    sel_idx = frame_idx[windows]

    frames = torch.empty(len(windows), F, d, dtype=torch.float16, device=dev)
    entry, st = hip.lib("f16").rv_window_gather, hip.stream()
    c_args = (hip.ptr(resident), hip.dtype_code(resident), d, None, hip.ptr(row), 1, 1, L, d, 625, 5, len(windows), F, hip.ptr(frames), hip.RV_F16, None, st)

    def back_to_back():                                                 # the C entry itself: no allocation and no Python wrapper between the launches
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            entry(*c_args)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    def host_parts():
        t0 = time.perf_counter()
        host = torch.from_numpy(np.ascontiguousarray(array))[torch.from_numpy(sel_idx.astype(np.int64))].to(torch.float16)      # the gather + the cast, as stage_windows does them
        t1 = time.perf_counter()
        pinned = host.pin_memory()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        pinned.to(dev, non_blocking=True)
        torch.cuda.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t2) * 1e3

    def upload():
        fresh = ResidentFeatures(dev, 1 << 30, op_dtype="f16", stream=stager.stream)
        fresh._pinned = cache._pinned                                   # (the pinned buffer is kept across movies: not part of a miss)
        return host_ms(lambda: fresh.get("movie", array))

    forms = {"kernel_back_to_back": back_to_back,
             "call_synchronised": lambda: host_ms(lambda: ops.window_gather(resident, row, **kw)),
             "stage_resident": lambda: host_ms(lambda: stager.stage_resident(resident, windows, **GEOMETRY).wait()),
             "host_route": lambda: host_ms(lambda: stager.stage_windows(array, sel_idx).wait()),
             "host_parts": host_parts,
             "movie_upload": upload}
    got = {k: [] for k in forms}
    for r in range(warmup + rounds):
        for k, fn in forms.items():
            v = fn()
            if r >= warmup:
                got[k].append(v)
    want = stager.stage_windows(array, sel_idx).wait()
    have = stager.stage_resident(resident, windows, **GEOMETRY).wait()
    torch.cuda.synchronize()
    med = lambda xs: statistics.median(xs)                               # noqa: E731
    out = dict(L=L, d=d, source=str(np.dtype(src)), windows=len(windows), of_windows=W, frames=F, bytes_read=in_bytes, bytes_written=out_bytes,
               bit_equal_to_host_route=bool(torch.equal(want.view(torch.int16), have.view(torch.int16))))
    for k in ("kernel_back_to_back", "call_synchronised", "stage_resident", "host_route", "movie_upload"):
        out[k + "_ms"] = dict(median=med(got[k]), min=min(got[k]), max=max(got[k]))
    out["host_gather_cast_ms"] = med([p[0] for p in got["host_parts"]])
    out["host_copy_ms"] = med([p[1] for p in got["host_parts"]])
    kernel_s = out["kernel_back_to_back_ms"]["median"] * 1e-3
    out["kernel_bytes_per_s"] = (in_bytes + out_bytes) / kernel_s
    out["kernel_fraction_of_achievable_6.3TBps"] = out["kernel_bytes_per_s"] / ACHIEVABLE
    out["host_over_resident_end_to_end"] = out["host_route_ms"]["median"] / out["stage_resident_ms"]["median"]
    saved = out["host_route_ms"]["median"] - out["stage_resident_ms"]["median"]
    out["break_even_queries"] = out["movie_upload_ms"]["median"] / saved if saved > 0 else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "window_gather.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--lengths", type=int, nargs="+", default=[18000, 36000])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_gather_prof: needs the GPU (no timing is taken on a CPU)")
    hip.set_flavour("f16")
    dev = torch.device("cuda:0")
    stager = WindowStager(dev, op_dtype="f16")
    cases = []
    for L in args.lengths:
        for src in (np.float32, np.float16):
            for n in (100, 1 << 30):
                c = case(dev, stager, L, 768, src, n, args.rounds, args.warmup, args.reps)
                cases.append(c)
                print(json.dumps({k: c[k] for k in ("L", "source", "windows", "kernel_fraction_of_achievable_6.3TBps", "host_over_resident_end_to_end",
                                                     "break_even_queries", "bit_equal_to_host_route")}), flush=True)
    result = dict(device=torch.cuda.get_device_name(0), operand="f16", rounds=args.rounds, warmup=args.warmup, reps=args.reps,
                  host_threads=torch.get_num_threads(), cases=cases)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
