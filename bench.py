"""Benchmark of the hot path: video-segments/sec on the stage-2 100-segment recursion at Vicuna-7B scale.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  (N > 1: launched by the driver as ``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...``)

One "step" = one stage-2 recursion (zoom levels 4/2/1) of one query over this rank's 100 windows
[100 x 256 x 768] of synthetic CLIP features with random-init Vicuna-7B-shaped weights (hash-seeded, generated in
HBM), sampling at T = 0.05, decode length forced to G = 8 (eos disabled: random-init models never emit EOS).
Every step in flight works on its OWN video, query and window permutations (hash-seeded by the step index modulo the steps in
flight), so the prefills batched into one GEMM pass and the rows of a merged decode step are all different.
N ranks (``--gpus N`` without a launcher: this process starts ``torch.distributed.run`` with N ranks as a child and relays rank 0's line):
``--scaling queries`` (default; what "whole node" means here): whole recursions are dealt to the ranks - every rank runs the 1-GPU
pipeline on its own queries (``parallel.LOCAL``), no data-path collective, ONE RCCL all-gather of the per-call proposals at the end of the timed region
(the reference itself shards by query: e2e2.py:221-222).  ``--scaling segments``: a 100*N-window video per step, windows
block-partitioned, CLS rows and proposals exchanged by RCCL all-gathers inside every recursion (per-GPU work fixed).
``--scaling strong``: ONE 100-window recursion per step sharded over the N ranks (100/N windows each, the 7 calls dealt over the
ranks with a rotating start: single-query latency).  Inputs are resident in HBM when the timed region starts.

Prints ONE JSON line (rank 0) with the contract fields (``metric``, ``value``, ``unit``, ``higher_is_better``, ``dtype``, ``ms_per_step``
= milliseconds of one timed step).  A plain run does only what that headline needs: set-up, the untimed settle and W warm-up steps, the
K timed steps, ``--dump-outputs DIR`` and the line.  ``--dump-outputs DIR`` writes the last timed step's record (what a caller of the
recursion receives: inverted entropies, cosine scores, answers as code points, ...) as ``DIR/<name>.npy`` in float64; the inputs are
hash-seeded, so two runs with the same arguments see the same inputs.

``--full`` adds everything else, after the headline's timed region: ``roofline`` (dominant kernel, timed with HIP events on the launch
stream), ``clocks_during_the_timed_region``, ``cpu_baseline`` (the torch-fp32 CPU oracle on a bounded sample, N = 1 only) and the
``extra_measurements`` below.

The timed region is exactly K steps after W warm-up steps (and ``--settle`` untimed steps that belong to the set-up), with
``--streams`` steps in flight whose generates decode through one ``serve.DecodeServer`` (``--merge-decode``: shared KV pool,
every decode step ONE pass over the LLM weights for the rows of all steps in flight; records identical to running them one
by one).  ``value`` is the bf16 path, one video per step.  With ``--full``, at N = 1 the same loop is then timed again in
other configurations and reported under ``extra_measurements`` (never ``value``): FP8 decode weights, the full opt-in FP8
LLM path, two different videos batched per step, an EOS id configured (lagging device-side stop flag instead of a forced
length), and the other BASELINE.json workloads (``stage2_long_33``, ``stage1_dense``, ``stage1_sparse``; ``--workload X`` times
one of them alone as the line's ``value``).
"""
import argparse
import contextlib
import json
import math
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_BF16_PEAK_TF = 2500.0  # dense bf16 MFMA peak
METRIC = "video-segments/sec (whole node), stage-2 100-seg recursion, Vicuna-7B"
SENTENCE = ("a person opens the door and walks into the kitchen while another person is sitting at the table "
            "reading a newspaper and then both of them leave the room together")   # 20 words: with the v1 template P = 72 ids


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)        # (the driver's flags: a bare `python bench.py` measures what BENCH_rNN.json holds; 90 s in all)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--workload", default="stage2_long_100", choices=["stage2_long_100", "stage2_long_33", "stage1_dense", "stage1_sparse"],
                   help="BASELINE.json configuration timed as the line's value (default: the one the metric is quoted on)")
    p.add_argument("--scaling", default="queries", choices=["queries", "segments", "weak", "strong"],
                   help="N > 1: queries = whole recursions dealt to the ranks (the 1-GPU pipeline x N, one final all-gather of proposals); "
                        "segments (alias: weak) = 100 windows per rank of a 100*N-window video, two all-gathers per recursion; "
                        "strong = one 100-window recursion sharded over the ranks")
    p.add_argument("--identical-inputs", action="store_true",
                   help="measurement knob: every step in flight works on the SAME video / query / permutations (the round-2 bench; identical rows "
                        "toggle fewer bits and the power-capped GEMMs clock higher)")
    p.add_argument("--cpu-only", action="store_true", help="time the CPU baseline alone (no GPU work) and print its JSON object")
    p.add_argument("--windows", type=int, default=100, help="windows (segments) per GPU (weak) / per recursion (strong)")
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--lq", type=int, default=16)
    p.add_argument("--decode-steps", type=int, default=8)
    p.add_argument("--queries", type=int, default=1, help="queries of the same movie batched per step (contract default: 1)")
    p.add_argument("--streams", type=int, default=20,
                   help="recursions in flight, each on its own HIP stream (workspace slot per stream, weights shared): one recursion's "
                        "HBM-bound decode steps fill the gaps of the other's MFMA-bound adapter / prefill; 1 = strictly one at a time")
    p.add_argument("--merge-decode", type=int, default=1,
                   help="1: the generates of the steps in flight decode through ONE serve.DecodeServer (shared KV pool, merged decode steps: "
                        "one pass over the LLM weights per step for all of them; rows of up to 4 recursions = 28 <= 32)")
    p.add_argument("--pools", type=int, default=2,
                   help="KV pools of the DecodeServer; >= 2 switches on the gang policy: a pool is filled with generates first, then its merged "
                        "steps run with all rows while the next generates prefill into the other pool")
    p.add_argument("--encode-batch", type=int, default=1,
                   help="adapter calls of recursions in flight per rv_clip_encoder call (serve.DecodeServer encode_batch; 1 = every recursion encodes its own windows: the "
                        "default - the adapter alone runs 1.55 / 1.33 / 1.25 ms per recursion at 1 / 4 / 8 to a call, but the K = 20 pipeline measured level: 6262 vs 6267 "
                        "segments/s over four alternations at 1 / 8, DESIGN section 9)")
    p.add_argument("--prefill-batch", type=int, default=8,
                   help="LLM prefills of the steps in flight that may ride in ONE pass (the DecodeServer batches the waiting prefills of identical "
                        "geometry: GEMMs of up to N x 1005 rows); 1 = every step prefills on its own.  8 since round 6 (passes of 8 + 8 + 4 at K = 20: 6476 / 6470 / 6490 "
                        "against 6325 / 6351 / 6382 segments/s at 4, three alternations on one box; rounds 3 - 5 measured 8 level with 4)")
    p.add_argument("--pool-rows", type=int, default=0,
                   help="rows of a KV pool (<= 32: the weight-streaming decode kernel; 33 .. 144: the split-K kernel with LDS-shared activations); "
                        "0 = one gang for all the steps in flight: rows of a recursion (7) x min(streams, steps, 20) = 140 rows at --steps 20")
    p.add_argument("--eos", action="store_true", help="configure a real EOS id (2): the decode loop polls a lagging device-side stop flag")
    p.add_argument("--fp8-decode", action="store_true",
                   help="extra measurement (NOT the headline): decode steps stream FP8 (e4m3fn, per-row scale) weight copies - half the bytes")
    p.add_argument("--fp8-prefill", action="store_true",
                   help="extra measurement (NOT the headline): prefill GEMMs run FP8 x FP8 (activations quantised per row on the fly)")
    p.add_argument("--parity", action="store_true",
                   help="extra measurement (NOT the headline): the PARITY precision (engine option precision = 1: split-bf16 GEMM operands against "
                        "K-duplicated weights; the mode whose scores meet the north star's 1e-3 against the fp32 reference)")
    p.add_argument("--gemm-waves", type=int, default=0, choices=(0, 4, 8), help="waves per workgroup of the persistent prefill GEMMs (0 = the library default; see include/revision_hip.h)")
    p.add_argument("--gemm-cus", type=int, default=0, help="CUs the persistent prefill GEMMs occupy (0 = all); with --streams 2 the rest stay free for the other recursion's decode")
    p.add_argument("--s1-inflight", type=int, default=128,
                   help="stage-1 workloads: one-row generates (windows) in flight; they share KV pools of min(this, 128) rows, so a merged decode step serves "
                        "that many windows per pass over the weights (round 3: 32)")
    p.add_argument("--s1-prefill-batch", type=int, default=0, help="stage-1 workloads: prefills per pass (0 = 8 for stage1_sparse: 8 x 72 rows, 6 for stage1_dense: 6 x 327 rows = 8 row tiles)")
    p.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE", help="rv_ctx_set_option KEY VALUE on the engine (measurement knob, repeatable): e.g. --opt gemm_mhalf=0")
    p.add_argument("--gemm-variant", type=int, default=2, help="rv_ctx_set_option gemm_tile_variant (2 = auto; 6 = ring kernel only: measurement knob)")
    p.add_argument("--settle", type=int, default=16,
                   help="untimed steps run as part of the set-up, before the W warm-up steps (a fresh box starts at idle clocks; ~0.5 s)")
    p.add_argument("--host-profile", action="store_true",
                   help="measurement knob: cProfile the host side of the timed region and print the top entries to stderr (the line's value then includes the profiler's overhead)")
    p.add_argument("--op-dtype", default=None, choices=["f16", "bf16"],
                   help="operand flavour of the library (default: the package default, fp16 - the build that meets the north star's 1e-3; bf16 = the "
                        "reference's own GPU dtype).  At N = 1 the other flavour is timed as an extra leg after the headline.")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-extras", action="store_true", help="skip the extra legs timed AFTER the headline")
    p.add_argument("--cpu-full", action="store_true",
                   help="CPU baseline = the whole recursion (7 calls x (100 segment encodings + prefill + G decode steps), 32 layers) through the "
                        "oracle, 1 warm-up + 3 repeats, median (minutes); default: ONE such call timed once, x 7 identical calls")
    p.add_argument("--cpu-sample", action="store_true", help="CPU baseline from a sample (16 segments, 4 of 32 layers), labelled extrapolated")
    p.add_argument("--full", action="store_true",
                   help="also measure what the headline does not need, after its timed region: roofline legs, clocks, the CPU baseline, the extra legs "
                        "(N = 1) or the other scaling modes and the same-box N = 1 reference (N > 1); --no-extras / --no-cpu-baseline still drop parts")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's outputs (rank 0) as DIR/<name>.npy, float64")
    return p.parse_args()


class ClockSampler:
    """Shader clock (MHz) and socket power (W) of the benchmarked GPU, sampled from sysfs by a host thread while a leg runs - no GPU call, no
    child process: ``/sys/class/drm/card*/device/hwmon/hwmon*/{freq1_input,power1_input}`` (Hz / microwatts; what ``rocm-smi --showclocks
    --showpower`` prints).  The card is the one whose PCI address matches the torch device; a box that hides sysfs gives ``available: false``."""

    def __init__(self, dev, period=0.05):
        import glob
        self.period, self.samples, self._stop, self._thread = period, [], None, None
        want = None
        try:
            pr = torch.cuda.get_device_properties(dev)
            want = "%04x:%02x:%02x" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        except Exception:  # noqa: BLE001
            pass
        cands = []
        for h in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*")):
            if os.path.exists(os.path.join(h, "freq1_input")):
                addr = os.path.basename(os.path.realpath(os.path.join(h, "..", "..")))
                cands.append((h, addr))
        match = [h for h, addr in cands if want and addr.lower().startswith(want)]
        self.paths = match or [h for h, _ in cands]
        self.matched = bool(match)

    def _read(self):
        best = None
        for h in self.paths:     # (PCI match: one path; otherwise the busiest visible card)
            try:
                f = int(open(os.path.join(h, "freq1_input")).read()) / 1e6
                pw = int(open(os.path.join(h, "power1_input")).read()) / 1e6
            except Exception:  # noqa: BLE001
                continue
            if best is None or pw > best[1]:
                best = (f, pw)
        return best

    def __enter__(self):
        import threading
        self.samples = []
        if self.paths:
            self._stop = threading.Event()

            def loop():
                while not self._stop.is_set():
                    r = self._read()
                    if r is not None:
                        self.samples.append(r)
                    self._stop.wait(self.period)
            self._thread = threading.Thread(target=loop, daemon=True)
            self._thread.start()
        return self

    def __exit__(self, *exc):
        if self._thread is not None:
            self._stop.set()
            self._thread.join()
        return False

    def summary(self):
        if not self.samples:
            return {"available": False}
        f = sorted(s_[0] for s_ in self.samples)
        p = sorted(s_[1] for s_ in self.samples)
        n = len(f)
        return {"available": True, "samples": n, "sclk_mhz_mean": sum(f) / n, "sclk_mhz_median": f[n // 2], "sclk_mhz_min": f[0], "sclk_mhz_max": f[-1],
                "power_w_mean": sum(p) / n, "power_w_max": p[-1], "source": "sysfs hwmon freq1_input / power1_input, %d ms period%s" % (int(self.period * 1e3), "" if self.matched else " (busiest visible card: no PCI match)")}


def event_time_ms(fn, iters, warm=3):
    """Average duration of ``fn`` (one kernel launch) with HIP events on torch's current stream = the launch stream."""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def roofline_legs(model, n_calls, M, dec_rows=None, prefill_groups=1):
    """Time the path's heavy kernels in isolation on the shapes the recursion launches them with
    (M = rows of the prefill GEMM batch: shared prompt prefix once + the rest of every call)."""
    from revisionllm_amd import hip, ops
    eng, s = model.engine, model.shape
    dev = eng.device
    OP = eng.op_dtype
    legs = {}
    # (1) prefill gate/up GEMM + SiLU*mul epilogue: [M,4096] x [22016,4096]^T  (MFMA-bound); M = the rows of one prefill pass of the timed
    #     region: prefill_groups steps' prefills ride together (serve.DecodeServer, rv_llm_prefill_pool_groups)
    M = M * prefill_groups
    x = torch.randn(M, s.hidden, device=dev).to(OP)
    w = eng.weight("llm.L0.wgu")
    out = torch.empty(M, s.inter, dtype=OP, device=dev)
    event_time_ms(lambda: ops.gemm(x, w, act=hip.RV_ACT_SILU_MUL, out=out, w_packed=True, ctx=eng), 20)     # (clock settles under the power limit)
    ms = event_time_ms(lambda: ops.gemm(x, w, act=hip.RV_ACT_SILU_MUL, out=out, w_packed=True, ctx=eng), 64)
    # the clock this kernel sustains: the hwmon sensors refresh every few tens of ms, so they are read over a 0.4 s run of the same launches
    smp = ClockSampler(dev, period=0.02)
    with smp:
        ms_long = event_time_ms(lambda: ops.gemm(x, w, act=hip.RV_ACT_SILU_MUL, out=out, w_packed=True, ctx=eng), 640, warm=0)
    flops = 2.0 * M * s.hidden * 2 * s.inter
    # M <= 8192 rows: the persistent 256x256x64 ping-pong kernel (one 512-thread workgroup per CU), whole panels + stream-K tail
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    legs["prefill_gateup_gemm"] = dict(kernel="gemm_pp_sk<1,2,0,4,0>", bound="mfma", ms=ms, achieved=flops / ms / 1e9,
                                       peak=MFMA_BF16_PEAK_TF, unit="TFLOP/s", algorithmic=flops, grid_threads=(cus & ~7) * 512, rows=M,
                                       prefills_per_launch=prefill_groups, clocks=dict(smp.summary(), avg_launch_ms_over_the_sampled_run=ms_long))
    # (2) decode gate/up weight-streaming projection: reads W [22016,4096] bf16 once  (HBM-bound); rotate layers so the
    #     256 MB infinity cache cannot serve the weights.  rows = what a merged decode step of the timed region carries (gang policy:
    #     a full pool of generates): <= 16 rows: the 512-thread kernel, 17 .. 32: two MFMA column blocks per weight fragment on
    #     256-thread workgroups, 33 .. 144: the split-K kernel with LDS-shared activations (gemm_rows.hip, fragment-packed rows)
    dec_rows = dec_rows or n_calls
    ws = [eng.weight(f"llm.L{i}.wgu") for i in range(s.layers)]
    state = {"i": 0}
    nbytes = 2.0 * s.hidden * 2 * s.inter
    if dec_rows <= 32:
        xs = torch.randn(dec_rows, s.hidden, device=dev).to(OP)
        outs = torch.empty(dec_rows, s.inter, dtype=OP, device=dev)

        def gemv():
            ops.gemm(xs, ws[state["i"] % len(ws)], act=hip.RV_ACT_SILU_MUL, out=outs, w_packed=True, ctx=eng)
            state["i"] += 1
        kname = "gemv_stream<2,1,2,1,0,3,2,4>" if dec_rows > 16 else "gemv_stream<2,1,2,1,0,2,1,8>"
        gthreads = (2 * s.inter // 32) * (256 if dec_rows > 16 else 512)
    else:
        f = eng.lib.rv_gemm_rows
        mbp = ops.xp_blocks(dec_rows)
        xs = (torch.randn(mbp * 16 * s.hidden, device=dev) * 0.1).to(OP)          # fragment-packed rows (any values: timing)
        outs = torch.empty(mbp * 16 * s.inter, dtype=OP, device=dev)
        planes = torch.zeros(40 << 20, dtype=torch.uint8, device=dev)
        arrive = torch.zeros(4096, dtype=torch.int32, device=dev)

        def gemv():
            rc = f(hip.ptr(xs), hip.ptr(ws[state["i"] % len(ws)]), None, hip.ptr(outs), dec_rows, 2 * s.inter, s.hidden, hip.ptr(planes), hip.ptr(arrive),
                   hip.RV_ACT_SILU_MUL, hip.dtype_code(outs), hip.stream())
            assert rc == 0, hip.last_error()
            state["i"] += 1
        # what rows_splits / rows_by_split (gemm_rows.hip) pick for this shape (344 column groups): 4 row blocks: one workgroup per group;
        # 5: 4 splits = 1376 items on a persistent grid of 2 workgroups per CU; 8 / 9: 2 splits = 688 items, one workgroup per CU
        cgs, slots = 2 * s.inter // 64, (cus & ~7) * (2 if mbp <= 5 else 1)
        split = 1 if mbp == 4 else 4 if mbp == 5 else 2
        pers = split > 1 and cgs * split > slots
        kname = f"rows_kernel{'_p' if pers else ''}<{mbp},{8 // split},1,1>"
        gthreads = (slots if pers else cgs * split) * 320
    ms = event_time_ms(gemv, 64, warm=4)
    legs["decode_gateup_gemv"] = dict(kernel=kname, bound="hbm", ms=ms, achieved=nbytes / ms / 1e6, peak=HBM_PEAK_GBS, unit="GB/s", algorithmic=nbytes,
                                      rows=dec_rows, grid_threads=gthreads, timing="64 back-to-back launches of this kernel alone (layers rotated); "
                                      "inside a decode step it runs between dependent launches: see decode_step and in_step")
    # (2b) one whole merged decode step at that row count, as rv_llm_decode_rows runs it (32 blocks x (qkv+RoPE, attention, o, gate/up, down) +
    #      lm_head), rows at position ~ prompt + 4: algorithmic bytes = every weight once (6.607e9 x 2 B) + the rows' K / V
    R = dec_rows
    pos_at = 175
    pool, smax = eng.new_kv_pool(R, 192)
    pos = torch.full((R,), pos_at, dtype=torch.int32, device=dev)
    hrow = (torch.randn(R, s.hidden, device=dev) * 0.02)
    lg = torch.empty(R, s.vocab, dtype=torch.float32, device=dev)
    prev_slot, eng.slot = eng.slot, 170
    try:
        # rows in groups of n_calls (the calls of one recursion) share the 32-position prompt prefix, as in the pipeline (serve.DecodePool.join)
        share = (torch.tensor([(r_ // n_calls * n_calls) | (32 << 16) for r_ in range(R)], dtype=torch.int32, device=dev) if n_calls > 1 and R % n_calls == 0 else None)
        ms = event_time_ms(lambda: eng.llm_decode_rows(hrow, pos, pool, smax, logits=lg, row_share=share), 12, warm=3)
    finally:
        eng.slot = prev_slot
    step_bytes = 6.607e9 * 2 + 2.0 * s.layers * (pos_at + 1) * s.hidden * 2 * R
    legs["decode_step"] = dict(kernel="rv_llm_decode_rows (one merged step, all its launches)", bound="hbm", ms=ms, achieved=step_bytes / ms / 1e6, peak=HBM_PEAK_GBS,
                               unit="GB/s", algorithmic=step_bytes, rows=R, grid_threads=0)
    del pool, lg
    # (3) the "feature scan": dense nn.Linear(768 -> 4096) projector over 100 segments x 256 frames (stage1_dense adapter);
    #     algorithmic bytes = features in + tokens out (2.49 MB / segment), weights (6.3 MB) amortised.
    #     Kernel: the A-resident GEMM (gemm_arows.hip): rows resident in LDS, A read once, C written once
    if "proj.w" not in eng._keep:
        eng.init_synthetic(seed=0, llm=False, clip=False, linear=True)
    xf = torch.randn(100 * 256, 768, device=dev).to(OP)
    ms = event_time_ms(lambda: eng.project_dense(xf, OP), 20)
    nbytes = xf.numel() * 2 + 100 * 256 * s.hidden * 2
    legs["dense_projector_scan"] = dict(kernel="gemm_arows_kernel<1,0,7,2>", bound="hbm", ms=ms, achieved=nbytes / ms / 1e6, peak=HBM_PEAK_GBS,
                                        unit="GB/s", algorithmic=nbytes, grid_threads=cus * 512,
                                        tflops=2.0 * 100 * 256 * 768 * s.hidden / ms / 1e9)
    # (4) the adapter's widest K = 768 GEMM (FFN-1 + ReLU over 100 x 257 rows), MFMA-bound
    xa = torch.randn(100 * 257, 768, device=dev).to(OP)
    if "adp.enc.0.w1" in eng._keep:
        w1, b1 = eng.weight("adp.enc.0.w1"), eng.weight("adp.enc.0.b1")
        oa = torch.empty(xa.shape[0], w1.shape[0], dtype=OP, device=dev)
        ms = event_time_ms(lambda: ops.gemm(xa, w1, bias=b1, act=hip.RV_ACT_RELU, out=oa, w_packed=True, ctx=eng), 20)
        fl = 2.0 * xa.shape[0] * 768 * w1.shape[0]
        legs["adapter_ffn1_gemm"] = dict(kernel="gemm_arows_kernel<1,1,7,2>", bound="mfma", ms=ms, achieved=fl / ms / 1e9, peak=MFMA_BF16_PEAK_TF,
                                         unit="TFLOP/s", algorithmic=fl, grid_threads=cus * 512)
    return legs


def committed_profile(name):
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return json.load(f)


def pmc_traffic(kernel, grid_threads):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC summary (separate FETCH_SIZE /
    WRITE_SIZE passes, gfx950 x2 correction on FETCH_SIZE; tools/pmc_summary.py).  None if no summary matches."""
    want = kernel.replace(" ", "")
    for fname in ("r6_pmc_traffic.json", "r5_pmc_traffic.json", "r4_pmc_traffic.json", "r3_pmc_traffic.json", "r2_pmc_traffic.json", "r1_pmc_traffic.json"):
        d = committed_profile(fname)
        if d is None:
            continue
        for row in d["kernels"]:
            if row["kernel"].replace(" ", "") == want and row["grid_threads"] == grid_threads:
                return row["traffic_bytes_per_launch"]
    return None


def host_cpu():
    cores = os.cpu_count() or 1
    try:
        import psutil
        cores = psutil.cpu_count(logical=False) or cores
    except Exception:  # noqa: BLE001
        pass
    # the cores this process may use: a shared host hands a job a slice of its cores (affinity mask, OMP_NUM_THREADS), and a thread
    # pool sized by the whole host only slows itself down
    try:
        cores = min(cores, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and int(omp) > 0:
        cores = min(cores, int(omp))
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except Exception:  # noqa: BLE001
        pass
    return cores, model


def cpu_baseline(args, n_calls, P):
    """The torch-fp32 CPU oracle (CPU restatement of load_pretrained_model -> inference) on the host cores, as the reference
    executes the recursion: every call re-encodes its 100 video tokens (zoom duplicates included), then prefill + G decode steps.

    default     ONE full call (ClipEncoder on all 100 segment rows + prefill S + G decode steps, all 32 layers) timed once after
                a one-layer warm-up; recursion = 7 such calls (identical work per call): bounded to ~10-30 s of CPU work
    --cpu-full  the whole recursion through ``oracle.sampling.generate`` (7 calls), 1 warm-up + 3 repeats, median
    --cpu-sample  16 segments, 4 of 32 layers, scaled up: labelled extrapolated
    Weights are random normal of the reference's shapes (timing only), generated with torch (multi-threaded)."""
    from oracle import llama as o_llama
    from oracle import sampling as o_sampling
    from revisionllm_amd.utils import synth
    torch.set_grad_enabled(False)
    cores, cpu_model = host_cpu()
    torch.set_num_threads(cores)
    seed, W, Tn, G = args.seed, args.windows, args.frames, args.decode_steps
    L = 4 if args.cpu_sample else 32
    ns = 16 if args.cpu_sample else W
    gen = torch.Generator().manual_seed(seed)
    shape = synth.LlamaShape(layers=L)
    cfg = o_llama.LlamaCfg(layers=L)
    w = {}
    for name, shp, a, base in synth.llama_spec(shape):
        w[name] = torch.empty(shp).normal_(0, 0.02, generator=gen) if len(shp) > 1 else torch.ones(shp)
    wa = {}
    for name, shp, a, base in synth.clip_encoder_spec():
        if len(shp) > 1:
            wa[name] = torch.empty(shp).normal_(0, a / 1.732, generator=gen)
        else:
            wa[name] = torch.ones(shp) if ("norm" in name and "weight" in name) else torch.zeros(shp)
    feat = torch.empty(ns, Tn, 768).normal_(generator=gen)
    q = (torch.empty(1, args.lq, 768).normal_(generator=gen), torch.ones(1, args.lq))
    ids = torch.from_numpy(synth.synthetic_prompt_ids(P, 40, seed))[None]

    def one_call(n_layers=None):
        """One LLM call as inference() drives it: adapter on the call's video rows, splice, prefill, G - 1 decode steps."""
        t0 = time.perf_counter()
        tm = {}
        o_sampling.generate(ids, feat[None], q, w, wa, cfg, adapter_kw=dict(hierarchy=True), do_sample=True, temperature=0.05, top_k=50,
                            max_new_tokens=G, eos_token_id=-1, uniforms=torch.full((G, 1), 0.5), n_layers=n_layers, timings=tm)
        stage_log.append(tm)
        return time.perf_counter() - t0

    stage_log = []

    def stage_split(calls):
        """Seconds per stage summed over the given calls' timing dicts (adapter = ClipEncoder on the call's rows + splice)."""
        return {k: round(sum(c[k] for c in calls), 2) for k in ("adapter", "prefill", "decode")}

    info = dict(unit="segments/s", cores=cores, cpu=cpu_model, kind="port")
    if args.cpu_full and not args.cpu_sample:
        def recursion():
            return sum(one_call() for _ in range(n_calls))
        recursion()
        del stage_log[:]
        times = [recursion() for _ in range(3)]
        t_rec = statistics.median(times)
        med = times.index(t_rec)
        info.update(value=W / t_rec, extrapolated=False, repeats=3, stage_seconds=stage_split(stage_log[med * n_calls:(med + 1) * n_calls]),
                    sample=f"torch-fp32 oracle, whole recursion as the reference executes it: {n_calls} calls x (ClipEncoder on {W} segment rows + "
                           f"prefill + {G - 1} decode steps, 32 layers), 1 warm-up + 3 repeats, median {t_rec:.1f} s (all: {[round(t, 1) for t in times]})")
        return info
    one_call(n_layers=1)                               # warm-up: thread pool, allocator, one layer's pass
    del stage_log[:]
    t_call = one_call()
    if args.cpu_sample:
        t_rec = n_calls * t_call * (32.0 / L) * (W / ns)
        info.update(value=W / t_rec, extrapolated=True,
                    sample=f"torch-fp32 oracle SAMPLE: one call with {ns} of {W} segment rows through {L} of 32 layers ({t_call:.2f} s), scaled "
                           f"x{32 // L} (layers) x{W // ns} (segments) x{n_calls} (calls): extrapolated, an upper bound on the time, indicative only")
        return info
    t_rec = n_calls * t_call
    info.update(value=W / t_rec, extrapolated="x%d identical calls" % n_calls, repeats=1,
                stage_seconds_per_call=stage_split(stage_log), full_run="profiles/r4_cpu_full.json (--cpu-full: all calls, 3 repeats, median)",
                sample=f"torch-fp32 oracle: ONE full call of the recursion as the reference executes it (ClipEncoder on {W} segment rows x {Tn} frames, "
                       f"prefill S={P - 1 + W}, {G - 1} KV-cached decode steps, all 32 layers; driven through oracle.sampling.generate = the CPU "
                       f"restatement of inference()) timed once after a one-layer warm-up: {t_call:.1f} s; recursion = {n_calls} such calls "
                       f"= {t_rec:.1f} s.  --cpu-full runs all {n_calls} calls, 3 repeats, median")
    return info


def dump_outputs(path, rec):
    """``--dump-outputs``: what the timed path handed its caller in the last timed step, one float64 ``<name>.npy`` per array under
    ``path``.  A stage-2 record: per call (in plan order) the inverted entropies, the window group (start, zoom), the answer as unicode
    code points (-1 padded) and the window indexes, plus the proposals' cosine scores (rank 0's own record at N > 1).  A stage-1
    workload: every tensor of the last generate's output."""
    import numpy as np
    arrays = {}
    if isinstance(rec, dict) and "answers" in rec:
        for k in ("max_entropy", "mean_entropy", "score_cos", "starts", "hierarchy_zooms"):
            arrays[k] = np.asarray(rec[k], dtype=np.float64)
        n = max([len(a) for a in rec["answers"]] + [1])
        arrays["answers_codepoints"] = np.array([[ord(c) for c in a] + [-1] * (n - len(a)) for a in rec["answers"]], dtype=np.float64).reshape(-1, n)
        arrays["window_indexes"] = np.concatenate([np.asarray(i, dtype=np.float64).ravel() for i in rec["indexes"]])
    else:
        for k, v in rec.items():
            if isinstance(v, (list, tuple)) and v and all(torch.is_tensor(t) for t in v):
                v = torch.stack(list(v))
            if torch.is_tensor(v):
                arrays[k] = v.detach().cpu().double().numpy()
    total = sum(a.nbytes for a in arrays.values())
    if total > 64 << 20:
        raise RuntimeError(f"bench: --dump-outputs would write {total} bytes (limit 64 MiB)")
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), a)


def spawn_ranks(args):
    """``python bench.py --gpus N`` without a launcher: start N ranks with ``torch.distributed.run`` as a CHILD process (this
    process has not touched the GPU), relay what it prints and return its exit status."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def main():
    args = parse()
    if args.scaling == "weak":
        args.scaling = "segments"
    if args.cpu_only:
        from revisionllm_amd.eval import stage2
        print(json.dumps({"cpu_baseline": cpu_baseline(args, len(stage2.plan_groups(100, 100)), 72)}), flush=True)
        return 0
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return spawn_ranks(args)
    # The contract is ONE JSON line on rank 0's stdout.  Libraries write there too (RCCL's version banner sits in a stdio buffer and comes out at process exit,
    # i.e. BEHIND the line): from here on descriptor 1 is stderr, and the line goes to the saved descriptor.
    sys.stdout.flush()
    line_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s) (WORLD_SIZE); start it as "
                         f"`python bench.py --gpus {world}` or with torch.distributed.run --nproc-per-node {args.gpus}")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    import torch.distributed as dist
    backend = os.environ.get("REVISION_DIST_BACKEND", "nccl")   # "gloo": plumbing smoke test with several ranks on one GPU
    local = local % max(torch.cuda.device_count(), 1)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
        else:
            dist.init_process_group(backend)
    dev = torch.device(f"cuda:{local}")
    torch.cuda.set_device(dev)
    if world > 1:
        # the communicator must reach every rank before anything is timed: counted by a collective, not assumed from the environment
        one_ = torch.ones(1, device=dev)
        dist.all_reduce(one_)
        if int(one_.item()) != world or dist.get_world_size() != world:
            sys.stderr.write(f"bench: the process group reaches {int(one_.item())} rank(s) of a group of {dist.get_world_size()}, expected {world}\n")
            dist.destroy_process_group()
            return 3

    from revisionllm_amd import ops, parallel, sched
    from revisionllm_amd.eval import stage2
    from revisionllm_amd.inference import _prompt_ids
    from revisionllm_amd.model import ReVisionLlamaForCausalLM
    from revisionllm_amd.utils import synth

    def hier_args(**kw):
        d = dict(clip_adapter=True, cross_attn=False, clip_adapter_text=True, clip_adapter_feature="cls", hierarchy=True,
                 adapter_input_dim=768, pretrain_clip_adapter=None, pretrain_mm_mlp_adapter=None)
        d.update(kw)
        return SimpleNamespace(**d)

    from revisionllm_amd import hip
    if args.op_dtype:
        hip.set_flavour(args.op_dtype)
    OP = hip.op_dtype()             # torch dtype of the 16-bit operands (features, weights, activation copies, KV caches)
    DT = {"f16": "fp16", "bf16": "bf16"}[hip.flavour()]     # the line's `dtype`: the arithmetic type of the GEMM / attention operands (f32 accumulation, f32 residual stream)
    model = ReVisionLlamaForCausalLM(synth.VICUNA_7B, device=dev)
    model.get_model().initialize_vision_modules(hier_args())
    eng = model.engine
    headline = args.workload == "stage2_long_100"
    # extra legs (--full, single GPU, after the headline's timed region).  The FP8 copies are resident from the start and switched off
    # for the headline.
    extras = (args.full and world == 1 and headline and not args.no_extras and not args.fp8_decode and not args.fp8_prefill and args.queries == 1
              and not args.eos)
    eng.init_synthetic(seed=args.seed, llm=True, clip=True, fp8_decode=args.fp8_decode or extras, fp8_prefill=args.fp8_prefill or extras,
                       parity=extras or args.parity)
    eng.set_option("precision", 1 if args.parity else 0)
    eng.set_option("fp8_decode", 1 if args.fp8_decode else 0)
    eng.set_option("fp8_prefill", 1 if args.fp8_prefill else 0)
    eng.set_option("gemm_cus", args.gemm_cus)
    if args.gemm_waves:
        eng.set_option("gemm_waves", args.gemm_waves)
    shared_gpu = world > max(torch.cuda.device_count(), 1)
    if shared_gpu:
        # plumbing run (several ranks on ONE GPU, e.g. REVISION_DIST_BACKEND=gloo on a 1-GPU box): the persistent stream-K prefill GEMMs
        # wait in-kernel for ALL their workgroups, and two PROCESSES on one device would each hold half the CUs - output-tiled kernels only
        args.gemm_variant = 6
    eng.set_option("gemm_tile_variant", args.gemm_variant)
    for kv in args.opt:
        k_, v_ = kv.split("=", 1)
        eng.set_option(k_, int(v_))
    model.generation_config.eos_token_id = 2 if args.eos else None     # None: forced decode length
    tok = synth.FakeTokenizer()
    G = args.decode_steps

    # ---------------------------------------------------------------- stage-2 recursion workloads -------------------------------------
    strong = args.scaling == "strong" and world > 1
    by_query = args.scaling == "queries" and world > 1       # whole recursions per rank: the 1-GPU pipeline on every rank
    batch = 33 if args.workload == "stage2_long_33" else 100
    W = (33 if args.workload == "stage2_long_33" else args.windows) * (1 if (strong or by_query) else world)
    lo, hi = (0, W) if by_query else parallel.shard_bounds(W, rank, world)
    Wl, Tn = hi - lo, args.frames
    # queries mode: the recursion's own "world" is this rank alone (parallel.LOCAL: the sharded driver then issues no collective and no
    # sub-communicator exists)
    own_group = parallel.LOCAL if by_query else None
    plan = stage2.plan_groups(W, batch)
    torch.manual_seed(args.seed + (rank if by_query else 0))      # the device-side sampling draws (torch.rand in generate)

    def hashed(shape, dtype, name):
        return ops.init_hash_(torch.empty(*shape, dtype=dtype, device=dev), name, args.seed, synth.SQRT3)

    def input_set(k, nq=1, W_=None, Wl_=None, batch_=None, per_rank=None):
        """The inputs of step k: ``nq`` recursions, each over its OWN video (this rank's windows of it), with its own query tokens,
        query CLS feature, sentence (same word count: the prompts keep one geometry, the token ids differ) and window permutations.
        Queries / permutations are identical on all ranks when a recursion is sharded over them (segments / strong), per-rank in
        queries mode; k = 0 of rank 0 reproduces the round-2 bench's single input."""
        W_, Wl_, batch_ = W_ or W, Wl_ or Wl, batch_ or batch
        per_rank = by_query if per_rank is None else per_rank      # queries / permutations per rank (queries mode) or identical on all ranks
        qtag = f".r{rank}" if per_rank else ""
        tag = "" if k == 0 else f".s{k}"
        plan_ = stage2.plan_groups(W_, batch_)
        g = torch.Generator().manual_seed(args.seed * 100003 + k * 17 + (rank * 7919 if per_rank else 0))
        feats_ = [hashed((Wl_, Tn, 768), OP, f"bench.feat{i if nq > 1 else ''}{'' if W_ == W else W_}.r{rank}{tag}") for i in range(nq)]
        sent = SENTENCE if k == 0 else SENTENCE.replace("kitchen", f"kitchen{k}").replace("newspaper", f"newspaper{k}")
        qs = [(hashed((args.lq, 768), OP, f"bench.q{i if nq > 1 else ''}{qtag}{tag}"),
               hashed((768,), torch.float32, f"bench.qcls{i if nq > 1 else ''}{qtag}{tag}"), sent) for i in range(nq)]
        return {"qs": qs, "perms": [stage2.make_perms(plan_, g, W=W_) for _ in range(nq)], "feats": feats_ if nq > 1 else feats_[0]}

    n_sets = 1 if args.identical_inputs else max(1, args.streams)
    sets_cache = {}

    def input_sets(nq=1, **kw):
        key = (nq, tuple(sorted(kw.items())))
        if key not in sets_cache:
            sets_cache[key] = [input_set(k, nq, **kw) for k in range(n_sets)]
        return sets_cache[key]
    qf, qc = input_sets()[0]["qs"][0][:2]
    stages = parallel.HipStages(model, tok)
    server = None
    if args.merge_decode:
        from revisionllm_amd import serve
        if not args.pool_rows:      # one merged decode pass for everything in flight: the weights stream once per step for all of it
            rows_rec = len(stage2.plan_groups(W, batch)) * args.queries
            args.pool_rows = rows_rec * max(1, min(args.streams, args.steps, 144 // rows_rec))
        server = serve.DecodeServer(model, rows=args.pool_rows, smax=192 if batch + 72 + G <= 192 else 256, gmax=max(16, G), pools=args.pools, gang=args.pools > 1,
                                    prefill_batch=args.prefill_batch, encode_batch=args.encode_batch)
        stages.server = server

    work = {"sets": input_sets(args.queries), "W": W, "batch": batch, "G": G, "group": own_group, "by_query": by_query}
    streams = [torch.cuda.Stream(dev) for _ in range(max(1, args.streams))] if args.streams > 1 else None
    counter = {"i": 0}
    inter = sched.Interleaver(servers=[server] if server is not None else ())

    def launch():
        """Start one step as a scheduler task bound to the next HIP stream / workspace slot."""
        s_ = work["sets"][counter["i"] % len(work["sets"])]
        kw = dict(batch=work["batch"], perms=s_["perms"], max_new_tokens=work["G"], group=work["group"])
        def g(task):
            return parallel.launch_queries_sharded_steps(stages, tok, s_["feats"], work["W"], s_["qs"], turn=task, **kw)
        if streams is None:
            counter["i"] += 1
            return inter.add(sched.Task(g, None, eng, 0))
        k = counter["i"] % len(streams)
        counter["i"] += 1
        streams[k].wait_stream(torch.cuda.current_stream(dev))     # inputs written on the caller's stream
        return inter.add(sched.Task(g, streams[k], eng, k))

    def collect(task):
        return parallel.collect_queries(inter.finish(task))[0]

    def run(n):
        """n steps.  A step's device work is enqueued before the previous steps' records are collected (``--streams`` steps in
        flight, each on its own HIP stream), so one step's HBM-bound decode launches fill the gaps of the other's MFMA-bound
        adapter / prefill and the host-side exchange / assembly overlaps device work; every step's work and record are
        produced inside the timed region.  With an EOS id the tasks yield at their stop-flag polls and are resumed round-robin."""
        rec, pending, scores = None, [], []
        depth = max(1, work.get("depth", args.streams))

        def take():
            r = collect(pending.pop(0))
            if work["by_query"]:
                scores.append(r["max_entropy"] + r["mean_entropy"])
            return r
        for _ in range(n):
            pending.append(launch())
            if len(pending) > depth:
                rec = take()
        while pending:
            rec = take()
        if work["by_query"] and scores:
            # the ONE exchange of this mode: the per-call proposals (1/max_entropy, 1/mean_entropy of every call of every recursion this
            # rank ran) all-gathered over RCCL, ordered against the persistent prefill GEMMs like every collective of the path
            mine = torch.tensor(scores, dtype=torch.float32, device=dev)
            work["gathered"] = parallel._gated(stages, world, lambda: parallel._all_gather_cat(mine, None))
        return rec

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    rank_times = {}

    def timed(fn_run, steps=None, warm=None, local=False, tag=None):
        """W warm-up steps, then EXACTLY K steps bracketed by barrier + synchronize; max over ranks.  -> (seconds, last record).
        ``local``: this rank alone (no barrier, no reduction: the N = 1 reference run rank 0 makes while the others wait).
        ``tag``: keep every rank's own time under that name (``rank_times``: the skew the max hides)."""
        sync_ = torch.cuda.synchronize if local else sync
        steps = args.steps if steps is None else steps
        fn_run(args.warmup if warm is None else warm)
        sync_()
        prof = None
        if args.host_profile and rank == 0:
            import cProfile
            prof = cProfile.Profile()
            prof.enable()
        t0 = time.perf_counter()
        rec = fn_run(steps)
        t_host = time.perf_counter() - t0           # all launches made, records collected; the device may still be running
        torch.cuda.synchronize()
        dt_own = time.perf_counter() - t0           # this rank's own work done (before the closing barrier)
        sync_()
        dt = time.perf_counter() - t0
        if prof is not None:
            import pstats
            prof.disable()
            sys.stderr.write(f"[host profile] {steps} steps: host loop {t_host * 1e3:.1f} ms, with the final device sync {dt * 1e3:.1f} ms\n")
            pstats.Stats(prof, stream=sys.stderr).sort_stats("tottime").print_stats(22)
        if world > 1 and not local:
            t = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
            if tag is not None:
                own = torch.tensor([dt_own], device=dev, dtype=torch.float64)
                allt = [torch.zeros_like(own) for _ in range(world)]
                dist.all_gather(allt, own)
                ts = [float(x.item()) for x in allt]
                rank_times[tag] = {"per_rank_seconds": ts, "skew": (max(ts) - min(ts)) / max(ts), "slowest_rank": ts.index(max(ts))}
        return dt, rec

    # ---------------------------------------------------------------- stage-1 workloads (one window per step) --------------------------
    def stage1_runner(kind):
        """stage1_dense: 1 window x 256 frames -> nn.Linear projector -> 256 video tokens (S = P - 1 + 256) -> G decode steps.
        stage1_sparse: 1 window x 1024 frames + query tokens -> ClipEncoder 'cls' -> 1 video token -> G decode steps
        (eval_nlq_negative.py:281-298: windows are the LLM's batch rows; BASELINE configs quote 1 segment)."""
        m1 = ReVisionLlamaForCausalLM(synth.VICUNA_7B, engine=eng)
        if kind == "stage1_dense":
            m1.get_model().initialize_vision_modules(hier_args(clip_adapter=False, clip_adapter_text=False, hierarchy=False))
            if not eng.has_linear:
                eng.init_synthetic(seed=args.seed, llm=False, clip=False, linear=True)
            frames, qfeat = 256, None
        else:
            m1.get_model().initialize_vision_modules(hier_args(hierarchy=False))
            frames = 1024
            qfeat = (qf[None], torch.ones(1, args.lq))
        m1.generation_config.eos_token_id = None
        x = ops.init_hash_(torch.empty(1, frames, 768, dtype=OP, device=dev), f"bench.s1.{kind}", args.seed, synth.SQRT3)
        ids = _prompt_ids("<video>\n" + "During which frames can we see {}?".format(SENTENCE), tok, 1)[0]
        gkw = dict(images=x, query_feats=qfeat, do_sample=True, temperature=0.05, max_new_tokens=G, return_dict_in_generate=True)

        S = ids.shape[1] - 1 + (frames if kind == "stage1_dense" else 1)
        if args.merge_decode and streams is not None:
            # windows in flight share the weight passes like the stage-2 recursions do: one-row generates fill a KV pool of up to 128 rows
            # (gang policy), their prefills ride 6 / 7 to a pass (serve.best_prefill_batch), a merged decode step serves the whole pool
            from revisionllm_amd import serve
            NB = max(1, args.s1_inflight)
            pb1 = args.s1_prefill_batch or (8 if kind == "stage1_sparse" else 6)
            server1 = serve.DecodeServer(m1, rows=min(NB, 128), smax=(S + G + 31) // 32 * 32, gmax=max(16, G), pools=2, gang=True, prefill_batch=pb1,
                                         slot=150)
            inter1 = sched.Interleaver(servers=[server1])
            streams1 = [torch.cuda.Stream(dev) for _ in range(NB)]

            # every window in flight is its OWN window (32 distinct ones, window i of a step group = set i); the adapter of a group of
            # windows runs as ONE call over [group, frames, 768] - the reference's stage-1 driver hands inference() a batch of windows
            # too (eval_nlq_negative.py:281-298) - and each window then decodes as its own one-row generate through the server
            xs = ops.init_hash_(torch.empty(NB, frames, 768, dtype=OP, device=dev), f"bench.s1.{kind}.windows", args.seed, synth.SQRT3)
            enc_stream = torch.cuda.Stream(dev)
            gkw1 = {k_: v_ for k_, v_ in gkw.items() if k_ not in ("images", "query_feats")}

            def run1(n):
                out, pending = None, []
                for base in range(0, n, NB):
                    nb = min(NB, n - base)
                    enc_stream.wait_stream(torch.cuda.current_stream(dev))
                    prev_slot, eng.slot = eng.slot, 31
                    with torch.cuda.stream(enc_stream):
                        qb = None if qfeat is None else (qf[None].expand(nb, -1, -1).contiguous(), torch.ones(nb, args.lq))
                        rows, rps = m1.encode_images(xs[:nb], qb)
                        rows = rows.view(nb, rps, -1)
                        enc_done = torch.cuda.Event()
                        enc_done.record()
                    eng.slot = prev_slot
                    rows.record_stream(enc_stream)
                    for i in range(nb):
                        k = (base + i) % NB
                        streams1[k].wait_event(enc_done)
                        pending.append(inter1.add(sched.Task(m1.generate_steps(ids, video_rows=rows[i], rows_per_sample=rps, server=server1, **gkw1),
                                                             streams1[k], eng, 200 + k)))
                        if len(pending) > NB:
                            out = inter1.finish(pending.pop(0))
                while pending:
                    out = inter1.finish(pending.pop(0))
                eng.slot = 0
                return out
            return run1, dict(prompt_tokens=int(ids.shape[1]), prefill_len=int(S), frames=frames, windows_per_step=1, windows_in_flight=NB,
                              inputs="%d distinct windows in flight" % NB,
                              adapter="one call per group of up to %d windows in flight ([%d, %d, 768] -> %s)" % (NB, NB, frames, "ClipEncoder, CLS out" if kind != "stage1_dense" else "Linear projector"),
                              decode="merged (serve.DecodeServer: %d-row pools, prefills %d to a pass)" % (min(NB, 128), pb1))

        def run1(n):
            out = None
            for i in range(n):
                if streams is not None:
                    k = i % len(streams)
                    eng.slot = k
                    streams[k].wait_stream(torch.cuda.current_stream(dev))
                    with torch.cuda.stream(streams[k]):
                        out = m1.generate(ids, **gkw)
                else:
                    out = m1.generate(ids, **gkw)
            return out
        S = ids.shape[1] - 1 + (frames if kind == "stage1_dense" else 1)
        return run1, dict(prompt_tokens=int(ids.shape[1]), prefill_len=int(S), frames=frames, windows_per_step=1)

    sync()       # weights / inputs were written on the default stream; the step streams do not wait for it implicitly
    headline_clocks = n1_ref = out1 = None
    if args.workload.startswith("stage1"):
        run1, wl_cfg = stage1_runner(args.workload)
        if args.settle > 0:
            run1(args.settle)
            sync()
        dt, out1 = timed(run1)
        if not torch.isfinite(out1["entropy"]).all():
            raise RuntimeError("bench: non-finite entropies")
        value, rec = args.steps * world / dt, None       # (stage-1 workloads: every rank times its own windows)
    else:
        if args.settle > 0:
            # set-up, untimed: at least one whole K-step run, so that every gang shape, pass size, pinned-buffer size and host code path of the timed
            # region has run once (the first process on a fresh box paged parts of them in inside a 10-step timed region: 22.1 vs 18.0 ms per step).
            # Beyond 64 steps the pipeline repeats itself: 64 steps plus the remainder of K over the steps in flight end in the timed region's tail
            # shape, and the set-up stays bounded however long the timed region is
            run(max(args.settle, args.steps if args.steps <= 64 else 64 + args.steps % max(1, args.streams)))
            sync()
        if world > 1 and args.full:
            # the same box's N = 1 value, measured in THIS process tree: rank 0 runs the 1-GPU pipeline alone (its own videos / queries, no collective) while
            # the other ranks wait at the barrier below - the denominator of every per-mode efficiency in this line
            if rank == 0:
                saved_w = dict(work)
                key = ("mode", "n1")
                if key not in sets_cache:
                    sets_cache[key] = [input_set(k, 1, W_=args.windows, Wl_=args.windows, batch_=batch, per_rank=True) for k in range(n_sets)]
                work.update(sets=sets_cache[key], W=args.windows, batch=batch, group=parallel.LOCAL, by_query=False)
                t1, _ = timed(run, local=True)
                n1_ref = {"value": args.windows * args.steps / t1, "unit": "segments/s", "ms_per_step": t1 / args.steps * 1e3,
                          "note": "rank 0 alone, same process tree, before the N-rank timing (the other ranks idle at a barrier)"}
                work.clear()
                work.update(saved_w)
            sync()
        sampler = ClockSampler(dev) if args.full else None
        with sampler or contextlib.nullcontext():
            dt, rec = timed(run, tag="headline")
        headline_clocks = sampler.summary() if sampler is not None else None
        if any(e != e for e in rec["max_entropy"]) or not all(rec["answers"]):
            raise RuntimeError(f"bench: the last record is not finite / empty: {rec['answers']} {rec['max_entropy']}")
        value = W * args.queries * args.steps * (world if by_query else 1) / dt
        wl_cfg = {}
        if by_query and work["gathered"].shape[0] != world * args.steps:
            raise RuntimeError(f"bench: the final all-gather returned {tuple(work['gathered'].shape)} proposals rows for {world} ranks x {args.steps} steps")

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, rec if rec is not None else out1)

    extra = {}
    if args.full and headline and world == 1 and not args.no_extras:
        # SUSTAINED: the headline is a K-step burst (20 steps = 0.3 s: pipeline fill and drain included, clocks not yet settled under the socket power
        # limit).  The same run() for >= 10 s right behind it, with the shader clock and socket power sampled next to it
        try:
            n_sus = max(args.steps, int(10.0 / (dt / args.steps)) + 1)
            with sampler:
                t_sus, _ = timed(run, steps=n_sus, warm=0)
            extra["sustained"] = {"value": W * args.queries * n_sus / t_sus, "unit": "segments/s", "ms_per_step": t_sus / n_sus * 1e3, "steps": n_sus, "seconds": t_sus,
                                  "ratio_to_the_headline": (W * args.queries * n_sus / t_sus) / value, "clocks": sampler.summary(),
                                  "note": "same workload, pipeline, steps in flight and inputs as the headline, run for >= 10 s (the headline keeps the contract's K)"}
        except Exception as e:  # noqa: BLE001 - an extra leg must never cost the headline line
            extra["sustained"] = {"error": f"{type(e).__name__}: {e}"[:300]}
    if extras:
        def leg(name, nq, fp8, fp8p=False, eos=False, merged=True, par=False):
            stages.server = server if merged else None
            work["sets"] = input_sets(nq)
            eng.set_option("fp8_decode", int(fp8))
            eng.set_option("fp8_prefill", int(fp8p))
            eng.set_option("precision", int(par))
            model.generation_config.eos_token_id = 2 if eos else None
            t, _ = timed(run)
            extra[name] = {"value": W * nq * args.steps / t, "unit": "segments/s",
                           "ms_per_step": t / args.steps * 1e3, "recursions_per_step": nq,
                           "batch": f"{nq} videos x {W} windows, one query each" if nq > 1 else f"1 video x {W} windows",
                           "decode_weights": "fp8 e4m3fn, per-row scale (same pools and merged steps as the headline)" if fp8 else DT,
                           "prefill_gemms": "fp8 x fp8 MFMA (e4m3fn weights per-row scale, activations quantised per row on the fly)" if fp8p else DT}
            if fp8 or fp8p:
                extra[name]["scores_within_1e-3"] = False      # proposals (timestamps) equal the fp32 reference's, entropy scores within 14 % (tests/test_gpu_full_depth_conditioned.py)
            if par:
                extra[name].update(decode_weights=DT, prefill_gemms=DT + " x 2: split operands [hi | lo] against K-duplicated weights",
                                   precision="PARITY (rv_ctx_set_option precision = 1): every GEMM operand and Q carry 16 mantissa bits; the mode in which "
                                             "1/max_entropy, 1/mean_entropy meet 1e-3 against the fp32 reference (tests/test_gpu_full_depth_conditioned.py); "
                                             "unfused decode steps through the generic kernels")
            if not merged:
                extra[name]["decode"] = "every step in flight runs its own decode passes (no DecodeServer): the round-1 pipeline"
            if eos:
                extra[name]["eos"] = ("EOS id 2 configured (random-init weights practically never emit it, so all G steps still run): the cost shown is "
                                      "that of the device-side stop flags (one tiny reduction + pinned D2H copy per generate and step, looked at when "
                                      "the copy has landed: never a host wait)")
        for name, nq, fp8, fp8p, eos, merged, par in (("eos_enabled", 1, False, False, True, True, False), ("separate_decode_passes", 1, False, False, False, False, False),
                                                      ("fp8_decode_weights", 1, True, False, False, True, False),
                                                      ("fp8_llm_path", 1, True, True, False, True, False), ("two_videos_per_step", 2, False, False, False, True, False),
                                                      ("two_videos_per_step_fp8_decode_weights", 2, True, False, False, True, False),
                                                      ("two_videos_per_step_fp8_llm_path", 2, True, True, False, True, False),
                                                      ("parity_precision", 1, False, False, False, True, True)):
            try:
                leg(name, nq, fp8, fp8p, eos, merged, par)
            except Exception as e:  # noqa: BLE001 - an extra leg must never cost the headline line
                extra[name] = {"error": f"{type(e).__name__}: {e}"[:300]}
                try:
                    torch.cuda.synchronize()
                except Exception:  # noqa: BLE001
                    pass
        eng.set_option("fp8_decode", 0)
        eng.set_option("fp8_prefill", 0)
        eng.set_option("precision", 0)
        model.generation_config.eos_token_id = None
        stages.server = server
        work["sets"] = input_sets(1)

        def small_leg(name, fn, note):
            try:
                t, n = fn()
                extra[name] = {"value": W * n / t, "unit": "segments/s", "ms_per_step": t / n * 1e3, "note": note}
            except Exception as e:  # noqa: BLE001
                extra[name] = {"error": f"{type(e).__name__}: {e}"[:300]}
                try:
                    torch.cuda.synchronize()
                except Exception:  # noqa: BLE001
                    pass

        def identical():
            work["sets"] = input_sets(1)[:1]
            try:
                return timed(run)[0], args.steps
            finally:
                work["sets"] = input_sets(1)
        if n_sets > 1:
            small_leg("identical_inputs_in_flight", identical,
                      "the round-2 bench: every step in flight works on the SAME video / query / permutations (identical rows toggle fewer bits: the "
                      "power-capped GEMMs clock higher); the headline gives every step its own inputs")

        def latency():
            work["depth"], stages.server = 1, None
            try:
                return timed(run, steps=8, warm=2)[0], 8
            finally:
                work.pop("depth", None)
                stages.server = server
        small_leg("one_recursion_latency", latency,
                  "ONE recursion at a time, start to finish (no other step in flight, its own prefill and decode passes): ms_per_step = the latency of "
                  "a single query's 100-window recursion; 8 recursions after 2 warm-up")

        def prefill_only():
            work["G"] = 1
            try:
                return timed(run)[0], args.steps
            finally:
                work["G"] = G
        small_leg("prefill_only_G1", prefill_only,
                  "G = 1: adapter + prefill + the first sampled token only, no KV-cached decode step (SURVEY 8d: separates the phases); same pipeline, "
                  "same steps in flight")
        # steady state with wider gangs: 140-row pools (20 recursions per merged step on the 9-row-block split-K kernel), 40 steps in flight,
        # 80 timed steps after 40 warm-up steps - what the pipeline sustains when the fill / drain of a 20-step run no longer matters
        if server is not None and args.pools > 1 and world == 1:
            old_streams = streams
            try:
                from revisionllm_amd import serve
                work["sets"] = input_sets(1)
                wide = serve.DecodeServer(model, rows=140, smax=server.Smax, gmax=max(16, G), pools=2, gang=True, prefill_batch=args.prefill_batch, slot=130, encode_batch=args.encode_batch)
                inter.servers.append(wide)
                stages.server = wide
                streams = [torch.cuda.Stream(dev) for _ in range(40)]
                work["depth"] = 40
                t, _ = timed(run, steps=80, warm=40)
                extra["steady_state_140_row_pools"] = {"value": W * 80 / t, "unit": "segments/s", "ms_per_step": t / 80 * 1e3, "steps": 80, "warmup": 40,
                                                       "steps_in_flight": 40, "rows_per_merged_step": wide.rows_served / max(1, wide.steps_run),
                                                       "note": "same workload and kernels; longer run, wider gangs (NOT the headline: the headline keeps the contract's K / W)"}
            except Exception as e:  # noqa: BLE001
                extra["steady_state_140_row_pools"] = {"error": f"{type(e).__name__}: {e}"[:300]}
                try:
                    torch.cuda.synchronize()
                except Exception:  # noqa: BLE001
                    pass
            finally:
                work.pop("depth", None)
                stages.server = server
                streams = old_streams
        # the other BASELINE.json workloads
        try:
            work.update(sets=input_sets(1, W_=33, Wl_=33, batch_=33), W=33, batch=33)
            t, _ = timed(run)
            extra["workload_stage2_long_33"] = {"value": 33 * args.steps / t, "unit": "segments/s", "ms_per_step": t / args.steps * 1e3,
                                                "config": "33 windows x 256 frames, batch 33: 9 calls (5 + 3 + 1) presenting 32 x8 / 33 video tokens "
                                                          "(8 / 16 / 33 windows x zoom 4 / 2 / 1): two batched generates (8 rows + 1 row), 1 GPU, same pipeline as the headline"}
        except Exception as e:  # noqa: BLE001
            extra["workload_stage2_long_33"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        for kind in ("stage1_dense", "stage1_sparse"):
            try:
                run1, cfg1 = stage1_runner(kind)
                n1 = max(args.steps, 2 * cfg1.get("windows_in_flight", 32))      # two full gangs of windows: a K = 20 run is pipeline fill and drain only
                t, _ = timed(run1, steps=n1, warm=n1 // 2)
                S1 = cfg1["prefill_len"]
                entry = {"value": n1 / t, "unit": "segments/s", "ms_per_step": t / n1 * 1e3, "steps": n1, "warmup": n1 // 2, "config": cfg1,
                         "prefill_flops": 2.0 * S1 * 6.476e9 + 2.6e5 * S1 * S1 + 2.6e8}
                if kind == "stage1_sparse":      # adapter alone: SURVEY 8d: 46.9 GFLOP per 1024-frame segment (MFMA-bound)
                    x1 = ops.init_hash_(torch.empty(32, 1024, 768, dtype=OP, device=dev), "bench.s1.a", args.seed, synth.SQRT3)
                    q32 = qf[None].expand(32, -1, -1).contiguous()
                    ms32 = event_time_ms(lambda: eng.clip_encoder(x1, q32, torch.ones(32, args.lq), "cls"), 5)
                    ms1 = event_time_ms(lambda: eng.clip_encoder(x1[:1], qf[None], torch.ones(1, args.lq), "cls"), 10)
                    entry["roofline"] = {"stage": "sparse adapter (ClipEncoder, 32 windows x 1024 frames in ONE call, CLS out): what the windows in flight run",
                                         "bound": "mfma", "achieved": 32 * 46.9 / ms32, "peak": MFMA_BF16_PEAK_TF, "unit": "TFLOP/s",
                                         "frac": 32 * 46.9 / ms32 / MFMA_BF16_PEAK_TF, "avg_ms": ms32,
                                         "one_window_alone": {"achieved": 46.9 / ms1, "frac": 46.9 / ms1 / MFMA_BF16_PEAK_TF, "avg_ms": ms1,
                                                              "note": "ONE 1025-row sequence: 5-9 row tiles per GEMM on 256 CUs - a latency-bound chain of ~40 launches"}}
                extra["workload_" + kind] = entry
            except Exception as e:  # noqa: BLE001
                extra["workload_" + kind] = {"error": f"{type(e).__name__}: {e}"[:300]}
                try:
                    torch.cuda.synchronize()
                except Exception:  # noqa: BLE001
                    pass

    if extras:
        # The headline pipeline once more on the weights the 1e-3 parity statement is ASSERTED on: synth.CONDITIONED, the amplitudes
        # of goldens G8c / G8d - same tensors, shapes, kernels and launch plans; only the values differ.  A throughput number and a 1e-3 number on the same
        # weights.  (Last of the in-process legs: it replaces the engine's LLM weights; the roofline legs below time kernels, not values.)
        try:
            eng.init_synthetic(seed=args.seed, llm=True, clip=True, cond=synth.CONDITIONED)
            stages.server = server
            work.update(sets=input_sets(1), W=W, batch=batch)         # (the stage2_long_33 leg above left its own geometry behind)
            t, _ = timed(run)
            fx = {}
            try:
                with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "g8_fp32_vs_fp64.json")) as f_:
                    fx = json.load(f_)
            except Exception:  # noqa: BLE001
                pass
            extra["conditioned_weights"] = {
                "value": W * args.steps / t, "unit": "segments/s", "ms_per_step": t / args.steps * 1e3, "ratio_to_the_headline": W * args.steps / t / value,
                "weights": "synth.CONDITIONED (goldens G8c / G8d): embeddings at the RMS of the adapter's CLS rows, residual branches 1/8 of the stream, a peaked lm_head",
                "scores_vs_reference_fp32": "1/max_entropy, 1/mean_entropy within 1e-3 of the reference's fp32 CPU record for every call, every pipeline shape "
                                            "(asserted: tests/test_gpu_full_depth_conditioned.py; measured <= 3.5e-4 in the fp16 build)",
                "reference_fp32_vs_fp64_on_these_weights": fx.get("g8c", {}).get("fp32_vs_fp64"),
                "reference_fp32_vs_fp64_on_the_headline_weights": fx.get("g8", {}).get("fp32_vs_fp64"),
                "note": "the headline's plain N(0, 0.02) weights (BASELINE.json: 'random-init Vicuna-7B') give near-uniform T = 0.05 distributions whose entropies are "
                        "ill-conditioned: tests/golden/g8_fp32_vs_fp64.json holds the distance of the reference's OWN fp32 run from a float64 run of the same call on both "
                        "weight sets (make_goldens.py g8x)"}
        except Exception as e:  # noqa: BLE001
            extra["conditioned_weights"] = {"error": f"{type(e).__name__}: {e}"[:300]}
            try:
                torch.cuda.synchronize()
            except Exception:  # noqa: BLE001
                pass

    if extras and not os.environ.get("REVISION_BENCH_CHILD"):
        # the OTHER operand flavour of the library on the same box, same flags, as a child process (its own engine and weights; this process idles
        # meanwhile): bf16 operands = the reference's own GPU dtype, whose scores sit 2e-3 from the fp32 reference (asserted 3e-3), next to the
        # default fp16 build (3e-4, asserted at the north star's 1e-3)
        other_fl = "bf16" if hip.flavour() == "f16" else "f16"
        try:
            import subprocess
            cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--full", "--no-extras", "--no-cpu-baseline",
                   "--op-dtype", other_fl, "--seed", str(args.seed), "--streams", str(args.streams), "--prefill-batch", str(args.prefill_batch), "--encode-batch", str(args.encode_batch), "--pools", str(args.pools)]
            r_ = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, REVISION_BENCH_CHILD="1"))
            line = [l for l in r_.stdout.splitlines() if l.startswith("{")][-1]
            o_ = json.loads(line)
            extra["operands_" + other_fl] = {"value": o_["value"], "unit": o_["unit"], "ms_per_step": o_["ms_per_step"], "dtype": o_["dtype"],
                                             "ratio_to_the_headline": o_["value"] / value, "roofline_frac": o_["roofline"]["frac"],
                                             "roofline_avg_launch_ms": o_["roofline"]["avg_launch_ms"],
                                             "entropy_scores_vs_fp32_reference": ("within 3e-3 (measured 2.1e-3 on G8c, 1.5e-3 on G8d): NOT the north star's 1e-3" if other_fl == "bf16"
                                                                                  else "within 1e-3 (measured 2.9e-4 on G8c, 2.2e-4 on G8d)"),
                                             "note": "the same bench in a child process with --op-dtype %s (librevision_hip%s.so)" % (other_fl, "_bf16" if other_fl == "bf16" else "")}
        except Exception as e:  # noqa: BLE001
            extra["operands_" + other_fl] = {"error": f"{type(e).__name__}: {e}"[:300]}
    rccl_seen = None
    if args.full and world > 1 and headline and not args.no_extras and not args.workload.startswith("stage1"):
        # The one multi-GPU run the driver makes must also measure the split the north star's 60 % target is about: after the headline
        # (whatever --scaling asked for) the OTHER modes are timed on the same ranks - ``segments`` (a 100 * N-window video per step, windows
        # block-partitioned, all-gather #1 of the CLS rows and #2 of the proposals inside every recursion) and ``strong`` (ONE 100-window
        # recursion sharded over the ranks) - and reported under extra_measurements next to the ratio to the headline.
        one = torch.ones(1, device=dev)
        dist.all_reduce(one)                                   # ranks the communicator really reaches (read back from the collective)
        rccl_seen = {"backend": dist.get_backend(), "world_size_of_the_group": dist.get_world_size(), "ranks_counted_by_an_all_reduce": int(one.item())}
        if rccl_seen["ranks_counted_by_an_all_reduce"] != world or rccl_seen["world_size_of_the_group"] != world:
            # a communicator that does not reach every rank makes every number of this run meaningless: fail loudly on EVERY rank (same value everywhere)
            sys.stderr.write(f"bench: the process group reaches {rccl_seen} ranks, expected {world}\n")
            dist.destroy_process_group()
            return 3
        head_mode = "queries" if by_query else ("strong" if strong else "segments")
        saved = dict(work)

        def record_digest(rec_):
            """A recursion's record as every rank holds it after the exchanges: sha256 over answers + scores -> 8 bytes as an int64."""
            import hashlib
            h_ = hashlib.sha256(repr((rec_["answers"], [round(float(x), 7) for x in rec_["max_entropy"]], [round(float(x), 7) for x in rec_["mean_entropy"]],
                                      rec_.get("starts"), rec_.get("hierarchy_zooms"))).encode()).digest()
            return int.from_bytes(h_[:7], "little")
        for mode in ("queries", "segments", "strong"):
            if mode == head_mode:
                continue
            srv = None
            ok = torch.ones(1, device=dev)
            try:
                pq = mode == "queries"
                Wm = args.windows * (1 if mode in ("strong", "queries") else world)
                lo_m, hi_m = (0, Wm) if pq else parallel.shard_bounds(Wm, rank, world)
                key = ("mode", mode)
                if key not in sets_cache:
                    sets_cache[key] = [input_set(k, 1, W_=Wm, Wl_=hi_m - lo_m, batch_=batch, per_rank=pq) for k in range(n_sets)]
                work.update(sets=sets_cache[key], W=Wm, batch=batch, group=parallel.LOCAL if pq else None, by_query=pq)
                stages._seq_next = 0                           # the rotating call deal restarts identically on every rank
                if server is not None:
                    # KV pools sized for what THIS rank decodes in this mode: whole recursions (7 rows each), or its share of the calls dealt
                    # over the ranks (7 calls over 8 ranks: 0 or 1 row per recursion in flight) - a gang must be able to fill up
                    from revisionllm_amd import serve
                    nc_m = len(stage2.plan_groups(Wm, batch))
                    in_flight = max(1, min(args.streams, args.steps))
                    b_max = nc_m if pq else -(-nc_m // world)
                    rows_m = b_max * max(1, min(in_flight, 144 // b_max)) if pq else min(144, max(b_max, in_flight * nc_m // world))
                    srv = serve.DecodeServer(model, rows=rows_m, smax=server.Smax, gmax=max(16, G), pools=args.pools, gang=args.pools > 1,
                                             prefill_batch=args.prefill_batch, slot=180 + 20 * ("queries", "segments", "strong").index(mode), encode_batch=args.encode_batch)
                    inter.servers.append(srv)
                    stages.server = srv
            except Exception as e:  # noqa: BLE001 - set-up failed on THIS rank (e.g. no memory for the extra KV pools)
                ok.zero_()
                extra["scaling_" + mode] = {"error": f"set-up: {type(e).__name__}: {e}"[:300]}
            # a leg issues collectives: it runs only if EVERY rank finished its set-up (a rank that raised while the others walked into the
            # all-gather would hang the job until the NCCL timeout and cost the headline line)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            try:
                if float(ok.item()) > 0:
                    t, rec_m = timed(run, tag="scaling_" + mode)
                    v = Wm * args.steps * (world if pq else 1) / t
                    entry = {"value": v, "unit": "segments/s", "ms_per_step": t / args.steps * 1e3, "n_gpus": world,
                             "kv_pool_rows_per_rank": rows_m if server is not None else None,
                             "windows_per_step_all_ranks": Wm * (world if pq else 1), "ratio_to_the_headline_mode": v / value,
                             "headline_mode": head_mode, "rank_times": rank_times.get("scaling_" + mode),
                             "what": {"queries": "whole recursions per rank, one final all-gather (no data-path collective)",
                                      "segments": "a 100 * N-window video per step, windows block-partitioned over the ranks, RCCL all-gather of the CLS rows "
                                                  "and of the proposals inside every recursion (weak scaling of the segment-parallel split)",
                                      "strong": "ONE 100-window recursion per step sharded over the ranks, the 7 calls dealt with a rotating start "
                                                "(strong scaling: ratio = efficiency against N x the per-GPU rate)"}[mode]}
                    if not pq and rec_m is not None:
                        # segments / strong: all-gather #2 hands EVERY rank the whole record - it must be the same record on all of them
                        d_ = torch.tensor([record_digest(rec_m)], dtype=torch.int64, device=dev)
                        all_d = [torch.zeros_like(d_) for _ in range(world)]
                        dist.all_gather(all_d, d_)
                        same = len({int(x.item()) for x in all_d}) == 1
                        entry["records_identical_on_all_ranks"] = same
                        if not same:
                            extra["FAILED_records_differ_between_ranks"] = mode
                    extra["scaling_" + mode] = entry
                elif "scaling_" + mode not in extra:
                    extra["scaling_" + mode] = {"skipped": "another rank failed to set this leg up"}
            except Exception as e:  # noqa: BLE001 - an extra leg must never cost the headline line
                extra["scaling_" + mode] = {"error": f"{type(e).__name__}: {e}"[:300]}
                try:
                    torch.cuda.synchronize()
                except Exception:  # noqa: BLE001
                    pass
            finally:
                if srv is not None and srv in inter.servers:
                    inter.servers.remove(srv)
                stages.server = server
        work.clear()
        work.update(saved)
        if rccl_seen is not None:
            extra["rccl_ranks_seen"] = rccl_seen

    if rank == 0:
        ids1, _ = _prompt_ids("<video>\n" + stage2.QUERY_TEMPLATE.format(SENTENCE), tok, 1)
        P = ids1.shape[1]
        S = P - 1 + batch
        n_calls_rank = len(parallel.deal(len(plan), 0, world))
        row_map = model.build_row_map(ids1.repeat(n_calls_rank, 1), batch)
        P0 = model._common_text_prefix(row_map) if n_calls_rank > 1 else 0
        M_prefill = P0 + n_calls_rank * (S - P0)
        roof = None
        if args.full:
            eng.set_option("fp8_decode", 0)
            eng.set_option("fp8_prefill", 0)
            # generates per merged decode step of the timed region: a full pool under the gang policy, else what the run averaged
            gang = max(1, args.pool_rows // n_calls_rank) if (server is not None and args.pools > 1) else 1
            if server is not None and args.pools <= 1:
                gang = max(1, min(args.pool_rows // n_calls_rank, round(server.rows_served / max(1, server.steps_run) / n_calls_rank)))
            pf_groups = 1
            if server is not None and server.prefill_batch > 1 and server.pf_batches:
                pf_groups = max(server.pf_hist, key=server.pf_hist.get)       # the pass size that served most steps of this run: 1, 2, 4 or 8 prefills
            legs = roofline_legs(model, n_calls_rank, M_prefill, dec_rows=min(144, gang * n_calls_rank), prefill_groups=pf_groups)
            # dominant = the larger share of a recursion: 32 prefill launches shared by `pf_groups` recursions, or 32 x G decode launches
            # shared by `gang` recursions
            dom = max((legs[k] for k in ("prefill_gateup_gemm", "decode_gateup_gemv")),
                      key=lambda l: l["ms"] * (32 / pf_groups if l["bound"] == "mfma" else 32 * G / gang))
            traffic = pmc_traffic(dom["kernel"], dom["grid_threads"])
            other = {k: {"kernel": v["kernel"], "achieved": v["achieved"], "unit": v["unit"], "frac": v["achieved"] / v["peak"], "avg_launch_ms": v["ms"],
                         **({"tflops": v["tflops"]} if "tflops" in v else {}), **({"rows": v["rows"]} if "rows" in v else {}),
                         **({"timing": v["timing"]} if "timing" in v else {}),
                         **({"prefills_per_launch": v["prefills_per_launch"]} if "prefills_per_launch" in v else {})} for k, v in legs.items()}
            for fname in ("r6_pmc_mfma.json", "r5_pmc_mfma.json", "r4_pmc_mfma.json", "r3_pmc_mfma.json", "r2_pmc_mfma.json"):
                pmc = committed_profile(fname)
                if pmc is not None:
                    other["prefill_gemm_pmc"] = dict(pmc.get("summary") or {}, source="profiles/" + fname)
                    break
            # the decode gate/up kernel INSIDE a decode step (rocprofv3 kernel trace of isolated steps, committed): the number to price it with
            for fname in ("r6_decode_steps.json", "r5_decode_steps.json", "r4_decode_steps.json", "r3_decode_steps.json", "r2_decode_steps.json"):
                prof = committed_profile(fname)
                ks = [] if prof is None else prof.get("rows", {}).get(str(legs["decode_gateup_gemv"]["rows"]), {}).get("kernels", [])
                want = legs["decode_gateup_gemv"]["kernel"].replace(" ", "")
                row = next((r_ for r_ in ks if r_["kernel"].replace(" ", "") == want), None)
                if row is not None:
                    nb = legs["decode_gateup_gemv"]["algorithmic"]
                    other["decode_gateup_gemv"]["in_step"] = {"avg_launch_ms": row["avg_us"] / 1e3, "achieved": nb / row["avg_us"] / 1e3, "unit": "GB/s",
                                                              "frac": nb / row["avg_us"] / 1e3 / HBM_PEAK_GBS,
                                                              "source": f"profiles/{fname} (rocprofv3 kernel trace of isolated {legs['decode_gateup_gemv']['rows']}-row steps)"}
                    break
            # the dominant kernel inside a batched prefill pass (other kernels between its launches: the clock is not pinned at the power cap
            # by one kernel), from the committed rocprofv3 summary of tools/prefill_prof.sh - next to the live back-to-back figure above
            pf_name = next((n_ for n_ in ("r6_prefill_pass.json", "r5_prefill_pass.json", "r4_prefill_pass.json") if committed_profile(n_) is not None), "r3_prefill_pass.json")
            pf = committed_profile(pf_name)
            if pf is not None and pf.get("rows") == dom.get("rows"):
                row = next((r_ for r_ in pf.get("kernels", []) if r_["kernel"].replace(" ", "") == dom["kernel"].replace(" ", "")), None)
                if row is not None:
                    fl = dom["algorithmic"]
                    roof_in_situ = {"avg_launch_ms": row["avg_us"] / 1e3, "achieved": fl / row["avg_us"] / 1e6, "unit": "TFLOP/s",
                                    "frac": fl / row["avg_us"] / 1e6 / MFMA_BF16_PEAK_TF,
                                    "source": f"profiles/{pf_name} (rocprofv3 kernel trace of batched prefill passes at this row count)"}
                else:
                    roof_in_situ = None
            else:
                roof_in_situ = None
            roof = {"kernel": dom["kernel"], "bound": dom["bound"], "achieved": dom["achieved"], "peak": dom["peak"],
                    "unit": dom["unit"], "frac": dom["achieved"] / dom["peak"], "traffic": traffic,
                    "avg_launch_ms": dom["ms"], "algorithmic_per_launch": dom["algorithmic"],
                    "timing": "64 back-to-back launches of this kernel alone, HIP events on the launch stream (sustained: the socket power limit sets the clock)",
                    **({"clocks": dom["clocks"], "clock_adjusted_frac": (dom["algorithmic"] / dom["clocks"]["avg_launch_ms_over_the_sampled_run"] / 1e9) / (dom["peak"] * dom["clocks"]["sclk_mhz_mean"] / 2400.0),
                        "clock_adjusted_note": "frac against the peak AT THE CLOCK THE KERNEL RAN AT (peak x mean sclk / 2400 MHz): what the kernel leaves on the table "
                                               "apart from the socket power limit"}
                       if dom.get("clocks", {}).get("available") and dom["bound"] == "mfma" else {}),
                    **({"in_situ": roof_in_situ} if roof_in_situ else {}), "other": other}
        out = {
            "metric": METRIC,
            "value": value, "unit": "segments/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "dtype": DT + " (fp8 e4m3 LLM weights / prefill GEMMs: extra measurement)" if (args.fp8_decode or args.fp8_prefill) else DT, "data": "synthetic",
            "config": {"workload": args.workload, "windows_per_gpu": Wl, "windows_total": W * (world if by_query else 1), "frames": Tn, "clip_dim": 768, "query_tokens": args.lq,
                       "inputs": ("every step in flight has its OWN video, query (tokens, CLS feature, sentence ids) and window permutations: %d distinct "
                                  "input sets, step k uses set k mod %d" % (n_sets, n_sets) if n_sets > 1 else
                                  "ONE input set shared by all steps in flight (--identical-inputs / --streams 1)"),
                       "queries_per_step": args.queries, "videos_per_step": 1, "batch": batch, "zooms": [4, 2, 1], "llm_calls_per_recursion": len(plan),
                       "prompt_tokens": int(P), "prefill_len": int(S), "shared_prefix": int(P0), "prefill_gemm_rows": int(M_prefill), "decode_steps": G,
                       "llm": "Vicuna-7B shapes, random-init (hash-seeded)", "sampling": "do_sample T=0.05 top_k=50",
                       "recursion": "batched (CLS per window encoded once, the 7 calls of a recursion batched in one generate)",
                       "eos": "id 2, lagging device-side stop flag" if args.eos else "disabled (forced decode length)",
                       "steps_in_flight": max(1, args.streams), "settle_steps": args.settle, **wl_cfg,
                       "decode": ("merged: the generates of the steps in flight share one KV pool and every decode step is ONE pass over the weights for all "
                                  "their rows (serve.DecodeServer; %.1f rows per merged step)" % (server.rows_served / max(1, server.steps_run))
                                  if server is not None else "per step: every step in flight runs its own decode passes"),
                       "prefill": ("batched: up to %d waiting prefills of the steps in flight ride in one pass (serve.DecodeServer; %.2f per pass in this run)"
                                   % (server.prefill_batch, server.pf_tickets / max(1, server.pf_batches)) + "; steps by pass size: %s" % dict(sorted(server.pf_hist.items()))
                                   if server is not None and server.prefill_batch > 1 else "one pass per step"),
                       "adapter": ("batched: up to %d waiting adapter calls of the steps in flight run as one rv_clip_encoder call, a query per recursion "
                                   "(serve.DecodeServer.submit_encode; %.2f per call in this run)" % (server.encode_batch, server.enc_tickets / max(1, server.enc_batches))
                                   if server is not None and getattr(server, "encode_batch", 1) > 1 else "one call per recursion"),
                       "parallelism": ("single GPU" if world == 1 else
                                       f"queries x{world}: whole recursions dealt to the ranks (each rank = the 1-GPU pipeline on its own videos / queries), "
                                       "one RCCL all-gather of the per-call proposals at the end of the timed region" if by_query else
                                       f"{'one recursion sharded' if strong else 'segments'} x{world} + RCCL all-gather of CLS rows and proposals in every recursion")
                                      + (f" [PLUMBING RUN: {world} ranks share {torch.cuda.device_count()} GPU(s), backend {backend}, stream-K GEMMs off - not a measurement]"
                                         if shared_gpu else "")},
        }
        if roof is not None:
            out["roofline"] = roof
        if headline_clocks is not None:
            out["clocks_during_the_timed_region"] = headline_clocks
        if world > 1:
            out["rank_times"] = rank_times.get("headline")
            if n1_ref is not None:
                out["n1_reference_same_box"] = n1_ref
                out["efficiency_vs_same_box_n1"] = value / (world * n1_ref["value"])
                for k_, e_ in extra.items():
                    if k_.startswith("scaling_") and isinstance(e_, dict) and "value" in e_:
                        e_["efficiency_vs_same_box_n1"] = e_["value"] / (world * n1_ref["value"])
        if rec is not None:
            out["answers_sample"] = rec["answers"][:2] if not os.environ.get("REVISION_BENCH_ALL_ANSWERS") else rec["answers"]
        if extra:
            out["extra_measurements"] = extra       # NOT the headline: a different batch per step / reduced-precision weights / other workloads
        if args.full and world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(args, len(stage2.plan_groups(100, 100)), int(P))
            except Exception as e:  # noqa: BLE001 - the reported baseline must never cost the line
                out["cpu_baseline"] = {"value": None, "unit": "segments/s", "cores": 0, "kind": "port", "sample": f"failed: {type(e).__name__}: {e}"[:300]}
        sys.stdout.flush()
        os.write(line_fd, (json.dumps(out) + "\n").encode())
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if "FAILED_records_differ_between_ranks" in extra:       # (decided from an all-gather: the same on every rank)
        sys.stderr.write("bench: the ranks hold different records after the exchanges of mode %s\n" % extra["FAILED_records_differ_between_ranks"])
        return 4


if __name__ == "__main__":
    sys.exit(main() or 0)
