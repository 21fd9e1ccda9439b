"""Mixed-geometry prefill passes, measured: the 100-window stage-2 pipeline at 7B shapes with 20 recursions in flight whose query sentences have DIFFERENT
word counts (a fixed, seeded draw of 6 .. 24 words), through ``serve.DecodeServer``

  (a) ``mixed_prefill=False`` - tickets of different geometry go one to a pass (the path of every earlier build, bit for bit): the yardstick
  (b) ``mixed_prefill=True``  - packed mixed passes (rv_llm_prefill_pool_mixed)
  (c) the cheaper alternative: every ticket right-padded to the longest S of the draw and batched through the existing ragged entry
      (rv_llm_prefill_pool_groups_ragged, each sequence's own last valid row) - ``PaddedServer`` below, a bench-only server: it needs one B and one P0,
      which this workload has (one window count, one prompt prefix)
  (u) the uniform-length run (every sentence 20 words, ``mixed_prefill=False``): passes of 8 tickets, the ceiling

alternated in ONE process on one device (a, b, c, u, a, b, c, u, ..), ``--repeats`` rounds of ``--steps`` recursions each after a warm-up round that is not
counted.  Writes segments/s per setting (median, min, max over the rounds), every round's ``pf_hist``, the padded-row share of (c) and the spread between
repeats to ``profiles/r7_mixed_prefill.json``.

    python tools/mixed_prefill_bench.py [--steps 40] [--repeats 5] [--out profiles/r7_mixed_prefill.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORDS = ("a person opens the door and walks into the kitchen while another person is sitting at the table reading a newspaper and then both of them "
         "leave the room together after a short while").split()
WORD_COUNTS = list(range(6, 25))


def padded_server(serve, ops, seq_pad):
    """``DecodeServer`` whose prefill tickets are right-padded (zero rows) to sequences of ``seq_pad`` positions (shared prefix included) on submission and batched through the ragged entry
    whatever their own lengths: setting (c).  The generate joins the pool at its own length (model.generate_steps), so the pad positions of the cache are
    overwritten by the first decode steps before they are read - the ragged entry's contract."""

    class PaddedServer(serve.DecodeServer):
        rows_total = rows_pad = 0

        def submit_prefill(self, job, h, B, P0, lens=None):
            S, s_pad = (h.shape[0] - P0) // B, seq_pad - P0
            if lens is None and S <= s_pad:
                if S < s_pad:
                    body = torch.nn.functional.pad(h[P0:].view(B, S, -1), (0, 0, 0, s_pad - S)).reshape(B * s_pad, -1)
                    h = torch.cat([h[:P0], body]).contiguous()
                lens = (P0 + S,) * B
                PaddedServer.rows_total += P0 + B * s_pad
                PaddedServer.rows_pad += B * (s_pad - S)
            return super().submit_prefill(job, h, B, P0, lens)

        def _pump_prefill(self, partial=False, force=False):
            if not self.pf_queue:
                return False
            self.pf_inflight = [e for e in self.pf_inflight if not e.query()]
            lead = self.pf_queue[0]
            geom = lambda t: t.key[:4] + (t.lens is None,)          # (everything but the sequences' own lengths)
            n = 1
            while n < len(self.pf_queue) and n < self.prefill_batch and geom(self.pf_queue[n]) == geom(lead):
                n += 1
            full = n == self.prefill_batch or n < len(self.pf_queue)
            if not full and not force and not (partial and not self.pf_inflight):
                return False
            if lead.lens is None:
                return super()._pump_prefill(partial, force)
            n = serve.best_prefill_batch(n, int(lead.h.shape[0]), self.cus_per_xcd)
            batch, self.pf_queue = self.pf_queue[:n], self.pf_queue[n:]
            eng, pool = self.model.engine, lead.job.pool
            prev, eng.slot = eng.slot, self.pf_slot
            with torch.cuda.stream(self.pf_stream):
                for t in batch:
                    self.pf_stream.wait_event(t.event)
                    t.h.record_stream(self.pf_stream)
                Mg, S_ = lead.h.shape[0], lead.S
                last = [g * Mg + lead.P0 + b * S_ + (t.lens[b] - lead.P0 - 1) for g, t in enumerate(batch) for b in range(lead.B)]
                logits = eng.llm_prefill_pool_groups(torch.cat([t.h for t in batch]) if n > 1 else lead.h, n, lead.B, lead.P0, pool.kv, pool.R,
                                                     [t.job.r0 for t in batch], pool.Smax, last_rows=ops.h2d(torch.tensor(last, dtype=torch.int32), eng.device))
                ev = torch.cuda.Event()
                ev.record(self.pf_stream)
            eng.slot = prev
            for i, t in enumerate(batch):
                t.first, t.ready, t.h = logits[i * t.B:(i + 1) * t.B], ev, None
            self.pf_inflight.append(ev)
            self.pf_batches += 1
            self.pf_tickets += n
            self.pf_hist[n] = self.pf_hist.get(n, 0) + n
            return True

    return PaddedServer


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=40, help="recursions per timed round")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--in-flight", type=int, default=20)
    p.add_argument("--windows", type=int, default=100)
    p.add_argument("--frames", type=int, default=256)
    p.add_argument("--lq", type=int, default=16)
    p.add_argument("--decode-steps", type=int, default=8)
    p.add_argument("--prefill-batch", type=int, default=8)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--op-dtype", default=None, choices=["f16", "bf16"])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7_mixed_prefill.json"))
    args = p.parse_args()

    from revisionllm_amd import hip, ops, parallel, sched, serve
    from revisionllm_amd.eval import stage2
    from revisionllm_amd.inference import _prompt_ids
    from revisionllm_amd.model import ReVisionLlamaForCausalLM
    from revisionllm_amd.utils import synth
    if args.op_dtype:
        hip.set_flavour(args.op_dtype)
    OP = hip.op_dtype()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    model = ReVisionLlamaForCausalLM(synth.VICUNA_7B, device=dev)
    model.get_model().initialize_vision_modules(SimpleNamespace(clip_adapter=True, cross_attn=False, clip_adapter_text=True, clip_adapter_feature="cls", hierarchy=True,
                                                                adapter_input_dim=768, pretrain_clip_adapter=None, pretrain_mm_mlp_adapter=None))
    eng = model.engine
    eng.init_synthetic(seed=args.seed, llm=True, clip=True)
    model.generation_config.eos_token_id = None
    tok = synth.FakeTokenizer()
    W = batch = args.windows
    G = args.decode_steps
    plan = stage2.plan_groups(W, batch)
    rows_rec = len(plan)
    n_sets = args.in_flight

    def hashed(shape, dtype, name):
        return ops.init_hash_(torch.empty(*shape, dtype=dtype, device=dev), name, args.seed, synth.SQRT3)

    draw = torch.Generator().manual_seed(args.seed + 7)
    counts = [WORD_COUNTS[int(torch.randint(len(WORD_COUNTS), (1,), generator=draw))] for _ in range(n_sets)]

    def input_sets(words):
        out = []
        for k in range(n_sets):
            g = torch.Generator().manual_seed(args.seed * 100003 + k * 17)
            sent = " ".join(WORDS[:words[k]]).replace("kitchen", f"kitchen{k}")
            out.append({"feats": hashed((W, args.frames, 768), OP, f"mixb.feat.s{k}"), "perms": [stage2.make_perms(plan, g, W=W)],
                        "qs": [(hashed((args.lq, 768), OP, f"mixb.q.s{k}"), hashed((768,), torch.float32, f"mixb.qcls.s{k}"), sent)]})
        return out

    sets = {"mixed": input_sets(counts), "uniform": input_sets([20] * n_sets)}
    prompt_len = {w: int(_prompt_ids("<video>\n" + stage2.QUERY_TEMPLATE.format(" ".join(WORDS[:w])), tok, 1)[0].shape[1]) for w in sorted(set(counts + [20]))}
    stages = parallel.HipStages(model, tok)
    streams = [torch.cuda.Stream(dev) for _ in range(args.in_flight)]
    pool_rows = rows_rec * max(1, min(args.in_flight, 144 // rows_rec))
    smax = 256

    # (c): positions of the longest sequence of the draw = its prompt's tokens with the <video> token replaced by the window tokens
    Padded = padded_server(serve, ops, max(prompt_len[w] for w in counts) - 1 + batch)

    def run_round(which, mixed, n):
        make = Padded if mixed == "pad" else serve.DecodeServer
        mixed = mixed is True
        server = make(model, rows=pool_rows, smax=smax, gmax=max(16, G), pools=2, gang=True, prefill_batch=args.prefill_batch, mixed_prefill=mixed)
        stages.server = server
        inter = sched.Interleaver(servers=[server])
        ss = sets[which]
        pending, rec = [], None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            s_ = ss[i % len(ss)]
            k = i % len(streams)
            streams[k].wait_stream(torch.cuda.current_stream(dev))
            pending.append(inter.add(sched.Task(lambda task, s_=s_: parallel.launch_queries_sharded_steps(stages, tok, s_["feats"], W, s_["qs"], batch=batch, perms=s_["perms"],
                                                                                                         max_new_tokens=G, turn=task), streams[k], eng, k)))
            if len(pending) > args.in_flight:
                rec = parallel.collect_queries(inter.finish(pending.pop(0)))[0]
        while pending:
            rec = parallel.collect_queries(inter.finish(pending.pop(0)))[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        eng.slot = 0
        stages.server = None
        assert rec is not None
        return {"segments_per_s": n * W / dt, "seconds": dt, "pf_hist": {str(k): v for k, v in sorted(server.pf_hist.items())}, "pf_batches": server.pf_batches,
                "pf_tickets": server.pf_tickets}

    settings = [("a_uniform_server", "mixed", False), ("b_mixed_prefill", "mixed", True), ("c_padded_ragged", "mixed", "pad"), ("u_uniform_lengths", "uniform", False)]
    for name, which, mixed in settings:          # warm-up round (allocations, first launches): not counted
        run_round(which, mixed, max(args.in_flight, args.steps // 2))
    rounds = {name: [] for name, _, _ in settings}
    for _ in range(args.repeats):
        for name, which, mixed in settings:      # alternated: drift of the device hits every setting alike
            rounds[name].append(run_round(which, mixed, args.steps))

    def stats(rs):
        v = [r["segments_per_s"] for r in rs]
        return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread_rel": (max(v) - min(v)) / statistics.median(v), "rounds": rs}

    res = {name: stats(rs) for name, rs in rounds.items()}
    lens = [prompt_len[w] for w in counts]
    longest = max(lens)
    out = {"tool": "tools/mixed_prefill_bench.py", "operand_flavour": hip.flavour(), "device": torch.cuda.get_device_name(dev), "windows": W, "frames": args.frames,
           "in_flight": args.in_flight, "steps_per_round": args.steps, "repeats": args.repeats, "prefill_batch": args.prefill_batch, "decode_steps": G,
           "word_counts": counts, "prompt_tokens": lens, "settings": res,
           "ratio_b_over_a": res["b_mixed_prefill"]["median"] / res["a_uniform_server"]["median"],
           "ratio_b_over_c": res["b_mixed_prefill"]["median"] / res["c_padded_ragged"]["median"],
           "ratio_b_over_uniform_lengths": res["b_mixed_prefill"]["median"] / res["u_uniform_lengths"]["median"],
           "padded_row_share_of_c": Padded.rows_pad / max(1, Padded.rows_total), "longest_prompt_tokens": longest}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("ratio_b_over_a", "ratio_b_over_c", "ratio_b_over_uniform_lengths", "padded_row_share_of_c")} | {n: {k: round(v, 1) if k != "spread_rel" else round(v, 4) for k, v in s.items() if k != "rounds"}
                                                                                               for n, s in res.items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
