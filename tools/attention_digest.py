"""SHA-256 digests of what the attention kernels write, for a fixed case list: the check that a change of csrc/attention.hip leaves every output bit where
it was.

    REVISION_HIP_LIB=... REVISION_HIP_LIB_BF16=... python tools/attention_digest.py [--out FILE] [--per-case]     (default: profiles/attention_digest.json)

Run it once on a build of the parent commit (the two variables name its libraries) and once on this tree's build, in a fresh process each on the same
machine; the two files must hold the same digests.  Both operand flavours run.

  rv_attention   every record of tests/attention_oracle.CASES with every probe of the record, on the fenced buffers of its layout (``contig`` included: the
                 buffers ops.attention would build): the digest covers the WHOLE output buffer, fences and all.  A group = (case group, kernel form, head
                 width); --per-case keeps one digest per record instead.
  engine         the launches rv_attention cannot reach, on the TINY geometry (3 blocks, 4 heads of 128): logits and every byte of the KV pool (block l + 1's
                 K / V are made from block l's attention output) of one pass each -
                   pair, pair_groups   shared prefix + per-call rows (k_attention_pair; G = 1 and 2)      } with the key blocks staged in LDS (attn_lds = 1)
                   groups              G = 2 prefills without a prefix (k_attention_groups)               } and fetched per wave (attn_lds = 0)
                   mixed               three groups of different geometry (k_attention_mixed)             }
                   prefill             a lone two-sequence prefill (k_attention, 128-wide heads)          }
                   rows7, rows24       a merged decode step with per-row positions (one row inactive, two at other positions), 7 rows and 24 (the
                                       fragment-packed output); _shared: with share hints (sibling r + 1, 64 positions) on caches that differ
                   qs_*                the parity precision (``precision`` = 1: split queries, split output): pair, groups, prefill and a 7-row decode step
"""
import argparse
import hashlib
import json
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import attention_oracle as ao  # noqa: E402
from revisionllm_amd import engine, hip  # noqa: E402
from revisionllm_amd.utils import synth  # noqa: E402

DEV = "cuda:0"


def raw_bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()


def attention_cases(fl):
    """("group:case", bytes of the output buffer) of every record and probe."""
    lib = hip.lib(fl)
    for c in ao.CASES:
        pad = ao.make_mask(c.mask, c.Bk, c.Lk)
        padd = pad.to(DEV).contiguous() if pad is not None else None
        for probe in c.probes:
            q, k, v = ao.case_inputs(c, probe, fl)
            L = ao.build_layout(c.layout, q, k, v, fl, causal=c.causal, q_pos0=c.q_pos0, kv_div=c.B // c.Bk)
            qb = L.q_buf.to(DEV)
            kb, vb, out = (qb if L.k_buf is L.q_buf else L.k_buf.to(DEV)), L.vt_buf.to(DEV), L.out_buf.to(DEV)
            rc = lib.rv_attention(*L.args(qb.data_ptr(), kb.data_ptr(), vb.data_ptr(), out.data_ptr(), padd.data_ptr() if padd is not None else None, hip.stream()))
            torch.cuda.synchronize()
            assert rc == 0, (ao.case_id(c), rc)
            yield f"{c.group}/{c.form}/dh{c.dh}:{ao.case_id(c)}/{probe}", raw_bytes(out)


def rnd(name, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(zlib.crc32(name.encode()))).mul(0.02).to(DEV)


def engine_cases(fl):
    """("engine/<form>", logits bytes + pool bytes) of one pass per engine-only launch."""
    D, V, R, Smax = synth.TINY.hidden, synth.TINY.vocab, 32, 128

    def make(parity):
        e = engine.Engine(synth.TINY, adapter_text=False, device=DEV, op_dtype=fl)
        e.init_synthetic(seed=7, llm=True, clip=False, parity=parity)
        if parity:
            e.set_option("precision", 1)
        return e

    def nan_logits(n):
        return torch.full((n, V), float("nan"), device=DEV)

    def done(name, logits, kv):
        torch.cuda.synchronize()
        assert bool(torch.isfinite(logits).all()), name
        return "engine/" + name, raw_bytes(logits) + raw_bytes(kv)

    def prefills(e, tag):
        pool, _ = e.new_kv_pool(R, Smax)
        yield done(tag + "pair", e.llm_prefill_pool(rnd("pair", 32 + 3 * 40, D), 3, 32, pool, R, 2, Smax, logits=nan_logits(3)), pool)
        pool, _ = e.new_kv_pool(R, Smax)
        yield done(tag + "pair_groups", e.llm_prefill_pool_groups(rnd("pg", 2 * (32 + 3 * 40), D), 2, 3, 32, pool, R, [1, 9], Smax, logits=nan_logits(6)), pool)
        pool, _ = e.new_kv_pool(R, Smax)
        yield done(tag + "groups", e.llm_prefill_pool_groups(rnd("gr", 2 * 3 * 40, D), 2, 3, 0, pool, R, [1, 9], Smax, logits=nan_logits(6)), pool)
        kv, _ = e.new_kv(2, Smax, reuse=False)
        yield done(tag + "prefill", e.llm_forward(rnd("pf", 2, 70, D), 0, kv, Smax, logits=nan_logits(2)), kv)

    e = make(False)
    for lds in (1, 0):
        e.set_option("attn_lds", lds)
        tag = "lds%d/" % lds
        yield from prefills(e, tag)
        groups = [(3, 32, 40, 1), (1, 0, 70, 9), (2, 17, 33, 12)]
        pool, _ = e.new_kv_pool(R, Smax)
        h = rnd("mx", sum(P0 + B * S for B, P0, S, _ in groups), D)
        yield done(tag + "mixed", e.llm_prefill_pool_mixed(h, groups, pool, R, Smax, logits=nan_logits(6)), pool)
    e.set_option("attn_lds", 1)
    for n in (7, 24):
        base, _ = e.new_kv_pool(n, Smax)
        e.llm_prefill_pool(rnd("rows%d" % n, n * 70, D), n, 0, base, n, 0, Smax)
        pos = torch.full((n,), 70, dtype=torch.int32)
        pos[3], pos[1], pos[5] = -1, 33, 64                                # an inactive row; keys ending inside and at the end of a block
        share = torch.tensor([((r + 1) % n) | 64 << 16 for r in range(n)], dtype=torch.int32)
        for name, hint in (("rows%d" % n, None), ("rows%d_shared" % n, share.to(DEV))):
            pool = base.clone()
            lg = e.llm_decode_rows(rnd("step%d" % n, n, D), pos.to(DEV), pool, Smax, logits=nan_logits(n), row_share=hint)
            lg[3] = 0                                                      # (an inactive row's logits are unspecified)
            yield done(name, lg, pool)
    e = make(True)
    yield from prefills(e, "qs_")
    base, _ = e.new_kv_pool(7, Smax)
    e.llm_prefill_pool(rnd("qsrows", 7 * 70, D), 7, 0, base, 7, 0, Smax)
    pos = torch.full((7,), 70, dtype=torch.int32)
    pos[3], pos[1] = -1, 33
    lg = e.llm_decode_rows(rnd("qsstep", 7, D), pos.to(DEV), base, Smax, logits=nan_logits(7))
    lg[3] = 0
    yield done("qs_rows7", lg, base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_digest.json"))
    ap.add_argument("--per-case", action="store_true", help="one digest per rv_attention record and probe (to find the case behind a differing group)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "attention_digest needs the GPU"
    res, calls = {}, 0
    for fl in ("f16", "bf16"):
        hip.set_flavour(fl)
        groups = {}
        for gen in (attention_cases(fl), engine_cases(fl)):
            for name, data in gen:
                h = groups.setdefault(name if a.per_case else name.split(":")[0], hashlib.sha256())
                h.update(name.encode() + b"\0" + data)
                calls += fl == "f16"
        res[fl] = {g: h.hexdigest() for g, h in groups.items()}
    out = dict(abi=hip.lib("f16").rv_abi_version(), cases=calls, groups=len(res["f16"]), digests=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(dict(out=a.out, cases=out["cases"], groups=out["groups"], sha256_of_digests=hashlib.sha256(json.dumps(res, sort_keys=True).encode()).hexdigest())))


if __name__ == "__main__":
    main()
