"""Merged decode steps: several generates share one KV pool and their KV-cached decode steps run as ONE pass over the weights
(rows at different positions, up to 32 rows).  A row's results must not depend on what it is batched with."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import SEED, T, feats, fl, op, rel_err, tol

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("M,N,K,act", [(21, 4096, 4096, 0), (32, 22016, 4096, 2), (17, 4096, 11008, 0), (28, 32000, 4096, 0), (21, 512, 1408 // 128 * 128, 0)])
def test_weight_streaming_kernel_17_to_32_rows(M, N, K, act):
    """rv_gemm with 17 .. 32 rows: the weight-streaming kernel with two MFMA column blocks per weight fragment.  Rows 0 .. 15 are
    BIT-identical to the 16-row launch of the same rows, rows 16 .. to a 16-row launch of THOSE rows; vs float64; fp8 weights too."""
    from revisionllm_amd import hip, ops
    dev = "cuda:0"
    g = torch.Generator().manual_seed(M * 7 + N)
    a = (torch.randn(M, K, generator=g) * 0.5).to(op()).to(dev)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(op()).to(dev)
    wp = ops.pack_fragments(w)
    res = torch.randn(M, N // 2 if act == 2 else N, generator=g).to(dev) if act == 0 else None
    od = op() if act == 2 else torch.float32
    y = ops.gemm(a, wp, residual=res, out_dtype=od, act=act, w_packed=True)
    lo = ops.gemm(a[:16], wp, residual=None if res is None else res[:16], out_dtype=od, act=act, w_packed=True)
    hi = ops.gemm(a[16:], wp, residual=None if res is None else res[16:], out_dtype=od, act=act, w_packed=True)
    assert torch.equal(y[:16], lo) and torch.equal(y[16:], hi)
    z = a.double() @ w.double().t()
    if act == 2:
        z3 = z.view(M, N // 32, 2, 16)
        z = (torch.nn.functional.silu(z3[:, :, 0]) * z3[:, :, 1]).reshape(M, N // 2)
    else:
        z = z + res.double()
    assert rel_err(y.float().cpu(), z.cpu()) < (1.5e-2 if act == 2 else 1e-4)
    assert torch.equal(y, ops.gemm(a, w, residual=res, out_dtype=od, act=act))              # row-major weights: same sums
    w8, sc = ops.pack_fragments_fp8(w.float())
    y8 = ops.gemv_fp8(a, w8, sc, residual=res, out_dtype=od, act=act)
    lo8 = ops.gemv_fp8(a[:16], w8, sc, residual=None if res is None else res[:16], out_dtype=od, act=act)
    assert torch.equal(y8[:16], lo8)


def _engine(layers=2, vocab=2048):
    from revisionllm_amd import engine
    from revisionllm_amd.utils import synth
    eng = engine.Engine(synth.LlamaShape(layers=layers, vocab=vocab), adapter_text=False, device="cuda:0")
    eng.init_synthetic(seed=SEED, llm=True, clip=False)
    return eng


def test_merged_decode_rows_equal_separate_generates():
    """Three 'generates' (7, 7 and 3 rows; prompts of different lengths: 171, 171 and 140) prefilled into ONE pool and decoded by merged
    steps (17 then, with the third group inactive, 14 active rows) against the same three run on their own caches: logits of every
    step BIT-identical, caches bit-identical; inactive rows leave their cache untouched."""
    eng = _engine()
    D, V, H = 4096, 2048, 32
    groups = [(7, 171), (7, 171), (3, 140)]
    R, Smax = 32, 192
    g = torch.Generator().manual_seed(3)
    hs = [torch.randn(B, S, D, generator=g).mul(0.02).cuda() for B, S in groups]
    steps = 4
    toks = [[torch.randn(B, 1, D, generator=g).mul(0.02).cuda() for _ in range(steps)] for B, S in groups]
    # --- reference: every group on its own cache
    ref_logits, ref_kv = [], []
    for (B, S), h, tk in zip(groups, hs, toks):
        kv, sm = eng.new_kv(B, Smax, reuse=False)
        assert sm == Smax
        out = [eng.llm_forward(h.clone(), 0, kv, Smax)]
        for s_ in range(steps):
            out.append(eng.llm_forward(tk[s_].clone(), S + s_, kv, Smax))
        ref_logits.append(out)
        ref_kv.append(kv)
    # --- pool: rows 0-6, 7-13, 14-16 (+ 15 unused rows)
    pool, sm = eng.new_kv_pool(R, Smax)
    row0 = [0, 7, 14]
    pos = torch.full((R,), -1, dtype=torch.int32, device="cuda:0")
    first = []
    for (B, S), h, r0 in zip(groups, hs, row0):
        first.append(eng.llm_prefill_pool(h.clone().view(B * S, D), B, 0, pool, R, r0, Smax))
        pos[r0:r0 + B] = S
    for gi in range(3):
        assert torch.equal(first[gi], ref_logits[gi][0])
    for s_ in range(steps):
        active = [0, 1, 2] if s_ < 2 else [0, 1]          # the third group stops after two steps
        hrow = torch.zeros(R, D, device="cuda:0")
        p = torch.full((R,), -1, dtype=torch.int32, device="cuda:0")
        for gi in active:
            B, S = groups[gi]
            hrow[row0[gi]:row0[gi] + B] = toks[gi][s_][:, 0]
            p[row0[gi]:row0[gi] + B] = S + s_
        logits = eng.llm_decode_rows(hrow, p, pool, Smax)
        for gi in active:
            B = groups[gi][0]
            assert torch.equal(logits[row0[gi]:row0[gi] + B], ref_logits[gi][1 + s_]), (s_, gi)
    # caches: K rows / V^T columns of every group equal its own-cache run up to the positions it wrote
    L = 2
    halfp = pool.numel() // 2
    kp = pool[:halfp].view(L, R, H, Smax, 128)
    vp = eng.vt_logical(pool[halfp:], L, R, H, Smax=Smax)          # (blocked by 8 positions on the device)
    for gi, ((B, S), r0) in enumerate(zip(groups, row0)):
        n = S + (2 if gi == 2 else steps)
        half = ref_kv[gi].numel() // 2
        kr = ref_kv[gi][:half].view(L, B, H, Smax, 128)
        vr = eng.vt_logical(ref_kv[gi][half:], L, B, H, Smax=Smax)
        assert torch.equal(kp[:, r0:r0 + B, :, :n], kr[:, :, :, :n]) and torch.equal(vp[:, r0:r0 + B, :, :, :n], vr[..., :n])
    assert (kp[:, 14:17, :, 142:] == 0).all()                 # the stopped group's rows were not written after it went inactive
    assert (kp[:, 17:] == 0).all() and (vp[:, 17:] == 0).all()    # unused rows never touched


@pytest.mark.parametrize("n_groups,R", [(6, 48), (9, 64), (10, 70), (11, 80), (16, 112), (18, 128), (19, 133), (20, 140), (20, 144)])
def test_wide_pools_33_to_144_rows_equal_separate_generates(n_groups, R):
    """Merged decode steps with 33 .. 144 rows (the split-K kernel: activations shared through LDS, 1 - 8 workgroups per column group,
    partial planes folded as subtrees of the 8-way tree): every group's logits at every step BIT-identical to the same group decoded
    on its own cache by the <= 16-row kernel; groups at different positions, the last one leaving after two steps."""
    eng = _engine()
    D = 4096
    rng = np.random.RandomState(n_groups)
    groups = [(7, int(rng.randint(40, 120))) for _ in range(n_groups)]
    Smax = 160
    g = torch.Generator().manual_seed(5)
    hs = [torch.randn(B, S, D, generator=g).mul(0.02).cuda() for B, S in groups]
    steps = 3
    toks = [[torch.randn(B, 1, D, generator=g).mul(0.02).cuda() for _ in range(steps)] for B, S in groups]
    ref = []
    for (B, S), h, tk in zip(groups, hs, toks):
        kv, sm = eng.new_kv(B, Smax, reuse=False)
        out = [eng.llm_forward(h.clone(), 0, kv, Smax)]
        for s_ in range(steps):
            out.append(eng.llm_forward(tk[s_].clone(), S + s_, kv, Smax))
        ref.append(out)
    pool, sm = eng.new_kv_pool(R, Smax)
    row0 = [7 * i for i in range(n_groups)]
    for (B, S), h, r0, want in zip(groups, hs, row0, ref):
        assert torch.equal(eng.llm_prefill_pool(h.clone().view(B * S, D), B, 0, pool, R, r0, Smax), want[0])
    for s_ in range(steps):
        active = range(n_groups) if s_ < 2 else range(n_groups - 1)
        hrow = torch.zeros(R, D, device="cuda:0")
        p = torch.full((R,), -1, dtype=torch.int32, device="cuda:0")
        for gi in active:
            B, S = groups[gi]
            hrow[row0[gi]:row0[gi] + B] = toks[gi][s_][:, 0]
            p[row0[gi]:row0[gi] + B] = S + s_
        logits = eng.llm_decode_rows(hrow, p, pool, Smax)
        for gi in active:
            assert torch.equal(logits[row0[gi]:row0[gi] + 7], ref[gi][1 + s_]), (s_, gi)


@pytest.mark.parametrize("G,P0", [(3, 40), (2, 0), (4, 48), (6, 40)])       # (6 x 7 = 42 last rows: the last block's row form in two pieces of <= 32)
def test_batched_prefill_groups_match_separate_prefills(G, P0):
    """rv_llm_prefill_pool_groups: G prefills of identical geometry ([P0 shared prefix ; 7 x S'] each) in ONE pass against the same G
    prefills one at a time: logits and caches agree to GEMM summation order (the stream-K split points depend on the row count, so
    not bit for bit), and with tiny prefills (the 128-row tile kernel either way) exactly."""
    eng = _engine()
    D, H, L = 4096, 32, 2
    B, S, Smax, R = 7, 96, 160, 32 if G <= 4 else 64
    g = torch.Generator().manual_seed(11 + G)
    hs = [torch.randn(P0 + B * S, D, generator=g).mul(0.02).cuda() for _ in range(G)]
    row0 = [3 + 7 * i for i in range(G)]
    pool_a, _ = eng.new_kv_pool(R, Smax)
    pool_b, _ = eng.new_kv_pool(R, Smax)
    sep = [eng.llm_prefill_pool(h.clone(), B, P0, pool_a, R, r0, Smax).clone() for h, r0 in zip(hs, row0)]
    bat = eng.llm_prefill_pool_groups(torch.cat(hs).contiguous(), G, B, P0, pool_b, R, row0, Smax)
    for gi in range(G):
        assert rel_err(bat[gi * B:(gi + 1) * B].cpu(), sep[gi].cpu()) < 1e-2, gi       # (bf16 activations: a different f32 summation order moves roundings)
    half = pool_a.numel() // 2
    ka, kb = pool_a[:half].view(L, R, H, Smax, 128).float(), pool_b[:half].view(L, R, H, Smax, 128).float()
    va, vb = eng.vt_logical(pool_a[half:], L, R, H, Smax=Smax).float(), eng.vt_logical(pool_b[half:], L, R, H, Smax=Smax).float()
    n = P0 + S
    assert rel_err(kb[:, :, :, :n].cpu(), ka[:, :, :, :n].cpu()) < 1e-2 and rel_err(vb[..., :n].cpu(), va[..., :n].cpu()) < 1e-2
    assert (kb[:, :3] == 0).all() and (kb[:, 3 + 7 * G:] == 0).all() and (kb[:, :, :, n:] == 0).all()      # nothing outside the groups' rows / positions
    # one decode step from either pool: same logits to the same tolerance
    pos = torch.full((R,), -1, dtype=torch.int32, device="cuda:0")
    pos[3:3 + 7 * G] = n
    hrow = torch.randn(R, D, generator=g).mul(0.02).cuda()
    la = eng.llm_decode_rows(hrow.clone(), pos, pool_a, Smax)
    lb = eng.llm_decode_rows(hrow.clone(), pos, pool_b, Smax)
    assert rel_err(lb[3:3 + 7 * G].cpu(), la[3:3 + 7 * G].cpu()) < 1e-2


@pytest.mark.parametrize("G,B,P0,S", [(4, 7, 32, 139), (3, 7, 40, 96), (2, 7, 0, 96), (1, 5, 32, 171)])
def test_prefill_attention_with_lds_staged_keys_is_bit_identical(G, B, P0, S):
    """The prefill's causal attention with its key blocks staged in LDS once per 64-row workgroup (attention.hip attn_body_lds<128, 1>, option ``attn_lds``) against the
    per-wave form of rounds 1 - 5: logits AND every byte of the KV pool equal - shared prefix + per-call rows (the pair launch), several prefills to a pass
    (groups), no shared prefix (the groups launch), a lone prefill."""
    eng = _engine()
    D, R, Smax = 4096, 64, 256
    g = torch.Generator().manual_seed(31 + G)
    hs = torch.randn(G * (P0 + B * S), D, generator=g).mul(0.02).cuda()
    row0 = [3 + B * i for i in range(G)]
    outs = []
    for v in (1, 0):
        eng.set_option("attn_lds", v)
        pool, _ = eng.new_kv_pool(R, Smax)
        lg = (eng.llm_prefill_pool_groups(hs.clone(), G, B, P0, pool, R, row0, Smax) if G > 1 else eng.llm_prefill_pool(hs.clone(), B, P0, pool, R, row0[0], Smax))
        outs.append((lg.clone(), pool.clone()))
    eng.set_option("attn_lds", 1)
    assert torch.isfinite(outs[0][0]).all() and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _tiny_model(parity=False):
    from revisionllm_amd.model import ReVisionLlamaForCausalLM
    from revisionllm_amd.utils import synth
    m = ReVisionLlamaForCausalLM(synth.TINY, device="cuda:0")
    m.get_model().initialize_vision_modules(SimpleNamespace(clip_adapter=True, cross_attn=False, pretrain_clip_adapter=None,
                                                            pretrain_mm_mlp_adapter=None, clip_adapter_text=True, clip_adapter_feature="cls",
                                                            hierarchy=True, adapter_input_dim=768))
    m.engine.init_synthetic(seed=SEED, llm=True, clip=True, parity=parity)
    if parity:
        m.engine.set_option("precision", 1)
    m.generation_config.eos_token_id = None
    return m


@pytest.mark.parametrize("G,B,P0,S", [(4, 7, 32, 139), (3, 7, 40, 96), (2, 7, 0, 96), (1, 5, 32, 171), (4, 1, 0, 327), (8, 7, 32, 139), (2, 3, 17, 61)])
def test_prefill_qkv_epilogue_through_lds_writes_the_same_bytes(G, B, P0, S):
    """The fused q / k / v epilogue of the persistent prefill GEMM staged through LDS (gemm_pp.hip pp_epilogue_rope_lds, option ``qkv_lds``: whole 128-byte row slabs
    of Q / K, 16-byte pieces of 8 positions of V^T, 2-byte stores only where a group of 8 positions is cut by a tile edge or a sequence end) against the per-lane
    stores of rounds 1 - 5: the logits and EVERY byte of the KV pool are equal - shared prefix, no prefix, one / several / eight prefills to a pass, one-row
    sequences of 327 positions, short odd geometry (sequence ends inside tiles, groups of positions cut everywhere)."""
    eng = _engine()
    D, R, Smax = 4096, 64, 352
    g = torch.Generator().manual_seed(41 + G + S)
    hs = torch.randn(G * (P0 + B * S), D, generator=g).mul(0.02).cuda()
    row0 = [1 + B * i for i in range(G)]
    outs = []
    for v in (1, 0):
        eng.set_option("qkv_lds", v)
        pool, _ = eng.new_kv_pool(R, Smax)
        lg = (eng.llm_prefill_pool_groups(hs.clone(), G, B, P0, pool, R, row0, Smax) if G > 1 else eng.llm_prefill_pool(hs.clone(), B, P0, pool, R, row0[0], Smax))
        outs.append((lg.clone(), pool.clone()))
    eng.set_option("qkv_lds", 1)
    assert torch.isfinite(outs[0][0]).all() and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][1].float().abs().max()) > 0


def test_batched_adapter_calls_equal_separate_ones():
    """``DecodeServer(encode_batch=4)``: the adapter calls of recursions in flight ride in ONE rv_clip_encoder call (a query per recursion, grouped fold
    GEMMs): every recursion's CLS rows equal its own call's up to the GEMM plans' summation order (at these few rows the K = 2048 FFN-2 takes a stream-K plan
    that depends on the total row count: one 16-bit rounding moves, measured 3.9e-4 of the largest element in fp16 - with or without the folded attention,
    i.e. a property of the engine at small row counts, not of the batching; at the bench's 100 x 256-frame recursions the rows are bit-identical) - whatever it
    was batched with (3 tickets: a full batch is not needed, ``flush`` launches what waits)."""
    from revisionllm_amd import serve
    m = _tiny_model()
    eng = m.engine
    srv = serve.DecodeServer(m, rows=32, smax=64, gmax=8, pools=2, gang=True, prefill_batch=1, encode_batch=4)
    feats_ = [feats(f"be.x{i}", (9, 32, 768), bf16=fl()).to(op()).cuda() for i in range(3)]
    qfs = [feats(f"be.q{i}", (6, 768), bf16=fl()).to(op()).cuda() for i in range(3)]
    want = [eng.clip_encoder(f, q[None], torch.ones(1, 6), "cls").clone() for f, q in zip(feats_, qfs)]
    tickets = [srv.submit_encode(f, q) for f, q in zip(feats_, qfs)]
    assert all(t.ready is None for t in tickets) and not srv.pump()          # a partial batch waits ...
    assert srv.flush() and all(t.ready is not None for t in tickets)          # ... until nothing else can move
    tickets[0].ready.synchronize()
    assert srv.enc_batches == 1 and srv.enc_tickets == 3
    for t, w in zip(tickets, want):
        assert t.cls.shape == w.shape and rel_err(t.cls.cpu(), w.cpu()) < tol(8e-3)


@pytest.mark.parametrize("n_passes,streams,pools,pbatch", [(3, 3, 1, 1), (5, 2, 1, 1), (7, 6, 2, 1), (9, 8, 3, 1), (7, 6, 2, 4)])
def test_recursions_through_the_decode_server_equal_sequential(n_passes, streams, pools, pbatch):
    """Several stage-2 recursions in flight on their own HIP streams, their generates decoding through ONE DecodeServer (shared KV
    pool, merged steps with rows at different positions, rows joining and leaving as prefills complete) against the same
    recursions run one after the other through the classic loop: records identical (answers, entropies, cosine scores).
    ``pools`` > 1: the gang policy (a pool is filled with four 8-row generates, sealed, and stepped with all 32 rows while the
    next recursions prefill into the other pool; the last, partly filled pool is run when nothing else is left).
    ``pbatch`` > 1: the waiting prefills of identical geometry ride in one pass (``rv_llm_prefill_pool_groups``); at these sizes every
    GEMM is on the 128-row tile kernel whatever the batch, so the records stay identical."""
    from revisionllm_amd import parallel, sched, serve
    from revisionllm_amd.eval import stage2
    from revisionllm_amd.utils import synth
    m = _tiny_model()
    tok = synth.FakeTokenizer(vocab=synth.TINY.vocab)
    st = parallel.HipStages(m, tok)
    W, batch = 13, 8
    feat = feats("s2.feat", (W, 16, 768), bf16=fl()).to(op()).cuda()
    qfs = [feats(f"ms.q{i}", (5 + i % 3, 768), bf16=fl()).to(op()).cuda() for i in range(n_passes)]
    qc = feats("s2.qc", (768,)).cuda()
    plan = stage2.plan_groups(W, batch)                      # 4 + 2 + 2 calls -> generates of 8 rows (same row count per level here)
    perms = stage2.make_perms(plan, torch.Generator().manual_seed(1))
    unis = [torch.rand(6, len(plan), generator=torch.Generator().manual_seed(10 + i)) for i in range(n_passes)]
    kw = dict(batch=batch, perms=[perms], max_new_tokens=6)
    seq = [parallel.run_queries_sharded(st, tok, feat, W, [(qfs[i], qc, f"query {i}")], uniforms=unis[i], **kw)[0] for i in range(n_passes)]
    server = serve.DecodeServer(m, rows=32, smax=128, gmax=16, pools=pools, gang=pools > 1, prefill_batch=pbatch)
    st.server = server
    hs = [torch.cuda.Stream("cuda:0") for _ in range(streams)]
    torch.cuda.synchronize()
    inter = sched.Interleaver(servers=[server])
    pending, par = [], []
    for i in range(n_passes):
        pending.append(inter.add(sched.Task(lambda t, i=i: parallel.launch_queries_sharded_steps(st, tok, feat, W, [(qfs[i], qc, f"query {i}")],
                                                                                              uniforms=unis[i], turn=t, **kw),
                                            hs[i % streams], m.engine, i % streams)))
        if len(pending) > streams:
            par.append(parallel.collect_queries(inter.finish(pending.pop(0)))[0])
    while pending:
        par.append(parallel.collect_queries(inter.finish(pending.pop(0)))[0])
    m.engine.slot = 0
    assert server.steps_run > 0 and server.rows_served > server.steps_run * len(plan) * 0.99      # the merged steps really carried the rows
    if n_passes == 3:
        assert server.rows_served > server.steps_run * len(plan)                                   # ... of more than one recursion at a time
    if pbatch > 1:
        assert server.pf_tickets > server.pf_batches > 0                                          # some prefills really rode together
    if pools > 1:
        assert server.rows_served > server.steps_run * len(plan) * 1.5, (server.rows_served, server.steps_run)   # gangs (the three levels of a recursion are
                                                                                                   # sequential generates, so pools also run partly filled here)
    for a, b in zip(seq, par):
        assert a["answers"] == b["answers"] and a["max_entropy"] == b["max_entropy"] and a["mean_entropy"] == b["mean_entropy"]
        assert a["score_cos"] == b["score_cos"]
    assert not server.jobs and sum(n for _, n, _ in server.free) == 32 * pools                     # every row was given back


def test_ragged_generate_of_a_33_window_recursion_equals_the_two_generate_form():
    """A 33-window recursion at batch 33 has 9 calls: 8 present 32 video tokens, one 33.  Through a DecodeServer with batched prefills they now
    run as ONE generate of right-padded sequences (``rv_llm_prefill_pool_groups_ragged``: the head reads every sequence's last VALID row; every
    row then decodes from its own length) instead of two generates with two prefill passes.  Records of 4 recursions in flight: the ragged form
    against the two-generate form (``server.ragged = False``) and against the sequential classic loop - answers equal, entropies to 1e-5 (the
    prefill GEMMs see other row counts), and the ragged run really used one ticket per recursion."""
    from revisionllm_amd import parallel, sched, serve
    from revisionllm_amd.eval import stage2
    from revisionllm_amd.utils import synth
    m = _tiny_model()
    tok = synth.FakeTokenizer(vocab=synth.TINY.vocab)
    st = parallel.HipStages(m, tok)
    W, batch, n = 33, 33, 4
    plan = stage2.plan_groups(W, batch)
    assert len(plan) == 9
    feat = feats("rg.feat", (W, 16, 768), bf16=fl()).to(op()).cuda()
    qfs = [feats(f"rg.q{i}", (5 + i % 3, 768), bf16=fl()).to(op()).cuda() for i in range(n)]
    qc = feats("rg.qc", (768,)).cuda()
    perms = stage2.make_perms(plan, torch.Generator().manual_seed(2), W=W)
    unis = [torch.rand(6, len(plan), generator=torch.Generator().manual_seed(20 + i)) for i in range(n)]
    kw = dict(batch=batch, perms=[perms], max_new_tokens=6)
    seq = [parallel.run_queries_sharded(st, tok, feat, W, [(qfs[i], qc, f"query {i}")], uniforms=unis[i], **kw)[0] for i in range(n)]

    def pipeline(ragged):
        server = serve.DecodeServer(m, rows=27, smax=160, gmax=16, pools=2, gang=True, prefill_batch=4)      # (<= 32 rows: the tiny model's K = 512 is below the wide kernel's)
        server.ragged = ragged
        st.server = server
        hs = [torch.cuda.Stream("cuda:0") for _ in range(n)]
        torch.cuda.synchronize()
        inter = sched.Interleaver(servers=[server])
        tasks = [inter.add(sched.Task(lambda t, i=i: parallel.launch_queries_sharded_steps(st, tok, feat, W, [(qfs[i], qc, f"query {i}")], uniforms=unis[i],
                                                                                           turn=t, **kw), hs[i], m.engine, i)) for i in range(n)]
        recs = [parallel.collect_queries(inter.finish(t))[0] for t in tasks]
        m.engine.slot = 0
        st.server = None
        assert not server.jobs and sum(k for _, k, _ in server.free) == 27 * 2
        return recs, server
    rag, sv_r = pipeline(True)
    two, sv_t = pipeline(False)
    assert sv_r.pf_tickets == n and sv_t.pf_tickets == 2 * n                     # one generate per recursion instead of two
    for a, b, c in zip(seq, rag, two):
        assert a["answers"] == b["answers"] == c["answers"]
        assert a["starts"] == b["starts"] and a["hierarchy_zooms"] == b["hierarchy_zooms"] and a["score_cos"] == b["score_cos"]
        for k in ("max_entropy", "mean_entropy"):
            assert rel_err(b[k], a[k]) < 1e-5 and rel_err(c[k], a[k]) < 1e-5, k


def test_ragged_generate_that_no_pool_can_take_falls_back_to_equal_geometry_groups():
    """whether a recursion completes must not depend on the DecodeServer's capacity.  The 9 calls of a 33-window recursion
    form a ragged batch (8 x 32 + 1 x 33 video tokens); with a server whose pools hold only 8 rows (``fits`` is false for the padded batch), with a
    server whose Smax is too short, and with no server at all, ``generate_steps`` runs them as equal-geometry sub-batches (the two-generate form
    of round 3) instead of raising - same answers, entropies to 1e-5 of the ragged run through a server that CAN take it."""
    from revisionllm_amd import parallel, sched, serve
    from revisionllm_amd.eval import stage2
    from revisionllm_amd.utils import synth
    m = _tiny_model()
    tok = synth.FakeTokenizer(vocab=synth.TINY.vocab)
    st = parallel.HipStages(m, tok)
    W = batch = 33
    plan = stage2.plan_groups(W, batch)
    feat = feats("rg.feat", (W, 16, 768), bf16=fl()).to(op()).cuda()
    qf, qc = feats("rg.q0", (5, 768), bf16=fl()).to(op()).cuda(), feats("rg.qc", (768,)).cuda()
    perms = stage2.make_perms(plan, torch.Generator().manual_seed(2), W=W)
    uni = torch.rand(6, len(plan), generator=torch.Generator().manual_seed(20))
    kw = dict(batch=batch, perms=[perms], max_new_tokens=6)

    def through(server):
        st.server = server
        inter = sched.Interleaver(servers=[server] if server is not None else ())
        task = inter.add(sched.Task(lambda t: parallel.launch_queries_sharded_steps(st, tok, feat, W, [(qf, qc, "query 0")], uniforms=uni, turn=t, **kw),
                                    torch.cuda.Stream("cuda:0"), m.engine, 0))
        rec = parallel.collect_queries(inter.finish(task))[0]
        m.engine.slot = 0
        st.server = None
        return rec
    roomy = serve.DecodeServer(m, rows=27, smax=160, gmax=16, pools=2, gang=True, prefill_batch=4)
    want = through(roomy)
    assert roomy.pf_tickets == 1                                                   # (one ragged generate)
    small = serve.DecodeServer(m, rows=8, smax=160, gmax=16, pools=2, gang=True, prefill_batch=4)          # 9 rows do not fit 8
    short = serve.DecodeServer(m, rows=27, smax=64, gmax=16, pools=2, gang=True, prefill_batch=4)          # S + G > Smax
    for server in (small, short, None):
        got = through(server)
        assert got["answers"] == want["answers"] and got["starts"] == want["starts"] and got["score_cos"] == want["score_cos"]
        for k in ("max_entropy", "mean_entropy"):
            assert rel_err(got[k], want[k]) < 1e-5, k
    assert small.pf_tickets == 2 and short.pf_tickets == 0       # two sub-batches through the pools, one after the other / nothing fits: both groups decode alone


@pytest.mark.parametrize("pools", [1, 2])
def test_decode_server_with_eos_equals_classic_loop(pools):
    """EOS in the merged path (``pools`` = 2: under the gang policy, the partly filled pool sealed when the scheduler runs dry): generates whose rows emit EOS at different steps (teacher-forced) leave the pool early; sequences and
    entropies equal the classic loop's (pad after a row's EOS, cut at the step where all rows are done)."""
    from revisionllm_amd import sched, serve
    from revisionllm_amd.utils import synth
    m = _tiny_model()
    m.generation_config.eos_token_id, m.generation_config.pad_token_id = 2, 0
    P = 40
    ids = T(synth.synthetic_prompt_ids(P, 20, SEED, vocab=synth.TINY.vocab))[None]
    cases = []
    forced_sets = [torch.tensor([[7, 9, 11], [2, 12, 13], [5, 14, 15], [6, 2, 2], [8, 9, 10], [8, 9, 10]]),           # ends after step 3
                   torch.tensor([[9, 9], [9, 9], [9, 9], [9, 9], [9, 9], [9, 9]]),                                       # never ends: 6 steps
                   torch.tensor([[2], [9], [9], [9], [9], [9]])]                                                         # ends at step 0
    for i, forced in enumerate(forced_sets):
        B = forced.shape[1]
        feat = feats(f"eoss.feat{i}", (B, 6, 16, 768), bf16=fl())
        q = (feats(f"eoss.q{i}", (B, 5, 768), bf16=fl()), torch.ones(B, 5))
        kw = dict(images=feat, query_feats=q, do_sample=True, temperature=0.05, max_new_tokens=6, forced_tokens=forced, return_dict_in_generate=True,
                  uniforms=torch.full((6, B), 0.5))
        cases.append((ids.repeat(B, 1), kw, m.generate(ids.repeat(B, 1), **kw)))
    assert [c[2]["sequences"].shape[1] - P for c in cases] == [4, 6, 1]
    server = serve.DecodeServer(m, rows=16, smax=96, gmax=8, pools=pools, gang=pools > 1)
    inter = sched.Interleaver(servers=[server])
    streams = [torch.cuda.Stream("cuda:0") for _ in range(3)]
    tasks = [inter.add(sched.Task(m.generate_steps(c[0], server=server, **c[1]), streams[i], m.engine, i)) for i, c in enumerate(cases)]
    outs = [inter.finish(t) for t in tasks]
    m.engine.slot = 0
    for (ids_, kw, want), got in zip(cases, outs):
        assert torch.equal(got["sequences"], want["sequences"]) and torch.equal(got["entropy"], want["entropy"])
        assert torch.equal(got["entropy_raw"], want["entropy_raw"])
    assert not server.jobs and not server.draining and sum(n for _, n, _ in server.free) == 16 * pools


@pytest.mark.parametrize("parity", [False, True])
def test_one_row_generates_in_flight_share_prefill_passes_and_decode_steps(parity):
    """The stage-1 shape of the pipeline (bench.py ``workload_stage1_*``): six ONE-row generates (own window features each, no shared
    prefix) in flight - prefills of identical geometry ride four / two to a pass with P0 = 0 (their attention in ONE launch for all groups,
    ``k_attention_groups``), decode steps merged in a gang-filled pool - against the classic loop: same sequences and entropies (tiny
    model: the tile GEMM serves every pass size).  ``parity``: the same in the parity precision (split Q, split attention output)."""
    from revisionllm_amd import sched, serve
    from revisionllm_amd.utils import synth
    m = _tiny_model(parity)
    P = 40
    ids = T(synth.synthetic_prompt_ids(P, 20, SEED, vocab=synth.TINY.vocab))[None]
    cases = []
    for i in range(6):
        feat = feats(f"s1row.feat{i}", (1, 6, 16, 768), bf16=fl())
        q = (feats(f"s1row.q{i}", (1, 5, 768), bf16=fl()), torch.ones(1, 5))
        kw = dict(images=feat, query_feats=q, do_sample=True, temperature=0.05, max_new_tokens=5, return_dict_in_generate=True,
                  uniforms=torch.rand(5, 1, generator=torch.Generator().manual_seed(100 + i)))
        cases.append((kw, m.generate(ids, **kw)))
    server = serve.DecodeServer(m, rows=16, smax=96, gmax=8, pools=2, gang=True, prefill_batch=4)
    inter = sched.Interleaver(servers=[server])
    streams = [torch.cuda.Stream("cuda:0") for _ in range(6)]
    tasks = [inter.add(sched.Task(m.generate_steps(ids, server=server, **kw), streams[i], m.engine, i)) for i, (kw, _) in enumerate(cases)]
    outs = [inter.finish(t) for t in tasks]
    m.engine.slot = 0
    assert server.pf_tickets == 6 and server.pf_batches <= 3 and max(server.pf_hist) >= 2          # passes of 4 + 2 (or 4 + 1 + 1)
    assert server.rows_served > server.steps_run                                                  # merged steps carried several windows
    for (kw, want), got in zip(cases, outs):
        assert torch.equal(got["sequences"], want["sequences"]) and torch.equal(got["entropy"], want["entropy"])


def test_eos_job_running_all_its_steps_keeps_its_last_column():
    """Regression: EOS configured, ``max_new_tokens == gmax``, greedy stepping: a generate that has produced all its
    tokens waits in ``draining`` for its stop flags while ANOTHER generate keeps stepping in the same pool; the later merged steps
    scatter all rows and must not touch the finished generate's last column (they used to write token 0 / a stale entropy there)."""
    from revisionllm_amd import sched, serve
    from revisionllm_amd.utils import synth
    m = _tiny_model()
    m.generation_config.eos_token_id, m.generation_config.pad_token_id = 2, 0
    P, G = 40, 8
    ids = T(synth.synthetic_prompt_ids(P, 20, SEED, vocab=synth.TINY.vocab))[None]
    cases = []
    for i, steps in enumerate((G, G, 3)):           # two full-length generates and a short one that joins later
        B = 2
        feat = feats(f"eosg.feat{i}", (B, 6, 16, 768), bf16=fl())
        q = (feats(f"eosg.q{i}", (B, 5, 768), bf16=fl()), torch.ones(B, 5))
        forced = torch.full((steps, B), 9 + i)
        kw = dict(images=feat, query_feats=q, do_sample=True, temperature=0.05, max_new_tokens=steps, forced_tokens=forced, return_dict_in_generate=True,
                  uniforms=torch.full((steps, B), 0.5))
        cases.append((ids.repeat(B, 1), kw, m.generate(ids.repeat(B, 1), **kw)))
    server = serve.DecodeServer(m, rows=16, smax=96, gmax=G, pools=1, gang=False)          # greedy: jobs step as soon as they have joined
    inter = sched.Interleaver(servers=[server])
    streams = [torch.cuda.Stream("cuda:0") for _ in range(3)]
    tasks = [inter.add(sched.Task(m.generate_steps(cases[0][0], server=server, **cases[0][1]), streams[0], m.engine, 0))]
    for _ in range(3):                               # let the first generate get a few steps ahead of the others
        inter.pump()
        torch.cuda.synchronize()
    tasks += [inter.add(sched.Task(m.generate_steps(c[0], server=server, **c[1]), streams[i], m.engine, i)) for i, c in enumerate(cases) if i > 0]
    outs = [inter.finish(t) for t in tasks]
    m.engine.slot = 0
    for (ids_, kw, want), got in zip(cases, outs):
        assert torch.equal(got["sequences"], want["sequences"]) and torch.equal(got["entropy"], want["entropy"])
    assert not server.jobs and not server.draining and sum(n for _, n, _ in server.free) == 16


def test_a_failing_generate_fails_alone_and_gives_its_rows_back():
    """Regression: with several generates in flight under the gang policy, an exception in ONE task's generator is raised by
    ``finish`` of THAT task only; its rows go back to the pool, so the pool can still seal and step for the others, and the
    scheduler does not spin."""
    from revisionllm_amd import sched, serve
    from revisionllm_amd.utils import synth
    m = _tiny_model()
    P = 40
    ids = T(synth.synthetic_prompt_ids(P, 20, SEED, vocab=synth.TINY.vocab))[None]
    server = serve.DecodeServer(m, rows=8, smax=96, gmax=8, pools=2, gang=True, prefill_batch=1)
    inter = sched.Interleaver(servers=[server])
    streams = [torch.cuda.Stream("cuda:0") for _ in range(4)]

    def make(i, sampling_t):
        feat = feats(f"fail.feat{i}", (2, 6, 16, 768), bf16=fl())
        q = (feats(f"fail.q{i}", (2, 5, 768), bf16=fl()), torch.ones(2, 5))
        return dict(images=feat, query_feats=q, do_sample=True, temperature=sampling_t, max_new_tokens=4, return_dict_in_generate=True,
                    uniforms=torch.full((4, 2), 0.5))
    kws = [make(0, 0.05), make(1, 0.7), make(2, 0.05), make(3, 0.05)]            # generate 1 asks for other sampling settings: join() raises
    want = [m.generate(ids.repeat(2, 1), **kw) for kw in kws]
    tasks = [inter.add(sched.Task(m.generate_steps(ids.repeat(2, 1), server=server, **kws[0]), streams[0], m.engine, 0))]
    while not server.pools[0].jobs:                 # generate 0 joins first: its sampling settings are the pool's
        inter.pump()
    tasks += [inter.add(sched.Task(m.generate_steps(ids.repeat(2, 1), server=server, **kw), streams[i], m.engine, i)) for i, kw in enumerate(kws) if i > 0]
    results = []
    for i, t in enumerate(tasks):
        try:
            results.append(inter.finish(t))
        except ValueError as e:
            assert i == 1 and "sampling settings" in str(e)
            results.append(None)
    m.engine.slot = 0
    assert [r is None for r in results] == [False, True, False, False]
    for i in (0, 2, 3):
        assert torch.equal(results[i]["sequences"], want[i]["sequences"]) and torch.equal(results[i]["entropy"], want[i]["entropy"])
    assert all(p.pending == 0 and p.live == 0 for p in server.pools) and sum(n for _, n, _ in server.free) == 16


@pytest.mark.parametrize("R", [70, 112, 140])
def test_fp8_decode_weights_in_wide_merged_steps_7b_layer(R):
    """The fp8 LLM path of BASELINE configs[4] through the MERGED pipeline's kernels: one Vicuna-7B-shaped block + lm_head, R rows
    (ten / sixteen 7-row generates) prefilled into one KV pool, then merged decode steps streaming the FP8 weight copies
    (rv_llm_decode_rows above 32 rows: the split-K kernel) - against the CPU oracle running its decode steps on the same fake-quantised
    weights (``oracle.llama.fp8_decode_weights``), and bit-identical per generate to the <= 16-row FP8 kernel."""
    from oracle import llama
    from revisionllm_amd import engine
    from revisionllm_amd.utils import synth
    shape = synth.LlamaShape(layers=1, vocab=2048)
    eng = engine.Engine(shape, adapter_text=False, device="cuda:0")
    eng.init_synthetic(seed=SEED, llm=True, clip=False, fp8_decode=True)
    D, S, Smax, steps = 4096, 40, 64, 3
    n = R // 7
    g = torch.Generator().manual_seed(R)
    hs = [torch.randn(7, S, D, generator=g).mul(0.02) for _ in range(n)]
    toks = [[torch.randn(7, 1, D, generator=g).mul(0.02) for _ in range(steps)] for _ in range(n)]
    pool, sm = eng.new_kv_pool(R, Smax)
    for i in range(n):
        eng.llm_prefill_pool(hs[i].cuda().view(7 * S, D).contiguous(), 7, 0, pool, R, 7 * i, Smax)
    got = []
    for s_ in range(steps):
        hrow = torch.zeros(R, D, device="cuda:0")
        p = torch.full((R,), -1, dtype=torch.int32, device="cuda:0")
        for i in range(n):
            hrow[7 * i:7 * i + 7] = toks[i][s_][:, 0].cuda()
            p[7 * i:7 * i + 7] = S + s_
        got.append(eng.llm_decode_rows(hrow, p, pool, Smax).clone())
    # (a) the <= 16-row FP8 kernel on each generate's own cache: same bits
    for i in (0, n - 1):
        kv, _ = eng.new_kv(7, Smax, reuse=False)
        eng.llm_forward(hs[i].cuda().clone(), 0, kv, Smax)
        for s_ in range(steps):
            want = eng.llm_forward(toks[i][s_].cuda().clone(), S + s_, kv, Smax)
            assert torch.equal(got[s_][7 * i:7 * i + 7], want), (i, s_)
    # (b) the oracle with the same fake-quantised decode weights (prefill on the bf16 weights), generates 0 and n - 1
    w = {k: T(v) for k, v in synth.build_numpy(synth.llama_spec(shape), SEED).items()}
    w = {k: (v.to(op()).float() if v.dim() == 2 else v) for k, v in w.items()}
    cfg = llama.LlamaCfg(shape.hidden, shape.inter, shape.layers, shape.heads, shape.vocab, shape.eps, shape.theta)
    w8 = llama.fp8_decode_weights(w, cfg)
    for i in (0, n - 1):
        cache = llama.KVCache(cfg.layers)
        llama.forward(hs[i], w, cfg, cache=cache, last_only=True)
        for s_ in range(steps):
            want = llama.forward(toks[i][s_], w8, cfg, cache=cache)[:, -1]
            want16 = None
            assert rel_err(got[s_][7 * i:7 * i + 7].cpu(), want) < 2e-2, (i, s_)
    # it really is the quantised weights that ran: switching the copies off changes the logits
    eng.set_option("fp8_decode", 0)
    hrow = torch.zeros(R, D, device="cuda:0")
    p = torch.full((R,), S + steps, dtype=torch.int32, device="cuda:0")
    a16 = eng.llm_decode_rows(hrow + 0.01, p, pool, Smax).clone()
    eng.set_option("fp8_decode", 1)
    p2 = torch.full((R,), S + steps, dtype=torch.int32, device="cuda:0")
    a8 = eng.llm_decode_rows(hrow + 0.01, p2, pool, Smax)
    assert not torch.equal(a16, a8)


# ---- the device-side promises of the merged decode step (include/revision_hip.h, rv_llm_decode_rows / rv_llm_decode_rows_shared): positions at the
# ---- pool's capacity, the share hint, violating hint words.  Positions and hints live on the device - nothing can be returned for them, so every
# ---- pool here is a VIEW into a larger zero tensor (one cache row of slack on either side) and a stray store or read stays in memory the test owns.
class _GuardedPool:
    """A KV pool of R rows ([L, R, H, Smax, 128] + its V^T twin) between two guard bands of one cache row (H * Smax * 128 elements) each."""

    def __init__(self, eng, L, R, H, Smax, big=None):
        self.eng, self.L, self.R, self.H, self.Smax = eng, L, R, H, Smax
        self.n = eng.lib.rv_kv_bytes(eng._ctx, R, Smax) // 2
        assert self.n == 2 * L * R * H * Smax * 128
        self.band = H * Smax * 128
        self.big = torch.zeros(self.n + 2 * self.band, dtype=eng.op_dtype, device="cuda:0") if big is None else big
        self.kv = self.big[self.band:self.band + self.n]          # what the engine is given

    def clone(self):
        return _GuardedPool(self.eng, self.L, self.R, self.H, self.Smax, self.big.clone())

    def k(self):
        return self.kv[:self.n // 2].view(self.L, self.R, self.H, self.Smax, 128)

    def vt_raw(self):          # (blocked by 8 positions, as on the device)
        return self.kv[self.n // 2:].view(self.L, self.R, self.H, self.Smax // 8, 128, 8)

    def vt(self):              # logical [L, R, H, 128, Smax], as 16-bit patterns
        return self.eng.vt_logical(self.kv[self.n // 2:].view(torch.int16), self.L, self.R, self.H, Smax=self.Smax)

    def bits(self):            # the whole tensor, guard bands included, as 16-bit patterns (byte-for-byte comparisons)
        return self.big.view(torch.int16)

    def guards_clean(self):
        b = self.bits()
        return not bool(b[:self.band].any()) and not bool(b[self.band + self.n:].any())

    def own_cache_of(self, r):
        """A cache of its own (one row) holding the bytes of row r."""
        kv1, _ = self.eng.new_kv(1, self.Smax, reuse=False)
        h1 = kv1.numel() // 2
        kv1[:h1].view(self.L, 1, self.H, self.Smax, 128).copy_(self.k()[:, r:r + 1])
        kv1[h1:].view(self.L, 1, self.H, self.Smax // 8, 128, 8).copy_(self.vt_raw()[:, r:r + 1])
        return kv1


def _changed_positions(after, before):
    """-> (K, V^T) bool [L, R, H, Smax]: the positions of every (layer, row, head) at which at least one byte differs between two pools."""
    dk = (after.k().view(torch.int16) != before.k().view(torch.int16)).any(-1)
    dv = (after.vt() != before.vt()).any(-2)
    return dk, dv


_EDGE_SMAX, _EDGE_S = 160, 96


class _EdgeSetup:
    """What the edge tests of one flavour share: the engines (2 blocks with 16-bit decode weights / 1 block with the FP8 copies, as the FP8 test above) and,
    per row count, ONE prefilled guard-banded pool of per-row DIFFERENT caches (never stepped: every test works on clones)."""

    def __init__(self):
        self.engs, self.pools = {}, {}

    def eng(self, fp8=False):
        if fp8 not in self.engs:
            if fp8:
                from revisionllm_amd import engine
                from revisionllm_amd.utils import synth
                e = engine.Engine(synth.LlamaShape(layers=1, vocab=2048), adapter_text=False, device="cuda:0")
                e.init_synthetic(seed=SEED, llm=True, clip=False, fp8_decode=True)
            else:
                e = _engine(layers=2, vocab=2048)
            self.engs[fp8] = e
        return self.engs[fp8]

    def pool(self, R, fp8=False, P0=0):
        """R rows prefilled in one pass to _EDGE_S positions: P0 = 0 - every row its own random prompt; P0 > 0 - the first P0 positions shared."""
        key = (R, fp8, P0)
        if key not in self.pools:
            eng = self.eng(fp8)
            p = _GuardedPool(eng, 1 if fp8 else 2, R, 32, _EDGE_SMAX)
            g = torch.Generator().manual_seed(1000 + R + P0)
            h = torch.randn(P0 + R * (_EDGE_S - P0), 4096, generator=g).mul(0.02).cuda()
            lg = eng.llm_prefill_pool(h, R, P0, p.kv, R, 0, _EDGE_SMAX)
            assert torch.isfinite(lg).all() and p.guards_clean()
            self.pools[key] = p
        return self.pools[key]


@pytest.fixture(scope="module")
def edge(op_flavour):
    s = _EdgeSetup()
    yield s
    s.pools.clear()
    s.engs.clear()


def _capacity_case(eng, before, R, D, S, check_own_cache):
    """Assertions 1 - 3 (and 4) of the capacity tests on a prefilled pool ``before`` (S positions per row; modified here: pass a clone)."""
    L, H, Smax = before.L, before.H, before.Smax
    last, picked = 5, [0, 2, R - 1, 4]                       # the row at the last legal slot; the rows that go past capacity (first and last row among them)
    g = torch.Generator().manual_seed(77 + R)
    # the Smax - 1 row attends to EVERY slot of its cache: positions S .. Smax - 2 hold finite random operand values, written directly
    before.k()[:, last, :, S:Smax - 1] = torch.randn(L, H, Smax - 1 - S, 128, generator=g).mul(0.5).to(eng.op_dtype).cuda()
    assert S % 8 == 0
    before.vt_raw()[:, last, :, S // 8:] = torch.randn(L, H, (Smax - S) // 8, 128, 8, generator=g).mul(0.5).to(eng.op_dtype).cuda()
    before.vt_raw()[:, last, :, -1, :, 7] = 0                 # (slot Smax - 1 itself: the step writes it)
    hrow = torch.randn(R, D, generator=g).mul(0.02).cuda()
    pos_a = torch.full((R,), S, dtype=torch.int32)
    pos_a[last] = Smax - 1
    pos_a[picked] = -1
    pos_b = pos_a.clone()
    pos_b[picked] = torch.tensor([Smax, Smax + 7, Smax + 32, -1], dtype=torch.int32)      # (no further: the overshoot of a missed guard stays inside the band)
    in_range = [r for r in range(R) if r not in picked]
    pa, pb = before.clone(), before.clone()
    la = eng.llm_decode_rows(hrow.clone(), pos_a.cuda(), pa.kv, Smax)
    lb = eng.llm_decode_rows(hrow.clone(), pos_b.cuda(), pb.kv, Smax)
    assert pa.guards_clean() and pb.guards_clean()
    # 1. the in-range rows do not see what the others are
    assert torch.isfinite(la[in_range]).all() and torch.equal(la[in_range], lb[in_range])
    # 2. rows past capacity stored nothing, anywhere: the same bytes as with those rows inactive
    assert torch.equal(pa.bits(), pb.bits())
    # 3. against the pool before the step: exactly position row_pos[r] of every in-range row r changed, in every layer and head, in K and in V^T
    want = torch.zeros(R, Smax, dtype=torch.bool)
    want[in_range, pos_a[in_range].long()] = True
    want = want.cuda()[None, :, None, :].expand(L, R, H, Smax)
    dk, dv = _changed_positions(pb, before)
    assert torch.equal(dk, want) and torch.equal(dv, want)
    if check_own_cache:
        # 4. the row at the last legal slot: what rv_llm_forward(S = 1, pos0 = Smax - 1) gives for it alone, on a cache of its own holding the same bytes
        kv1 = before.own_cache_of(last)
        one = eng.llm_forward(hrow[last].clone().view(1, 1, D), Smax - 1, kv1, Smax)
        assert torch.equal(lb[last:last + 1], one)
        assert torch.equal(kv1.view(torch.int16), pb.own_cache_of(last).view(torch.int16))


@pytest.mark.parametrize("fp8", [False, True], ids=["w16", "fp8"])
@pytest.mark.parametrize("R", [7, 24, 40, 140])
def test_rows_at_and_past_the_pools_capacity(edge, R, fp8):
    """rv_llm_decode_rows, the header's promise: "a row with row_pos[r] >= Smax is treated like an inactive one - nothing is stored, no other row's cache is
    touched".  One step with most rows at 96, one at Smax - 1 = 159 (the last legal slot; its cache behind 96 filled by hand) and four rows inactive,
    against the same step with three of the four at Smax, Smax + 7 and Smax + 32: in-range logits bit-identical, the pools byte-identical (guard bands
    included), only position row_pos[r] of the in-range rows changed; the 159 row equals rv_llm_forward(S = 1, pos0 = 159) on a cache of its own.
    R = 7 / 24: the weight-streaming kernels' store (kernels.h qkv_rope_store_t); 40 / 140: the wide kernel's (gemm_rows.hip rows_qkv_finish), split and
    persistent; the attention's guard (attention.hip attn_body) in all of them; 16-bit and FP8 decode weights."""
    _capacity_case(edge.eng(fp8), edge.pool(R, fp8).clone(), R, 4096, _EDGE_S, True)


@pytest.mark.parametrize("R", [7, 24])
def test_rows_at_and_past_the_pools_capacity_parity_precision(R):
    """The same in the parity precision, whose q / k / v rows are rotated and appended by the stand-alone kernel (rowops.hip qkv_rope_split_kernel ->
    qkv_rope_store_t<true>): the tiny model, Smax = 64, rows at 40, one at 63, three at 64 / 71 / 96."""
    eng = _tiny_model(parity=True).engine
    L, H, D, Smax, S = 3, 4, 512, 64, 40
    p = _GuardedPool(eng, L, R, H, Smax)
    h = torch.randn(R * S, D, generator=torch.Generator().manual_seed(R)).mul(0.02).cuda()
    assert torch.isfinite(eng.llm_prefill_pool(h, R, 0, p.kv, R, 0, Smax)).all() and p.guards_clean()
    _capacity_case(eng, p, R, D, S, False)


def _word(sibling, length):
    return sibling | length << 16


@pytest.mark.parametrize("R", [7, 40, 140])
def test_share_hint_is_followed_for_whole_key_blocks_only(edge, R):
    """rv_llm_decode_rows_shared on a pool whose rows hold DIFFERENT caches, so that following a hint shows: a row with the word sibling | len << 16 reads
    the whole 32-key blocks below len (n = 32 * (len // 32) positions) from the sibling's cache rows and everything else from its own.  The hinted step on
    the original pool against the NULL-hint step on a pool in which those positions were COPIED from the siblings: logits and the K / V^T appended at
    96 bit-identical (the second block's K / V depend on the first block's attention).  Siblings below and above the row (the offset's sign), the row
    itself, an inactive sibling; len 31 / 32 / 33 / 64 / 95 / 97 = row_pos + 1.  (Logits of the one inactive row are unspecified: not compared.)"""
    eng, base = edge.eng(), edge.pool(R)
    Smax, pos0 = _EDGE_SMAX, _EDGE_S
    idle = 6
    hints = [(0, 3, 97), (1, 0, 31), (2, 5, 32), (3, 1, 33), (4, 4, 64), (5, idle, 95)]            # (row, sibling, len)
    if R > 7:
        hints += [(R - 1, 0, 64), (8, R - 2, 97), (R - 2, R - 1, 95), (9, idle, 33), (R // 2, R // 2, 97)]
    pos = torch.full((R,), pos0, dtype=torch.int32)
    pos[idle] = -1
    active = [r for r in range(R) if r != idle]
    share = torch.zeros(R, dtype=torch.int32)
    expect = base.clone()
    for r, s, ln in hints:
        assert s < R and ln <= pos0 + 1
        share[r] = _word(s, ln)
        n = 32 * (ln // 32)
        expect.k()[:, r, :, :n] = base.k()[:, s, :, :n]
        expect.vt_raw()[:, r, :, :n // 8] = base.vt_raw()[:, s, :, :n // 8]
    hrow = torch.randn(R, 4096, generator=torch.Generator().manual_seed(5 + R)).mul(0.02).cuda()
    hinted, plain = base.clone(), base.clone()
    lh = eng.llm_decode_rows(hrow.clone(), pos.cuda(), hinted.kv, Smax, row_share=share.cuda())
    le = eng.llm_decode_rows(hrow.clone(), pos.cuda(), expect.kv, Smax)
    ln_ = eng.llm_decode_rows(hrow.clone(), pos.cuda(), plain.kv, Smax)
    assert hinted.guards_clean() and expect.guards_clean() and plain.guards_clean()
    assert torch.isfinite(lh[active]).all() and torch.equal(lh[active], le[active])
    assert torch.equal(hinted.k()[:, :, :, pos0].view(torch.int16), expect.k()[:, :, :, pos0].view(torch.int16))
    assert torch.equal(hinted.vt()[..., pos0], expect.vt()[..., pos0])
    dk, dv = _changed_positions(hinted, base)                  # a hint is about READS: the hinted step stores what any step stores
    want = torch.zeros(R, Smax, dtype=torch.bool)
    want[active, pos0] = True
    want = want.cuda()[None, :, None, :].expand(2, R, 32, Smax)
    assert torch.equal(dk, want) and torch.equal(dv, want)
    # not vacuous: a followed hint shows in the row's logits; len 31 (no whole block) and the row itself read what the NULL hint reads
    for r, s, ln in hints:
        same = torch.equal(lh[r], ln_[r])
        assert same == (ln < 32 or s == r), (r, s, ln)
    hinted_rows = [r for r, _, _ in hints]
    others = [r for r in active if r not in hinted_rows]
    assert torch.equal(lh[others], ln_[others])


@pytest.mark.parametrize("R", [7, 40, 140])
def test_share_hint_on_identical_prefixes_changes_nothing(edge, R):
    """Where the prefix really is identical (rv_llm_prefill_pool with a shared prefix of 40 positions leaves it in all R rows) the hint sibling = 0, len = 40
    in every row cannot change a result: logits and the whole pool bit-identical to the NULL-hint step."""
    eng, base = edge.eng(), edge.pool(R, P0=40)
    assert torch.equal(base.k()[:, 1:, :, :40], base.k()[:, :1, :, :40].expand(-1, R - 1, -1, -1, -1)) and not torch.equal(base.k()[:, 1, :, 40:96], base.k()[:, 0, :, 40:96])
    pos = torch.full((R,), _EDGE_S, dtype=torch.int32, device="cuda:0")
    share = torch.full((R,), _word(0, 40), dtype=torch.int32, device="cuda:0")
    hrow = torch.randn(R, 4096, generator=torch.Generator().manual_seed(9 + R)).mul(0.02).cuda()
    hinted, plain = base.clone(), base.clone()
    lh = eng.llm_decode_rows(hrow.clone(), pos, hinted.kv, _EDGE_SMAX, row_share=share)
    lp = eng.llm_decode_rows(hrow.clone(), pos, plain.kv, _EDGE_SMAX)
    assert torch.isfinite(lh).all() and torch.equal(lh, lp) and torch.equal(hinted.bits(), plain.bits()) and hinted.guards_clean()


@pytest.mark.parametrize("R", [7, 40])
def test_violating_hint_words_are_ignored_and_bad_calls_refused(edge, R):
    """"A word that violates [the contract] is IGNORED by the kernel (the row reads its own cache), never followed out of bounds": sibling = R (the first row
    outside the pool), len = row_pos + 2, a word with the sign bit set and -1, each in a row of its own next to rows with valid hints - the violating rows'
    logits and cache rows are those of the NULL-hint step, the guard bands stay zero.  And what the HOST can see is refused with RV_ERR_ARG before anything is
    launched - R = 0, R = 145, Smax = 100, Smax = 65536 (shared entry), a NULL row_pos - after which the context still gives the baseline logits."""
    from revisionllm_amd import hip
    eng, base = edge.eng(), edge.pool(R)
    Smax, pos0, D, V = _EDGE_SMAX, _EDGE_S, 4096, 2048
    bad = {1: _word(R, 64), 3: _word(0, pos0 + 2), 4: _word(1, 64) - (1 << 31), 6: -1}
    good = {2: _word(5, 64), 5: _word(0, 97)}
    if R > 7:
        bad.update({R - 1: _word(R, 97), 20: _word(0, 32767), 21: -(1 << 31)})
        good.update({R - 2: _word(7, 96)})
    share = torch.zeros(R, dtype=torch.int32)
    for r, w in {**bad, **good}.items():
        share[r] = w
    pos = torch.full((R,), pos0, dtype=torch.int32, device="cuda:0")
    hrow = torch.randn(R, D, generator=torch.Generator().manual_seed(13 + R)).mul(0.02).cuda()
    hinted, plain = base.clone(), base.clone()
    lh = eng.llm_decode_rows(hrow.clone(), pos, hinted.kv, Smax, row_share=share.cuda())
    lp = eng.llm_decode_rows(hrow.clone(), pos, plain.kv, Smax)
    assert hinted.guards_clean() and plain.guards_clean()
    unhinted = [r for r in range(R) if r not in good]
    assert torch.isfinite(lh).all() and torch.equal(lh[unhinted], lp[unhinted])
    assert torch.equal(hinted.k()[:, unhinted].view(torch.int16), plain.k()[:, unhinted].view(torch.int16))
    assert torch.equal(hinted.vt_raw()[:, unhinted].view(torch.int16), plain.vt_raw()[:, unhinted].view(torch.int16))
    for r in good:                                             # (the valid hints of the same step WERE followed)
        assert not torch.equal(lh[r], lp[r]), r
    # ---- host-side refusals
    big_h = torch.zeros(145, D, device="cuda:0")
    big_pos = torch.full((145,), pos0, dtype=torch.int32, device="cuda:0")
    big_share = torch.zeros(145, dtype=torch.int32, device="cuda:0")
    lg = torch.empty(145, V, device="cuda:0")
    ws = eng._workspace("llm", eng.lib.rv_llm_ws_bytes(eng._ctx, 144, 1))
    kv = base.clone()

    def call(shared, R_, Smax_, row_pos):
        if shared:
            rc = eng.lib.rv_llm_decode_rows_shared(eng._ctx, hip.ptr(big_h), R_, hip.ptr(row_pos), hip.ptr(big_share), hip.ptr(kv.kv), Smax_, hip.ptr(lg), hip.ptr(ws),
                                                   ws.numel(), hip.stream())
        else:
            rc = eng.lib.rv_llm_decode_rows(eng._ctx, hip.ptr(big_h), R_, hip.ptr(row_pos), hip.ptr(kv.kv), Smax_, hip.ptr(lg), hip.ptr(ws), ws.numel(), hip.stream())
        hip.check(rc, "rv_llm_decode_rows_shared" if shared else "rv_llm_decode_rows")

    for shared in (False, True):
        for R_, Smax_, row_pos in ((0, Smax, big_pos), (145, Smax, big_pos), (R, 100, big_pos), (R, Smax, None)):
            with pytest.raises(hip.HipLibraryError, match=r"status -1"):
                call(shared, R_, Smax_, row_pos)
    with pytest.raises(hip.HipLibraryError, match=r"status -1"):
        call(True, R, 65536, big_pos)
    torch.cuda.synchronize()
    assert torch.equal(kv.bits(), base.bits())                 # nothing was launched
    again = base.clone()
    assert torch.equal(eng.llm_decode_rows(hrow.clone(), pos, again.kv, Smax), lp) and torch.equal(again.bits(), plain.bits())


_SWEEP_POS = (1, 30, 31, 32, 33, 63, 64, 95, 96, 126, 127, 128, 129, 130)


def test_positions_at_key_block_edges_vs_float64_oracle():
    """One merged step of a 40-row pool (one Vicuna-7B-shaped block + lm_head, prefilled to 130 positions, Smax = 160) with 14 rows at the positions 1, 30, 31,
    32, 33, 63, 64, 95, 96, 126, 127, 128, 129 and 130 - the key counts at which the split decode attention has waves without a block, an exactly full last
    block, a last block of one key - and the others inactive.  A row stepping at p < 130 overwrites slot p and sees the keys 0 .. p (what the ragged prefill
    relies on).  Each stepped row against oracle.llama.forward in float64 on its first p prompt rows + the step's row, and bit-identical to
    rv_llm_forward(S = 1, pos0 = p) on a cache of its own.
    Largest rel_err over the 14 rows, measured on an MI355X: fp16 1.224e-3 (rows 7.9e-4 .. 1.2e-3), bf16 9.102e-3 (5.2e-3 .. 9.1e-3) - no position stands
    out.  The house rule (~2.5 x the measured value: 3.1e-3 / 2.3e-2) would be LOOSER than the tol(1.2e-2) that test_llm_prefill_and_decode asserts (2e-3 in
    fp16, 1.2e-2 in bf16), so that bound is the one asserted; the kernels are deterministic, the margin (1.6 x / 1.3 x) is not a statistical one."""
    from oracle import llama
    from revisionllm_amd import engine
    from revisionllm_amd.utils import synth
    shape = synth.LlamaShape(layers=1, vocab=2048)
    eng = engine.Engine(shape, adapter_text=False, device="cuda:0")
    eng.init_synthetic(seed=SEED, llm=True, clip=False)
    D, R, S, Smax = 4096, 40, 130, 160
    g = torch.Generator().manual_seed(130)
    hs = torch.randn(R, S, D, generator=g).mul(0.02)
    tok = torch.randn(R, D, generator=g).mul(0.02)
    rows = [3 * i for i in range(len(_SWEEP_POS))]              # 0, 3, .. 39: in all three 16-row blocks of the wide kernel (the third holds 8 rows)
    pool = _GuardedPool(eng, 1, R, 32, Smax)
    eng.llm_prefill_pool(hs.cuda().view(R * S, D).contiguous(), R, 0, pool.kv, R, 0, Smax)
    before = pool.clone()
    pos = torch.full((R,), -1, dtype=torch.int32)
    pos[rows] = torch.tensor(_SWEEP_POS, dtype=torch.int32)
    got = eng.llm_decode_rows(tok.cuda().clone(), pos.cuda(), pool.kv, Smax)
    assert pool.guards_clean() and torch.isfinite(got[rows]).all()
    for r, p in zip(rows, _SWEEP_POS):
        one = eng.llm_forward(tok[r].cuda().clone().view(1, 1, D), p, before.own_cache_of(r), Smax)
        assert torch.equal(got[r:r + 1], one), p
    w = {k: T(v) for k, v in synth.build_numpy(synth.llama_spec(shape), SEED).items()}
    w = {k: (v.to(op()).double() if v.dim() == 2 else v.double()) for k, v in w.items()}
    cfg = llama.LlamaCfg(shape.hidden, shape.inter, shape.layers, shape.heads, shape.vocab, shape.eps, shape.theta)
    got = got.cpu()
    worst = 0.0
    for r, p in zip(rows, _SWEEP_POS):
        x = torch.cat([hs[r, :p], tok[r:r + 1]])[None].double()
        ref = llama.forward(x, w, cfg, last_only=True)[0, -1]
        assert ref.dtype == torch.float64
        worst = max(worst, rel_err(got[r], ref))
    print(f"positions sweep ({fl()}): largest rel_err over {len(rows)} rows {worst:.3e}")
    assert worst < tol(1.2e-2)


def test_handoff_status_travels_as_one_snapshot_and_still_raises():
    """Round 4: the hand-off status words of all workspaces go to pinned host memory as ONE snapshot behind a recursion's results
    (``Engine.handoff_status_async``) instead of one ``.item()`` per workspace when the record is collected.  A clean run yields a clean
    snapshot; a status word that a kernel's bounded wait would have set is reported through the snapshot AND through the synchronous
    form, names its workspace, and is cleared so that the next check is clean again."""
    from revisionllm_amd import hip
    m = _tiny_model()
    eng = m.engine
    P = 40
    from revisionllm_amd.utils import synth
    ids = T(synth.synthetic_prompt_ids(P, 20, SEED, vocab=synth.TINY.vocab))[None]
    feat = feats("status.feat", (1, 6, 16, 768), bf16=fl())
    q = (feats("status.q", (1, 5, 768), bf16=fl()), torch.ones(1, 5))
    m.generate(ids, images=feat, query_feats=q, do_sample=False, max_new_tokens=3)       # workspaces exist now
    snap = eng.handoff_status_async()
    assert snap is not None and len(snap[0]) == snap[1].numel() >= 1
    torch.cuda.synchronize()
    eng.check_handoff_status(snap)                                                         # clean
    eng.check_handoff_status()
    key = snap[0][0]
    eng._ws[key][8188:8192].view(torch.int32).fill_(1)                                     # what a timed-out in-kernel wait writes
    bad = eng.handoff_status_async()
    torch.cuda.synchronize()
    with pytest.raises(hip.HipLibraryError, match="hand-off wait timed out"):
        eng.check_handoff_status(bad)
    eng.check_handoff_status()                                                             # cleared by the failed check
    eng._ws[key][8188:8192].view(torch.int32).fill_(1)
    with pytest.raises(hip.HipLibraryError, match="hand-off wait timed out"):
        eng.check_handoff_status()
    eng.check_handoff_status()
