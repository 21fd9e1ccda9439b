"""GPU parity tests: every HIP entry point, called through the C ABI, against the CPU oracle on the same
seeded inputs.  Both sides see identical (bf16-representable) weights and inputs, so differences come only
from bf16 activation rounding between kernels and fp32 accumulation order.  Tolerances are stated per test:
  f32 outputs of a single kernel ........ 2e-5 relative (max-norm)
  bf16 outputs / chained bf16 kernels ... 8e-3 relative (bf16 eps = 3.9e-3; measured <= 3.8e-3), full adapter / logits 1e-2
"""
import math

import numpy as np
import pytest
import torch

from helpers import SEED, T, clip_weights, feats, fl, linear_weights, llama_weights, op, rel_err, tol

pytestmark = pytest.mark.gpu

F32_TOL = 2e-5
BF16_TOL = 8e-3        # bf16 flavour (measured <= 3.8e-3: one bf16 rounding of the output + bf16 inputs); the fp16 flavour is held to 1/6 of it (helpers.tol; measured <= 5.9e-4)


@pytest.fixture(scope="module")
def dev(op_flavour):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import hip
    hip.lib()  # fail loudly if the extension is missing
    return torch.device("cuda:0")


def bf(x):
    return x.to(op())


def test_abi_version(dev):
    from revisionllm_amd import hip
    assert hip.lib().rv_abi_version() == 5 and hip.lib().rv_operand_dtype() == hip.dtype_code(torch.empty(0, dtype=op()))


def test_init_hash_bit_exact(dev):
    from revisionllm_amd import ops
    from revisionllm_amd.utils import hashinit
    for n, a, base in ((1000, 0.02, 0.0), (70001, 0.1, 1.0)):
        ref = hashinit.hash_uniform(n, hashinit.tensor_key("x.y", 3), a, base)
        t = ops.init_hash_(torch.empty(n, device=dev), "x.y", 3, a, base)
        assert np.array_equal(t.cpu().numpy(), ref)
        tb = ops.init_hash_(torch.empty(n, dtype=op(), device=dev), "x.y", 3, a, base)
        assert np.array_equal(tb.float().cpu().numpy(), hashinit.round_op(ref, fl()))
    # offset form used for sub-blocks
    ref = hashinit.hash_uniform(500, hashinit.tensor_key("x.y", 3), 0.02, 0.0, offset=123)
    t = ops.init_hash_(torch.empty(500, device=dev), "x.y", 3, 0.02, 0.0, offset=123)
    assert np.array_equal(t.cpu().numpy(), ref)


@pytest.mark.parametrize("M,N,K", [(300, 768, 768), (130, 512, 1408), (1190, 4096, 512), (257, 2304, 768), (1, 4096, 4096),
                                    (7, 1024, 11008), (16, 32000, 512), (17, 768, 2048), (100, 4096, 768), (1197, 4096, 4096),
                                    (1057, 22016, 1024), (5000, 1536, 768), (129, 256, 11008),
                                    # >= 8 row tiles of 256 (batched prefills): the stream-K teams take groups of 4 / 2 adjacent panels (last group ragged)
                                    (2010, 2560, 1024), (4020, 4352, 2048), (3000, 1280, 4096),
                                    # 32 row tiles (8 prefills to a pass): teams of a QUARTER of the m-tiles x 4 panels
                                    (8040, 4352, 2048)])
@pytest.mark.parametrize("out", ["bf16", "f32"])
def test_gemm(dev, M, N, K, out):
    from revisionllm_amd import hip, ops
    a = feats(f"gemm.a.{M}.{K}", (M, K), bf16=fl())
    w = feats(f"gemm.w.{N}.{K}", (N, K), bf16=fl()) * (1.0 / math.sqrt(K))
    w = bf(w).float()
    bias = feats(f"gemm.b.{N}", (N,))
    res = feats(f"gemm.r.{M}.{N}", (M, N))
    od = op() if out == "bf16" else torch.float32
    tol_ = tol(BF16_TOL) if out == "bf16" else F32_TOL * 5
    ad, wd = bf(a).to(dev), bf(w).to(dev)
    ref0 = a.double() @ w.double().t()
    y = ops.gemm(ad, wd, out_dtype=od)
    assert rel_err(y.float().cpu(), ref0) < tol_
    wpk = ops.pack_fragments(wd) if N % 16 == 0 else None          # fragment-packed layout (what the engine binds)
    if wpk is not None:
        yp = ops.gemm(ad, wpk, out_dtype=od, w_packed=True, stream_k=False)
        assert torch.equal(yp, y)                                    # same arithmetic, different HBM layout -> bit-identical
        for variant in (0, 1, 3, 4, 6):                              # other pipelines (4 = 256x256 ping-pong): same sums, same order
            opt = hip.Options(gemm_tile_variant=variant, gemm_arows=0)
            assert torch.equal(ops.gemm(ad, wpk, out_dtype=od, w_packed=True, stream_k=False, ctx=opt), y)
        for variant in (5, 2):                                       # persistent stream-K ping-pong: forced / where the policy picks it
            opt = hip.Options(gemm_tile_variant=variant)
            ys = ops.gemm(ad, wpk, out_dtype=od, w_packed=True, stream_k=True, ctx=opt)
            assert rel_err(ys.float().cpu(), ref0) < tol_
            for _ in range(3):                                       # fixed split-k summation order: deterministic (and a race screen)
                assert torch.equal(ys, ops.gemm(ad, wpk, out_dtype=od, w_packed=True, stream_k=True, ctx=opt))
    y = ops.gemm(ad, wd, bias=bias.to(dev), residual=res.to(dev), out_dtype=od, act=hip.RV_ACT_RELU)
    ref = torch.relu(ref0 + bias.double()) + res.double()
    assert rel_err(y.float().cpu(), ref) < tol_
    if N % 32 == 0:
        y = ops.gemm(ad, wd, out_dtype=od, act=hip.RV_ACT_SILU_MUL)
        assert torch.equal(ops.gemm(ad, wpk, out_dtype=od, act=hip.RV_ACT_SILU_MUL, w_packed=True, stream_k=False), y)
        r3 = ref0.view(M, N // 32, 2, 16)
        ref = (torch.nn.functional.silu(r3[:, :, 0]) * r3[:, :, 1]).reshape(M, N // 2)
        assert rel_err(y.float().cpu(), ref) < tol_
        for variant in (4, 5):
            opt = hip.Options(gemm_tile_variant=variant)
            ys = ops.gemm(ad, wpk, bias=None, out_dtype=od, act=hip.RV_ACT_SILU_MUL, w_packed=True, stream_k=True, ctx=opt)
            assert rel_err(ys.float().cpu(), ref) < tol_
        if wpk is not None:                                          # bias + relu + residual epilogue of the ping-pong kernels
            for variant in (4, 5):
                opt = hip.Options(gemm_tile_variant=variant)
                ys = ops.gemm(ad, wpk, bias=bias.to(dev), residual=res.to(dev), out_dtype=od, act=hip.RV_ACT_RELU, w_packed=True, stream_k=True, ctx=opt)
                assert rel_err(ys.float().cpu(), torch.relu(ref0 + bias.double()) + res.double()) < tol_


def _stream_k_piece_lengths(M, N, K, cus, mhalf=2):
    """Host mirror of launch_sk's work division (csrc/gemm_pp.hip): the set of k-tile counts of the stream-K pieces of a launch on ``cus`` CUs."""
    cdiv = lambda a, b: -(-a // b)      # noqa: E731
    tiles_m, tiles_n, nk, per_x = cdiv(M, 256), N // 256, K // 64, (cus & ~7) >> 3
    pg = per_x // tiles_m if (tiles_m >= 8 and per_x // tiles_m >= 2) else 1
    tm, mhs = tiles_m, 0
    if mhalf and tiles_m >= 10 and tiles_m % 2 == 0 and tiles_m <= per_x:
        tm2, pg2 = tiles_m // 2, per_x // (tiles_m // 2)
        if tm2 * pg2 > tiles_m * pg or (tm2 * pg2 == tiles_m * pg and tm2 + pg2 < tiles_m + pg):
            tm, pg, mhs = tm2, pg2, 1
        if mhs == 1 and mhalf >= 2 and tm >= 16 and tm % 2 == 0 and (tm // 2) * (per_x // (tm // 2)) >= tm * pg:
            tm, pg, mhs = tm // 2, per_x // (tm // 2), 2
    ts = tm * pg
    teams = 8 * (per_x // ts) if (pg > 1 or mhs) else (8 * (per_x // tiles_m) if tiles_m <= per_x else 0)
    groups = cdiv(tiles_n, pg) << mhs
    total = (groups - groups // teams * teams) * nk
    out = set()
    for t in range(teams):
        u, e = t * total // teams, (t + 1) * total // teams
        while u < e:
            n = min(nk - u % nk, e - u)
            out.add(n)
            u += n
    return out


@pytest.mark.parametrize("M,N,K,cus,short", [(1005, 22016, 2048, 256, {1, 2, 3}), (1005, 22016, 4096, 248, {2, 3}), (1005, 22016, 4096, 176, {3}),
                                             (1190, 22016, 4096, 216, {3}), (1005, 2560, 4096, 256, {2})])
def test_stream_k_pieces_of_one_two_and_three_k_tiles(dev, M, N, K, cus, short):
    """The k-split main loop of the persistent prefill GEMM (round 6) peels its last three k-tiles and shortens its prologue for work items of one or two
    k-tiles: launches whose stream-K tail is cut into pieces that short (found with the host mirror above; ``gemm_cus`` moves the cuts) against float64, plain
    and gated epilogues, and bit-stable over repeats."""
    from revisionllm_amd import hip, ops
    assert short <= _stream_k_piece_lengths(M, N, K, cus), "the work division changed: pick shapes that still cut pieces this short"
    a = feats(f"gemm.a.{M}.{K}", (M, K), bf16=fl())
    w = bf(feats(f"gemm.w.{N}.{K}", (N, K), bf16=fl()) * (1.0 / math.sqrt(K))).float()
    ad, wpk = bf(a).to(dev), ops.pack_fragments(bf(w).to(dev))
    ref0 = a.double() @ w.double().t()
    opt = hip.Options(gemm_tile_variant=5, gemm_cus=cus)
    y = ops.gemm(ad, wpk, out_dtype=op(), w_packed=True, stream_k=True, ctx=opt)
    assert rel_err(y.float().cpu(), ref0) < tol(BF16_TOL)
    for _ in range(3):
        assert torch.equal(y, ops.gemm(ad, wpk, out_dtype=op(), w_packed=True, stream_k=True, ctx=opt))
    if N % 512 == 0:
        yg = ops.gemm(ad, wpk, out_dtype=op(), act=hip.RV_ACT_SILU_MUL, w_packed=True, stream_k=True, ctx=opt)
        r3 = ref0.view(M, N // 32, 2, 16)
        assert rel_err(yg.float().cpu(), (torch.nn.functional.silu(r3[:, :, 0]) * r3[:, :, 1]).reshape(M, N // 2)) < tol(BF16_TOL)
        assert torch.equal(yg, ops.gemm(ad, wpk, out_dtype=op(), act=hip.RV_ACT_SILU_MUL, w_packed=True, stream_k=True, ctx=opt))


@pytest.mark.parametrize("M,N,K,act,out,res", [
    (25600, 4096, 768, 0, "bf16", False),      # dense projector, 100 windows x 256 frames (the "feature scan")
    (25700, 1536, 768, 0, "bf16", False),      # adapter Q/K projection (100 x 257 rows)
    (25700, 768, 768, 0, "f32", True),         # adapter out projection + residual (32-column wave slices)
    (25700, 2048, 768, 1, "bf16", False),      # adapter FFN-1 + ReLU
    (16385, 512, 1024, 3, "f32", False),       # K = 1024, QuickGELU, ragged rows (5 row fragments per workgroup)
    (13000, 256, 512, 0, "bf16", True),        # 4 fragments, a partly filled last workgroup
    (20000, 1024, 256, 1, "bf16", False),      # K = 256: one body of 8 k-steps per slice
    (102500, 768, 768, 0, "bf16", False),      # two rounds of workgroups (100 segments x 1025 rows)
])
def test_gemm_a_resident_kernel_is_bit_identical_to_the_ring_kernel(dev, M, N, K, act, out, res):
    """The A-resident kernel (gemm_arows.hip: a workgroup keeps its rows in LDS and walks N) accumulates every output in the same
    k order with the same MFMA as the 128x128 ring kernel, so results are BIT-identical; and correct against float64."""
    from revisionllm_amd import hip, ops
    g = torch.Generator().manual_seed(M + N + K)
    a = (torch.randn(M, K, generator=g) * 0.5).to(op()).to(dev)
    w = (torch.randn(N, K, generator=g) * (1.0 / math.sqrt(K))).to(op()).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    r = torch.randn(M, N, generator=g).to(dev) if res else None
    od = op() if out == "bf16" else torch.float32
    wp = ops.pack_fragments(w)
    ring = ops.gemm(a, wp, bias=bias, residual=r, out_dtype=od, act=act, w_packed=True, stream_k=False, ctx=hip.Options(gemm_arows=0))
    rows = ops.gemm(a, wp, bias=bias, residual=r, out_dtype=od, act=act, w_packed=True, stream_k=False, ctx=hip.Options(gemm_arows=1))
    assert torch.equal(ring, rows)
    assert torch.equal(rows, ops.gemm(a, wp, bias=bias, residual=r, out_dtype=od, act=act, w_packed=True, stream_k=False))   # default: on
    sel = torch.arange(0, M, max(1, M // 97), device=dev)                 # a sample of rows against float64
    z = a[sel].double() @ w.double().t() + bias.double()
    z = torch.relu(z) if act == 1 else (z * torch.sigmoid(1.702 * z) if act == 3 else z)
    if res:
        z = z + r[sel].double()
    assert rel_err(rows[sel].float().cpu(), z.cpu()) < (tol(BF16_TOL) if out == "bf16" else F32_TOL * 5)
    # a strided A (row stride > K), as the engine passes views
    big = torch.zeros(M, K + 64, dtype=op(), device=dev)
    big[:, :K] = a
    assert torch.equal(ops.gemm(big[:, :K], wp, bias=bias, residual=r, out_dtype=od, act=act, w_packed=True, stream_k=False), rows)


@pytest.mark.parametrize("M,N,K,act,out,res", [
    (1005, 4096, 4096, 0, "f32", True),        # o projection of one recursion's prefill: pure split-k stream-K
    (1005, 22016, 4096, 2, "bf16", False),     # gate/up: whole panels + a stream-K tail, gated epilogue
    (4020, 22016, 4096, 2, "bf16", False),     # four prefills to a pass: teams of two panels
    (4020, 4096, 11008, 0, "f32", True),       # down projection
    (2010, 12288, 4096, 0, "bf16", False),
    (700, 4096, 11008, 0, "f32", False),       # ragged last row tile
])
def test_four_wave_persistent_gemm_is_bit_identical_to_the_eight_wave_form(dev, M, N, K, act, out, res):
    """Option gemm_waves = 4 (one wave per SIMD owning 128 x 128 outputs, accumulators in AGPRs; gemm_pp.hip pp4_mainloop) sums every
    output in the same k order with the same MFMA as the eight-wave ping-pong form, whole panels and stream-K shares alike: results are
    BIT-identical; and correct against float64 on a sample of rows."""
    from revisionllm_amd import hip, ops
    g = torch.Generator().manual_seed(M + N + K)
    a = (torch.randn(M, K, generator=g) * 0.5).to(op()).to(dev)
    w = (torch.randn(N, K, generator=g) * (1.0 / math.sqrt(K))).to(op()).to(dev)
    n_out = N // 2 if act == hip.RV_ACT_SILU_MUL else N
    r = torch.randn(M, n_out, generator=g).to(dev) if res else None
    od = op() if out == "bf16" else torch.float32
    wp = ops.pack_fragments(w)
    y8 = ops.gemm(a, wp, residual=r, out_dtype=od, act=act, w_packed=True, ctx=hip.Options(gemm_waves=8))
    y4 = ops.gemm(a, wp, residual=r, out_dtype=od, act=act, w_packed=True, ctx=hip.Options(gemm_waves=4))
    assert torch.equal(y8, y4)
    sel = torch.arange(0, M, max(1, M // 61), device=dev)
    z = a[sel].double() @ w.double().t()
    if act == hip.RV_ACT_SILU_MUL:                                   # gate / up rows interleaved in 16-row groups (ops.pack_fragments input order)
        z = z.view(len(sel), N // 32, 2, 16)
        z = (torch.nn.functional.silu(z[:, :, 0]) * z[:, :, 1]).reshape(len(sel), N // 2)
    if res:
        z = z + r[sel].double()
    assert rel_err(y4[sel].float().cpu(), z.cpu()) < (tol(BF16_TOL) if out == "bf16" else F32_TOL * 5)


@pytest.mark.parametrize("M,N,K,act,out,res", [
    (4020, 22016, 4096, 2, "bf16", False),     # 16 row tiles: teams of 8 x 4 tiles instead of 16 x 2; 86 panels: ragged last panel group + stream-K tail
    (4020, 4096, 11008, 0, "f32", True),       # down projection: 16 panels = 8 units of (4 panels, m-half), one per team
    (4020, 12288, 4096, 0, "f32", False),
    (3015, 4096, 4096, 0, "f32", True),        # 12 row tiles: 6 x 5 (30 workgroups per XCD instead of 24), 16 panels in groups of 5: ragged
    (2500, 22016, 4096, 2, "bf16", False),     # 10 row tiles: 5 x 6
])
def test_half_height_stream_k_teams_equal_the_full_height_teams(dev, M, N, K, act, out, res):
    """Option gemm_mhalf (round 4, gemm_pp.hip pp_sk_body): a team of the persistent stream-K GEMM covers half the row tiles of twice as many
    panels.  A tile that is computed whole sums the same k-tiles in the same order under both team shapes - bit-identical; only the panels
    of the stream-K tail (cut at different k) may differ in the last bits.  Both settings are checked against float64 on sampled rows."""
    from revisionllm_amd import hip, ops
    g = torch.Generator().manual_seed(M + N + K + 1)
    a = (torch.randn(M, K, generator=g) * 0.5).to(op()).to(dev)
    w = (torch.randn(N, K, generator=g) * (1.0 / math.sqrt(K))).to(op()).to(dev)
    n_out = N // 2 if act == hip.RV_ACT_SILU_MUL else N
    r = torch.randn(M, n_out, generator=g).to(dev) if res else None
    od = op() if out == "bf16" else torch.float32
    wp = ops.pack_fragments(w)
    y1 = ops.gemm(a, wp, residual=r, out_dtype=od, act=act, w_packed=True, ctx=hip.Options(gemm_mhalf=1, gemm_tile_variant=5))
    y0 = ops.gemm(a, wp, residual=r, out_dtype=od, act=act, w_packed=True, ctx=hip.Options(gemm_mhalf=0, gemm_tile_variant=5))
    y1b = ops.gemm(a, wp, residual=r, out_dtype=od, act=act, w_packed=True, ctx=hip.Options(gemm_mhalf=1, gemm_tile_variant=5))
    assert torch.equal(y1, y1b)                                       # deterministic for a given shape
    same = (y1 == y0).float().mean().item()
    assert same > 0.80, same                                          # whole panels: identical bits
    assert rel_err(y1.float().cpu(), y0.float().cpu()) < (tol(BF16_TOL) if out == "bf16" else 1e-5)
    sel = torch.arange(0, M, max(1, M // 61), device=dev)
    z = a[sel].double() @ w.double().t()
    if act == hip.RV_ACT_SILU_MUL:
        z = z.view(len(sel), N // 32, 2, 16)
        z = (torch.nn.functional.silu(z[:, :, 0]) * z[:, :, 1]).reshape(len(sel), N // 2)
    if res:
        z = z + r[sel].double()
    for y in (y1, y0):
        assert rel_err(y[sel].float().cpu(), z.cpu()) < (tol(BF16_TOL) if out == "bf16" else F32_TOL * 5)


@pytest.mark.parametrize("M,N,K", [(9, 1024, 256), (771, 4096, 1024), (1000, 1024, 4096)])
def test_gemm_quick_gelu_epilogue(dev, M, N, K):
    """bias + QuickGELU (x * sigmoid(1.702 x), the CLIP MLP activation) fused into the GEMM epilogue: every kernel family."""
    from revisionllm_amd import hip, ops
    a = feats(f"qg.a.{M}.{K}", (M, K), bf16=fl())
    w = bf(feats(f"qg.w.{N}.{K}", (N, K), bf16=fl()) * (1.0 / math.sqrt(K))).float()
    bias = feats(f"qg.b.{N}", (N,))
    z = a.double() @ w.double().t() + bias.double()
    ref = z * torch.sigmoid(1.702 * z)
    ad, wd = bf(a).to(dev), bf(w).to(dev)
    y = ops.gemm(ad, wd, bias=bias.to(dev), act=hip.RV_ACT_QUICK_GELU)
    assert rel_err(y.float().cpu(), ref) < tol(BF16_TOL)
    wpk = ops.pack_fragments(wd)
    for variant in (2, 4, 5, 6):
        opt = hip.Options(gemm_tile_variant=variant)
        yp = ops.gemm(ad, wpk, bias=bias.to(dev), act=hip.RV_ACT_QUICK_GELU, out_dtype=torch.float32, w_packed=True, stream_k=True, ctx=opt)
        assert rel_err(yp.cpu(), ref) < F32_TOL * 5


@pytest.mark.parametrize("M,N,K,act", [(7, 4096, 4096, 0), (1, 12288, 4096, 0), (16, 4096, 11008, 0), (7, 22016, 4096, 2), (3, 512, 1408 // 128 * 128, 0)])
def test_gemv_fp8_weights(dev, M, N, K, act):
    """Decode projection with FP8 (e4m3fn) fragment-packed weights + per-row scales against the same quantised weights in
    float64: the only differences are bf16 inputs (exact) and f32 accumulation."""
    from revisionllm_amd import hip, ops
    a = bf(feats(f"f8.a.{M}.{K}", (M, K), bf16=fl()))
    w = feats(f"f8.w.{N}.{K}", (N, K)) * (1.0 / math.sqrt(K))
    q, scale = ops.quantize_rows_fp8(w)
    wdq = q.float().double() * scale.double()[:, None]
    ref = a.double() @ wdq.t()
    w8, sc = ops.pack_fragments_fp8(w.to(dev))
    assert torch.equal(sc.cpu(), scale)
    if act == hip.RV_ACT_SILU_MUL:
        r3 = ref.view(M, N // 32, 2, 16)
        ref = (torch.nn.functional.silu(r3[:, :, 0]) * r3[:, :, 1]).reshape(M, N // 2)
        y = ops.gemv_fp8(a.to(dev), w8, sc, act=act, out_dtype=torch.float32)
        assert rel_err(y.cpu(), ref) < F32_TOL * 5
    else:
        res = feats(f"f8.r.{M}.{N}", (M, N))
        y = ops.gemv_fp8(a.to(dev), w8, sc, residual=res.to(dev), out_dtype=torch.float32)
        assert rel_err(y.cpu(), ref + res.double()) < F32_TOL * 5
        yb = ops.gemv_fp8(a.to(dev), w8, sc, out_dtype=op())
        assert rel_err(yb.float().cpu(), ref) < tol(BF16_TOL)


@pytest.mark.parametrize("M,N,K,act", [(1005, 4096, 4096, 0), (1005, 4096, 11008, 0), (1005, 22016, 4096, 2), (700, 4096, 11008, 0),
                                        (2010, 4096, 4096, 0), (2010, 4096, 11008, 0)])
def test_gemm_fp8_prefill(dev, M, N, K, act):
    """Opt-in FP8 x FP8 prefill GEMM (v_mfma_scale_f32_16x16x128_f8f6f4 on the persistent ping-pong kernel): the device
    quantiser reproduces the host quantiser's bytes and scales, and the product equals the float64 product of the same
    quantised operands up to f32 accumulation (asymmetric random operands: a swapped or permuted k would show)."""
    from revisionllm_amd import hip, ops
    x = bf(feats(f"f8p.x.{M}.{K}", (M, K), bf16=fl()))
    x[3] = 0                                                  # an all-zero row: scale 1, bytes 0
    w = feats(f"f8p.w.{N}.{K}", (N, K)) * (1.0 / math.sqrt(K))
    amax = x.float().abs().amax(dim=1)                          # the activation quantiser: IEEE f32, one reciprocal per row
    sx = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    qx = (x.float() * (1.0 / sx)[:, None]).to(torch.float8_e4m3fn)
    a8, sa = ops.quant_rows_fp8(x.to(dev))
    assert torch.equal(sa.cpu(), sx) and torch.equal(a8.cpu(), qx.view(torch.uint8))
    if K == 4096 and act == 0:                                  # fused RMSNorm + quantiser == quantiser(RMSNorm)
        h = feats(f"f8p.h.{M}", (M, K)).to(dev)
        wn = (1.0 + 0.1 * feats("f8p.wn", (K,))).to(dev)
        q1, s1 = ops.rmsnorm_quant_fp8(h, wn, 1e-5)
        q2, s2 = ops.quant_rows_fp8(ops.rmsnorm(h, wn, 1e-5))
        assert torch.equal(q1, q2) and torch.equal(s1, s2)
    qw, sw_ref = ops.quantize_rows_fp8(w)
    w8p, sw = ops.pack_fragments_fp8_prefill(w.to(dev))
    assert torch.equal(sw.cpu(), sw_ref)
    ref = (qx.float().double() @ qw.float().double().t()) * sx.double()[:, None] * sw_ref.double()[None]
    if act == hip.RV_ACT_SILU_MUL:
        r3 = ref.view(M, N // 32, 2, 16)
        ref = (torch.nn.functional.silu(r3[:, :, 0]) * r3[:, :, 1]).reshape(M, N // 2)
        y = ops.gemm_fp8(a8, sa, w8p, sw, act=act, out_dtype=op())
        assert rel_err(y.float().cpu(), ref) < tol(BF16_TOL)
    else:
        res = feats(f"f8p.r.{M}.{N}", (M, N))
        y = ops.gemm_fp8(a8, sa, w8p, sw, residual=res.to(dev), out_dtype=torch.float32)
        assert rel_err(y.cpu(), ref + res.double()) < F32_TOL * 5
        y2 = ops.gemm_fp8(a8, sa, w8p, sw, residual=res.to(dev), out_dtype=torch.float32)
        assert torch.equal(y, y2)                             # deterministic hand-off order


def test_gemm_fp8_prefill_refuses_shapes_without_a_plan(dev):
    """rv_gemm_fp8 exists in the persistent stream-K form only: a shape without a plan is an argument error with the
    reason, not a silent fall back to another kernel."""
    from revisionllm_amd import hip, ops
    a8 = torch.zeros(64, 512, dtype=torch.uint8, device=dev)
    sa = torch.ones(64, device=dev)
    w8p = torch.zeros(256 * 512, dtype=torch.uint8, device=dev)
    sw = torch.ones(256, device=dev)
    with pytest.raises(hip.HipLibraryError, match="no persistent FP8 plan"):
        ops.gemm_fp8(a8, sa, w8p, sw)


def test_gemm_strided_rows_and_inplace_residual(dev):
    from revisionllm_amd import ops
    x = bf(feats("gemm.s", (20, 5, 768), bf16=fl())).to(dev)
    w = bf(feats("gemm.sw", (4096, 768), bf16=fl()) * 0.03).to(dev)
    y = ops.gemm(x[:, 0], w, out_dtype=torch.float32)      # row stride 5*768 (CLS selection)
    assert rel_err(y.cpu(), x[:, 0].float().cpu() @ w.float().cpu().t()) < 1e-4
    h = feats("gemm.h", (20, 4096)).to(dev)
    h0 = h.clone()
    ops.gemm(x[:, 1].contiguous(), w, residual=h, out_dtype=torch.float32, out=h)  # C aliases the residual
    assert rel_err(h.cpu(), h0.cpu() + x[:, 1].float().cpu() @ w.float().cpu().t()) < 1e-4


def test_gemm_rejects_bad_arguments(dev):
    from revisionllm_amd import hip, ops
    a = torch.zeros(4, 100, dtype=op(), device=dev)
    w = torch.zeros(8, 100, dtype=op(), device=dev)
    with pytest.raises(hip.HipLibraryError, match="multiple of 64"):
        ops.gemm(a, w)


def test_layernorm_rmsnorm_sinepos(dev):
    from oracle import adapter, llama
    from revisionllm_amd import ops
    x = feats("ln.x", (37, 768)) * 3 + 0.5
    w, b = feats("ln.w", (768,)) * 0.1 + 1, feats("ln.b", (768,)) * 0.05
    pos = feats("ln.pos", (5, 768))
    y32, y16, yp = ops.layernorm(x.to(dev), w.to(dev), b.to(dev), pos=pos.to(dev), period=5)
    ref = torch.nn.functional.layer_norm(x, (768,), w, b, 1e-5)
    assert rel_err(y32.cpu(), ref) < F32_TOL
    assert rel_err(y16.float().cpu(), ref) < tol(BF16_TOL)
    refp = ref + pos[torch.arange(37) % 5]
    assert rel_err(yp.float().cpu(), refp) < tol(BF16_TOL)
    for d in (512, 4096):
        x = feats(f"rms.x{d}", (9, d)) * 2
        w = feats(f"rms.w{d}", (d,)) * 0.1 + 1
        y = ops.rmsnorm(x.to(dev), w.to(dev), 1e-5)
        assert rel_err(y.float().cpu(), llama.rmsnorm(x, w, 1e-5)) < tol(BF16_TOL)
    for Tn in (1, 16, 256, 1024):
        p = ops.sine_pos(Tn, 768, dev)
        assert (p.cpu() - adapter.sine_pos_embed(Tn)).abs().max() < 2e-5


def test_fp16_saturating_conversions_never_produce_inf(dev):
    """The range guard of the fp16 build: activations of magnitude 1e4 - inside fp16's range - go through norms, GEMMs,
    the gated epilogue and a whole Llama block without an inf or NaN, and still match the oracle; a GEMM OUTPUT beyond +-65504 stored as fp16 comes
    out as +-65504 (saturated), never inf, while the same product with an f32 output is exact.  (The bf16 build has fp32's exponent range: skipped.)"""
    if fl() != "f16":
        pytest.skip("fp16 range guard")
    from oracle import llama
    from revisionllm_amd import hip, ops
    from revisionllm_amd.utils import synth
    # (1) planted 1e4-magnitude activations: RMSNorm, LayerNorm and a GEMM on them are finite and right
    x = feats("sat.x", (40, 4096)) * 2
    x[:, 7] = 1.0e4
    x[3, 100:164] = -1.2e4
    w = feats("sat.w", (4096,)) * 0.1 + 1
    y = ops.rmsnorm(x.to(dev), w.to(dev), 1e-5)
    assert torch.isfinite(y).all() and rel_err(y.float().cpu(), llama.rmsnorm(x, w, 1e-5)) < tol(BF16_TOL)
    a = (feats("sat.a", (130, 512), bf16=fl()) * 1.0e4).clamp(-6.0e4, 6.0e4)          # |a| up to 1.7e4: representable, 3 x below the limit
    wm = bf(feats("sat.wm", (64, 512), bf16=fl()) * (1.0 / math.sqrt(512))).float()
    ref = a.to(op()).double() @ wm.double().t()                                          # |ref| ~ 1e4
    y32 = ops.gemm(a.to(op()).to(dev), wm.to(op()).to(dev), out_dtype=torch.float32)
    y16 = ops.gemm(a.to(op()).to(dev), wm.to(op()).to(dev), out_dtype=op())
    assert rel_err(y32.cpu(), ref) < F32_TOL * 5 and torch.isfinite(y16).all() and rel_err(y16.float().cpu(), ref) < tol(BF16_TOL)
    # (2) a product beyond the fp16 range: f32 output exact, fp16 output saturated at +-65504 (what an inf would have been), finite everywhere
    big = torch.full((32, 512), 300.0)
    big[1] = -300.0
    wb = torch.full((48, 512), 1.0)
    r32 = ops.gemm(big.to(op()).to(dev), wb.to(op()).to(dev), out_dtype=torch.float32)
    r16 = ops.gemm(big.to(op()).to(dev), wb.to(op()).to(dev), out_dtype=op())
    assert torch.equal(r32.cpu(), torch.full((32, 48), 153600.0) * torch.tensor([1.0, -1.0] + [1.0] * 30)[:, None])
    assert torch.isfinite(r16).all() and torch.equal(r16.float().cpu(), r32.cpu().clamp(-65504.0, 65504.0))
    # ... and through the gated epilogue silu(gate) * up (the one activation copy whose size follows the checkpoint): 300 * 512 = 1.5e5 per column
    gu = ops.gemm(big.to(op()).to(dev), torch.ones(64, 512, dtype=op(), device=dev), act=hip.RV_ACT_SILU_MUL, w_packed=False)
    assert torch.isfinite(gu).all() and float(gu.float().abs().max()) == 65504.0
    # (3) a whole block of the tiny Llama on a residual stream with 1e4-magnitude "massive activations": finite, and the oracle's result
    eng = _tiny_engine(dev)
    shape = synth.TINY
    cfg = llama.LlamaCfg(shape.hidden, shape.inter, shape.layers, shape.heads, shape.vocab, shape.eps, shape.theta)
    wl = llama_weights(shape, bf16=fl())
    w32 = llama_weights(shape, bf16=False)
    for k_ in wl:
        if "norm" in k_:
            wl[k_] = w32[k_]
    h = feats("sat.h", (2, 40, shape.hidden)) * 0.5
    h[:, :, 11] = 1.0e4
    h[1, 5, 200:232] = -8.0e3
    pos = torch.arange(40)[None].expand(2, 40)
    cos, sin = llama.rope_cos_sin(pos, cfg.head_dim, cfg.theta)
    bias = llama._bias_from_mask(torch.ones(2, 40, dtype=torch.bool), 40, 0, h.dtype)
    want = llama.decoder_layer(h, wl, 0, cfg, cos, sin, bias, llama.KVCache(cfg.layers))
    kv, Smax = eng.new_kv(2, 64, reuse=False)
    got = eng.llm_layers(h.clone().to(dev).contiguous(), 0, kv, Smax, 0, 1).cpu()
    assert torch.isfinite(got).all()
    assert float((got - want).abs().max() / (want - h).abs().max()) < tol(1e-2)          # against what the block ADDED to the stream


def test_fp16_saturation_is_reported(dev):
    """VERDICT r5 #6 / ADVICE r5: the fp16 build's stores saturate instead of overflowing - and now SAY so, and a NaN stays a NaN.  (a) a GEMM row whose
    products leave +-65504 comes out saturated, the library's sticky count (rv_numeric_status_bind / option "saturated") goes up, every other row is
    bit-identical to the run without the planted row; a NaN planted in one input row yields NaN in that output row only (rounds 1 - 5: -65504);
    (b) the same through the Llama engine in its prefill form and in BOTH decode forms (rv_llm_forward S = 1 and the merged rv_llm_decode_rows): a NaN
    planted in one sequence's residual stream gives NaN logits for that sequence and bit-identical logits for the others; a 1e7 residual row (the fused
    RMSNorm operand w * h of the decode kernels) is counted, warned about once by check_handoff_status, and leaves the other rows unchanged.
    The bf16 build: NaN behaviour the same, the count stays 0."""
    from revisionllm_amd import hip, ops
    f16 = fl() == "f16"
    status = hip.numeric_status(fl(), dev)
    count = lambda: int(status[0].item()) & 0xffffffff
    a = feats("satr.a", (48, 512), bf16=fl())
    w = feats("satr.w", (64, 512), bf16=fl())
    clean = ops.gemm(a.to(op()).to(dev), w.to(op()).to(dev), out_dtype=op())
    c0 = count()
    big = a.clone()
    big[5] = 300.0 * torch.sign(w[0])                     # row 5 . w[0] = 300 * sum |w[0]| ~ 1.3e5
    got = ops.gemm(big.to(op()).to(dev), w.to(op()).to(dev), out_dtype=op())
    keep = torch.arange(48) != 5
    assert torch.isfinite(got).all() and torch.equal(got[keep], clean[keep])
    if f16:
        assert float(got[5, 0]) == 65504.0 and count() > c0
    else:
        assert count() == c0 == 0
    nan = a.clone()
    nan[7, 33] = float("nan")
    got = ops.gemm(nan.to(op()).to(dev), w.to(op()).to(dev), out_dtype=op())
    keep = torch.arange(48) != 7
    assert torch.isnan(got[7]).all() and torch.equal(got[keep], clean[keep])
    # (b) the engine
    eng = _tiny_engine(dev)
    D = eng.shape.hidden
    eng.on_saturation = "warn"
    eng.saturated(reset=True)
    h0 = feats("satr.h", (3, 24, D)) * 0.5

    def prefill(h):
        kv, Smax = eng.new_kv(3, 64, reuse=False)
        return eng.llm_forward(h.clone().to(dev).contiguous(), 0, kv, Smax).clone(), kv, Smax
    base, kv, Smax = prefill(h0)
    hn = h0.clone()
    hn[1, 9, 17] = float("nan")
    got, _, _ = prefill(hn)
    assert torch.isnan(got[1]).all() and torch.equal(got[[0, 2]], base[[0, 2]])
    assert eng.saturated() == 0
    h1 = feats("satr.h1", (3, 1, D)) * 0.5
    for form in ("forward", "decode_rows"):
        def step(h):
            kv2 = kv.clone()
            if form == "forward":
                return eng.llm_forward(h.clone().to(dev).contiguous(), 24, kv2, Smax).clone()
            return eng.llm_decode_rows(h[:, 0].clone().to(dev).contiguous(), torch.full((3,), 24, dtype=torch.int32, device=dev), kv2, Smax).clone()
        base1 = step(h1)
        assert torch.isfinite(base1).all() and eng.saturated() == 0
        hn = h1.clone()
        hn[2, 0, 5] = float("nan")
        got = step(hn)
        assert torch.isnan(got[2]).all() and torch.equal(got[:2], base1[:2]), form
        hb = h1.clone()
        hb[0, 0, 40:44] = 1.0e7                  # w_next * h of the fused-RMSNorm operand leaves the fp16 range in four elements of row 0
        got = step(hb)
        assert torch.isfinite(got).all() and torch.equal(got[1:], base1[1:]), form
        if f16:
            assert eng.saturated() > 0, form
            eng.saturated_seen = 0
            with pytest.warns(RuntimeWarning, match="saturated"):
                eng.check_handoff_status()
            eng.on_saturation = "raise"
            eng.saturated_seen = 0
            with pytest.raises(hip.HipLibraryError, match="saturated"):
                eng.check_handoff_status()
            eng.on_saturation = "warn"
            assert eng.saturated(reset=True) > 0 and eng.saturated() == 0
        else:
            assert eng.saturated() == 0


def _ref_attn(q, k, v, causal, pad, q_pos0, kv_div):
    B, Lq, H, dh = q.shape
    k = k.repeat_interleave(kv_div, 0)
    v = v.repeat_interleave(kv_div, 0)
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) / math.sqrt(dh)
    if pad is not None:
        s = s.masked_fill(pad.repeat_interleave(kv_div, 0)[:, None, None, :].bool(), float("-inf"))
    if causal:
        qi = torch.arange(Lq)[:, None] + q_pos0
        s = s.masked_fill((torch.arange(k.shape[1])[None, :] > qi)[None, None], float("-inf"))
    p = torch.softmax(s, -1)
    return torch.einsum("bhqk,bkhd->bqhd", p, v.double()).reshape(B, Lq, H * dh)


@pytest.mark.parametrize("case", ["self96", "cross96", "causal128", "decode128", "long96", "split96", "split128", "vit64", "text64"])
def test_attention(dev, case):
    from revisionllm_amd import ops
    cfg = {"self96": (3, 3, 257, 257, 8, 96, False, False, 0), "cross96": (6, 2, 50, 13, 8, 96, False, True, 0),
           "causal128": (2, 2, 171, 171, 4, 128, True, False, 0), "decode128": (3, 3, 1, 173, 4, 128, True, False, 172),
           "long96": (1, 1, 1025, 1025, 8, 96, False, False, 0), "split96": (4, 2, 9, 77, 8, 96, False, True, 0),
           "split128": (2, 2, 16, 300, 4, 128, True, False, 284), "vit64": (3, 3, 257, 257, 16, 64, False, False, 0),
           "text64": (2, 2, 77, 77, 12, 64, True, False, 0)}[case]
    B, Bk, Lq, Lk, H, dh, causal, use_pad, q_pos0 = cfg
    q = feats(f"at.q.{case}", (B, Lq, H, dh), bf16=fl())
    k = feats(f"at.k.{case}", (Bk, Lk, H, dh), bf16=fl())
    v = feats(f"at.v.{case}", (Bk, Lk, H, dh), bf16=fl())
    pad = None
    if use_pad:
        pad = torch.zeros(Bk, Lk, dtype=torch.uint8)
        pad[1, 9:] = 1
    y = ops.attention(bf(q).to(dev), bf(k).to(dev), bf(v).to(dev), causal=causal, key_pad=pad.to(dev) if pad is not None else None,
                      q_pos0=q_pos0)
    ref = _ref_attn(q, k, v, causal, pad, q_pos0, B // Bk)
    assert rel_err(y.float().cpu(), ref) < tol(BF16_TOL)


_EDGE_LK = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160)


@pytest.mark.parametrize("Lq,Lk", [(Lq, Lk) for Lq in (1, 16) for Lk in _EDGE_LK if Lq <= Lk])
def test_decode_attention_at_key_block_edges(dev, Lq, Lk):
    """The key-split decode form (Lq <= 16: wave w of a workgroup takes the 32-key blocks w, w + 4, .. and the four partial (m, l, O) are merged
    through LDS) with the key count at every edge of that split, against float64: fewer blocks than waves (the idle waves enter the merge with
    m = -inf), an exactly full last block, a last block of ONE key, one key in all, a second round of blocks that only wave 0 has (129, 159, 160).
    Causal with the queries at the END of the keys (q_pos0 = Lk - Lq), as a KV-cached step has them; Lq = 16: every query row its own key count."""
    from revisionllm_amd import ops
    B, H, dh = 3, 4, 128
    q = feats(f"ate.q.{Lq}.{Lk}", (B, Lq, H, dh), bf16=fl())
    k = feats(f"ate.k.{Lq}.{Lk}", (B, Lk, H, dh), bf16=fl())
    v = feats(f"ate.v.{Lq}.{Lk}", (B, Lk, H, dh), bf16=fl())
    y = ops.attention(bf(q).to(dev), bf(k).to(dev), bf(v).to(dev), causal=True, q_pos0=Lk - Lq)
    ref = _ref_attn(q, k, v, True, None, Lk - Lq, 1)
    assert torch.isfinite(y).all() and rel_err(y.float().cpu(), ref) < tol(BF16_TOL)


@pytest.mark.parametrize("Lk,hidden_from", [(13, 9), (32, 20), (33, 32), (128, 96), (129, 128)])
def test_padded_split_attention_at_key_block_edges(dev, Lk, hidden_from):
    """The key-split form with a key-padding mask (the adapter's text cross-attention: 96-wide heads, 9 queries, not causal, 4 query batches over
    2 key batches) at the block edges, against float64.  The mask hides the keys hidden_from .. Lk - 1 of key batch 1 and none of batch 0: a tail
    inside the only block, the whole single-key last block (33: hidden in one batch, live in the other), a whole block of one wave (128: wave 3
    merges with m = -inf), the single key of a second round (129)."""
    from revisionllm_amd import ops
    B, Bk, Lq, H, dh = 4, 2, 9, 8, 96
    q = feats(f"atp.q.{Lk}", (B, Lq, H, dh), bf16=fl())
    k = feats(f"atp.k.{Lk}", (Bk, Lk, H, dh), bf16=fl())
    v = feats(f"atp.v.{Lk}", (Bk, Lk, H, dh), bf16=fl())
    pad = torch.zeros(Bk, Lk, dtype=torch.uint8)
    pad[1, hidden_from:] = 1
    assert 0 < hidden_from < Lk
    y = ops.attention(bf(q).to(dev), bf(k).to(dev), bf(v).to(dev), causal=False, key_pad=pad.to(dev))
    ref = _ref_attn(q, k, v, False, pad, 0, B // Bk)
    assert torch.isfinite(y).all() and rel_err(y.float().cpu(), ref) < tol(BF16_TOL)


@pytest.mark.parametrize("Tn,N", [(256, 5), (1024, 2), (130, 3)])
def test_attention_with_lds_staged_keys_is_bit_identical(dev, Tn, N):
    """The long-key attention form (attention.hip attn_body_lds: key blocks staged in LDS once per 128 query rows, option ``attn_lds``) performs the per-tile
    operations of the per-wave form in the same order: the ClipEncoder's outputs - every frame row, through both self-attention layers over T + 1 keys - are
    BIT-identical with the option on and off (T + 1 = 257 / 1025 / 131 keys: partial last key block, a last workgroup with one live wave)."""
    eng = _tiny_engine(dev)
    x = feats(f"al.x.{Tn}", (N, Tn, 768), bf16=fl())
    q = feats("al.q", (1, 7, 768), bf16=fl())
    m = torch.ones(1, 7)
    outs = {}
    for v in (1, 0):
        eng.set_option("attn_lds", v)
        outs[v] = eng.clip_encoder(x, q, m, "all").clone()
    eng.set_option("attn_lds", 1)
    assert torch.isfinite(outs[1]).all() and torch.equal(outs[0], outs[1])


def test_project_dense(dev):
    from oracle import adapter
    from revisionllm_amd import engine
    from revisionllm_amd.utils import synth
    eng = engine.Engine(synth.LlamaShape(layers=0), device=dev)
    eng.init_synthetic(seed=SEED, llm=False, clip=False, linear=True)
    w = linear_weights(bf16=fl())
    x = feats("pd.x", (3, 256, 768), bf16=fl())
    y = eng.project_dense(x)
    ref = adapter.dense_projector(x, w["weight"], w["bias"])
    assert rel_err(y.cpu(), ref) < 1e-4
    assert rel_err(eng.project_dense(x, op()).float().cpu(), ref) < tol(BF16_TOL)


@pytest.mark.parametrize("text", [True, False])
@pytest.mark.parametrize("Tn", [16, 256])
def test_clip_encoder(dev, text, Tn):
    """Full sparse adapter (2 T2V + 2 self layers + projector), N=4 sequences sharing 2 texts."""
    from oracle import adapter
    from revisionllm_amd import engine
    from revisionllm_amd.utils import synth
    eng = engine.Engine(synth.LlamaShape(layers=0), adapter_text=text, device=dev)
    eng.init_synthetic(seed=SEED, llm=False, clip=True, clip_prefix="mm_projector.")
    w = clip_weights(text=text, bf16=fl())
    # vectors stay fp32 on the device; rebuild them un-rounded for the oracle
    w32 = clip_weights(text=text, bf16=False)
    for k_ in w:
        if w[k_].dim() == 1:
            w[k_] = w32[k_]
    N, Nq, Lq = 4, 2, 7
    x = feats(f"ce.x.{Tn}", (N, Tn, 768), bf16=fl())
    txt = feats("ce.txt", (Nq, Lq, 768), bf16=fl())
    mask = torch.tensor([[1] * 7, [1, 1, 1, 1, 0, 0, 0]], dtype=torch.float32)
    y = eng.clip_encoder(x, txt, mask, "cls")
    qf = txt.repeat_interleave(N // Nq, 0)
    qm = mask.repeat_interleave(N // Nq, 0)
    ref = adapter.clip_encoder(x, w, qf if text else None, qm if text else None, text, "cls", True)[:, 0]
    assert rel_err(y.cpu(), ref) < tol(1e-2)
    yall = eng.clip_encoder(x, txt, mask, "all")
    refall = adapter.clip_encoder(x, w, qf if text else None, qm if text else None, text, "all", False)
    assert rel_err(yall.cpu(), refall) < tol(1e-2)
    assert rel_err(yall[:, 0].cpu(), y.cpu()) < 1e-6


def _tiny_engine(dev, text=True):
    from revisionllm_amd import engine
    from revisionllm_amd.utils import synth
    eng = engine.Engine(synth.TINY, adapter_text=text, device=dev)
    eng.init_synthetic(seed=SEED, llm=True, clip=True)
    return eng


def test_llm_prefill_and_decode(dev):
    """TINY Llama (3 layers, dH=128): prefill logits, then 3 KV-cached decode steps, vs the oracle."""
    from oracle import llama
    from revisionllm_amd.utils import synth
    eng = _tiny_engine(dev)
    shape = synth.TINY
    cfg = llama.LlamaCfg(shape.hidden, shape.inter, shape.layers, shape.heads, shape.vocab, shape.eps, shape.theta)
    w = llama_weights(shape, bf16=fl())
    w32 = llama_weights(shape, bf16=False)
    for k_ in w:
        if "norm" in k_:
            w[k_] = w32[k_]
    B, S = 3, 45
    ids = torch.from_numpy(np.stack([synth.synthetic_prompt_ids(S, 5, s, vocab=shape.vocab) for s in range(B)]))
    ids[:, 5] = 7
    emb = w["model.embed_tokens.weight"][ids]
    cache = llama.KVCache(cfg.layers)
    ref = llama.forward(emb, w, cfg, cache=cache)[:, -1]
    kv, Smax = eng.new_kv(B, 64)
    h = eng.splice_embed(ids.int(), None)
    assert rel_err(h.cpu(), emb) < 1e-6
    logits = eng.llm_forward(h, 0, kv, Smax)
    assert rel_err(logits.cpu(), ref) < tol(1.2e-2)
    for step in range(3):
        nxt = ref.argmax(-1)
        e1 = w["model.embed_tokens.weight"][nxt][:, None]
        ref = llama.forward(e1, w, cfg, cache=cache)[:, -1]
        h1 = eng.splice_embed(nxt.int()[:, None], None)
        logits = eng.llm_forward(h1, S + step, kv, Smax)
        assert rel_err(logits.cpu(), ref) < tol(1.2e-2), step


def test_sample_and_scores(dev):
    from oracle import sampling, scores
    from revisionllm_amd import ops
    logits = feats("smp.logits", (5, 32000)) * 1.3
    u = torch.tensor([0.0, 0.3, 0.55, 0.9, 0.999])
    for (temp, k, p) in ((0.05, 50, 0.6), (1.0, 50, 1.0), (0.7, 20, 0.9), (2.0, 64, 0.3)):
        o = ops.sample(logits.to(dev), u.to(dev), True, temp, k, p)
        sc = sampling.process_logits(logits, temp, k, p)
        tok = sampling.select_token(sc, u)
        assert (o["tokens"].cpu().long() == tok).all(), (temp, k, p)
        keep = torch.isfinite(sc).sum(-1)
        assert (o["n_keep"].cpu().long() == keep).all()
        ent = scores.entropy_statistics(sc[:, None])[:, 0]
        assert torch.allclose(o["entropy_proc"].cpu(), ent, rtol=1e-4, atol=1e-6)
        raw = scores.entropy_statistics(logits[:, None])[:, 0]
        assert torch.allclose(o["entropy_raw"].cpu(), raw, rtol=1e-5)
        for b in range(5):
            n = int(keep[b])
            idx = o["topk_idx"][b, :n].cpu().long()
            assert torch.allclose(o["topk_val"][b, :n].cpu(), sc[b, idx], rtol=1e-6)
    o = ops.sample(logits.to(dev), None, False)
    assert (o["tokens"].cpu().long() == logits.argmax(-1)).all()
    # ties: quantised logits produce many equal scores, some straddling the K-th place (lowest index must win)
    lt = (logits * 2).round() / 2
    lt[4, :] = 1.25                      # a fully tied row
    lt[4, 100] = 3.0
    for (temp, k, p) in ((1.0, 50, 1.0), (0.5, 7, 0.95), (1.0, 64, 0.7)):
        o = ops.sample(lt.to(dev), u.to(dev), True, temp, k, p)
        srt = torch.sort(lt / temp, descending=True, stable=True, dim=-1)
        assert (o["topk_idx"][:, :k].cpu().long() == srt.indices[:, :k]).all(), (temp, k, p)
        assert torch.allclose(o["topk_val"][:, :k].cpu(), srt.values[:, :k], rtol=1e-6)
    # max / min / mean to 1e-5 relative; std is a difference of nearly equal entropies (H ~ 10, std ~ 5e-4),
    # so it is only compared to 2e-5 ABSOLUTE (= 2e-6 of H, fp32 resolution of the inputs)
    st = ops.entropy_stats((logits.view(1, 5, 32000) * 0.5).to(dev))
    ref = scores.entropy_statistics(logits.view(1, 5, 32000) * 0.5)
    assert torch.allclose(st[:, :3].cpu(), ref[:, :3], rtol=1e-5) and abs(float(st[0, 3]) - float(ref[0, 3])) < 2e-5
    sc = sampling.process_logits(logits, 0.05, 50, 0.6)
    st = ops.entropy_stats(sc.view(1, 5, 32000).to(dev))
    assert torch.allclose(st.cpu(), scores.entropy_statistics(sc.view(1, 5, 32000)), rtol=1e-4, atol=2e-5)
    st1 = ops.entropy_stats(logits[:1, None].to(dev))
    assert torch.isnan(st1[0, 3])


def test_sample_without_a_top_k_filter(dev):
    """top_k = 0 / None (HF: filter disabled - what a checkpoint's generation_config.json may ask for; VERDICT r4 missing #3): every token is a candidate,
    only top-p trims.  Against the oracle's warper chain + inverse-CDF draw: drawn token, number of kept tokens, threshold (= the smallest kept
    processed score), entropy of the processed distribution; a peaked row (T = 0.05), flat rows, ties across the draw, and through generate()."""
    from oracle import sampling, scores
    from revisionllm_amd import ops
    logits = feats("smp0.logits", (6, 32000)) * 1.3
    logits[5] = (logits[5] * 2).round() / 2                      # a row with many exactly tied scores
    u = torch.tensor([0.0, 0.3, 0.55, 0.9, 0.999, 0.42])
    for (temp, p) in ((0.05, 1.0), (0.05, 0.6), (1.0, 1.0), (1.0, 0.9), (0.7, 0.3), (2.0, 0.95)):
        o = ops.sample(logits.to(dev), u.to(dev), True, temp, 0, p)
        sc = sampling.process_logits(logits, temp, 0, p)
        keep = torch.isfinite(sc).sum(-1)
        # the ascending cumulative sum of TopPLogitsWarper is a sequential f32 sum in the oracle and a tree of partial sums on the device: a
        # token whose inclusive sum lands within rounding of 1 - top_p may fall on either side - at most one token of difference per row
        nk = o["n_keep"].cpu().long()
        # (row 5 holds exactly tied scores: the reference's unstable ascending sort removes an arbitrary part of a tie group that straddles the cut,
        # the kernel keeps the whole group - compared on the rows with distinct scores)
        assert ((nk - keep).abs()[:5] <= 1).all(), (temp, p, nk.tolist(), keep.tolist())
        assert nk[5] >= keep[5]
        same = nk == keep
        thr = torch.where(torch.isfinite(sc), sc, torch.full_like(sc, float("inf"))).amin(-1)
        assert torch.allclose(o["threshold"].cpu()[same], thr[same], rtol=1e-6)
        ent = scores.entropy_statistics(sc[:, None])[:, 0]
        assert torch.allclose(o["entropy_proc"].cpu()[same], ent[same], rtol=2e-4, atol=1e-5)
        # the draw: the oracle's token wherever its uniform is not within 2e-6 of a step of the descending CDF (f32 sums in another order; a flat
        # row's steps are 3e-5 wide)
        pr = torch.softmax(sc.double(), -1)
        srt = torch.sort(pr, descending=True, stable=True, dim=-1)
        cum = srt.values.cumsum(-1)
        safe = ((cum - u[:, None].double()).abs().amin(-1) > 2e-6) & same
        tok = sampling.select_token(sc, u)
        assert (o["tokens"].cpu().long()[safe] == tok[safe]).all(), (temp, p)
        assert safe.sum() >= 4
        assert (o["topk_idx"].cpu() == -1).all()                 # no candidate list in this mode
    # two exactly tied candidates straddling the draw: the lower index first (the oracle's stable descending sort)
    lt = torch.full((1, 32000), -30.0)
    lt[0, 17] = lt[0, 4711] = 2.0
    lt[0, 99] = 1.0
    for uu, want in ((0.10, 17), (0.40, 17), (0.50, 4711), (0.80, 4711), (0.95, 99)):
        o = ops.sample(lt.to(dev), torch.tensor([uu]).to(dev), True, 1.0, 0, 1.0)
        assert int(o["tokens"][0]) == want == int(sampling.select_token(sampling.process_logits(lt, 1.0, 0, 1.0), torch.tensor([uu]))[0]), (uu, int(o["tokens"][0]))


def test_sample_with_a_top_k_wider_than_the_candidate_list(dev):
    """top_k > 64 (HF allows any; the kernel's candidate list holds 64): TopKLogitsWarper by threshold - every score below the top_k-th largest goes, a
    tie at that place stays whole - then top-p and the draw as in the unfiltered path.  Against the oracle's warper chain: kept counts (exact for
    top_p = 1, ties included), threshold, processed entropy, drawn tokens; top_k >= V equals top_k = 0; top_k = 65 next to the list path's 64."""
    from oracle import sampling, scores
    from revisionllm_amd import ops
    logits = feats("smpk.logits", (6, 32000)) * 1.3
    logits[5] = (logits[5] * 2).round() / 2                      # many exactly tied scores: the k-th place lies inside a tie group
    u = torch.tensor([0.0, 0.3, 0.55, 0.9, 0.999, 0.42])
    for k in (65, 100, 1000, 31999):
        for (temp, p) in ((1.0, 1.0), (0.7, 0.9), (2.0, 0.5)):
            o = ops.sample(logits.to(dev), u.to(dev), True, temp, k, p)
            sc = sampling.process_logits(logits, temp, k, p)
            keep = torch.isfinite(sc).sum(-1)
            nk = o["n_keep"].cpu().long()
            if p >= 1.0:
                assert torch.equal(nk, keep), (k, nk.tolist(), keep.tolist())        # a count, not a sum: exact, the tie group at the k-th place whole
                assert nk[5] > k or k == 31999
            else:
                assert ((nk - keep).abs()[:5] <= 1).all(), (k, temp, p, nk.tolist(), keep.tolist())
            same = nk == keep
            thr = torch.where(torch.isfinite(sc), sc, torch.full_like(sc, float("inf"))).amin(-1)
            assert torch.allclose(o["threshold"].cpu()[same], thr[same], rtol=1e-6)
            ent = scores.entropy_statistics(sc[:, None])[:, 0]
            assert torch.allclose(o["entropy_proc"].cpu()[same], ent[same], rtol=2e-4, atol=1e-5)
            pr = torch.softmax(sc.double(), -1)
            cum = torch.sort(pr, descending=True, stable=True, dim=-1).values.cumsum(-1)
            safe = ((cum - u[:, None].double()).abs().amin(-1) > 2e-6) & same
            tok = sampling.select_token(sc, u)
            assert (o["tokens"].cpu().long()[safe] == tok[safe]).all(), (k, temp, p)
            assert safe.sum() >= 4
            assert (o["topk_idx"].cpu() == -1).all()
    # short / ragged vocabularies (padding lanes must never count as candidates)
    for V in (1024, 1500, 4099):
        x = feats(f"smpk.v{V}", (4, V)) * 2.0
        for k in (65, 100, V - 1):
            o = ops.sample(x.to(dev), u[:4].to(dev), True, 0.8, k, 1.0)
            sc = sampling.process_logits(x, 0.8, k, 1.0)
            assert torch.equal(o["n_keep"].cpu().long(), torch.isfinite(sc).sum(-1)), (V, k)
            assert torch.allclose(o["threshold"].cpu(), torch.where(torch.isfinite(sc), sc, torch.full_like(sc, float("inf"))).amin(-1), rtol=1e-6)
            pr = torch.softmax(sc.double(), -1)
            cum = torch.sort(pr, descending=True, stable=True, dim=-1).values.cumsum(-1)
            safe = (cum - u[:4, None].double()).abs().amin(-1) > 2e-6
            assert (o["tokens"].cpu().long()[safe] == sampling.select_token(sc, u[:4])[safe]).all() and safe.sum() >= 3, (V, k)
    # top_k >= V removes nothing: the same outputs as top_k = 0, bit for bit
    for k in (32000, 50000):
        a, b = ops.sample(logits.to(dev), u.to(dev), True, 0.7, k, 0.9), ops.sample(logits.to(dev), u.to(dev), True, 0.7, 0, 0.9)
        for name in a:
            assert torch.equal(a[name].cpu(), b[name].cpu()), (k, name)
    # 65 by threshold next to 64 from the list: one more candidate, below the list's last
    a, b = ops.sample(logits[:5].to(dev), u[:5].to(dev), True, 0.05, 65, 1.0), ops.sample(logits[:5].to(dev), u[:5].to(dev), True, 0.05, 64, 1.0)
    assert torch.equal(a["n_keep"].cpu(), b["n_keep"].cpu() + 1)
    assert (a["threshold"] <= b["topk_val"][:, 63]).all()


def test_sample_fast_path_equals_general_path(dev):
    """The compacted-candidate selection (default) and the general 16-round selection give identical outputs, bit for bit:
    decode-like rows, rows with ties across the k-th place (the fast path hands over), a nearly flat row (> 1024 candidates)."""
    from revisionllm_amd import hip, ops
    logits = feats("smpf.logits", (7, 32000)) * 1.7
    lt = (logits * 2).round() / 2
    flat = logits * 1e-6
    flat[3] = 0.25
    u = torch.tensor([0.0, 0.2, 0.4, 0.6, 0.8, 0.95, 0.9999])
    small = [feats(f"smpf.v{v}", (7, v)) * 2.0 for v in (1024, 1500, 4099, 32768)]
    small.append((small[1] * 4).round() / 4)          # short rows with ties
    opts = [hip.Options(sample_variant=v) for v in (0, 1)]
    for x in [logits, lt, flat] + small:
        for (temp, k, p) in ((0.05, 50, 1.0), (0.05, 50, 0.6), (1.0, 64, 0.9), (0.7, 7, 1.0), (1.0, 1, 1.0)):
            outs = [ops.sample(x.to(dev), u.to(dev), True, temp, k, p, ctx=o) for o in opts]
            for name in outs[0]:
                assert torch.equal(outs[0][name].cpu(), outs[1][name].cpu()), (name, temp, k, p)


def test_topk_cosine(dev):
    from oracle import scores
    from revisionllm_amd import ops
    feat = feats("tc.feat", (4, 250, 768), bf16=fl())
    q = feats("tc.q", (768,))
    y = ops.topk_cosine(bf(feat).to(dev), q.to(dev), 3)
    ref = torch.stack([scores.stage2_cosine(feat[i:i + 1], q)[0] for i in range(4)])
    assert rel_err(y.cpu(), ref) < 1e-4
    y = ops.topk_cosine(feat[0, 5:19][None].to(dev), q.to(dev), 3)
    assert rel_err(y.cpu(), scores.stage1_cosine(feat[0, 5:19], q)) < 1e-4
    y = ops.topk_cosine(feat[0, 5:19][None].to(dev), q.to(dev), 0)
    assert rel_err(y.cpu(), scores.stage1_cosine(feat[0, 5:19], q, topk_pool=False)) < 1e-4


@pytest.mark.parametrize("M", [33, 56, 70, 112, 128, 129, 140, 144])
@pytest.mark.parametrize("N,K,act", [(22016, 4096, 2), (4096, 4096, 0), (4096, 11008, 0), (12288, 4096, 0), (32000, 4096, 0)])
def test_gemm_rows_split_k_decode_kernel_vs_float64(dev, M, N, K, act):
    """The decode projection kernel of the HEADLINE (33 .. 144 fragment-packed rows, split-K with LDS-shared activations,
    csrc/gemm_rows.hip through rv_gemm_rows) directly against the float64 product of the same bf16 operands, for every projection
    shape of a Vicuna-7B block + lm_head, at the row counts the bench's pools run (56, 70, 112) and the edges (33, 128)."""
    from revisionllm_amd import hip, ops
    g = torch.Generator().manual_seed(M * 131 + N)
    x = (torch.randn(M, K, generator=g) * 0.5).to(op()).to(dev)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(op()).to(dev)
    wp = ops.pack_fragments(w)
    y = ops.gemm_rows(x, wp, act=act, out_dtype=torch.float32)
    z = x.double() @ w.double().t()
    if act == hip.RV_ACT_SILU_MUL:
        z3 = z.view(M, N // 32, 2, 16)
        z = (torch.nn.functional.silu(z3[:, :, 0]) * z3[:, :, 1]).reshape(M, N // 2)
    assert y.shape == z.shape
    assert rel_err(y.float().cpu(), z.cpu()) < (1.5e-2 if act == hip.RV_ACT_SILU_MUL else 1e-4)     # bf16 output / f32 output of f32 sums
    # a second launch on the same (never cleaned) arrival counters gives the same bits
    assert torch.equal(y, ops.gemm_rows(x, wp, act=act, out_dtype=torch.float32))


@pytest.mark.parametrize("M", [56, 70, 112, 140])
@pytest.mark.parametrize("N,K,act", [(22016, 4096, 2), (4096, 11008, 0), (32000, 4096, 0)])
def test_gemm_rows_fp8_weights_vs_float64_and_the_16_row_kernel(dev, M, N, K, act):
    """FP8 (e4m3fn, per-row scale) weights in the 33 .. 144-row decode kernel (opt-in fp8 LLM path, BASELINE configs[4]): against the
    float64 product of the DEQUANTISED weights, and bit-identical per row to the <= 16-row FP8 kernel (rv_gemv_fp8) - the widening to
    bf16 is exact and the summation order is the shared one."""
    from revisionllm_amd import hip, ops
    g = torch.Generator().manual_seed(M * 17 + N)
    x = (torch.randn(M, K, generator=g) * 0.5).to(op()).to(dev)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dev)
    w8, sc = ops.pack_fragments_fp8(w)
    q, sc2 = ops.quantize_rows_fp8(w)
    assert torch.equal(sc, sc2)
    wd = q.double() * sc.double()[:, None]                                # what the kernel multiplies by (scales applied in the epilogue)
    y = ops.gemm_rows(x, w8, act=act, out_dtype=torch.float32, w_scale=sc)
    z = x.double() @ wd.t()
    if act == hip.RV_ACT_SILU_MUL:
        z3 = z.view(M, N // 32, 2, 16)
        z = (torch.nn.functional.silu(z3[:, :, 0]) * z3[:, :, 1]).reshape(M, N // 2)
    assert rel_err(y.float().cpu(), z.cpu()) < (1.5e-2 if act == hip.RV_ACT_SILU_MUL else 1e-4)
    od = op() if act == hip.RV_ACT_SILU_MUL else torch.float32
    for r0 in (0, 16, M - 16):
        lo = ops.gemv_fp8(x[r0:r0 + 16], w8, sc, out_dtype=od, act=act)
        assert torch.equal(y[r0:r0 + 16], lo), r0
