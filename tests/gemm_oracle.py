"""Host side of the exact-sum tests of ``rv_gemm`` (tests/test_gemm_reference_logic.py on the CPU, tests/test_gpu_gemm_edges.py on the GPU): no GPU needed.

The idea.  Operands are drawn so that every partial sum of a product is exactly representable in f32: A holds integers in [-4, 4], W multiples of 1/2 in
[-2, 2], bias and residual multiples of 1/2 in [-8, 8].  A product is then a multiple of 1/2 of magnitude <= 8, and with K <= 2048 every partial sum plus
bias and residual stays below 2^16 half-units - far below the 2^24 an f32 significand holds (``exactness_bound`` proves it per case from the value ranges).
The f32 accumulation is therefore exact in ANY order, under any association and any split-K / stream-K hand-off, so with no activation or ReLU an f32 output
must EQUAL the float64 reference and a 16-bit output must equal it rounded to nearest-even: no tolerance.  One dropped, doubled or misplaced k-fragment, row
or column changes an integer.  With SILU_MUL / QuickGELU the pre-activation is still exact and the only error is the device activation's own.

This module holds
  * ``exact_operands`` / ``gemm_reference`` / ``exactness_bound``;
  * host mirrors of the dispatch conditions of ``rv_gemm_impl`` (csrc/gemm.hip, gemm_pp.hip, gemm_arows.hip) that a case relies on, each taking the CU
    count as an argument, and ``dispatch_form``: the kernel form a call reaches;
  * the case table (``cases(device_cus)``): every record names the form it is MEANT to reach, and ``check_form`` fails when the mirrors disagree.
"""
import zlib
from collections import namedtuple

import torch

from revisionllm_amd.hip import RV_ACT_NONE, RV_ACT_QUICK_GELU, RV_ACT_RELU, RV_ACT_SILU_MUL
from test_gpu_kernels import _stream_k_piece_lengths   # the host mirror of launch_sk's work division (imported, not copied)

# ---------------------------------------------------------------- operands ----------------------------------------------------------------
A_MAX, W_MAX, EPI_MAX = 4, 2, 8          # |A| <= 4 (integers), |W| <= 2 (multiples of 1/2), |bias|, |residual| <= 8 (multiples of 1/2)
K_MAX = 2048                             # the longest reduction in the table
SENTINEL = -1984.0                       # guard value of the output buffers: exactly representable in fp16, bf16 and f32 (-31 * 64), and no result of a case


def _seed(case_id):
    return zlib.crc32(case_id.encode())


def _nonzero(g, shape, amax):
    """Integers in [-amax, amax] without 0 (dense operands: a dropped element always changes a sum)."""
    v = torch.randint(0, 2 * amax, shape, generator=g)
    return (v - amax + (v >= amax).long()).float()


def exact_operands(case, dtype):
    """-> (A [M, K] and W [N, K] in ``dtype``, bias [N] and residual [M, n_out] in f32) of a case, seeded by its id: CPU tensors, W row-major."""
    g = torch.Generator().manual_seed(_seed(case.id))
    a = _nonzero(g, (case.M, case.K), A_MAX)
    w = _nonzero(g, (case.N, case.K), 2 * W_MAX) * 0.5
    bias = torch.randint(-2 * EPI_MAX, 2 * EPI_MAX + 1, (case.N,), generator=g).float() * 0.5
    res = torch.randint(-2 * EPI_MAX, 2 * EPI_MAX + 1, (case.M, n_out(case.N, case.act)), generator=g).float() * 0.5
    a16, w16 = a.to(dtype), w.to(dtype)
    assert torch.equal(a16.float(), a) and torch.equal(w16.float(), w)       # representable in both 16-bit types
    return a16, w16, bias, res


def n_out(N, act):
    return N // 2 if act == RV_ACT_SILU_MUL else N


def exactness_bound(case):
    """Largest magnitude, in half-units, that any partial sum of the case (any order, any split) plus bias plus residual can reach, from the VALUE RANGES
    (not from the drawn sample).  Exact f32 accumulation needs it below 2^24; a 16-bit fp16 output needs the value itself inside fp16's range."""
    assert case.K <= K_MAX
    half_units = 2 * A_MAX * W_MAX * case.K + 2 * EPI_MAX + 2 * EPI_MAX      # K products of <= 16 half-units, bias and residual of <= 16 each
    assert half_units < 2 ** 24, (case.id, half_units)
    assert half_units / 2 < 65504, (case.id, half_units)                     # never saturates an fp16 output
    return half_units


def cast_rne(z, dtype, saturate=False):
    """float64 -> f32 / fp16 / bf16, round to nearest even.  Through f32: exact for the exact cases (asserted by the caller), and what the kernels do with an
    activation's f32 value.  ``saturate``: the fp16 build's conversions clamp to +-65504 instead of producing inf (a documented property of the library)."""
    z = z.float()
    if dtype == torch.float16 and saturate:
        z = z.clamp(-65504.0, 65504.0)
    return z.to(dtype)


def epilogue_reference(z, bias, res, act, out_dtype=None, exact=True):
    """act(z + bias) + res on the float64 product ``z`` [M, N]; ``out_dtype``: rounded to nearest even into it.  SILU_MUL: gate / up rows of W are interleaved in
    16-row groups, as ops.pack_fragments takes them.  ``exact``: assert that the result is representable in f32 (no activation / ReLU on exact operands)."""
    M, N = z.shape
    if bias is not None:
        z = z + bias.double()
    if act == RV_ACT_RELU:
        z = torch.relu(z)
    elif act == RV_ACT_SILU_MUL:
        z3 = z.view(M, N // 32, 2, 16)
        z = (torch.nn.functional.silu(z3[:, :, 0]) * z3[:, :, 1]).reshape(M, N // 2)
    elif act == RV_ACT_QUICK_GELU:
        z = z * torch.sigmoid(1.702 * z)
    if res is not None:
        z = z + res.double()
    if exact:
        assert act in (RV_ACT_NONE, RV_ACT_RELU) and torch.equal(z.float().double(), z)
    return z if out_dtype is None else cast_rne(z, out_dtype, saturate=not exact)


def gemm_reference(a, w, bias, res, act, out_dtype=None, exact=True):
    """act(a @ w.T + bias) + res in float64, on the operands' device (see epilogue_reference)."""
    return epilogue_reference(a.double() @ w.double().t(), bias, res, act, out_dtype, exact)


# ---------------------------------------------------------------- dispatch mirrors ----------------------------------------------------------------
PBM, PBN, PBK = 256, 256, 64                    # gemm_pp.hip
AR_LDS_MAX, AR_PAD = 160 * 1024, 2              # gemm_arows.hip


def cdiv(a, b):
    return -(-a // b)


def gemv(M, N, K, no_stream=False):
    """The ``gemv`` predicate of rv_gemm_impl: the weight-streaming decode kernel takes the call."""
    return M <= (16 if no_stream else 32) and K % 128 == 0 and N % 16 == 0


def decode_form(M, N, act):
    """launch_gemv / launch_gemv_mb: row blocks (MB) and column tiles per workgroup (NT)."""
    return "decode_mb%d_nt%d" % (2 if M > 16 else 1, 2 if (act == RV_ACT_SILU_MUL or N >= 16384) else 1)


def pp_num_cus(device_cus, gemm_cus=0):
    want = gemm_cus & ~7
    return want if 0 < want <= device_cus else device_cus


def gemm_pp_supported(packed, M, N, K):
    return bool(packed) and M > 16 and N % PBN == 0 and K % PBK == 0


def pp_teams(M, cus):
    tiles_m, per_x = cdiv(M, PBM), cus >> 3
    return 8 * (per_x // tiles_m) if tiles_m <= per_x else 0


def gemm_pp_sk_supported(packed, M, N, K, cus):
    return gemm_pp_supported(packed, M, N, K) and pp_teams(M, cus) > 0 and cus <= 1023 and (N // PBN) * (K // PBK) < (1 << 30)


def gemm_pp_sk_plan(M, N, K, gated, cus, mhalf=2):
    tiles_m, per_x = cdiv(M, PBM), cus >> 3
    T, nk = pp_teams(M, cus), K // PBK
    if T == 0 or K < 2048:
        return 0
    ts = per_x // tiles_m * tiles_m
    if mhalf and tiles_m >= 10 and tiles_m % 2 == 0:
        ts = max(ts, tiles_m // 2 * (per_x // (tiles_m // 2)))
    if (per_x - ts) * 10 > per_x:
        return 0
    panels = N // PBN
    sk_panels = panels % T
    if sk_panels == 0 and panels >= T:
        return 4
    if not gated and N % 192 == 0 and (N // 192) % T == 0:
        return 3
    if sk_panels == 0:
        return 4
    if panels < T:
        if panels * 4 <= T and panels * nk >= 8 * T:
            return 4
        return 4 if (panels * 2 <= T and panels * nk >= 64 * T) else 0
    return 4 if (sk_panels * 8 >= T and sk_panels * nk >= 8 * T) else 0


def gemm_pp_dp_plan(M, N, K, gated, cus):
    if K < 2048:
        return 0
    t4 = cdiv(M, PBM) * (N // PBN)
    if t4 >= cus and t4 * 100 >= cdiv(t4, cus) * cus * 85:
        return 4
    if not gated and N % 192 == 0:
        t3 = cdiv(M, PBM) * (N // 192)
        if t3 >= cus and t3 * 100 >= cdiv(t3, cus) * cus * 75:
            return 3
    return 0


ArPlan = namedtuple("ArPlan", "rows_per_wg mf nw grid rcap")


def arows_rcap(K):
    return min((AR_LDS_MAX - 1024) // (K * 2 + AR_PAD * 16), 112)


def arows_plan(M, N, K, device_cus):
    """plan_for of gemm_arows.hip (the A-resident kernel deals rows over ALL CUs of the device: option gemm_cus does not apply) -> ArPlan or None."""
    if K % 256 != 0 or K > 1024 or not (N % 32 == 0 and (N // 32) % 8 == 0):
        return None
    rcap = arows_rcap(K)
    if rcap < 16:
        return None
    rounds = cdiv(M, device_cus * rcap)
    rpw = cdiv(M, device_cus * rounds)
    return ArPlan(rpw, (rpw + 15) // 16, 2, cdiv(M, rpw), rcap)


def gemm_arows_supported(packed, act, M, N, K, device_cus):
    if not packed or act == RV_ACT_SILU_MUL:
        return False
    p = arows_plan(M, N, K, device_cus)
    return p is not None and 4 <= p.mf <= 7


def dispatch_form(M, N, K, packed, act, device_cus, stream_k=False, gemm_tile_variant=2, gemm_cus=0, gemm_arows=1, gemm_waves=8, **_):
    """The kernel form rv_gemm_impl reaches for a valid call (bf16 / fp16 weights, no norm fusion), with the options at their defaults unless given."""
    gated = act == RV_ACT_SILU_MUL
    if gemv(M, N, K):
        return decode_form(M, N, act)
    if (gemm_arows & 15) and gemm_arows_supported(packed, act, M, N, K, device_cus):
        return "arows_mf%d" % arows_plan(M, N, K, device_cus).mf
    cus, v = pp_num_cus(device_cus, gemm_cus), gemm_tile_variant
    if gemm_pp_supported(packed, M, N, K):
        sk_ws = stream_k and gemm_pp_sk_supported(packed, M, N, K, cus)
        sk_plan = gemm_pp_sk_plan(M, N, K, gated, cus)
        if v in (4, 5) or (v == 2 and ((sk_ws and sk_plan != 0) or gemm_pp_dp_plan(M, N, K, gated, cus) != 0)):
            sk = sk_ws and (v == 5 or (v == 2 and sk_plan != 0))              # gemm_pp_launch gets the workspace
            if not sk:
                return "pp_tiled_nf3" if gemm_pp_dp_plan(M, N, K, gated, cus) == 3 else "pp_tiled"
            if not gated and gemm_pp_sk_plan(M, N, K, False, cus) == 3:
                return "pp_sk_nf3"                                             # 192-column panels: the eight-wave kernel only
            return "pp_sk_w4" if gemm_waves == 4 else "pp_sk"
    if not packed:
        return "tile2_rowmajor"
    return {1: "ring4", 3: "p5", 0: "tile2"}.get(v, "ring3")


def stream_k_team_units(M, N, K, cus):
    """k-tile units of the stream-K tail per team for launches of one panel per team (fewer than 8 row tiles, the table's case): team t owns units
    [t * total // T, (t + 1) * total // T) of the tail's (panel, k-tile) space.  A team with 0 units and no whole panel is idle."""
    tiles_m, tiles_n, nk = cdiv(M, PBM), N // PBN, K // PBK
    assert tiles_m < 8
    T = pp_teams(M, cus)
    whole = tiles_n // T * T
    total = (tiles_n - whole) * nk
    return [(t + 1) * total // T - t * total // T for t in range(T)], whole // T


def stream_k_pieces(M, N, K, cus):
    return _stream_k_piece_lengths(M, N, K, cus)


# ---------------------------------------------------------------- the case table ----------------------------------------------------------------
# runs of a case: (output "f32" | "op16", epilogue, guard columns).  Epilogues: "plain" (no bias / activation / residual), "brr" (bias + ReLU + residual),
# "br" (bias + ReLU), "act" (the case's own activation: SILU_MUL without bias, QuickGELU with bias).  Guard columns 12 make ldc % 8 == 4 wherever
# n_out % 8 == 0 (the direct 16-bit epilogue of gemm_tile_p4), 16 make ldc % 8 == 0 (its LDS-transposed one).
Case = namedtuple("Case", "id group form M N K packed act opts stream_k lda_pad runs pieces guard_rows")
DEFAULT_RUNS = (("f32", "plain", 12), ("op16", "plain", 12), ("f32", "brr", 12), ("op16", "brr", 12))
TILE_RUNS = DEFAULT_RUNS + (("op16", "plain", 16), ("op16", "br", 16), ("op16", "brr", 16))
ACT_RUNS = (("f32", "act", 12), ("op16", "act", 12), ("op16", "act", 16))
ARES_RUNS = (("f32", "brr", 12), ("op16", "plain", 12), ("op16", "br", 16))
EXACT_EPILOGUES = ("plain", "brr", "br")
AROWS_GUARD_ROWS = 128      # the A-resident kernel handles up to 112 rows per workgroup: guards deep enough that a store of a whole block past M stays inside the buffer


def _case(group, form, M, N, K, packed=True, act=RV_ACT_NONE, opts=None, stream_k=False, lda_pad=0, runs=None, pieces=None, guard_rows=3, tag=""):
    opts = dict(opts or {})
    if runs is None:
        runs = ACT_RUNS if act != RV_ACT_NONE else DEFAULT_RUNS
    o = "".join("-%s%d" % (k.replace("gemm_", "")[:4], v) for k, v in sorted(opts.items()))
    cid = "%s-%s-%dx%dx%d-%s%s%s%s%s" % (group, form, M, N, K, "pk" if packed else "rm", {0: "", 1: "-relu", 2: "-silu", 3: "-qgelu"}[act], o,
                                        "-lda%d" % lda_pad if lda_pad else "", "-" + tag if tag else "")
    return Case(cid, group, form, M, N, K, packed, act, tuple(sorted(opts.items())), stream_k, lda_pad, tuple(runs), pieces, guard_rows)


def arows_m_for(rows_per_wg, K, device_cus):
    """The largest M of ONE round whose even deal gives ``rows_per_wg`` rows per workgroup (rows_per_wg <= rcap)."""
    assert rows_per_wg <= arows_rcap(K)
    return rows_per_wg * device_cus


def cases(device_cus=256):
    """The case table for a device of ``device_cus`` CUs (the A-resident rows depend on it; everything else is fixed)."""
    S, Q = RV_ACT_SILU_MUL, RV_ACT_QUICK_GELU
    out = []
    # 1. decode kernel: K % 128 == 0, N % 16 == 0, M <= 32.  M = 16 | 17: one | two row blocks (MB); N >= 16384 or SILU_MUL: two column tiles (NT); N = 16400: the last
    #    workgroup of the NT = 2 form has half its columns; K = 128 / 384: fewer k-blocks (1 / 3) than the 8 virtual k-waves; 1152: 9, an uneven share
    for M in (1, 15, 16, 17, 31, 32):
        for K in (128, 384, 1152):
            for N in (16, 48):
                for packed in (True, False):
                    out.append(_case("decode", decode_form(M, N, 0), M, N, K, packed))
    for M in (1, 16, 17, 32):
        for K, packed in ((128, True), (128, False), (384, True), (384, False)) + (((1152, True),) if M == 32 else ()):
            out.append(_case("decode", "decode_mb%d_nt2" % (2 if M > 16 else 1), M, 16400, K, packed))
    for M in (1, 17, 32):
        for K in (128, 384):
            for N in (32, 96):
                for packed in (True, False):
                    out.append(_case("decode", "decode_mb%d_nt2" % (2 if M > 16 else 1), M, N, K, packed, act=S))
    for packed in (True, False):
        out.append(_case("decode", "decode_mb2_nt1", 17, 48, 384, packed, lda_pad=64))
    # 2. just outside the decode kernel: the tile kernels take it
    for packed in (True, False):
        form = "ring3" if packed else "tile2_rowmajor"
        for K in (128, 384, 1152):
            for N in (16, 48):
                out.append(_case("outside", form, 33, N, K, packed))
        out.append(_case("outside", form, 33, 16400, 128, packed))
        for N in (16, 48):
            out.append(_case("outside", form, 8, N, 192, packed))           # K % 128 != 0
    out.append(_case("outside", "tile2_rowmajor", 8, 100, 128, False))       # N % 16 != 0 (row-major only: packed W needs N % 16 == 0)
    # 3. tile kernels: K = 64 .. 192 is 2, 4, 6 k-steps of 32 - the shortened prologues of the 3- and 4-stage rings; N = 1152 is 9 column tiles (XCD panel dealing + a left-over
    #    panel); N = 16, 112, 144: ragged column tiles (nt_max clamping at an N that is no multiple of 128)
    for variant, form in ((2, "ring3"), (1, "ring4"), (3, "p5"), (0, "tile2")):
        vo = {} if variant == 2 else {"gemm_tile_variant": variant}
        for M in (33, 127, 128, 129):
            for K in (64, 128, 192, 448):
                for N in (16, 112, 128, 144, 1152):
                    out.append(_case("tile", form, M, N, K, True, opts=vo, runs=TILE_RUNS))
        for M in (33, 129):
            for K in (64, 192):
                for N in (128, 160, 1152):
                    out.append(_case("tile", form, M, N, K, True, act=S, opts=vo))
            out.append(_case("tile", form, M, 128, 192, True, act=Q, opts=vo))
            out.append(_case("tile", form, M, 144, 64, True, act=Q, opts=vo))
    for M in (33, 127, 128, 129):
        for K in (64, 128, 192, 448):
            for N in (4, 100, 132):
                out.append(_case("tile", "tile2_rowmajor", M, N, K, False, runs=TILE_RUNS))
    for M in (33, 129):
        out.append(_case("tile", "tile2_rowmajor", M, 96, 192, False, act=S))
        out.append(_case("tile", "tile2_rowmajor", M, 100, 64, False, act=Q))
    # 4. A-resident kernel: rows per workgroup at the support edge (49; one row fewer stays on the ring), an exact multiple of 16 (64), the two ends of MF = 6 (81, 96), the
    #    cap of one round and the rollover into two (rcap, rcap + 1), and a last workgroup of ONE row.  rcap = 112 at K <= 512, 103 at K = 768, 78 at K = 1024 (the LDS
    #    a block of rows needs), so MF = 6 is out of reach at K = 1024 (its cap is MF = 5), and at K = 1024 the two-round deal past the cap (40 rows) falls below 4
    #    fragments: back on the ring.  (Row counts are for 256 CUs; the table scales with the device.)
    for i, K in enumerate((256, 768, 1024)):
        rcap = arows_rcap(K)
        N = (256, 512)
        rows = [49, 64] + [r for r in (81, 96) if r <= rcap] + [rcap]
        for j, r in enumerate(rows):
            M = arows_m_for(r, K, device_cus) - (device_cus - 1 if r in (49, 81) else 0)      # 49 / 81: the FIRST M of that deal
            out.append(_case("ares", "arows_mf%d" % ((r + 15) // 16), M, N[(i + j) % 2], K, runs=ARES_RUNS, guard_rows=AROWS_GUARD_ROWS, tag="rpw%d" % r))
        out.append(_case("ares", "ring3", 48 * device_cus, N[i % 2], K, runs=ARES_RUNS, tag="rpw48"))
        M2 = rcap * device_cus + 1
        r2 = cdiv(M2, 2 * device_cus)
        form2 = "arows_mf%d" % ((r2 + 15) // 16) if 4 <= (r2 + 15) // 16 <= 7 else "ring3"
        out.append(_case("ares", form2, M2, N[(i + 1) % 2], K, runs=ARES_RUNS, guard_rows=AROWS_GUARD_ROWS, tag="rollover"))
        out.append(_case("ares", "arows_mf4", 64 * (device_cus - 1) + 1, N[i % 2], K, runs=ARES_RUNS, guard_rows=AROWS_GUARD_ROWS, tag="last1row"))
    out.append(_case("ares", "arows_mf6", arows_m_for(96, 256, device_cus), 512, 256, act=Q, runs=(("f32", "act", 12), ("op16", "act", 12)), guard_rows=AROWS_GUARD_ROWS, tag="rpw96"))
    # 5. ping-pong, output-tiled (forced: variant 4): 1 .. 5 k-tiles of 64, row tiles of 255 / 256 / 257 rows; M = 17, 32 reach it where the decode kernel does not
    #    take the call (K % 128 != 0).  (gemm_waves applies to the persistent form only: the four-wave setting must not change an output-tiled launch.)
    for waves in (8, 4):
        po = {"gemm_tile_variant": 4, "gemm_waves": waves}
        for M in (17, 32, 255, 256, 257):
            for N in (256, 768):
                for K in (64, 128, 192, 256, 320):
                    if M <= 32 and K % 128 == 0:
                        continue                                           # the decode kernel's (group 1)
                    out.append(_case("pp", "pp_tiled", M, N, K, opts=po))
        for M, K in ((32, 192), (257, 64), (257, 256)):
            out.append(_case("pp", "pp_tiled", M, 512, K, act=S, opts=po))
        out.append(_case("pp", "pp_tiled", 257, 256, 192, act=Q, opts=po))
    # 6. persistent stream-K (forced: variant 5) on 8 / 16 CUs (gemm_cus), so that the cuts fall on small shapes; ``pieces``: k-tile counts of stream-K pieces that must occur.
    #    17 rows reach it at K = 192 / 320 only: (17, 768, 256) has K % 128 == 0 and belongs to the decode kernel whatever the variant (test_gemm_reference_logic.py).
    for waves in (8, 4):
        form = "pp_sk_w4" if waves == 4 else "pp_sk"
        for cus, shapes in ((8, (((200, 768, 64), {1}), ((200, 768, 128), {1}), ((200, 768, 192), {1, 2}), ((200, 768, 256), {1, 2}), ((200, 768, 512), {1, 2, 3}),
                                 ((17, 768, 192), {1, 2}), ((17, 768, 320), {1, 2}), ((200, 2816, 256), {1, 2}))),
                            (16, (((200, 768, 64), {1}), ((200, 768, 256), {1}), ((200, 768, 512), {1, 2}), ((257, 768, 256), {1, 2}), ((512, 768, 256), {1, 2})))):
            for (M, N, K), pieces in shapes:
                out.append(_case("sk", form, M, N, K, opts={"gemm_tile_variant": 5, "gemm_cus": cus, "gemm_waves": waves}, stream_k=True, pieces=frozenset(pieces)))
        out.append(_case("sk", form, 200, 1024, 256, act=S, opts={"gemm_tile_variant": 5, "gemm_cus": 8, "gemm_waves": waves}, stream_k=True, pieces=frozenset({2})))
    out.append(_case("sk", "pp_sk_nf3", 200, 1536, 2048, opts={"gemm_cus": 8}, stream_k=True))      # the policy's own choice (variant 2): 192-column panels, 8 panels on 8 teams
    out.append(_case("pp", "pp_tiled_nf3", 200, 1536, 2048, opts={"gemm_cus": 8}))                  # ... and without a workspace: 8 output tiles of 192 columns
    out.append(_case("pp", "pp_tiled_nf3", 200, 1536, 2048, act=Q, opts={"gemm_cus": 8}))           # (its 16-bit QuickGELU form was dispatched to the f32 kernel)
    return out


def alias_cases(device_cus=256):
    """C aliasing the residual (f32), one shape per form."""
    return [_case("alias", "ring3", 129, 256, 128),
            _case("alias", "arows_mf6", arows_m_for(81, 256, device_cus) - (device_cus - 1), 256, 256, guard_rows=AROWS_GUARD_ROWS, tag="rpw81"),
            _case("alias", "pp_tiled", 200, 768, 256, opts={"gemm_tile_variant": 4}),
            _case("alias", "pp_sk", 200, 768, 256, opts={"gemm_tile_variant": 5, "gemm_cus": 8}, stream_k=True, pieces=frozenset({1, 2}))]


def case_cus(case, device_cus):
    return pp_num_cus(device_cus, dict(case.opts).get("gemm_cus", 0))


def check_form(case, device_cus):
    """The form the mirrors derive for the case's call must be the one the case names."""
    got = dispatch_form(case.M, case.N, case.K, case.packed, case.act, device_cus, stream_k=case.stream_k, **dict(case.opts))
    assert got == case.form, "the dispatch changed: pick a shape that still reaches %s (%s now reaches %s on %d CUs)" % (case.form, case.id, got, device_cus)
    if case.pieces is not None:
        have = stream_k_pieces(case.M, case.N, case.K, case_cus(case, device_cus))
        assert case.pieces <= have, "the work division changed: pick a shape that still cuts pieces of %s k-tiles (%s cuts %s)" % (sorted(case.pieces), case.id, sorted(have))
    if case.act == RV_ACT_SILU_MUL:
        assert all(r[1] == "act" for r in case.runs), case.id       # a gated case reaches another form than its plain shape would
    return got


FORMS_NAMED = ("decode_mb1_nt1", "decode_mb2_nt1", "decode_mb1_nt2", "decode_mb2_nt2", "tile2", "tile2_rowmajor", "ring3", "ring4", "p5",
               "arows_mf4", "arows_mf5", "arows_mf6", "arows_mf7", "pp_tiled", "pp_tiled_nf3", "pp_sk", "pp_sk_w4", "pp_sk_nf3")
