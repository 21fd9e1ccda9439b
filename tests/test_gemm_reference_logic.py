"""What the exact-sum GEMM tests (tests/test_gpu_gemm_edges.py) rest on, checked on the CPU: the operands of every case of tests/gemm_oracle.py keep f32
accumulation exact in any order, the fragment packing inverts, the host mirrors of the dispatch reproduce the facts the table was built from, every case
reaches the form it names, and the float64 reference equals a plain triple loop."""
import math

import pytest
import torch

import gemm_oracle as go
from revisionllm_amd import hip, ops

CUS = 256                         # an MI355X; the table is also checked for another CU count
ALL = go.cases(CUS) + go.alias_cases(CUS)


def test_case_ids_are_unique_and_every_named_form_is_reached():
    ids = [c.id for c in ALL]
    assert len(ids) == len(set(ids))
    for cus in (CUS, 304):
        table = go.cases(cus) + go.alias_cases(cus)
        forms = {go.check_form(c, cus) for c in table}
        assert forms == set(go.FORMS_NAMED), sorted(set(go.FORMS_NAMED) ^ forms)
        assert max(c.M * c.K for c in table) <= 38000 * 1024 and max(c.N for c in table if c.group != "decode" and c.group != "outside") <= 2816
    # the edges the table is there for, by name
    ragged_nt2 = [c for c in ALL if c.form.endswith("nt2") and c.N >= 16384 and c.N % 32 == 16]
    assert {c.form for c in ragged_nt2} == {"decode_mb1_nt2", "decode_mb2_nt2"}
    assert any(c.form == "arows_mf6" for c in ALL) and any(c.form == "pp_sk_nf3" for c in ALL)
    assert any(c.form == "pp_tiled" and c.M in (17, 32) for c in ALL) and any(c.form.startswith("pp_sk") and c.M == 17 for c in ALL)


def test_a_changed_dispatch_is_reported():
    c = next(c for c in ALL if c.form == "pp_sk_nf3")
    with pytest.raises(AssertionError, match="the dispatch changed: pick a shape that still reaches pp_sk_nf3"):
        go.check_form(c._replace(K=1024), CUS)              # K < 2048: the policy leaves it on the ring kernel
    c = next(c for c in ALL if c.pieces == frozenset({1, 2}))
    with pytest.raises(AssertionError, match="the work division changed"):
        go.check_form(c._replace(pieces=frozenset({7})), CUS)


def test_exactness_bound_holds_for_every_case():
    worst = max(go.exactness_bound(c) for c in ALL)
    assert worst == 16 * 2048 + 32 < 2 ** 16
    for dt in (torch.float16, torch.bfloat16):              # the sentinel of the guard rows / columns is exact in every output type and outside every result
        assert float(torch.tensor(go.SENTINEL).to(dt)) == go.SENTINEL
    assert abs(go.SENTINEL) % 0.5 == 0


def _sub(c, a, w):
    """Rows / columns of a large case for the CPU products: the property is per output element, the first and last rows and columns stand for the rest."""
    if a.shape[0] > 256:
        a = torch.cat([a[:64], a[-64:]])
    if w.shape[0] > 512:
        w = torch.cat([w[:128], w[-128:]])
    return a.float(), w.float()


@pytest.mark.parametrize("group", sorted({c.group for c in ALL}))
def test_f32_products_of_the_drawn_operands_are_exact_in_any_order(group):
    """A float32 matmul of the drawn operands in three shuffled k orders and in a 4-way split-k order equals the float64 product bit for bit, and so does every
    running partial sum of a shuffled order: what the zero-tolerance comparison on the GPU rests on."""
    seen = set()
    for c in (c for c in ALL if c.group == group):
        if (c.M, c.N, c.K, c.act) in seen and c.M * c.K > 1 << 20:
            continue
        seen.add((c.M, c.N, c.K, c.act))
        a16, w16, bias, res = go.exact_operands(c, torch.bfloat16 if len(seen) % 2 else torch.float16)
        assert (a16 == 0).sum() == 0 and (w16 == 0).sum() == 0                      # dense
        assert float(a16.float().abs().max()) <= go.A_MAX and float(w16.float().abs().max()) <= go.W_MAX and float(bias.abs().max()) <= go.EPI_MAX
        assert torch.equal(a16.float(), a16.float().round()) and torch.equal(w16.float() * 2, (w16.float() * 2).round())
        a, w = _sub(c, a16, w16)
        ref = a.double() @ w.double().t()
        g = torch.Generator().manual_seed(c.K + c.M)
        for _ in range(3):
            p = torch.randperm(c.K, generator=g)
            assert torch.equal((a[:, p] @ w[:, p].t()).double(), ref), c.id
        q = [slice(i * c.K // 4, (i + 1) * c.K // 4) for i in range(4)]
        parts = [a[:, s] @ w[:, s].t() for s in q]
        assert torch.equal(((parts[0] + parts[1]) + (parts[2] + parts[3])).double(), ref) and torch.equal((((parts[3] + parts[1]) + parts[0]) + parts[2]).double(), ref), c.id
        p = torch.randperm(c.K, generator=g)
        prod = a[:4, None, p] * w[None, :4, p]                                       # [4, 4, K] products in a shuffled order
        assert torch.equal(prod.cumsum(-1).double(), prod.double().cumsum(-1)), c.id
    other = go.exact_operands(ALL[0], torch.float16)[0]
    assert not torch.equal(other, go.exact_operands(ALL[1], torch.float16)[0][: other.shape[0], : other.shape[1]])     # different per case


def test_pack_fragments_inverts_on_the_tables_weight_shapes():
    shapes = sorted({(c.N, c.K) for c in ALL if c.packed})
    assert (16, 64) in shapes
    for N, K in shapes:
        if N * K > 1 << 22 and (N, K) != (16400, 1152):
            continue
        w = (torch.arange(N * K, dtype=torch.int64) % 65521 - 32768).to(torch.int16).view(N, K)      # (a prime period: no two rows of a fragment alike)
        wp = ops.pack_fragments(w)
        assert wp.shape == w.shape
        back = wp.view(N // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(N, K)
        assert torch.equal(back, w), (N, K)
    # the layout include/revision_hip.h documents, element by element, on the smallest shapes
    for N, K in ((16, 64), (48, 128)):
        w = torch.arange(N * K, dtype=torch.int16).view(N, K)
        flat = ops.pack_fragments(w).reshape(-1)
        for n in range(N):
            for k in range(K):
                lane = (n & 15) + 16 * ((k >> 3) & 3)
                assert int(flat[(((n >> 4) * (K // 32) + (k >> 5)) * 64 + lane) * 8 + (k & 7)]) == int(w[n, k])


def test_mirrors_reproduce_the_stream_k_cuts_the_table_names():
    assert go.stream_k_pieces(200, 768, 256, 8) == {1, 2}
    assert go.stream_k_pieces(257, 768, 256, 16) == {1, 2}
    units, whole = go.stream_k_team_units(200, 768, 64, 8)
    assert whole == 0 and sorted(units) == [0, 0, 0, 0, 0, 1, 1, 1]                 # three one-tile panels on eight teams: five teams without work
    units, whole = go.stream_k_team_units(200, 2816, 256, 8)
    assert whole == 1 and sum(units) == 3 * 4                                        # 8 whole panels + a tail of 3
    for c in (c for c in ALL if c.group in ("sk", "alias") and c.stream_k and c.form != "pp_sk_nf3"):
        cus = go.case_cus(c, CUS)
        units, _ = go.stream_k_team_units(c.M, c.N, c.K, cus)
        nk, u, pieces = c.K // go.PBK, 0, set()
        for n in units:                                                              # a team's range, cut at the panel boundaries
            e = u + n
            while u < e:
                step = min(nk - u % nk, e - u)
                pieces.add(step)
                u += step
        assert pieces == go.stream_k_pieces(c.M, c.N, c.K, cus), c.id
        assert c.pieces <= pieces


def test_mirrors_reproduce_the_plans_the_table_names():
    assert go.gemm_pp_sk_plan(200, 1536, 2048, False, 8) == 3                        # 8 panels of 192 columns on 8 teams
    assert go.gemm_pp_sk_plan(200, 1536, 2048, True, 8) != 3                         # never for the gated epilogue
    assert go.dispatch_form(200, 1536, 2048, True, hip.RV_ACT_NONE, CUS, stream_k=True, gemm_cus=8) == "pp_sk_nf3"
    assert go.dispatch_form(200, 1536, 2048, True, hip.RV_ACT_NONE, CUS, stream_k=False, gemm_cus=8) == "pp_tiled_nf3"        # without a workspace: 8 output tiles of 192 columns fill the 8 CUs
    assert go.gemm_pp_supported(True, 17, 256, 64) and not go.gemm_pp_supported(True, 16, 256, 64) and not go.gemm_pp_supported(False, 17, 256, 64)
    assert go.pp_teams(200, 8) == 8 and go.pp_teams(257, 8) == 0 and go.pp_teams(257, 16) == 8 and go.pp_teams(1005, 256) == 64
    assert go.gemm_pp_dp_plan(4096, 4096, 4096, False, 256) == 4 and go.gemm_pp_dp_plan(25700, 768, 2048, False, 256) == 3 and go.gemm_pp_dp_plan(4096, 4096, 1024, False, 256) == 0
    # the decode predicate and its forms
    assert go.gemv(32, 16, 128) and not go.gemv(33, 16, 128) and not go.gemv(8, 16, 192) and not go.gemv(8, 100, 128) and not go.gemv(17, 16, 128, no_stream=True)
    assert go.dispatch_form(17, 768, 256, True, 0, CUS, stream_k=True, gemm_tile_variant=5, gemm_cus=8) == "decode_mb2_nt1"     # K % 128 == 0: never the ping-pong kernel
    assert go.dispatch_form(17, 768, 192, True, 0, CUS, stream_k=True, gemm_tile_variant=5, gemm_cus=8) == "pp_sk"


def test_mirrors_reproduce_the_a_resident_row_deal():
    assert [go.arows_rcap(K) for K in (256, 512, 768, 1024)] == [112, 112, 103, 78]
    mf = {}
    for c in (c for c in ALL if c.group == "ares" and c.form.startswith("arows")):
        p = go.arows_plan(c.M, c.N, c.K, CUS)
        mf.setdefault(p.mf, []).append(p.rows_per_wg)
        assert c.form == "arows_mf%d" % p.mf
    assert sorted(mf) == [4, 5, 6, 7] and {81, 96} <= set(mf[6]) and 49 in mf[4] and 64 in mf[4] and 112 in mf[7]
    assert go.arows_plan(12289, 256, 256, CUS).rows_per_wg == 49 and not go.gemm_arows_supported(True, 0, 12288, 256, 256, CUS)       # the support edge
    assert go.arows_plan(112 * CUS + 1, 256, 256, CUS).rows_per_wg == 57                                                             # two rounds
    last = next(c for c in ALL if c.id.endswith("last1row"))
    p = go.arows_plan(last.M, last.N, last.K, CUS)
    assert p.grid == CUS and last.M - (p.grid - 1) * p.rows_per_wg == 1
    assert not go.gemm_arows_supported(True, hip.RV_ACT_SILU_MUL, 16384, 256, 256, CUS) and not go.gemm_arows_supported(False, 0, 16384, 256, 256, CUS)
    # the shapes of the existing bit-identity test (tests/test_gpu_kernels.py) give the MF values the issue lists: 4, 5, 7 - never 6
    old = [(25600, 4096, 768), (25700, 1536, 768), (25700, 768, 768), (25700, 2048, 768), (16385, 512, 1024), (13000, 256, 512), (20000, 1024, 256), (102500, 768, 768)]
    assert sorted({go.arows_plan(*s, CUS).mf for s in old}) == [4, 5, 7]


@pytest.mark.parametrize("act", [hip.RV_ACT_NONE, hip.RV_ACT_RELU, hip.RV_ACT_SILU_MUL, hip.RV_ACT_QUICK_GELU])
def test_reference_equals_a_plain_triple_loop(act):
    N = 32 if act == hip.RV_ACT_SILU_MUL else 8                   # the gated epilogue pairs 16-row groups: its smallest N is 32
    c = go._case("loop", "none", 5, N, 64, act=act)
    a, w, bias, res = go.exact_operands(c, torch.float16)
    gated = act == hip.RV_ACT_SILU_MUL
    ref = go.gemm_reference(a, w, None if gated else bias, None if gated else res, act, exact=act in (hip.RV_ACT_NONE, hip.RV_ACT_RELU))
    z = [[sum(float(a[m, k]) * float(w[n, k]) for k in range(64)) + (0.0 if gated else float(bias[n])) for n in range(N)] for m in range(5)]
    for m in range(5):
        for n in range(go.n_out(N, act)):
            if act == hip.RV_ACT_NONE:
                v = z[m][n]
            elif act == hip.RV_ACT_RELU:
                v = max(z[m][n], 0.0)
            elif act == hip.RV_ACT_QUICK_GELU:
                v = z[m][n] / (1.0 + math.exp(-1.702 * z[m][n]))
            else:
                gate, up = z[m][(n // 16) * 32 + n % 16], z[m][(n // 16) * 32 + 16 + n % 16]
                v = gate / (1.0 + math.exp(-gate)) * up
            v += 0.0 if gated else float(res[m, n])
            assert abs(float(ref[m, n]) - v) <= 1e-12 * max(1.0, abs(v)), (m, n)
    if act in (hip.RV_ACT_NONE, hip.RV_ACT_RELU):                 # the rounded forms: nearest even
        big = go.gemm_reference(a * 4, w, bias, res, act)         # (values up to a few hundred: bf16 keeps 8 bits of them)
        r16 = go.gemm_reference(a * 4, w, bias, res, act, torch.bfloat16)
        assert torch.equal(r16, big.float().to(torch.bfloat16)) and not torch.equal(r16.double(), big)
        assert ((big - r16.double()).abs() <= (big.abs() * 2 ** -8)).all()
    assert float(go.cast_rne(torch.tensor([257.0, 259.0, 1e6], dtype=torch.float64), torch.bfloat16)[0]) == 256.0      # ties to even: 257 -> 256, 259 -> 260
    assert float(go.cast_rne(torch.tensor([259.0], dtype=torch.float64), torch.bfloat16)[0]) == 260.0
    assert float(go.cast_rne(torch.tensor([1e6], dtype=torch.float64), torch.float16, saturate=True)[0]) == 65504.0
