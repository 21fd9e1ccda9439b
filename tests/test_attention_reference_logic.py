"""Guards what tests/test_gpu_attention_edges.py relies on - not the package: the float64 oracle of tests/attention_oracle.py against torch, the strided
buffer builder, the dispatch table, and - for EVERY record of the case table - that each fault a kernel could plausibly have (a mutant of the oracle) moves
the per-row error far above the bound the GPU tests assert on at least one of the record's probes.  No GPU, no library."""
import math

import pytest
import torch

import attention_oracle as ao
from helpers import BF16_TOL, feats

SENSITIVE = 4 * BF16_TOL          # a mutant must be at least this far from the oracle (the GPU tests assert row_err < 8e-3 / 1.33e-3)
FLAVOURS = ("f16", "bf16")


# ------------------------------------------------------------------ the oracle ------------------------------------------------------------------
def _random_problem(i):
    """(B, Bk, H, Lq, Lk, dh, causal, q_pos0, pad) of the i-th of 30 small problems: every third not causal, offsets in front of, at and past the key count,
    masks on two thirds, kv_div 1 .. 3."""
    g = torch.Generator().manual_seed(100 + i)
    r = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    Bk, kv_div, H, dh = r(1, 2), r(1, 3), r(1, 3), (8, 16, 24)[i % 3]
    Lq, Lk = r(1, 20), r(1, 40)
    causal = i % 3 != 0
    q_pos0 = r(0, Lk + 2) if causal else 0
    pad = None
    if i % 3 != 1:
        pad = (torch.rand(Bk, Lk, generator=g) < 0.4).to(torch.uint8)
        pad[0, r(0, Lk - 1)] = 0
        if Bk > 1 and i % 2:
            pad[1] = 1                     # an all-padded key batch
    return Bk * kv_div, Bk, H, Lq, Lk, dh, causal, q_pos0, pad


@pytest.mark.parametrize("i", range(30))
def test_oracle_equals_torch_sdpa_in_float64(i):
    B, Bk, H, Lq, Lk, dh, causal, q_pos0, pad = _random_problem(i)
    q = feats(f"arl.q.{i}", (B, Lq, H, dh)).double()
    k = feats(f"arl.k.{i}", (Bk, Lk, H, dh)).double()
    v = feats(f"arl.v.{i}", (Bk, Lk, H, dh)).double()
    scale = 0.37 if i % 5 == 0 else None
    got = ao.ref_attention(q, k, v, causal, pad, q_pos0, B // Bk, scale)
    # an explicit boolean mask, written out independently of ao.visibility
    allow = torch.ones(B, 1, Lq, Lk, dtype=torch.bool)
    for b in range(B):
        for j in range(Lk):
            if pad is not None and pad[b // (B // Bk), j]:
                allow[b, 0, :, j] = False
            for qi in range(Lq):
                if causal and j > q_pos0 + qi:
                    allow[b, 0, qi, j] = False
    kk, vv = k.repeat_interleave(B // Bk, 0), v.repeat_interleave(B // Bk, 0)
    want = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), kk.transpose(1, 2), vv.transpose(1, 2), attn_mask=allow,
                                                            scale=scale if scale is not None else ao.default_scale(dh)).transpose(1, 2)
    empty = ~allow.any(-1)[:, 0]                              # [B, Lq]: torch gives NaN or 0 there by version, the library's rule is a zero row
    assert bool((got[empty] == 0).all())
    assert got.shape == (B, Lq, H, dh) and got.dtype == torch.float64
    if bool((~empty).any()):
        assert float((got[~empty] - want[~empty]).abs().max()) < 1e-12


def test_oracle_equals_multihead_attention_key_padding_mask():
    """nn.MultiheadAttention with identity projections: the same numbers under a key_padding_mask, but for a batch with every key padded (the oracle: 0, the documented rule)."""
    B, Bk, H, Lq, Lk, dh = 4, 2, 3, 5, 11, 8
    E = H * dh
    mha = torch.nn.MultiheadAttention(E, H, bias=False, batch_first=True).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(E, dtype=torch.float64).repeat(3, 1))
        mha.out_proj.weight.copy_(torch.eye(E, dtype=torch.float64))
    q = feats("arl.mha.q", (B, Lq, H, dh)).double()
    k = feats("arl.mha.k", (Bk, Lk, H, dh)).double()
    v = feats("arl.mha.v", (Bk, Lk, H, dh)).double()
    pad = torch.zeros(Bk, Lk, dtype=torch.uint8)
    pad[0, 7:] = 1
    pad[0, 2] = 1
    pad[1] = 1
    rep = lambda t: t.repeat_interleave(2, 0)
    with torch.no_grad():
        want, _ = mha(q.reshape(B, Lq, E), rep(k).reshape(B, Lk, E), rep(v).reshape(B, Lk, E), key_padding_mask=rep(pad).bool(), need_weights=True)
    got = ao.ref_attention(q, k, v, False, pad, 0, 2, 1.0 / math.sqrt(dh)).reshape(B, Lq, E)
    assert float((got[:2] - want[:2]).abs().max()) < 1e-12
    assert bool((torch.isnan(want[2:]) | (want[2:] == 0)).all()) and bool((got[2:] == 0).all())        # (torch: NaN, or 0 from newer versions)


def test_row_err_is_per_row_and_floors_zero_rows():
    ref = torch.zeros(1, 3, 2, 4, dtype=torch.float64)
    ref[0, 0, 0] = 3.0
    ref[0, 1, 0] = 0.3
    y = ref.clone()
    y[0, 1, 0, 2] += 0.003                                    # 1 % of ITS row, 0.1 % of the largest element
    assert abs(ao.row_err(y, ref) - 0.01) < 1e-12
    y = ref.clone()
    y[0, 2, 1, 1] = 0.0015                                    # a zero row: compared with the floor 1e-3 * 3.0
    assert abs(ao.row_err(y, ref) - 0.5) < 1e-12
    y[0, 0, 1, 0] = float("nan")
    assert math.isnan(ao.row_err(y, ref)) and not ao.row_err(y, ref) < 1.0
    assert ao.row_err(ref, ref) == 0.0


# ------------------------------------------------------------------ the table ------------------------------------------------------------------
def test_case_table_reaches_every_form_and_edge():
    cs = ao.CASES
    forms = lambda group: [c.form for c in cs if c.group == group]
    assert forms("layout") == ["split", "wave", "lds", "lds1"] * 3 and forms("stress") == ["split", "wave", "lds", "lds1", "d512"]
    have = {(c.form, c.dh, c.Lq, c.Lk, c.causal, c.q_pos0) for c in cs if c.group == "edge"}
    # the switches of the launcher, from both sides
    for dh in (64, 96):
        assert ("wave", dh, 47, 95, False, 0) in have and ("lds", dh, 48, 129, False, 0) in have and ("lds", dh, 113, 96, False, 0) in have
        assert {("lds", dh, Lq, 129, False, 0) for Lq in (97, 112, 113)} <= have                     # a wave's second tile empty / one row / full
    assert ("wave", 128, 17, 63, False, 0) in have and ("lds1", 128, 17, 64, False, 0) in have and ("lds1", 128, 17, 64, True, 47) in have
    assert ("lds1", 128, 20, 100, True, 10) in have and ("wave", 128, 20, 60, True, 10) in have     # keys behind the last query
    assert ("lds1", 128, 65, 65, True, 0) in have and ("lds1", 128, 70, 65, False, 0) in have       # a workgroup with one live wave
    for c in cs:
        assert c.B % c.Bk == 0 and (c.B * c.H) % 8 != 0 and c.Lk <= 161 and c.Lq <= 129 and (not c.causal or c.q_pos0 >= 0)
        assert c.form == ao.dispatch(c.dh, c.Lq, c.Lk, c.causal, c.mask != "none")
        pad = ao.make_mask(c.mask, c.Bk, c.Lk)
        if pad is not None:
            assert c.Bk == 2 and not bool(pad[0].any()) and bool(pad[1].any()) and not bool(pad[1].all())
    masked = {(c.form, c.dh, c.Lk, c.mask, c.B // c.Bk) for c in cs if c.group == "mask"}
    for form in ("split", "wave"):
        for dh in (64, 96, 128):
            for Lk in (33, 129):
                assert {m for f, d, l, m, _ in masked if (f, d, l) == (form, dh, Lk)} >= set(ao.MASKS) - ({"interior"} if Lk == 33 else set())
    assert {kv for *_, kv in masked} == {2, 3}


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_probes_are_what_they_claim(flavour):
    c = next(c for c in ao.CASES if c.group == "stress" and c.form == "lds")
    sc = lambda q, k: torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * ao.default_scale(c.dh)
    q, k, v = ao.case_inputs(c, "ramp_up", flavour)
    assert bool((sc(q, k).diff(dim=-1) > 0.2).all())
    q, k, v = ao.case_inputs(c, "ramp_down", flavour)
    assert bool((sc(q, k).diff(dim=-1) < -0.2).all())
    for probe, s in (("spike0", 0), ("spike32", 32), ("spike_last", c.Lk - 1)):
        q, k, v = ao.case_inputs(c, probe, flavour)
        S = sc(q, k)
        rest = torch.cat([S[..., :s], S[..., s + 1:]], -1)
        assert float((S[..., s] - rest.amax(-1)).min()) >= 60.0
    q, k, v = ao.case_inputs(c, "flat", flavour)
    assert not bool(q.any())
    assert float((ao.case_reference(c, "flat", flavour) - v.double().mean(1, keepdim=True)).abs().max()) < 1e-12
    e = next(c for c in ao.CASES if c.group == "edge" and c.form == "lds")
    q, k, v = ao.case_inputs(e, "onehot", flavour)
    assert float(sc(q, k).std()) <= 0.25 and bool((v.sum(-1) == 1).all()) and bool((v[0, :, 0].argmax(-1) == torch.arange(e.Lk) % e.dh).all())
    ref = ao.case_reference(e, "onehot", flavour)
    assert float((ref.sum(-1) - 1).abs().max()) < 1e-12           # a row of the output is a probability vector over the key classes


# ------------------------------------------------------------------ the buffers ------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("family", ao.LAYOUTS)
def test_layout_round_trips_and_fences(family, flavour):
    B, Bk, H, Lq, Lk, dh = 4, 2, 3, 5, 37, 64
    q = feats("arl.lay.q", (B, Lq, H, dh), bf16=flavour)
    k = feats("arl.lay.k", (Bk, Lk, H, dh), bf16=flavour)
    v = feats("arl.lay.v", (Bk, Lk, H, dh), bf16=flavour)
    L = ao.build_layout(family, q, k, v, flavour, causal=True, q_pos0=32, kv_div=2)
    E, Lp = H * dh, 64
    # unpacking by the strides the ABI is handed returns the operands
    assert torch.equal(L.view_q().float(), q) and torch.equal(L.view_k().float(), k) and torch.equal(L.view_vt().float(), v.permute(0, 2, 3, 1))
    assert bool((L.view_vt(cols=Lp)[..., Lk:].float() == ao.VT_PAD).all())
    # the family's strides
    want = {"contig": dict(q_rs=E, k_rs=E, k_hs=dh, vt_ds=Lp, o_rs=E, o_bs=Lq * E), "fused": dict(q_rs=3 * E, k_rs=3 * E, k_hs=dh, vt_ds=Lp, o_rs=E),
            "cache": dict(q_rs=E, k_rs=dh, k_hs=(Lp + 64) * dh, vt_ds=Lp + 64, o_rs=E), "window": dict(q_rs=E, k_rs=E, k_hs=dh, vt_ds=Lp, o_rs=E + 8)}[family]
    assert all(getattr(L, n) == x for n, x in want.items())
    assert L.vt_ds % 32 == 0 and (family != "cache" or L.vt_ds >= Lp + 32) and (family != "window" or L.o_bs > Lq * L.o_rs)
    assert all(s % 8 == 0 for s in (L.q_rs, L.k_rs, L.k_hs, L.vt_ds, L.vt_hs, L.vt_bs, L.q_off, L.k_off)) and L.o_rs % 4 == 0 and L.o_off % 4 == 0
    # everything outside what the kernel may read (q rows < Lq, k rows < Lk, V^T columns < ceil32(Lk)) is NaN, everything inside is finite
    bufs = {id(b): b for b in (L.q_buf, L.k_buf, L.vt_buf)}
    may = {i: torch.zeros(b.numel(), dtype=torch.bool) for i, b in bufs.items()}
    L.view_q(may[id(L.q_buf)]).fill_(True)
    L.view_k(may[id(L.k_buf)]).fill_(True)
    L.view_vt(may[id(L.vt_buf)], cols=Lp).fill_(True)
    for i, b in bufs.items():
        assert bool(torch.isfinite(b.float()[may[i]]).all()) and bool(torch.isnan(b.float()[~may[i]]).all())
    fenced = sum(int((~m).sum()) for m in may.values())
    assert (fenced == 0) == (family == "contig")
    if family == "fused":
        assert L.k_buf is L.q_buf and fenced > L.q_buf.numel() // 3                      # the last third of every row at least
    # the output: all fill; the live words are exactly B * Lq * E; a stray write is seen wherever it lands outside them
    assert L.out_buf.dtype == torch.int16 and bool((L.out_buf == ao.NAN_FILL[flavour]).all()) and L.fence_intact(L.out_buf)
    assert bool(torch.isnan(L.out_buf.view(ao.OP[flavour]).float()).all())
    live = torch.zeros(L.out_buf.numel(), dtype=torch.bool)
    L.view_out(live).fill_(True)
    assert int(live.sum()) == B * Lq * E
    written = L.out_buf.clone()
    L.view_out(written).fill_(0)
    assert L.fence_intact(written)
    for pos in torch.nonzero(~live).flatten().tolist()[::97] + torch.nonzero(~live).flatten().tolist()[-1:]:
        w2 = written.clone()
        w2[pos] = 0
        assert not L.fence_intact(w2)
    assert (int((~live).sum()) > 0) == (family == "window")
    # the argument tuple matches the signature of the entry point
    from revisionllm_amd import hip
    args = L.args(4096, 8192, 12288, 16384, None, None)
    assert len(args) == len(hip.SIGNATURES["rv_attention"][1]) and args[0].value == 4096 + 2 * L.q_off and args[3].value == 8192 + 2 * L.k_off
    assert args[11].value == 16384 + 2 * L.o_off and args[14] is None


# ------------------------------------------------------------------ sensitivity ------------------------------------------------------------------
@pytest.mark.parametrize("c", ao.CASES, ids=ao.case_id)
def test_every_record_is_sensitive_to_every_mutant(c):
    """For each mutant that can touch the record: the largest row_err over the record's probes, oracle against mutant, in both flavours' inputs.  It must
    exceed 4 x 8e-3, i.e. a kernel with that fault cannot pass the GPU test of this record.  Printed (pytest -s) as  <record>: <mutant> <x the bound>."""
    line = []
    for flavour in FLAVOURS:
        worst = {}
        for probe in c.probes:
            q, k, v = ao.case_inputs(c, probe, flavour)
            ref = ao.case_reference(c, probe, flavour)
            for name in ao.MUTANTS:
                y = ao.mutant_attention(name, c, q, k, v)
                if y is not None:
                    worst[name] = max(worst.get(name, 0.0), ao.row_err(y, ref))
        assert worst, "no mutant applies: the record guards nothing"
        if c.causal:
            assert "diagonal_plus_1" in worst or "diagonal_minus_1" in worst
        if c.mask != "none":
            assert "mask_byte_unhidden" in worst and "mask_byte_hidden" in worst
        if c.Lk > 1:
            assert "drop_last_live_key" in worst and "swap_v_rows" in worst
        for name, e in worst.items():
            assert e > SENSITIVE, (ao.case_id(c), flavour, name, e)
        line.append(flavour + " " + ", ".join(f"{n} {e / BF16_TOL:.0f}x" for n, e in worst.items()))
    print(f"{ao.case_id(c)}: " + " | ".join(line))

