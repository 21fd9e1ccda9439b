"""The row-op and score kernels (rv_layernorm, rv_rmsnorm, rv_sine_pos, rv_quant_rows_fp8, rv_entropy_stats, rv_topk_cosine, rv_topk_pool) at every
instantiation, kernel switch and refusal, against float64 references computed on the CPU from the inputs after rounding to the type the kernel reads.

The references (``*_ref64`` below) are plain restatements of the operation; tests/test_scores_reference_logic.py checks them against oracle/scores.py and
oracle/sampling.py on the CPU, pins the NaN ranking they share with ``torch.topk``, checks the rank-gap condition of every top-k pooling seed used here
and measures how far the fp32 oracle itself is from float64 at T = 7937 (the basis of COSINE_BOUND)."""
import functools
import math
import os

import pytest
import torch

from helpers import BF16_TOL, F32_TOL, feats, fl, op, rel_err, tol

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")

# rv_topk_cosine: the project's number for this operation (test_gpu_kernels.test_topk_cosine).  It had only been measured at T = 250; at T = 7937 the
# fp32 oracle scores.stage2_cosine is 1.6e-6 (fp16-valued data) / 5.3e-6 (bf16-valued data) from float64 (test_scores_reference_logic.test_fp32_oracle_against_float64_at_T7937), well
# under the 2.5e-5 at which the bound would have had to follow the oracle's own error - so 1e-4 stays.
COSINE_BOUND = 1e-4
COSINE_ORACLE_LIMIT = 2.5e-5
POOL_BOUND = 1e-6            # f32 sums of k <= 64 exactly representable terms
GAP = 1e-4                   # smallest relative distance between neighbouring similarities among the first k + 1 ranks of a pooling case
LDS_BYTES = 64 * 1024


@pytest.fixture(scope="module", params=[None] if _FORCED else ["f16", "bf16"])
def flav(request, op_flavour):
    """Both operand flavours (the module list of conftest.py is fixed, so the module brings its own parameter; REVISION_TEST_FLAVOURS still narrows it)."""
    from revisionllm_amd import hip
    f = request.param or op_flavour or hip.flavour()
    prev = hip.set_flavour(f)
    yield f
    _write_worst(f)
    hip.set_flavour(prev)


@pytest.fixture(scope="module")
def dev(flav):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


_WORST = {}       # (flavour, family) -> worst value noted in this run


def _family(label):
    """The case family of a label: the kernel plus the words that name a path or a kind of case, without the shape figures (d768, T17, k3, ..)."""
    words = label.split()
    return " ".join([words[0]] + [w for w in words[1:] if not (w[0] in "dTVGBKkn" and w[1:2].isdigit()) and not w.startswith(("rows", "Nv", "Nt"))])


def _note(label, value):
    """A line that names the case in the RV_LOG_ERR file (profiles/rowops_scores_err_<flavour>.log); the worst value per family follows when the module
    is done (_write_worst, from the ``flav`` fixture)."""
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            fh.write(f"  rowops {fl()} {label} {value:.3e}\n")
    key = (fl(), _family(label))
    _WORST[key] = max(_WORST.get(key, 0.0), value)
    return value


def _write_worst(flavour):
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            for (f, family), v in sorted(_WORST.items()):
                if f == flavour:
                    fh.write(f"  rowops {f} worst of family: {family} {v:.3e}\n")


def _err(y, ref, label):
    return _note(label, rel_err(y.cpu(), ref))


def _rt(x, kind):
    """x (f32) rounded to what the kernel reads: "f16" / "bf16" -> through that type, "f32" -> unchanged."""
    return x if kind == "f32" else x.to({"f16": torch.float16, "bf16": torch.bfloat16}[kind]).float()


def _dt(kind):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[kind]


# ------------------------------------------------------------------ float64 references ------------------------------------------------------------------
def layernorm_ref64(x, w, b, eps=1e-5):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.double() + b.double()


def rmsnorm_ref64(x, w, eps):
    x = x.double()
    return w.double() * (x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps))


def entropy_stats_ref64(logits):
    """[B,G,V] -> [B,4] = max, min, mean, unbiased std (NaN for G = 1) over the G steps of H = -sum p log(p + 1e-10), every step kept."""
    p = torch.softmax(logits.double(), dim=2)
    h = -(p * torch.log(p + 1e-10)).sum(2)
    std = h.std(dim=1) if h.shape[1] > 1 else torch.full((h.shape[0],), float("nan"), dtype=torch.float64)
    return torch.stack([h.max(1).values, h.min(1).values, h.mean(1), std], dim=1)


def rank_order(sims, dim):
    """Indices along ``dim`` in torch.topk's order: NaN before every number, then the larger value, then the smaller index."""
    return torch.sort(sims, dim=dim, descending=True, stable=True).indices


def cosine_sims64(feat):
    """feat [n,T,d] -> the function q -> sims [n,T] of the column-normalised frames, float64."""
    f = feat.double()
    return f / torch.sqrt((f * f).sum(1, keepdim=True))


def topk_cosine_ref64(feat, q, k):
    """[n,T,d], [d] -> [n]: column norms over the frames, sims = <f_t / norm, q>, the sum of the min(k, T) first in rank order (k <= 0: the mean)."""
    sims = cosine_sims64(feat) @ q.double()
    if k <= 0:
        return sims.mean(1)
    kk = min(k, sims.shape[1])
    return torch.gather(sims, 1, rank_order(sims, 1)[:, :kk]).sum(1)


def topk_pool_ref64(text, video, k):
    """text [Nt,d], video [Nv,T,d] -> (pooled [Nv,Nt,d] float64, idx [Nv,Nt,k] in rank order, sims [Nv,T,Nt])."""
    v = video.double()
    sims = torch.einsum("vtd,jd->vtj", v, text.double())
    idx = rank_order(sims, 1)[:, :k].permute(0, 2, 1).contiguous()                    # [Nv,Nt,k]
    pooled = torch.stack([torch.stack([v[i, idx[i, j]].sum(0) for j in range(text.shape[0])]) for i in range(v.shape[0])])
    return pooled, idx, sims


def rank_gap(sims, k):
    """Smallest distance between neighbouring similarities among the first min(k + 1, T) ranks of every (video, text) pair, relative to the pair's
    largest |similarity|: above GAP no f32 rounding of a similarity can swap two of the selected frames or move the k-th place."""
    s = torch.sort(sims, dim=1, descending=True).values[:, :k + 1]
    if s.shape[1] < 2:
        return float("inf")
    return float(((s[:, :-1] - s[:, 1:]) / sims.abs().amax(1, keepdim=True)).min())


# ------------------------------------------------------------------ LayerNorm ------------------------------------------------------------------
LN_ROWS = (1, 3, 4, 5, 37)


def _ln_inputs(d, rows):
    x = feats(f"rse.ln.x.{d}.{rows}", (rows, d)) * 3 + 0.5
    x[rows // 2] = 300.0 + feats(f"rse.ln.off.{d}", (d,)) / math.sqrt(3.0)         # a large common offset, spread 1: E[x^2] - mean^2 in f32 would lose it
    if rows >= 3:
        x[rows - 1] = 2.5         # variance 0: eps decides.  (A constant whose f32 sums are exact: the mean's rounding would otherwise be amplified by
        #                           rsqrt(eps) = 316 - in any f32 LayerNorm, torch's included - which is not what this row is for.)
    w, b = feats(f"rse.ln.w.{d}", (d,)) * 0.1 + 1, feats(f"rse.ln.b.{d}", (d,)) * 0.05
    return x, w, b


@pytest.mark.parametrize("d", [256, 512, 768, 1024, 4096])
def test_layernorm_every_width(dev, d):
    """Every instantiation of k_layernorm, row counts around the four rows of a workgroup, with and without the position copy (a period that does not
    divide the rows), and with only one of the two plain copies wanted."""
    from revisionllm_amd import ops
    for rows in LN_ROWS:
        x, w, b = _ln_inputs(d, rows)
        ref = layernorm_ref64(x, w, b)
        period = 3 if rows > 3 else rows
        pos = feats(f"rse.ln.pos.{d}", (period, d))
        y32, y16, yp = ops.layernorm(x.to(dev), w.to(dev), b.to(dev), pos=pos.to(dev), period=period)
        e32 = _err(y32, ref, f"layernorm d{d} rows{rows} f32")
        e16 = _err(y16.float(), ref, f"layernorm d{d} rows{rows} op16")
        ep = _err(yp.float(), ref + pos.double()[torch.arange(rows) % period], f"layernorm d{d} rows{rows} pos")
        assert e32 < F32_TOL and e16 < tol(BF16_TOL) and ep < tol(BF16_TOL), (d, rows, e32, e16, ep)
        a32, a16, ap = ops.layernorm(x.to(dev), w.to(dev), b.to(dev), want=("f32",))
        assert a16 is None and ap is None and torch.equal(a32, y32)
        b32, b16, bp = ops.layernorm(x.to(dev), w.to(dev), b.to(dev), want=("op16",))
        assert b32 is None and bp is None and torch.equal(b16, y16)
        if rows >= 3:                                            # the constant row: finite, and the bias alone
            assert float((y32[rows - 1].cpu() - b).abs().max()) < 1e-6


def test_layernorm_refuses_other_widths_and_returns_on_no_rows(dev):
    from revisionllm_amd import hip, ops
    for d in (260, 2048):
        x = torch.zeros(4, d, device=dev)
        with pytest.raises(hip.HipLibraryError, match=r"unsupported width %d \(256, 512, 768, 1024, 4096\)" % d):
            ops.layernorm(x, torch.ones(d, device=dev), torch.zeros(d, device=dev))
    y32, y16, yp = ops.layernorm(torch.zeros(0, 768, device=dev), torch.ones(768, device=dev), torch.zeros(768, device=dev))
    assert y32.shape == (0, 768) and y16.shape == (0, 768) and yp is None
    # the entry point itself with rows = 0 and live buffers: success, nothing written
    x, w, b = (t.to(dev) for t in _ln_inputs(768, 4))
    out = torch.full((4, 768), 7.0, device=dev)
    rc = hip.lib(op()).rv_layernorm(hip.ptr(x), hip.ptr(w), hip.ptr(b), hip.ptr(out), None, None, None, 0, 0, 768, hip.stream())
    torch.cuda.synchronize()
    assert rc == 0 and bool((out == 7.0).all())


# ------------------------------------------------------------------ RMSNorm ------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 8, 252, 256, 260, 768, 1024, 5120, 512, 4096])
def test_rmsnorm_every_width(dev, d):
    """The generic kernel rmsnorm_kernel<0> (every width but 512 and 4096: one lane, a partly filled wave, one column group past 256, several rounds)
    next to the two register instantiations; row counts around the four rows of a workgroup; a zero row (eps alone under the root: output 0)."""
    from revisionllm_amd import ops
    for rows in (1, 4, 5, 9):
        x = feats(f"rse.rms.x.{d}.{rows}", (rows, d)) * 2
        if rows > 1:                                              # (rows = 1 keeps its random row: a single-row launch is held to the reference too)
            x[rows - 1] = 0
        w = feats(f"rse.rms.w.{d}", (d,)) * 0.1 + 1
        y = ops.rmsnorm(x.to(dev), w.to(dev), 1e-5)
        assert _err(y.float(), rmsnorm_ref64(x, w, 1e-5), f"rmsnorm d{d} rows{rows}") < tol(BF16_TOL), (d, rows)
        assert bool(torch.isfinite(y).all()) and (rows == 1 or bool((y[rows - 1] == 0).all()))
        assert float(y[0].float().abs().max()) > 0.5
    # (No bitwise case "d = 512 on the register kernel == the same row zero-padded on the generic kernel": the source adds the same squares in the same
    # order, but FMA contraction is free to fuse the unrolled register form and the generic loop differently, so the two sums need not be the same
    # sums; and at the d = 1024 padding the mean of squares halves, so the reciprocal root grows by sqrt(2), which no exact eps / weight factor undoes.)


def test_rmsnorm_refuses_a_width_that_is_no_multiple_of_four(dev):
    from revisionllm_amd import hip, ops
    with pytest.raises(hip.HipLibraryError, match="rmsnorm: bad arguments"):
        ops.rmsnorm(torch.zeros(2, 6, device=dev), torch.ones(6, device=dev), 1e-5)


# ------------------------------------------------------------------ sine_pos ------------------------------------------------------------------
@pytest.mark.parametrize("d", [768, 2, 6, 64, 255, 512, 1024, 4096])
def test_sine_pos_every_width(dev, d):
    """The table against oracle.adapter.sine_pos_embed in float64 (which accepts every width, odd ones included: 4096 = the LLM-wide adapter).  Bound
    2e-5 absolute, as test_layernorm_rmsnorm_sinepos has it: the angle reaches 2 pi and carries a few f32 roundings (division, powf), ~2e-6."""
    from oracle import adapter
    from revisionllm_amd import ops
    for Tn in (1, 2, 1024):
        p = ops.sine_pos(Tn, d, dev)
        e = _note(f"sine_pos d{d} T{Tn} abs", float((p.cpu().double() - adapter.sine_pos_embed(Tn, d, dtype=torch.float64)).abs().max()))
        assert p.shape == (Tn, d) and e < 2e-5, (d, Tn, e)


# ------------------------------------------------------------------ quant_rows_fp8 ------------------------------------------------------------------
def quant_ref(x16):
    """(bytes, scales) of the host quantiser on operand-typed rows, as test_gemm_fp8_prefill states it."""
    amax = x16.float().abs().amax(dim=1)
    sx = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return (x16.float() * (1.0 / sx)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), sx


def _quant_rows(K, rows):
    x = feats(f"rse.q8.{K}.{rows}", (rows, K), bf16=fl())
    if rows >= 5:
        x[1] = -x[1].abs() * 0.5
        x[1, K // 2] = -3.0                                       # the largest element of the row is negative
        x[2] = 0                                                  # an all-zero row: scale 1, bytes 0
        j = torch.arange(K) % 21                                  # a 2^20 dynamic range: quotients in e4m3's subnormals (< 2^-6) and below half the smallest (2^-10)
        x[3] = (1.0 + feats(f"rse.q8.m.{K}", (K,)).abs() * 0.4) * torch.pow(2.0, -j.float()) * 4.0
        x[3, ::2] *= -1
    return x.to(op())


@pytest.mark.parametrize("K", [8, 504, 512, 520, 4088, 4096, 4104, 11008])
def test_quant_rows_fp8_bytes_and_scales(dev, K):
    """Bytes and scales exactly: one lane busy (K = 8), the edges of a 512-column round, the end of the 4096 register-held columns and one vector past
    it, the re-read tail; contiguous and as column windows of wider tensors (ldx, ldq > K) whose surroundings must stay untouched."""
    from revisionllm_amd import ops
    for rows in (1, 5):
        x = _quant_rows(K, rows)
        qr, sr = quant_ref(x)
        if rows >= 5:
            assert float(x[1, K // 2]) == -3.0 and int(x[1].float().abs().argmax()) == K // 2 and float(x[1].float().max()) <= 0.0
            assert float(sr[1]) == float(torch.tensor(3.0) / 448.0)
            sub = qr[3] & 0x7f
            assert K < 21 or (bool((sub == 0).any()) and bool(((sub > 0) & (sub < 8)).any())), "the wide-range row no longer reaches zero and the subnormals"
        q, s = ops.quant_rows_fp8(x.to(dev))
        assert torch.equal(s.cpu(), sr) and torch.equal(q.cpu(), qr), (K, rows)
        wide = torch.zeros(rows, K + 24, dtype=op())
        wide[:, 8:8 + K] = x
        wide[:, :8], wide[:, 8 + K:] = 1000.0, -1000.0            # larger than every element of the window: a read outside it would change the scale
        dst = torch.full((rows, K + 16), 0xAB, dtype=torch.uint8, device=dev)
        q2, s2 = ops.quant_rows_fp8(wide.to(dev)[:, 8:8 + K], out=dst[:, 8:8 + K])
        assert q2.data_ptr() == dst[:, 8:].data_ptr() and q2.stride(0) == K + 16
        want = torch.full((rows, K + 16), 0xAB, dtype=torch.uint8)
        want[:, 8:8 + K] = qr
        assert torch.equal(s2.cpu(), sr) and torch.equal(dst.cpu(), want), (K, rows)
    _note(f"quant_rows_fp8 K{K} mismatching bytes", 0.0)


def test_quant_rows_fp8_refusals(dev):
    from revisionllm_amd import hip, ops
    with pytest.raises(hip.HipLibraryError, match="multiples of 8"):
        ops.quant_rows_fp8(torch.zeros(2, 12, dtype=op(), device=dev))
    # ldx = K + 4 at the entry point itself (the wrapper copies a window whose row stride the kernel cannot take)
    x, q, sc = torch.zeros(2, 64 + 4, dtype=op(), device=dev), torch.zeros(2, 64, dtype=torch.uint8, device=dev), torch.zeros(2, device=dev)
    rc = hip.lib(op()).rv_quant_rows_fp8(hip.ptr(x), 64 + 4, hip.ptr(q), 64, hip.ptr(sc), 2, 64, hip.stream())
    assert rc != 0
    with pytest.raises(hip.HipLibraryError, match="multiples of 8"):
        hip.check(rc, "rv_quant_rows_fp8")
    xw = _quant_rows(64, 5)                                           # ... and the wrapper's copy of such a window gives the plain answer
    wide = torch.zeros(5, 64 + 4, dtype=op())
    wide[:, :64] = xw
    qw, sw = ops.quant_rows_fp8(wide.to(dev)[:, :64])
    qr, sr = quant_ref(xw)
    assert torch.equal(sw.cpu(), sr) and torch.equal(qw.cpu(), qr)


# ------------------------------------------------------------------ entropy_stats ------------------------------------------------------------------
def _entropy_check(dev, logits, label):
    from revisionllm_amd import ops
    st = ops.entropy_stats(logits.to(dev)).cpu()
    ref = entropy_stats_ref64(logits)
    G = logits.shape[1]
    _note(f"entropy {label} max/min/mean rel", float(((st[:, :3].double() - ref[:, :3]).abs() / ref[:, :3].abs().clamp_min(1e-3)).max()))
    assert torch.allclose(st[:, :3].double(), ref[:, :3], rtol=1e-5), (label, st, ref)              # (atol: allclose's 1e-8, as test_sample_and_scores)
    if G == 1:
        assert bool(torch.isnan(st[:, 3]).all())
    else:
        e = float((st[:, 3].double() - ref[:, 3]).abs().max())
        _note(f"entropy {label} std abs / H", e / max(float(ref[:, 0].abs().max()), 1e-30))
        assert e <= 2e-6 * float(ref[:, 0].abs().max()), (label, st, ref)
    return st


@pytest.mark.parametrize("V,G,B", [(1, 1, 1), (1, 7, 3), (63, 2, 3), (63, 300, 1), (64, 1, 3), (64, 7, 1), (1000, 2, 1), (1000, 300, 3), (1025, 7, 3), (1025, 300, 1),
                                   (32000, 1, 1), (32000, 2, 3), (32000, 7, 1)])
def test_entropy_stats_shapes(dev, V, G, B):
    """Vocabularies below, at and just past the block's 1024 threads and its 64-lane waves, few and many steps (G = 300 only where the case stays a few MB)."""
    _entropy_check(dev, feats(f"rse.ent.{V}.{G}.{B}", (B, G, V)) * 1.3, f"V{V} G{G} B{B}")


def test_entropy_stats_peaked_and_flat_rows_and_the_step_limit(dev):
    from revisionllm_amd import hip, ops
    for V in (63, 1025):
        x = torch.full((1, 3, V), float("-inf"))
        x[0, :, V // 2] = torch.tensor([0.5, -2.0, 7.0])           # one finite score: p = 1 there, H = -log(1 + 1e-10), which is 0 in f32 - exactly
        st = _entropy_check(dev, x, f"V{V} one finite")
        assert bool((st == 0).all())
        flat = torch.full((2, 2, V), 1.25)
        st = _entropy_check(dev, flat, f"V{V} flat")
        assert torch.allclose(st[:, :3].double(), torch.full((2, 3), math.log(V), dtype=torch.float64), rtol=1e-5)
    with pytest.raises(hip.HipLibraryError, match="G=8193 too large"):
        ops.entropy_stats(torch.zeros(1, 8193, 4, device=dev))
    _entropy_check(dev, feats("rse.ent.g8192", (1, 8192, 4)), "V4 G8192")          # the last accepted step count (128 KB)


@pytest.mark.parametrize("V", [1000, 1500, 32000])
def test_sample_raw_entropy_is_bit_identical_to_entropy_stats(dev, V):
    """sample_kernel's comment: its raw entropy uses block_entropy()'s per-thread element order and block reductions, "so it is bit-identical to
    rv_entropy_stats on the same row"."""
    from revisionllm_amd import ops
    logits = (feats(f"rse.ent.bit.{V}", (3, V)) * 1.3).to(dev)
    raw = ops.sample(logits, None, False)["entropy_raw"]
    for b in range(3):
        assert torch.equal(raw[b], ops.entropy_stats(logits[b:b + 1, None])[0, 0]), (V, b)


# ------------------------------------------------------------------ topk_cosine ------------------------------------------------------------------
def cosine_plan(d, T, itemsize):
    """Host mirror of rv_topk_cosine's choice: "fast" (16-byte loads), "generic" or "refuse".  The source to keep in step is the body of
    ``extern "C" int rv_topk_cosine`` in revisionllm_amd/csrc/sample.hip (``vec``, ``chunks``, ``groups``, ``sm_fast`` and the RV_CHECK_ARG on
    5 * d + T): nothing on the device reports which kernel ran, so a change of that rule must be repeated here, or the T = 7936 / 7937 pair stops
    straddling the switch (test_scores_reference_logic.test_host_mirror_of_the_cosine_kernel_choice pins today's numbers)."""
    vec = 16 // itemsize
    chunks = d // vec
    groups = 1024 // chunks if 0 < chunks <= 1024 else 0
    if d % vec == 0 and groups > 0 and ((groups + 1) * d + T) * 4 <= LDS_BYTES:
        return "fast"
    return "generic" if (5 * d + T) * 4 <= LDS_BYTES else "refuse"


def last_T(d, itemsize, plan):
    """The largest T that ``cosine_plan`` answers with ``plan``: the answer moves fast -> generic -> refuse as T grows, so by bisection."""
    order = {"fast": 0, "generic": 1, "refuse": 2}
    lo, hi = 0, 1 << 20
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if order[cosine_plan(d, mid, itemsize)] <= order[plan] else (lo, mid - 1)
    assert lo > 0 and cosine_plan(d, lo, itemsize) == plan
    return lo


def cosine_inputs(n, T, d, kind, tag=""):
    """Frames that share a component along the query (similarities mostly positive, as CLIP features have them: the sums do not cancel) with a
    different weight per segment (a wrong block offset shows); -> (features as f32 holding ``kind``-representable values, q)."""
    q = feats(f"rse.tc.q.{d}{tag}", (d,))
    f = feats(f"rse.tc.f.{n}.{T}.{d}{tag}", (n, T, d)) + q * (0.15 + 0.1 * torch.arange(n, dtype=torch.float32))[:, None, None]
    return _rt(f, kind), q


def _cosine(dev, f, q, k, kind):
    from revisionllm_amd import ops
    return ops.topk_cosine(f.to(_dt(kind)).to(dev), q.to(dev), k).cpu()


def _kinds():
    return (fl(), "f32")


@pytest.mark.parametrize("d", [8, 64, 768, 4096, 12, 772, 6])
def test_topk_cosine_widths_of_both_kernels(dev, d):
    """The 16-byte-load kernel (d a multiple of the vector: 8 / 64 / 768 / 4096) and the generic kernel by width (d = 12, 772 with 16-bit features, d = 6 with
    f32).  d = 12 and 772 run the SAME values through the generic kernel (16-bit) and the 16-byte-load kernel (f32): they agree within the bound."""
    n, T = 5, 37
    got = {}
    for kind in _kinds():
        plan = cosine_plan(d, T, 2 if kind != "f32" else 4)
        assert plan == {8: "fast", 64: "fast", 768: "fast", 4096: "fast", 12: "generic" if kind != "f32" else "fast",
                        772: "generic" if kind != "f32" else "fast", 6: "generic"}[d]
        f, q = cosine_inputs(n, T, d, fl() if d in (12, 772) else kind)
        for k in (3, 0):
            y = _cosine(dev, f, q, k, kind)
            got[kind, k] = y
            assert _err(y, topk_cosine_ref64(f, q, k), f"topk_cosine {kind} {plan} d{d} T{T} k{k}") < COSINE_BOUND, (d, kind, k)
            assert _err(_cosine(dev, f[:1], q, k, kind), topk_cosine_ref64(f[:1], q, k), f"topk_cosine {kind} {plan} d{d} T{T} k{k} n1") < COSINE_BOUND
    if d in (12, 772):
        for k in (3, 0):
            assert _err(got[fl(), k], got["f32", k].double(), f"topk_cosine generic vs fast d{d} k{k}") < COSINE_BOUND


@pytest.mark.parametrize("T", [1, 2, 3, 4, 15, 16, 17, 63, 64, 65])
def test_topk_cosine_frame_counts(dev, T):
    """Frame counts around the 16 waves of the score loop and the 64 lanes of the selection, k below, at and above T (the sum takes min(k, T)), in both
    kernels (d = 64: 16-byte loads; d = 12 16-bit / d = 6 f32: generic), one and five segments."""
    for kind in _kinds():
        for d in (64, 12 if kind != "f32" else 6):
            f, q = cosine_inputs(5, T, d, kind)
            for k in (0, 1, 3, T, T + 5):
                for n in (1, 5):
                    y = _cosine(dev, f[:n], q, k, kind)
                    e = _err(y, topk_cosine_ref64(f[:n], q, k), f"topk_cosine {kind} {cosine_plan(d, T, 2 if kind != 'f32' else 4)} d{d} T{T} k{k} n{n}")
                    assert e < COSINE_BOUND, (kind, d, T, k, n, e)


def test_topk_cosine_two_identical_frames_among_the_top_three(dev):
    for kind in _kinds():
        for d in (768, 12 if kind != "f32" else 6):
            f, q = cosine_inputs(3, 40, d, kind, tag=".tie")
            first = rank_order(cosine_sims64(f) @ q.double(), 1)[:, 0]
            for i in range(3):
                f[i, (int(first[i]) + 7) % 40] = f[i, int(first[i])]
            sims = cosine_sims64(f) @ q.double()
            top = torch.sort(sims, 1, descending=True).values
            assert bool(((top[:, 0] == top[:, 1]) | (top[:, 1] == top[:, 2])).all()), "the copied frame is no longer among the top three"
            assert _err(_cosine(dev, f, q, 3, kind), topk_cosine_ref64(f, q, 3), f"topk_cosine {kind} d{d} tie") < COSINE_BOUND


def test_topk_cosine_at_the_lds_switch_between_the_kernels(dev):
    """d = 768 with 16-bit features: the last T the 16-byte-load kernel's LDS holds and the first the generic kernel takes over, both derived from the
    rule in rv_topk_cosine.  The fp32 oracle's own distance from float64 at this length goes into the log next to the asserted bound."""
    from oracle import scores
    T_fast = last_T(768, 2, "fast")
    assert cosine_plan(768, T_fast, 2) == "fast" and cosine_plan(768, T_fast + 1, 2) == "generic"
    f, q = cosine_inputs(1, T_fast + 1, 768, fl())
    ref = topk_cosine_ref64(f, q, 3)
    _note("topk_cosine T%d fp32 oracle (CPU) vs float64" % (T_fast + 1), rel_err(scores.stage2_cosine(f, q), ref))
    _note("topk_cosine asserted bound", COSINE_BOUND)
    for T in (T_fast, T_fast + 1):
        plan = cosine_plan(768, T, 2)
        for k in (3, 0):
            e = _err(_cosine(dev, f[:, :T], q, k, fl()), topk_cosine_ref64(f[:, :T], q, k), f"topk_cosine {fl()} {plan} d768 T{T} k{k}")
            assert e < COSINE_BOUND, (T, k, e)


def test_topk_cosine_lds_refusals_and_the_last_accepted_length(dev):
    from revisionllm_amd import hip, ops
    d16, d32 = 12, 6
    for kind, d in ((fl(), d16), ("f32", d32)):
        item = 2 if kind != "f32" else 4
        T = last_T(d, item, "generic")
        assert (5 * d + T) * 4 == LDS_BYTES and cosine_plan(d, T + 1, item) == "refuse"
        f, q = cosine_inputs(1, T + 1, d, kind)
        assert _err(_cosine(dev, f[:, :T], q, 3, kind), topk_cosine_ref64(f[:, :T], q, 3), f"topk_cosine {kind} generic d{d} T{T} k3") < COSINE_BOUND
        with pytest.raises(hip.HipLibraryError, match=r"5\*d \+ T too large for LDS"):
            _cosine(dev, f, q, 3, kind)
    assert cosine_plan(4096, 4096, 2) == "fast" and cosine_plan(4096, 4097, 2) == "refuse"             # d = 4096, 16-bit: fits neither kernel
    with pytest.raises(hip.HipLibraryError, match=r"5\*d \+ T too large for LDS"):
        ops.topk_cosine(torch.ones(1, 4097, 4096, dtype=op(), device=dev), torch.ones(4096, device=dev), 3)


def test_topk_cosine_non_finite_inputs_give_nan_as_the_reference_does(dev):
    """One NaN element, and one column that is zero in every frame (0 / 0 in its norm): every similarity of that segment is NaN; one +inf element: the
    similarity of its frame alone is NaN.  The reference (torch.topk ranks NaN greatest) returns NaN for k = 3 and 1 as for k = 0, and so do both
    kernels; the neighbouring segments keep their values.
    (Before the score kernels ranked NaN first, their k > 0 selection skipped every NaN and summed -inf.)"""
    for kind in _kinds():
        for d in (64, 12 if kind != "f32" else 6):
            f, q = cosine_inputs(5, 17, d, kind, tag=".nan")
            f[1, 9, d // 2] = float("nan")
            f[3, :, 1] = 0.0
            f[2, 4, 2] = float("inf")               # inf / inf: the similarity of frame 4 alone is NaN, the other 16 are numbers (the column gives them 0)
            nan_sims = torch.isnan(cosine_sims64(f) @ q.double()).sum(1).tolist()
            assert nan_sims == [0, 17, 1, 17, 0]
            for k in (3, 1, 0):                     # k = 1 and 3 < T: only a rank order with NaN FIRST takes segment 2's one NaN similarity into the sum
                ref = topk_cosine_ref64(f, q, k)
                assert torch.isnan(ref).tolist() == [False, True, True, True, False]
                y = _cosine(dev, f, q, k, kind)
                assert torch.isnan(y).tolist() == [False, True, True, True, False], (kind, d, k, y)
                ok = torch.tensor([0, 4])
                assert _err(y[ok], ref[ok], f"topk_cosine {kind} d{d} k{k} next to NaN segments") < COSINE_BOUND


# ------------------------------------------------------------------ topk_pool ------------------------------------------------------------------
POOL_CASES = [(1, 1, 768, 1, 1), (2, 3, 768, 1, 3), (3, 17, 768, 4, 3), (2, 64, 768, 2, 64), (2, 65, 772, 3, 5), (1, 250, 4096, 2, 3), (4, 14, 8, 5, 14)]
# one seed per case for which rank_gap >= GAP holds for the f16-, the bf16- and the f32-valued data alike (found by counting up from 0;
# test_scores_reference_logic.test_pool_seeds_keep_the_rank_gap re-checks every one on the CPU)
POOL_SEEDS = {(1, 1, 768, 1, 1): 0, (2, 3, 768, 1, 3): 0, (3, 17, 768, 4, 3): 0, (2, 64, 768, 2, 64): 12, (2, 65, 772, 3, 5): 0, (1, 250, 4096, 2, 3): 0,
              (4, 14, 8, 5, 14): 2}


@functools.lru_cache(maxsize=None)
def pool_inputs(case, kind, seed=None):
    Nv, T, d, Nt, k = case
    seed = POOL_SEEDS[case] if seed is None else seed
    video = _rt(feats(f"rse.tp.v.{case}", (Nv, T, d), seed=seed), kind)
    text = feats(f"rse.tp.t.{case}", (Nt, d), seed=seed)
    return video, text


def _pool(dev, text, video, k, kind):
    from revisionllm_amd import ops
    y, idx = ops.topk_pool(text.to(dev), video.to(_dt(kind)).to(dev), k, return_index=True)
    return y.cpu(), idx.cpu().long()


@pytest.mark.parametrize("case", POOL_CASES, ids=lambda c: "Nv%d-T%d-d%d-Nt%d-k%d" % c)
def test_topk_pool_geometries(dev, case):
    """k = 1, k = T (every frame listed: a permutation of 0 .. T - 1 in descending similarity), k = 64, T below / at / above the 64 lanes of the
    selection, a width that is no multiple of 256, several texts per video; the index list exactly, the pooled rows at 1e-6."""
    Nv, T, d, Nt, k = case
    for kind in _kinds():
        video, text = pool_inputs(case, kind)
        ref, ridx, sims = topk_pool_ref64(text, video, k)
        assert rank_gap(sims, k) >= GAP, "pick another seed for this case"
        y, idx = _pool(dev, text, video, k, kind)
        assert torch.equal(idx, ridx), (case, kind)
        assert _err(y, ref, f"topk_pool {kind} Nv{Nv} T{T} d{d} Nt{Nt} k{k}") < POOL_BOUND
        if k == T:
            assert torch.equal(torch.sort(idx, -1).values, torch.arange(T).expand(Nv, Nt, T))


def test_topk_pool_exact_ties_take_the_lower_index(dev):
    """Two bit-identical frames on the k-th and the (k + 1)-th place: the lower index is selected, whichever of the two it is."""
    case = (3, 17, 768, 4, 3)
    for kind in _kinds():
        video, text = pool_inputs(case, kind)
        video, text = video[:1].clone(), text[:1]
        third = int(rank_order(torch.einsum("vtd,jd->vtj", video.double(), text.double()), 1)[0, 2, 0])
        for other in ((third + 5) % 17, (third - 5) % 17):
            v = video.clone()
            v[0, other] = v[0, third]
            ref, ridx, sims = topk_pool_ref64(text, v, 3)
            assert ridx[0, 0, 2] == min(third, other) and max(third, other) not in ridx[0, 0].tolist()
            y, idx = _pool(dev, text, v, 3, kind)
            assert torch.equal(idx, ridx) and _err(y, ref, f"topk_pool {kind} tie at the k-th place") < POOL_BOUND


def test_topk_pool_refusals(dev):
    from revisionllm_amd import hip, ops
    v, t = torch.zeros(1, 70, 8, dtype=op(), device=dev), torch.zeros(1, 8, device=dev)
    for k in (0, 65):
        with pytest.raises(hip.HipLibraryError, match=r"k=%d must be in \[1, min\(64, T=70\)\]" % k):
            ops.topk_pool(t, v, k)
    with pytest.raises(hip.HipLibraryError, match=r"k=6 must be in \[1, min\(64, T=5\)\]"):
        ops.topk_pool(t, v[:, :5], 6)
    T = (LDS_BYTES - 256) // 4 - 8                                   # the last (d + T) * 4 + 256 that fits, then one more frame
    big = torch.zeros(1, T + 1, 8, dtype=op(), device=dev)
    assert ops.topk_pool(t, big[:, :T], 3).shape == (1, 1, 8)
    with pytest.raises(hip.HipLibraryError, match=r"d \+ T too large for LDS"):
        ops.topk_pool(t, big, 3)


def pool_nan_inputs(T, kind, nan_frames):
    video = _rt(feats(f"rse.tp.nan.{T}", (3, T, 768)), kind)
    text = feats("rse.tp.nan.t", (2, 768))
    for j, t_ in enumerate(nan_frames):
        video[1, t_, 100 + j] = float("nan")
    return video, text


def pool_nan_cases(T):
    return ((T // 2,), (0, T - 1))


def pool_nan_gap(sims, k, nan_frames):
    """rank_gap of the finite videos 0 and 2, and of video 1's finite frames for the k - len(nan_frames) places the NaN frames leave."""
    keep = [t for t in range(sims.shape[1]) if t not in nan_frames]
    return min(rank_gap(sims[[0, 2]], k), rank_gap(sims[1:2, keep], k - len(nan_frames)))


@pytest.mark.parametrize("T,k", [(3, 3), (17, 3)])
def test_topk_pool_nan_frames_are_selected_as_the_reference_selects_them(dev, T, k):
    """One and two frames with a NaN element in video 1 of 3 (never more than k, so the selected set is determined): torch.topk ranks their NaN
    similarity first, so the index list holds each of them and nothing outside [0, T), the pooled row is NaN exactly where the reference's is, and the
    other videos match their finite reference.  (Before the score kernels ranked NaN first, a round that found no number left stored index
    0x7fffffff: an LDS write and a global read far outside the video.)"""
    for kind in _kinds():
        for nan_frames in pool_nan_cases(T):
            video, text = pool_nan_inputs(T, kind, nan_frames)
            ref, ridx, sims = topk_pool_ref64(text, video, k)
            assert pool_nan_gap(sims, k, nan_frames) >= GAP
            y, idx = _pool(dev, text, video, k, kind)
            assert bool(((idx >= 0) & (idx < T)).all()), idx
            for j in range(2):
                got = idx[1, j].tolist()
                assert len(set(got)) == k and set(nan_frames) <= set(got), (got, nan_frames)
            assert torch.equal(idx, ridx)                            # the NaN frames first (smaller index first), then the numbers in rank order
            assert torch.equal(torch.isnan(y), torch.isnan(ref))
            assert torch.allclose(y.double(), ref, rtol=0, atol=POOL_BOUND * float(ref[[0, 2]].abs().max()), equal_nan=True)
            _err(y[[0, 2]], ref[[0, 2]], f"topk_pool {kind} T{T} k{k} next to {len(nan_frames)} NaN frame(s)")
