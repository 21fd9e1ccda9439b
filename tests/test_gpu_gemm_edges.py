"""``rv_gemm`` at the smallest edge shapes of every kernel form behind it, in both builds, with operands whose sums are EXACT (tests/gemm_oracle.py): with no
activation or ReLU an f32 output must equal the float64 reference and a 16-bit output must equal it rounded to nearest even - zero tolerance, every element of
every row.  A dropped, doubled or misplaced k-fragment, row or column, and a late or stale stream-K partial, change an integer.

Every call writes into a buffer with guard rows below M and guard columns right of n_out, pre-filled with a sentinel; the guards must come back untouched.
Guard columns of 12 give ``ldc % 8 == 4`` (the direct 16-bit epilogue of the ring kernels), 16 give ``ldc % 8 == 0`` (their LDS-transposed one); residuals
have ``ldr > n_out`` the same way.  Each case names the kernel form it is meant to reach; the host mirrors of the dispatch derive the form for this machine's CU
count and the case fails with "the dispatch changed: ..." when they disagree.

SILU_MUL / QuickGELU: the pre-activation is still exact, the only error is the device activation's own.  It is measured per ELEMENT against float64,
|y - ref| / |ref| (results too small to be told from zero: absolutely), and asserted at ~2.5 x the values measured on the first run (profiles/gemm_edges_err_*.log), never above the suite's single-kernel
bounds: ``F32_TOL * 5`` for f32 outputs; for 16-bit outputs one output ulp (2^-10 fp16, 2^-7 bf16) plus that f32 term, which stays within ``tol(BF16_TOL)``.

Every call made here is valid or is refused by the entry point before any launch."""
import os
import time

import pytest
import torch

import gemm_oracle as go
from helpers import BF16_TOL, F32_TOL, fl, tol

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")
COLLECT_CUS = 256                                                   # the table's groups and forms do not depend on the CU count; its A-resident row counts do
GROUP_FORMS = sorted({(c.group, c.form) for c in go.cases(COLLECT_CUS)})

# Per-element error of the device activations on exact pre-activations, asserted (see the module docstring).  Measured worst values (profiles/gemm_edges_err_*.log,
# the same in both builds and in every kernel form): f32 outputs SILU_MUL 3.4e-6, QuickGELU 5.1e-6 - the argument of v_exp_f32 is a rounded f32 product, |x| * 2^-24 at
# |x| up to 88 - asserted at 2.5 x; 16-bit outputs 4.9e-4 (fp16) and 3.9e-3 (bf16) = half an output ulp, the rounding itself: 2.5 x that is above the cap of one output
# ulp plus the f32 term, so the cap is what is asserted.
ACT_F32_BOUND = {"silu_mul": 8.6e-6, "quick_gelu": 1.3e-5}
F32_CAP = F32_TOL * 5
OUT_ULP = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7}
# Results too small to be told from zero are compared absolutely.  rv_silu multiplies by v_rcp_f32(1 + exp(-g)), whose subnormal results (g < -87.3) come out as 0: the
# product g * r * up then misses at most 2^-126 * 2^7 * 2^14 = 2^-105 (|g| < 128 there, |up| <= 8 * 2048), and QuickGELU's exp overflows to the same effect below that
# magnitude.  An fp16 output below its smallest normal 2^-14 has an absolute spacing of 2^-24.
LOW = {"f32": 2.0 ** -105, "bf16": 2.0 ** -105, "f16": 2.0 ** -14}         # |ref| below this: |y - ref| <= LOW_ABS instead of the relative bound
LOW_ABS = {"f32": 2.0 ** -105, "bf16": 2.0 ** -105, "f16": 2.0 ** -24}


def _act_err(out, ref, kind):
    """-> (worst |y - ref| / |ref| over the elements with |ref| >= LOW[kind], worst |y - ref| over the others)."""
    a, d = ref.abs(), (out.double() - ref).abs()
    lo = a < LOW[kind]
    rel = float((d[~lo] / a[~lo]).max()) if bool((~lo).any()) else 0.0
    return rel, (float(d[lo].max()) if bool(lo.any()) else 0.0)


@pytest.fixture(scope="module", params=[None] if _FORCED else ["f16", "bf16"])
def flav(request, op_flavour):
    """Both operand flavours (the module list of conftest.py is fixed, so the module brings its own parameter; REVISION_TEST_FLAVOURS still narrows it)."""
    from revisionllm_amd import hip
    f = request.param or op_flavour or hip.flavour()
    prev = hip.set_flavour(f)
    t0 = time.time()
    yield f
    _write_worst(f, time.time() - t0)
    _CTX.clear()
    hip.set_flavour(prev)


@pytest.fixture(scope="module")
def dev(flav):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


ACT_NAME = {go.RV_ACT_SILU_MUL: "silu_mul", go.RV_ACT_QUICK_GELU: "quick_gelu"}
_WORST = {}       # (flavour, form, activation, output) -> (worst per-element error, case id)
_CTX = {}


def _note(c, out_kind, value):
    log = os.environ.get("RV_LOG_ERR")
    act = ACT_NAME[c.act]
    if log:
        with open(log, "a") as fh:
            fh.write(f"  gemm_edges {fl()} {c.id} {act} {out_kind} {value:.3e}\n")
    key = (fl(), c.form, act, out_kind)
    if not value <= _WORST.get(key, (-1.0, ""))[0]:
        _WORST[key] = (value, c.id)


def _write_worst(flavour, seconds):
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            for (f, form, act, out_kind), (v, cid) in sorted(_WORST.items()):
                if f == flavour:
                    fh.write(f"  gemm_edges {f} worst of form {form}, {act}, {out_kind} output: {v:.3e} ({cid})\n")
            fh.write(f"  gemm_edges {flavour} wall time of the module: {seconds:.1f} s\n")


def _ctx(c):
    from revisionllm_amd import hip
    if not c.opts:
        return None
    key = (fl(), c.opts)
    if key not in _CTX:
        _CTX[key] = hip.Options(flavour=fl(), **dict(c.opts))
    return _CTX[key]


class _Operands:
    """A case's operands on the device (drawn once per case and flavour) and its float64 product."""

    def __init__(self, dev, c):
        from helpers import op
        from revisionllm_amd import ops
        a, w, bias, res = go.exact_operands(c, op())
        self.a, self.w, self.bias, self.res = a.to(dev), w.to(dev), bias.to(dev), res.to(dev)
        self.a_arg = self.a
        if c.lda_pad:                                                # a strided A: row stride K + pad, the pad holds finite garbage
            big = torch.full((c.M, c.K + c.lda_pad), 3.0, dtype=op(), device=dev)
            big[:, :c.K] = self.a
            self.a_arg = big[:, :c.K]
        self.w_arg = ops.pack_fragments(self.w) if c.packed else self.w
        self.z = self.a.double() @ self.w.double().t()


def _epilogue(c, epi):
    """-> (act, bias?, residual?) of a run."""
    if epi == "act":
        return c.act, c.act == go.RV_ACT_QUICK_GELU, False
    return {"plain": go.RV_ACT_NONE, "brr": go.RV_ACT_RELU, "br": go.RV_ACT_RELU}[epi], epi != "plain", epi == "brr"


def _run(dev, c, o, out_kind, epi, pad, alias=False):
    """One rv_gemm call of the case into a guarded buffer -> list of complaints (empty: exact / within the activation bound, guards intact)."""
    from helpers import op
    from revisionllm_amd import ops
    act, use_bias, use_res = _epilogue(c, epi)
    od = op() if out_kind == "op16" else torch.float32
    no = go.n_out(c.N, act)
    buf = torch.full((c.M + c.guard_rows, no + pad), go.SENTINEL, dtype=od, device=dev)
    out = buf[:c.M, :no]
    r = None
    if alias:                                                        # C aliases the residual (the engine's o / down projections)
        out.copy_(o.res)
        r = out
    elif use_res:
        rbuf = torch.full((c.M, no + 12), 0.25, dtype=torch.float32, device=dev)      # ldr > n_out
        rbuf[:, :no] = o.res
        r = rbuf[:, :no]
    ops.gemm(o.a_arg, o.w_arg, bias=o.bias if use_bias else None, residual=r, act=act, out=out, w_packed=c.packed, stream_k=c.stream_k, ctx=_ctx(c))
    what = f"{c.id} [{out_kind} {epi} ldc=n+{pad}{' alias' if alias else ''}]"
    bad = []
    if not bool((buf[c.M:] == go.SENTINEL).all()):
        rows = (buf[c.M:] != go.SENTINEL).any(dim=1).nonzero().flatten()
        bad.append(f"{what}: {len(rows)} guard rows below M written (first M+{int(rows[0])})")
    if not bool((buf[:c.M, no:] == go.SENTINEL).all()):
        bad.append(f"{what}: guard columns right of n_out written")
    exact = epi in go.EXACT_EPILOGUES
    ref = go.epilogue_reference(o.z, o.bias if use_bias else None, o.res if (use_res or alias) else None, act, exact=exact)
    if exact:
        want = go.cast_rne(ref, od)
        if not torch.equal(out, want):
            ne = out != want
            i = ne.nonzero()[0].tolist()
            bad.append(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ from the float64 reference, first at {i}: {float(out[i[0], i[1]])} != {float(want[i[0], i[1]])}")
        return bad
    kind = fl() if out_kind == "op16" else "f32"
    if kind == "f16":
        ref = ref.clamp(-65504.0, 65504.0)                           # the fp16 build's conversions saturate
    err, low = _act_err(out, ref, kind)
    _note(c, out_kind, err)
    f32_bound = ACT_F32_BOUND[ACT_NAME[c.act]]
    bound = f32_bound if kind == "f32" else OUT_ULP[kind] + f32_bound
    assert f32_bound <= F32_CAP and (kind == "f32" or bound <= tol(BF16_TOL))            # never above the suite's single-kernel bounds
    if not err < bound:
        bad.append(f"{what}: per-element error {err:.3e} >= {bound:.3e}")
    if not low <= LOW_ABS[kind]:
        bad.append(f"{what}: an element below {LOW[kind]:.1e} is off by {low:.3e}")
    return bad


def _report(bad):
    assert not bad, "%d failing runs:\n%s" % (len(bad), "\n".join(bad[:60]))


@pytest.mark.parametrize("group,form", GROUP_FORMS, ids=["%s-%s" % gf for gf in GROUP_FORMS])
def test_exact_sums_at_the_edges_of_every_form(dev, cus, group, form):
    """Every case of the table that belongs to this group and form: the mirror check for this machine's CU count, then all of its runs (stream-K cases twice)."""
    table = [c for c in go.cases(cus) if (c.group, c.form) == (group, form)]
    assert table, "the table has no case of this group and form on %d CUs" % cus
    bad = []
    for c in table:
        go.check_form(c, cus)
        assert go.exactness_bound(c) < 2 ** 24
        o = _Operands(dev, c)
        for _ in range(2 if c.stream_k else 1):
            for out_kind, epi, pad in c.runs:
                bad += _run(dev, c, o, out_kind, epi, pad)
    _report(bad)


def test_every_named_form_is_reached_on_this_machine(dev, cus):
    table = go.cases(cus)
    assert {go.check_form(c, cus) for c in table} == set(go.FORMS_NAMED)
    assert sorted({(c.group, c.form) for c in table}) == GROUP_FORMS


def test_stream_k_workspace_carries_nothing_from_one_shape_to_the_next(dev, cus):
    """A, B, A: three launches of different shapes (and team counts) on the same workspace, each exact - a stale partial or an epoch slip shows as a wrong integer."""
    pick = {c.id: c for c in go.cases(cus) if c.group == "sk" and c.form == "pp_sk"}
    A = next(c for c in pick.values() if (c.M, c.N, c.K) == (200, 768, 256) and dict(c.opts)["gemm_cus"] == 8)
    B = next(c for c in pick.values() if (c.M, c.N, c.K) == (257, 768, 256) and dict(c.opts)["gemm_cus"] == 16)
    C = next(c for c in pick.values() if (c.M, c.N, c.K) == (200, 2816, 256))
    ops_ = {c.id: _Operands(dev, c) for c in (A, B, C)}
    bad = []
    for c in (A, B, A, C, A, B):
        bad += _run(dev, c, ops_[c.id], "f32", "brr", 12)
        bad += _run(dev, c, ops_[c.id], "op16", "plain", 12)
    _report(bad)


def test_output_aliasing_the_residual(dev, cus):
    """C == residual (f32; what the engine does behind every o / down projection), one shape per form: ring, A-resident, ping-pong tiled and stream-K."""
    bad = []
    for c in go.alias_cases(cus):
        go.check_form(c, cus)
        o = _Operands(dev, c)
        for epi in ("plain", "brr"):
            bad += _run(dev, c, o, "f32", epi, 12, alias=True)
    _report(bad)


def test_argument_errors_leave_the_output_untouched(dev):
    """Each refused call comes back as HipLibraryError with its message, and the sentinel-filled output is as it was."""
    from helpers import op
    from revisionllm_amd import hip, ops
    M, K = 8, 128

    a = torch.ones(M, K, dtype=op(), device=dev)
    a_bad = torch.ones(M, K + 4, dtype=op(), device=dev)[:, :K]                       # lda % 8 == 4
    w = lambda n: torch.ones(n, K, dtype=op(), device=dev)                              # noqa: E731
    calls = [   # (message, A, N, packed, bias?, act, n_out, ldc)
        ("packed W needs N%16==0", a, 24, True, False, hip.RV_ACT_NONE, 24, 36),
        ("alignment", a, 32, False, False, hip.RV_ACT_NONE, 32, 34),                   # ldc % 4 == 2
        ("alignment", a_bad, 32, False, False, hip.RV_ACT_NONE, 32, 44),
        ("SILU_MUL needs N%32==0 and no bias/residual", a, 64, False, True, hip.RV_ACT_SILU_MUL, 32, 44),
        ("SILU_MUL needs N%32==0 and no bias/residual", a, 48, False, False, hip.RV_ACT_SILU_MUL, 24, 36),
    ]
    for msg, a_arg, N, packed, use_bias, act, no, ldc in calls:
        for od in (torch.float32, op()):
            base = torch.full((M + 3, ldc), go.SENTINEL, dtype=od, device=dev)
            with pytest.raises(hip.HipLibraryError, match=msg):
                ops.gemm(a_arg, w(N), bias=torch.ones(N, device=dev) if use_bias else None, act=act, out=base[:M, :no], w_packed=packed, stream_k=False)
            torch.cuda.synchronize()
            assert bool((base == go.SENTINEL).all()), msg
