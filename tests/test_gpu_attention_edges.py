"""``rv_attention`` at every kernel form, key-count and query-tile edge, mask pattern and buffer layout, in both builds, against the float64 oracle of
tests/attention_oracle.py and measured PER QUERY ROW (``row_err``): a late causal row is an average of a hundred values, ten times smaller than row 0, and a
fault that moves it by one key's weight disappears in a max-norm ratio over the tensor.

The cases are the records of ``attention_oracle.CASES``; tests/test_attention_reference_logic.py shows on the CPU that each of them fails (by at least
4 x the bound) for a dropped key, a shifted causal diagonal, a flipped mask byte, a stale staged block and two swapped V rows.

Bound: the kernel rounds P to the operand type once and the output once, everything else is f32 - two roundings of at most half an ulp each per element:
2 x 2^-11 = 9.8e-4 with fp16's 11 significant bits, 2 x 2^-8 = 7.8e-3 with bf16's 8 - so every comparison asserts row_err < tol(BF16_TOL) = 8e-3 / 1.33e-3, the
project's single-kernel bounds.  (Strictly that holds where V has one sign, as in the ``onehot`` probe; with V of both signs the rounding of P is relative to
sum p |v|, not to the row's largest |sum p v|, and the bound is met with the margin measured.)  Measured worst values, 7.9e-4 (fp16) and 6.4e-3 (bf16):
profiles/attention_edges_err_*.log.

Every call made here is valid or is refused by the entry point before any launch."""
import ctypes as C
import functools
import os

import pytest
import torch

import attention_oracle as ao
from helpers import BF16_TOL, fl, op, tol

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")
RV_ERR_ARG = -1


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


_WORST = {}       # (flavour, form, group) -> (worst row_err, case id / probe)


def _note(c, probe, value):
    """A line that names the case in the RV_LOG_ERR file (profiles/attention_edges_err_<flavour>.log); the worst value per form and group follows when the
    module is done (_write_worst, from the ``flav`` fixture)."""
    label = f"{ao.case_id(c)} {probe}"
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            fh.write(f"  attention {fl()} {label} {value:.3e}\n")
    key = (fl(), c.form, c.group)
    if not value <= _WORST.get(key, (-1.0, ""))[0]:
        _WORST[key] = (value, label)
    return value


def _write_worst(flavour):
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            for (f, form, group), (v, label) in sorted(_WORST.items()):
                if f == flavour:
                    fh.write(f"  attention {f} worst of form {form}, {group} cases: {v:.3e} ({label})\n")


# ------------------------------------------------------------------ calls ------------------------------------------------------------------
def _raw(dev, L, pad=None, null=None):
    """One rv_attention call on the buffers of a Layout (uploaded once per Layout; the output buffer fresh, all fill) -> (status, the output buffer's int16
    words on the device).  ``null``: 0 .. 3 = q / k / vt / out is handed over as NULL."""
    from revisionllm_amd import hip
    keep = getattr(L, "_dev", None)
    if keep is None:
        qb = L.q_buf.to(dev)
        keep = L._dev = (qb, qb if L.k_buf is L.q_buf else L.k_buf.to(dev), L.vt_buf.to(dev))
    out = L.out_buf.to(dev)
    padd = pad.to(dev).contiguous() if pad is not None else None
    args = list(L.args(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), out.data_ptr(), padd.data_ptr() if padd is not None else None, hip.stream()))
    if null is not None:
        args[(0, 3, 7, 11)[null]] = None
    rc = hip.lib(op()).rv_attention(*args)
    torch.cuda.synchronize()
    return rc, out


def _out_rows(L, words):
    return L.view_out(words.cpu().view(op())).float().reshape(L.B, L.Lq, L.H, L.dh)


def _run(dev, c, q, k, v, pad, layout=None):
    """The case's call on these operands -> ([B,Lq,H,dh] f32 on the host, fences intact?).  ``contig``: through ops.attention, else the C entry point on fenced buffers."""
    from revisionllm_amd import ops
    layout = layout or c.layout
    if layout == "contig":
        dt = op()
        y = ops.attention(q.to(dt).to(dev), k.to(dt).to(dev), v.to(dt).to(dev), causal=c.causal, key_pad=pad.to(dev) if pad is not None else None, q_pos0=c.q_pos0)
        return y.float().cpu().reshape(c.B, c.Lq, c.H, c.dh), True
    L = ao.build_layout(layout, q, k, v, fl(), causal=c.causal, q_pos0=c.q_pos0, kv_div=c.B // c.Bk)
    rc, words = _raw(dev, L, pad)
    assert rc == 0, rc
    return _out_rows(L, words), L.fence_intact(words)


@functools.lru_cache(maxsize=None)
def _first(form, group="edge", **want):
    return next(c for c in ao.CASES if c.form == form and c.group == group and all(getattr(c, n) == x for n, x in want.items()))


# ------------------------------------------------------------------ a, b, c, e: every record of the table ------------------------------------------------------------------
@pytest.mark.parametrize("c", ao.CASES, ids=ao.case_id)
def test_record_against_float64_per_row(dev, c):
    pad = ao.make_mask(c.mask, c.Bk, c.Lk)
    for probe in c.probes:
        q, k, v = ao.case_inputs(c, probe, fl())
        y, fenced = _run(dev, c, q, k, v, pad)
        e = _note(c, probe, ao.row_err(y, ao.case_reference(c, probe, fl())))
        print(f"{ao.case_id(c)} {probe} {fl()}: row_err {e:.3e}")
        assert bool(torch.isfinite(y).all()) and e < tol(BF16_TOL), (ao.case_id(c), probe, e)
        assert fenced, "a 16-bit word outside [b, row < Lq, col < H * dh] of the output buffer changed"


# ------------------------------------------------------------------ d. bitwise invariants ------------------------------------------------------------------
_ONE_PER_FORM = [("split", dict(dh=64, Lq=5, Lk=129, causal=False)), ("split", dict(dh=96, Lq=16, Lk=161, causal=True)),
                 ("split", dict(dh=128, Lq=5, Lk=129, causal=True)), ("wave", dict(dh=64, Lq=47, Lk=95)), ("wave", dict(dh=96, Lq=65, Lk=65, causal=True)),
                 ("wave", dict(dh=128, Lq=20, Lk=60)), ("lds", dict(dh=64, Lq=113, Lk=129)), ("lds", dict(dh=96, Lq=129, Lk=129)),
                 ("lds1", dict(dh=128, Lq=65, Lk=161, causal=True)), ("lds1", dict(dh=128, Lq=70, Lk=65, causal=False)), ("d512", dict(Lq=17, Lk=64))]


@pytest.mark.parametrize("form,want", _ONE_PER_FORM, ids=[f"{f}-" + "-".join(f"{n}{x}" for n, x in w.items()) for f, w in _ONE_PER_FORM])
def test_all_zero_mask_repeat_and_batch_position_change_no_bit(dev, form, want):
    """What the code's comments claim, on one record per form and head width: an all-zero key_pad leaves every bit (for the staged forms this sets their
    kernels against the per-wave PAD body on identical inputs); a second run repeats the first; the problem of batch 0 copied to batch B - 1 gives the
    rows of batch 0 there."""
    c = _first(form, **want)
    q, k, v = (t.clone() for t in ao.case_inputs(c, "random", fl()))
    q[c.B - 1], k[c.Bk - 1], v[c.Bk - 1] = q[0], k[0], v[0]
    y, _ = _run(dev, c, q, k, v, None)
    assert bool(torch.isfinite(y).all())
    assert torch.equal(_run(dev, c, q, k, v, None)[0], y), "two runs differ"
    assert torch.equal(y[c.B - 1], y[0]) and (c.B == 2 or not torch.equal(y[1], y[0])), "the same problem at batch 0 and at batch B - 1"
    z, _ = _run(dev, c, q, k, v, ao.make_mask("zeros", c.Bk, c.Lk))
    assert ao.dispatch(c.dh, c.Lq, c.Lk, c.causal, True) in ("wave", "split", "d512")
    assert torch.equal(z, y), f"an all-zero mask moved rows by up to {float((z - y).abs().max()):.3e}"


@pytest.mark.parametrize("dh", [64, 96])
def test_rows_do_not_depend_on_the_query_count(dev, dh):
    """On the same buffers at Lk = 129: rows 0 .. 46 of a call with Lq = 48 (the LDS-staged form) equal the rows of a call with Lq = 47 (the per-wave form)."""
    c = _first("lds", dh=dh, Lq=48, Lk=129)
    assert ao.dispatch(dh, 47, 129, False, False) == "wave"
    q, k, v = ao.case_inputs(c, "random", fl())
    L = ao.build_layout("contig", q, k, v, fl())
    rc, w48 = _raw(dev, L)
    assert rc == 0
    y48 = _out_rows(L, w48)
    L.Lq = 47                     # the strides still describe 48-row batches
    rc, w47 = _raw(dev, L)
    assert rc == 0
    y47 = _out_rows(L, w47)
    assert bool(torch.isfinite(y48).all()) and torch.equal(y47, y48[:, :47])
    assert L.fence_intact(w47), "the call with Lq = 47 wrote row 47"


# ------------------------------------------------------------------ f. refusals ------------------------------------------------------------------
def _refusals():
    r = [(f"null {n}", dict(null=i), "null tensor") for i, n in enumerate(("q", "k", "vt", "out"))]
    r += [(f"{n} = 0", {n: 0}, "empty problem") for n in ("B", "H", "Lq", "Lk", "kv_div")]
    r += [(f"{n} misaligned", {n: ("+", 2 if n == "o_rs" else 4)}, "stride alignment") for n in ("q_rs", "k_rs", "k_hs", "vt_ds", "vt_hs", "vt_bs", "o_rs")]
    r += [("vt_d_stride < ceil32(Lk)", dict(vt_ds=32), "multiple of 32 keys"), ("dh = 80", dict(dh=80), "head dim 80"),
          ("causal with q_pos0 < 0", dict(causal=True, q_pos0=-1), "q_pos0"), ("causal with q_pos0 < 0 and a mask", dict(causal=True, q_pos0=-3, mask=True), "q_pos0"),
          ("B % kv_batch_div != 0", dict(B=3, kv_div=2), "multiple of kv_batch_div")]
    return r


@pytest.mark.parametrize("name,change,text", _refusals(), ids=[r[0] for r in _refusals()])
def test_refusals_leave_the_output_alone(dev, name, change, text):
    """Each bad argument through the C ABI: RV_ERR_ARG, a message that names the fault, and not one word of a NaN-filled output written.  The buffers are those
    of a valid call (B = 4 over two key batches, Lk = 33, 64-wide heads), which is made first: the refusal is the argument's doing."""
    from revisionllm_amd import hip
    B, Bk, H, Lq, Lk, dh = 4, 2, 3, 5, 33, 64
    q, k, v = ao.probe_inputs("refusal", (B, Bk, H, Lq, Lk, dh), "random", fl())
    L = ao.build_layout("contig", q, k, v, fl(), kv_div=2)
    rc, words = _raw(dev, L)
    assert rc == 0 and ao.row_err(_out_rows(L, words), ao.ref_attention(q, k, v, kv_div=2)) < tol(BF16_TOL)
    change = dict(change)
    null, mask = change.pop("null", None), change.pop("mask", False)
    for n, x in change.items():
        setattr(L, n, getattr(L, n) + x[1] if isinstance(x, tuple) else x)
    rc, words = _raw(dev, L, pad=torch.zeros(Bk, Lk, dtype=torch.uint8) if mask else None, null=null)
    assert rc == RV_ERR_ARG, (name, rc)
    buf = C.create_string_buffer(512)
    hip.lib(op()).rv_last_error(buf, 512)
    assert text in buf.value.decode() and "attention" in buf.value.decode(), (name, buf.value)
    assert bool((words.cpu() == ao.NAN_FILL[fl()]).all()), "a refused call wrote to the output"
