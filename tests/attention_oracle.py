"""What the attention tests share (no GPU needed): a float64 statement of ``rv_attention``, a per-row error measure, input probes that make ONE key's weight
visible in the output, a builder of strided / fenced buffers for the C ABI, and the table of cases that tests/test_gpu_attention_edges.py runs on the GPU
and tests/test_attention_reference_logic.py vouches for on the CPU (oracle against torch, buffers round trip, every case sensitive to every mutant).

Shapes are [B, L, H, dh] for q / k / v and for the reference, as ``ops.attention`` takes them; a key batch serves ``kv_div`` consecutive query batches."""
import collections
import ctypes as C
import functools
import math
import os

import numpy as np
import torch

from helpers import feats

OP = {"f16": torch.float16, "bf16": torch.bfloat16}
NAN_FILL = {"f16": 0x7E01, "bf16": 0x7FC1}        # a quiet NaN with a payload bit: what the output buffers hold before a call
VT_PAD = 1000.0                                   # V^T columns Lk .. ceil32(Lk) - 1 (the ABI wants them finite): a dead key must weigh exactly 0


def ceil32(n):
    return (n + 31) // 32 * 32


# ------------------------------------------------------------------ the operation, float64 ------------------------------------------------------------------
def visibility(B, Lq, Lk, causal, key_pad, q_pos0, kv_div):
    """bool [B, Lq, Lk]: key j counts for query i of batch b iff it is not padded in key batch b // kv_div and (causal) j <= q_pos0 + i."""
    vis = torch.ones(B, Lq, Lk, dtype=torch.bool)
    if key_pad is not None:
        vis &= ~torch.as_tensor(key_pad).bool().repeat_interleave(kv_div, 0)[:, None, :]
    if causal:
        vis &= (torch.arange(Lk)[None, :] <= q_pos0 + torch.arange(Lq)[:, None])[None]
    return vis


def attend(q, k, v, vis, kv_div, scale):
    """softmax over the visible keys of q . k * scale, times v, in float64; a query without a visible key gives a zero row (the library's rule for an
    all-padded key batch; torch gives NaN there)."""
    k = k.double().repeat_interleave(kv_div, 0)
    v = v.double().repeat_interleave(kv_div, 0)
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k) * float(scale)
    s = s.masked_fill(~vis[:, None], float("-inf"))
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    den = e.sum(-1, keepdim=True)
    p = torch.where(den > 0, e / den.clamp_min(1e-300), torch.zeros_like(e))
    return torch.einsum("bhqk,bkhd->bqhd", p, v)


def default_scale(dh):
    return float(np.float32(1.0 / math.sqrt(dh)))        # what ops.attention hands the kernel (an f32 argument)


def ref_attention(q, k, v, causal=False, key_pad=None, q_pos0=0, kv_div=1, scale=None):
    """q [B,Lq,H,dh], k / v [Bk,Lk,H,dh] AS STORED (already rounded to the 16-bit type) -> [B,Lq,H,dh] float64."""
    B, Lq, _, dh = q.shape
    vis = visibility(B, Lq, k.shape[1], causal, key_pad, q_pos0, kv_div)
    return attend(q, k, v, vis, kv_div, default_scale(dh) if scale is None else scale)


def row_err(y, ref):
    """The worst query row and head ([.., dh] rows): max_c |y - ref| / max(max_c |ref|, 1e-3 * max |ref| of the tensor).  The floor only lets exact-zero rows
    compare absolutely.  A NaN in y gives NaN (which is below no bound).  RV_LOG_ERR=<file>: appends "<test file>:<line> <value>" as helpers.rel_err does."""
    y, ref = torch.as_tensor(y).double(), torch.as_tensor(ref).double()
    assert y.shape == ref.shape, (y.shape, ref.shape)
    floor = max(1e-3 * float(ref.abs().max()), 1e-30)
    r = (y - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(floor)
    e = float("nan") if bool(torch.isnan(r).any()) else float(r.max())
    log = os.environ.get("RV_LOG_ERR")
    if log:
        import inspect
        f = inspect.stack()[1]
        with open(log, "a") as fh:
            fh.write(f"{os.path.basename(f.filename)}:{f.lineno} {e:.3e}\n")
    return e


# ------------------------------------------------------------------ the cases ------------------------------------------------------------------
Case = collections.namedtuple("Case", "group form dh B Bk H Lq Lk causal q_pos0 mask layout probes")
EDGE_PROBES = ("onehot", "random")
STRESS_PROBES = ("ramp_up", "ramp_down", "spike0", "spike32", "spike_last", "flat")
MASKS = ("lead", "interior", "alt", "last", "first", "tail")
LAYOUTS = ("contig", "fused", "cache", "window")


def case_id(c):
    return (f"{c.group}-{c.form}-dh{c.dh}-B{c.B}k{c.Bk}-q{c.Lq}-k{c.Lk}" + (f"-causal{c.q_pos0}" if c.causal else "") +
            (f"-{c.mask}" if c.mask != "none" else "") + (f"-{c.layout}" if c.layout != "contig" else ""))


def dispatch(dh, Lq, Lk, causal, masked):
    """The kernel form k_attention picks (default options): "split" (Lq <= 16: four waves share the keys), "lds" (64 / 96-wide heads, staged keys, two tiles
    per wave), "lds1" (128-wide heads, staged keys), "wave" (each wave fetches its own keys), "d512"."""
    if dh == 512:
        return "d512"
    if Lq <= 16:
        return "split"
    if not masked and not causal and Lk >= 96 and Lq >= 48 and dh in (64, 96):
        return "lds"
    if dh == 128 and not masked and Lk >= 64:
        return "lds1"
    return "wave"


def make_mask(name, Bk, Lk):
    """uint8 [Bk, Lk] (1 = hidden) or None.  Key batch 0 is never masked; every further batch carries the pattern, shifted by its index where that keeps
    the pattern's kind, so that no two batches hide the same keys."""
    if name == "none":
        return None
    pad = torch.zeros(Bk, Lk, dtype=torch.uint8)
    if name == "zeros":
        return pad
    for b in range(1, Bk):
        if name == "lead":
            pad[b, :32] = 1
        elif name == "interior":
            pad[b, 32:64] = 1
        elif name == "alt":
            pad[b, (b - 1) % 2::2] = 1              # batch 1 hides the even keys (key 0 among them)
        elif name == "last":
            pad[b, :Lk - 1] = 1
        elif name == "first":
            pad[b, 1:] = 1
        elif name == "tail":
            pad[b, Lk - 5 - b:] = 1
        else:
            raise ValueError(name)
    return pad


def _case(group, dh, B, Bk, Lq, Lk, causal=False, q_pos0=0, mask="none", layout="contig", probes=EDGE_PROBES, H=None):
    H = H or (2 if dh == 512 else 3)
    return Case(group, dispatch(dh, Lq, Lk, causal, mask != "none"), dh, B, Bk, H, Lq, Lk, bool(causal), q_pos0, mask, layout, tuple(probes))


def _build_cases():
    cs = []
    # a. key-count and query-tile edges
    for dh in (64, 96, 128):
        for Lq in (1, 5, 16):
            for Lk in (1, 31, 32, 33, 127, 128, 129, 160, 161):
                cs.append(_case("edge", dh, 2, 2, Lq, Lk))
                if Lk >= Lq:
                    cs.append(_case("edge", dh, 2, 2, Lq, Lk, True, Lk - Lq))
        for L in (2, 16):
            cs.append(_case("edge", dh, 3, 3, L, L, True, 0))
    for dh in (64, 96):
        for L in (17, 33, 64, 65, 97):
            cs.append(_case("edge", dh, 2, 2, L, L, True, 0))
        for Lq in (17, 47):
            for Lk in (1, 31, 32, 33, 95):
                cs.append(_case("edge", dh, 3, 3, Lq, Lk))
        for Lq in (48, 49, 97, 112, 113, 128, 129):
            cs.append(_case("edge", dh, 2, 2, Lq, 129))
        for Lk in (96, 97, 127, 128, 160, 161):
            cs.append(_case("edge", dh, 3, 3, 113, Lk))
    for Lk in (1, 31, 33, 63):
        cs.append(_case("edge", 128, 3, 3, 17, Lk))
        if Lk > 1:
            cs.append(_case("edge", 128, 3, 3, 17, Lk, True, 0))        # (keys end before the queries do: the rows past Lk see every key)
    for L in (64, 65, 80, 81, 128, 129):
        cs.append(_case("edge", 128, 2, 2, L, L, True, 0))
    for Lq, Lk, p0 in ((17, 64, 47), (40, 100, 60), (65, 161, 96), (20, 100, 10), (20, 60, 10)):
        cs.append(_case("edge", 128, 3, 3, Lq, Lk, True, p0))
    for Lq, Lk in ((70, 65), (17, 64)):
        cs.append(_case("edge", 128, 3, 3, Lq, Lk))
    cs.append(_case("edge", 128, 3, 3, 81, 65, True, 0))                   # (the staged form with the keys ending before the queries do)
    cs.append(_case("edge", 96, 3, 3, 16, 5, True, 0))                     # (and the key-split form)
    for Lq, Lk in ((1, 31), (16, 33), (17, 64)):
        cs.append(_case("edge", 512, 2, 2, Lq, Lk))
    cs.append(_case("edge", 512, 2, 2, 65, 65, True, 0))
    cs.append(_case("edge", 512, 2, 2, 16, 33, mask="alt"))
    # b. mask patterns: two key batches under four and six query batches
    n = 0
    for dh in (64, 96, 128):
        for Lq in (9, 50):
            for Lk in (33, 129):
                for mask in MASKS:
                    if mask == "interior" and Lk < 64:
                        continue
                    cs.append(_case("mask", dh, (4, 6)[n % 2], 2, Lq, Lk, mask=mask))
                    n += 1
    cs.append(_case("mask", 96, 4, 2, 50, 129, True, 79, mask="alt"))
    cs.append(_case("mask", 64, 4, 2, 50, 50, True, 0, mask="alt"))           # query 0 of the masked batch sees key 0 only, which is hidden: a zero row
    # c. layouts: one case per form and family
    for layout in LAYOUTS[1:]:
        cs.append(_case("layout", 96, 4, 2, 9, 129, mask="alt", layout=layout))            # split
        cs.append(_case("layout", 64, 3, 3, 40, 65, True, 25, layout=layout))              # per-wave
        cs.append(_case("layout", 96, 3, 3, 113, 129, layout=layout))                      # LDS
        cs.append(_case("layout", 128, 3, 3, 65, 129, True, 64, layout=layout))            # LDS1
    # e. online-softmax stress: one shape per form
    cs.append(_case("stress", 96, 3, 3, 9, 129, True, 120, probes=STRESS_PROBES))
    cs.append(_case("stress", 64, 3, 3, 40, 65, True, 25, probes=STRESS_PROBES))
    cs.append(_case("stress", 96, 3, 3, 113, 129, probes=STRESS_PROBES))
    cs.append(_case("stress", 128, 3, 3, 65, 129, True, 64, probes=STRESS_PROBES))
    cs.append(_case("stress", 512, 2, 2, 17, 65, probes=STRESS_PROBES))
    ids = [case_id(c) for c in cs]
    assert len(set(ids)) == len(ids), "case ids must be unique"
    return cs


CASES = _build_cases()


# ------------------------------------------------------------------ inputs ------------------------------------------------------------------
def _round(x, flavour):
    return x.to(OP[flavour]).float()


def _sign_vector(dh):
    return torch.tensor([1.0 if (i * 7 // 3) % 2 == 0 else -1.0 for i in range(dh)])


@functools.lru_cache(maxsize=16)
def probe_inputs(cid, shape, probe, flavour):
    """(q [B,Lq,H,dh], k, v [Bk,Lk,H,dh]) float32 holding values of the flavour's 16-bit type.  ``shape`` = (B, Bk, H, Lq, Lk, dh); ``cid`` seeds the
    hash.  The callers must not modify what they get (it is cached)."""
    B, Bk, H, Lq, Lk, dh = shape
    qs, ks = (B, Lq, H, dh), (Bk, Lk, H, dh)
    q = feats(f"ao.q.{cid}.{probe}", qs, bf16=flavour)
    k = feats(f"ao.k.{cid}.{probe}", ks, bf16=flavour)
    v = feats(f"ao.v.{cid}.{probe}", ks, bf16=flavour)
    w = _sign_vector(dh)
    if probe == "random":
        pass
    elif probe == "onehot":
        # scores of standard deviation 0.25 (unit-variance q and k give 1 at scale 1 / sqrt(dh)); column d of the output is the summed probability of the keys
        # j = d (mod dh): one key's weight is 1 / ceil(Lk / dh) of it
        q, k = _round(q * 0.5, flavour), _round(k * 0.5, flavour)         # (halving is not exact among fp16's subnormals)
        v = (torch.arange(dh)[None, :] == (torch.arange(Lk) % dh)[:, None]).float()[None, :, None, :].expand(ks).contiguous()
    elif probe in ("ramp_up", "ramp_down"):
        # score(i, j) = g_i * a_j with a_j = j (ascending: the running maximum moves in every block) or -j (descending: it never moves after the first),
        # slopes g_i of 0.25 .. 0.5 per key
        g = torch.tensor([0.25, 0.3125, 0.375, 0.5])[torch.arange(Lq) % 4]
        a = torch.arange(Lk).float() * (1.0 if probe == "ramp_up" else -1.0)
        q = _round((g / math.sqrt(dh))[None, :, None, None] * w, flavour).expand(qs).contiguous()
        k = (a[None, :, None, None] * w).expand(ks).contiguous()          # |j| < 256: exact in both types
    elif probe.startswith("spike"):
        # q = the sign vector, k random / 2 (scores of a few units at most) but for ONE key = 8 * the sign vector: its score is 8 * sqrt(dh) >= 64
        s = {"spike0": 0, "spike32": 32, "spike_last": Lk - 1}[probe]
        q = w.expand(qs).contiguous()
        k = _round(k * 0.5, flavour)
        k[:, s] = 8.0 * w
    elif probe == "flat":
        q = torch.zeros(qs)
    else:
        raise ValueError(probe)
    for t in (q, k, v):
        assert torch.equal(_round(t, flavour), t), "probe values must be exact in the operand type"
    return q, k, v


def case_shape(c):
    return (c.B, c.Bk, c.H, c.Lq, c.Lk, c.dh)


def case_inputs(c, probe, flavour):
    return probe_inputs(case_id(c), case_shape(c), probe, flavour)


def case_reference(c, probe, flavour):
    q, k, v = case_inputs(c, probe, flavour)
    return ref_attention(q, k, v, c.causal, make_mask(c.mask, c.Bk, c.Lk), c.q_pos0, c.B // c.Bk)


# ------------------------------------------------------------------ mutants of the oracle ------------------------------------------------------------------
MUTANTS = ("drop_last_live_key", "drop_first_key_of_last_block", "diagonal_plus_1", "diagonal_minus_1", "mask_byte_unhidden", "mask_byte_hidden",
           "stale_last_block", "swap_v_rows")


def mutant_attention(name, c, q, k, v):
    """The oracle with ONE fault of the kind a kernel could have, or None where the fault cannot touch this case (no diagonal without ``causal``, no mask
    byte without a mask, no previous block under 33 keys, no pair of keys under two).  "Last" means the last key any query of the batch can see."""
    kv_div = c.B // c.Bk
    pad = make_mask(c.mask, c.Bk, c.Lk)
    scale = default_scale(c.dh)
    vis = visibility(c.B, c.Lq, c.Lk, c.causal, pad, c.q_pos0, kv_div)
    seen = vis.any(1)                                                                  # [B, Lk]
    last = [int(torch.nonzero(seen[b]).max()) if bool(seen[b].any()) else -1 for b in range(c.B)]
    if name in ("drop_last_live_key", "drop_first_key_of_last_block"):
        mv = vis.clone()
        for b in range(c.B):
            if last[b] >= 0:
                mv[b, :, last[b] if name == "drop_last_live_key" else last[b] // 32 * 32] = False
        return attend(q, k, v, mv, kv_div, scale) if not torch.equal(mv, vis) else None
    if name in ("diagonal_plus_1", "diagonal_minus_1"):
        if not c.causal:
            return None
        mv = visibility(c.B, c.Lq, c.Lk, True, pad, c.q_pos0 + (1 if name == "diagonal_plus_1" else -1), kv_div)
        return attend(q, k, v, mv, kv_div, scale) if not torch.equal(mv, vis) else None
    if name in ("mask_byte_unhidden", "mask_byte_hidden"):
        if pad is None:
            return None
        want = 1 if name == "mask_byte_unhidden" else 0
        idx = torch.nonzero(pad[c.Bk - 1] == want)
        if len(idx) == 0:
            return None
        p2 = pad.clone()
        p2[c.Bk - 1, int(idx[len(idx) // 2])] = 1 - want                                # the middle one of the batch's hidden / live keys
        mv = visibility(c.B, c.Lq, c.Lk, c.causal, p2, c.q_pos0, kv_div)
        return attend(q, k, v, mv, kv_div, scale) if not torch.equal(mv, vis) else None
    top = max(last)
    if name == "stale_last_block":
        j0 = top // 32 * 32
        if j0 < 32:
            return None
        k2, v2 = k.clone(), v.clone()
        n = min(c.Lk, j0 + 32) - j0
        k2[:, j0:j0 + n], v2[:, j0:j0 + n] = k[:, j0 - 32:j0 - 32 + n], v[:, j0 - 32:j0 - 32 + n]
        return attend(q, k2, v2, vis, kv_div, scale)
    if name == "swap_v_rows":
        if top < 1:
            return None
        v2 = v.clone()
        v2[:, top - 1], v2[:, top] = v[:, top], v[:, top - 1]
        return attend(q, k, v2, vis, kv_div, scale)
    raise ValueError(name)


# ------------------------------------------------------------------ strided, fenced buffers ------------------------------------------------------------------
class Layout:
    """The four buffers of one rv_attention call and where the operands sit in them.  ``q_buf`` / ``k_buf`` / ``vt_buf``: flat tensors of the operand type
    (``k_buf is q_buf`` in the fused family), NaN wherever the kernel has no business reading; ``out_buf``: flat int16, every word NAN_FILL.  Offsets and
    strides count elements."""

    def args(self, q_ptr, k_ptr, vt_ptr, out_ptr, pad_ptr, stream):
        """The ctypes arguments of rv_attention for buffers at these BASE addresses (ints; pad_ptr may be None)."""
        p = lambda base, off: C.c_void_p(base + 2 * off)
        return (p(q_ptr, self.q_off), self.q_rs, self.q_bs, p(k_ptr, self.k_off), self.k_rs, self.k_bs, self.k_hs, p(vt_ptr, 0), self.vt_bs, self.vt_hs,
                self.vt_ds, p(out_ptr, self.o_off), self.o_rs, self.o_bs, C.c_void_p(pad_ptr) if pad_ptr else None, self.B, self.H, self.dh, self.Lq, self.Lk,
                int(self.causal), self.q_pos0, self.kv_div, C.c_float(self.scale), stream)

    def view_q(self, buf=None):
        return torch.as_strided(self.q_buf if buf is None else buf, (self.B, self.Lq, self.H, self.dh), (self.q_bs, self.q_rs, self.dh, 1), self.q_off)

    def view_k(self, buf=None):
        return torch.as_strided(self.k_buf if buf is None else buf, (self.Bk, self.Lk, self.H, self.dh), (self.k_bs, self.k_rs, self.k_hs, 1), self.k_off)

    def view_vt(self, buf=None, cols=None):
        """[Bk, H, dh, cols] of V^T (cols: Lk by default; ceil32(Lk) is what the kernel may read)."""
        return torch.as_strided(self.vt_buf if buf is None else buf, (self.Bk, self.H, self.dh, cols or self.Lk), (self.vt_bs, self.vt_hs, self.vt_ds, 1), 0)

    def view_out(self, buf):
        """[B, Lq, H * dh] of an output buffer (the words the kernel must write)."""
        return torch.as_strided(buf, (self.B, self.Lq, self.H * self.dh), (self.o_bs, self.o_rs, 1), self.o_off)

    def fence_intact(self, out_words):
        """True iff every 16-bit word of the output buffer (flat int16, after the call) outside [b, row < Lq, col < H * dh] still holds the fill."""
        live = torch.zeros(out_words.numel(), dtype=torch.bool)
        self.view_out(live).fill_(True)
        return bool((out_words.cpu()[~live] == self.fill).all())


def build_layout(family, q, k, v, flavour, causal=False, q_pos0=0, kv_div=1, scale=None):
    """q [B,Lq,H,dh], k / v [Bk,Lk,H,dh] (float, values of the flavour's type) placed into the buffers of one family:
      contig   what ops.attention builds (V^T padded to exactly ceil32(Lk)), no spare room anywhere
      fused    q and k are the first and second third of one [B, Lmax + 2, 3 * H * dh] buffer (row stride 3 * H * dh for both; key batch kb is the k third of
               query batch kb * kv_div); the last third, the k thirds of the other batches and the rows behind Lq / Lk are NaN
      cache    head-major K [Bk, H, Smax, dh] and V^T [Bk, H, dh, Smax] with Smax = ceil32(Lk) + 64: K rows >= Lk and V^T columns >= ceil32(Lk) are NaN
      window   the output is a window of a wider buffer: 8 words in front, rows of H * dh + 8, 24 words between batches
    q has NaN rows behind Lq in every family but ``contig`` (three; at least two in ``fused``); the V^T columns Lk .. ceil32(Lk) - 1 hold VT_PAD everywhere."""
    B, Lq, H, dh = q.shape
    Bk, Lk = k.shape[0], k.shape[1]
    assert B == Bk * kv_div and family in LAYOUTS
    nan, dt = float("nan"), OP[flavour]
    L = Layout()
    L.family, L.B, L.Bk, L.H, L.dh, L.Lq, L.Lk, L.causal, L.q_pos0, L.kv_div = family, B, Bk, H, dh, Lq, Lk, causal, q_pos0, kv_div
    L.scale = default_scale(dh) if scale is None else scale
    L.fill = NAN_FILL[flavour]
    E, Lp = H * dh, ceil32(Lk)
    if family == "fused":
        rows = max(Lq, Lk) + 2
        buf = torch.full((B, rows, 3, E), nan)
        buf[:, :Lq, 0] = q.reshape(B, Lq, E)
        buf[::kv_div, :Lk, 1] = k.reshape(Bk, Lk, E)
        L.q_buf = L.k_buf = buf.reshape(-1).to(dt)
        L.q_off, L.q_rs, L.q_bs = 0, 3 * E, rows * 3 * E
        L.k_off, L.k_rs, L.k_bs, L.k_hs = E, 3 * E, kv_div * rows * 3 * E, dh
    else:
        qrows = Lq if family == "contig" else Lq + 3
        buf = torch.full((B, qrows, E), nan)
        buf[:, :Lq] = q.reshape(B, Lq, E)
        L.q_buf, L.q_off, L.q_rs, L.q_bs = buf.reshape(-1).to(dt), 0, E, qrows * E
    Smax = Lp + 64 if family == "cache" else Lp
    if family == "cache":
        buf = torch.full((Bk, H, Smax, dh), nan)
        buf[:, :, :Lk] = k.permute(0, 2, 1, 3)
        L.k_buf, L.k_off, L.k_rs, L.k_bs, L.k_hs = buf.reshape(-1).to(dt), 0, dh, H * Smax * dh, Smax * dh
    elif family != "fused":
        L.k_buf, L.k_off, L.k_rs, L.k_bs, L.k_hs = k.reshape(-1).to(dt), 0, E, Lk * E, dh
    vt = torch.full((Bk, H, dh, Smax), nan)
    vt[..., :Lk] = v.permute(0, 2, 3, 1)
    vt[..., Lk:Lp] = VT_PAD
    L.vt_buf, L.vt_bs, L.vt_hs, L.vt_ds = vt.reshape(-1).to(dt), H * dh * Smax, dh * Smax, Smax
    if family == "window":
        L.o_off, L.o_rs = 8, E + 8
        L.o_bs = Lq * L.o_rs + 24
        n = 8 + B * L.o_bs
    else:
        L.o_off, L.o_rs, L.o_bs = 0, E, Lq * E
        n = B * Lq * E
    L.out_buf = torch.full((n,), L.fill, dtype=torch.int32).to(torch.int16)
    return L
