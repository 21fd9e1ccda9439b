"""The stage-1 driver's device route on the GPU: ``rv_window_gather_rule`` with the clipped rule (``ops.window_gather_clipped`` /
``stage1.gather_windows`` / ``WindowStager.stage_resident_clipped``) against tests/stage1_oracle.py and against the host route
``stage_windows(features, stage1.cut_windows(...))``, bit for bit, ``frame_idx`` included; ``rv_proposal_cosine`` (``ops.proposal_cosine`` /
``stage1.proposal_cosines`` / ``score_query_device``) bit for bit against ``ops.topk_cosine`` on the contiguous slice and within 1e-4 of the float64
oracle (the bound tests/test_gpu_rowops_scores_edges.py holds ``rv_topk_cosine`` to); the epilogue against ``score_query``; the driver end to end.

Every direct call writes into buffers with 64 sentinel elements on either side of each output.  The video holds a NaN from each row's duration on and
in the ``ldv - d`` padding columns, and the window tensor of the proposal cases holds NaN in every frame no slice may read: a read outside a window or a
slice would show in the output.  The module runs in both builds."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stage1_oracle as SO
from helpers import fl

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")
PAD = 64
FENCE = -776.0                       # exact in f32, fp16 and bf16
NAN = float("nan")
F32 = torch.float32
SEED = 1234


@pytest.fixture(scope="module", params=[None] if _FORCED else ["f16", "bf16"])
def flav(request, op_flavour):
    from revisionllm_amd import hip
    f = request.param or op_flavour or hip.flavour()
    prev = hip.set_flavour(f)
    yield f
    hip.set_flavour(prev)


@pytest.fixture(scope="module")
def dev(flav):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


def op16():
    return torch.float16 if fl() == "f16" else torch.bfloat16


class _Guarded:
    """An output of ``n`` elements inside a sentinel-filled buffer behind a 64-element front fence."""

    def __init__(self, n, dtype, dev):
        self.n = n
        self.sentinel = -12345 if dtype == torch.int32 else FENCE
        self.buf = torch.full((n + 2 * PAD,), self.sentinel, dtype=dtype, device=dev)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + PAD * self.buf.element_size())

    def take(self, shape):
        b = self.buf.cpu()
        assert bool((b[:PAD] == self.sentinel).all()) and bool((b[PAD + self.n:] == self.sentinel).all()), "a write outside the output"
        return b[PAD:PAD + self.n].reshape(shape)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def durations(L, Ds):
    return (np.arange(L)[None, :] < np.asarray(Ds)[:, None]).astype(np.float32)


def features(M, L, d, seed, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, L, d, generator=g) * 3).to(dtype)


def fenced(video, mask):
    """The video with NaN from each row's duration on."""
    video = video.clone()
    if mask is not None:
        video[torch.from_numpy(mask) == 0] = NAN
    return video


def on_device(dev, video, pad=0):
    """[M, L, d] on the device as a view with a frame stride of d + pad elements, the padding columns holding NaN."""
    M, L, d = video.shape
    buf = torch.full((M, L, d + pad), NAN, dtype=video.dtype, device=dev)
    buf[:, :, :d] = video.to(dev)
    return buf[:, :, :d]


# ------------------------------------------------------------------ the gather ------------------------------------------------------------------
def run_gather(dev, video, mask, select, win, F, out_dtype, keep=None, pad=0, rule=1, stride=2):
    """The C entry on a CPU video [M, L, d], a numpy mask [M, L] or None and an integer select [R, keep] or None (``keep`` entries per video) ->
    (out CPU [R, keep, F, d], frame_idx numpy [R, keep, F]), after the sentinel checks."""
    from revisionllm_amd import hip
    M, L, d = video.shape
    if select is not None:
        select = np.ascontiguousarray(select, dtype=np.int32)
        R, keep = select.shape
        s = torch.from_numpy(select).to(dev)
    else:
        R, s = M, None
    v = on_device(dev, video, pad)
    m = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).to(dev) if mask is not None else None
    out = _Guarded(R * keep * F * d, out_dtype, dev)
    idx = _Guarded(R * keep * F, torch.int32, dev)
    lib = hip.lib(None if video.dtype == F32 and out_dtype == F32 else op16())
    rc = lib.rv_window_gather_rule(hip.ptr(v), hip.dtype_code(v), v.stride(1), hip.ptr(m), hip.ptr(s), R, R // M, L, d, win, stride, keep, F, out.ptr,
                                   hip._DT[out_dtype], idx.ptr, rule, hip.stream())
    hip.check(rc, "rv_window_gather_rule")
    torch.cuda.synchronize()
    return out.take((R, keep, F, d)), idx.take((R, keep, F)).numpy()


def same(got, ref, converting, what=""):
    """Bit equality, ``frame_idx`` included; where a converting path made a NaN, a NaN."""
    out, idx = got
    want, want_idx = ref[0], ref[1]
    assert np.array_equal(idx, want_idx), (what, "frame_idx", np.argwhere(idx != want_idx)[:4].tolist())
    assert out.dtype == want.dtype and out.shape == want.shape
    differ = bits(out) != bits(want)
    if converting:
        differ &= ~(torch.isnan(out) & torch.isnan(want))
    assert not bool(differ.any()), (what, "out", differ.nonzero()[:4].tolist())
    assert not bool(torch.isnan(out.float()).any()), (what, "a frame at or past a duration, or a padding column, was read")


def check_gather(dev, video, mask, select, win, F, keep=None, dtypes=None, pad=0, what=""):
    ref = None
    for vd, od in dtypes or ((F32, op16()), (F32, F32), (op16(), op16()), (op16(), F32)):
        v = fenced(video.to(vd), mask)
        ref = SO.gather(v, mask, select, win, F, od, saturate=fl() == "f16", keep=keep)
        same(run_gather(dev, v, mask, select, win, F, od, keep, pad), ref, vd != od, f"{what} {vd} -> {od}")
    return ref


@pytest.mark.parametrize("win", [10, 11, 4, 5])
@pytest.mark.parametrize("F", [1, 2, 7, 17])
def test_clipped_windows_at_every_duration(dev, win, F):
    """Even and odd windows, F on either side of a workgroup's 16 rows; D = L, L - 1, half + 1 (one window), half (none), and at win = 5 D = 15 (a void
    last window): every window of every row through a NULL select, against the oracle; the full rows against ``stage1.cut_windows`` too."""
    from revisionllm_amd.eval import stage1
    L, d, half = 47, 8, win // 2
    Ds = [L, L - 1, half + 1, half] + ([15] if win == 5 else [])
    mask = durations(L, Ds)
    video = features(len(Ds), L, d, win * 100 + F)
    keep = SO.window_count(L, win)
    ref = check_gather(dev, video, mask, None, win, F, keep=keep, dtypes=((F32, op16()), (op16(), F32)), what=f"win={win} F={F}")
    assert ref[2] == Ds and [SO.window_count(D, win) for D in Ds[:4]] == [keep, SO.window_count(L - 1, win), 1, 0]
    assert (ref[1][2, 0] >= 0).all() and (ref[1][2, 1:] == -1).all() and (ref[1][3] == -1).all()
    for row, D in ((0, L), (1, L - 1)):                                         # (win = 5 has void windows from D = 15 on: the host's rows for them are not compared)
        host = stage1.cut_windows(D, win, 1, F)
        for i, (s, e) in enumerate(SO.windows(D, win)):
            assert (ref[1][row, i] == -1).all() if SO.void(s, e) else np.array_equal(ref[1][row, i], host[i]), (D, i)
        assert (win == 5) == any(SO.void(s, e) for s, e in SO.windows(D, win))
    if win == 5:
        W15 = SO.window_count(15, 5)
        assert W15 == 7 and SO.windows(15, 5)[-1] == (15, 14) and (ref[1][4, W15 - 1] == -1).all() and (ref[1][4, W15 - 2] >= 0).all()
        assert not bool(ref[0][4, W15 - 1].any())


@pytest.mark.parametrize("d", [8, 16, 20, 768])
def test_columns_strides_dtypes_and_select_forms(dev, d):
    """d on and off the 16-byte pieces, a view with ldv > d, all four dtype pairs; select NULL equals select = arange; a select with -1, repeats, an index
    at and past W_r."""
    L, win, F = (199, 20, 9) if d != 768 else (60, 10, 5)
    Ds = [L, L - 30]
    mask = durations(L, Ds)
    video = features(2, L, d, d)
    keep = SO.window_count(L, win)
    pairs = None if d != 768 else ((F32, op16()),)
    for pad in (0, 3):
        ref = check_gather(dev, video, mask, None, win, F, keep=keep, dtypes=pairs, pad=pad, what=f"d={d} pad={pad} NULL")
    v = fenced(video, mask)
    arange = np.tile(np.arange(keep), (2, 1))
    same(run_gather(dev, v, mask, arange, win, F, op16(), pad=3), SO.gather(v, mask, None, win, F, op16(), saturate=fl() == "f16", keep=keep), True, "arange")
    W1 = SO.window_count(Ds[1], win)
    sel = np.array([[0, -1, 3, 3, keep - 1, keep, keep + 5, 1], [W1 - 1, W1, -1, 0, 0, 2 ** 31 - 1, -2 ** 31, W1 - 2]])
    ref = check_gather(dev, video, mask, sel, win, F, dtypes=pairs, pad=3, what=f"d={d} select")
    assert (ref[1][0, [1, 5, 6]] == -1).all() and (ref[1][0, [0, 2, 3, 4, 7]] >= 0).all() and np.array_equal(ref[1][0, 2], ref[1][0, 3])
    assert (ref[1][1, [1, 2, 5, 6]] == -1).all() and (ref[1][1, [0, 3, 4, 7]] >= 0).all()
    rows = check_gather(dev, video, mask, np.tile(sel, (3, 1))[[0, 2, 4, 1, 3, 5]], win, F, dtypes=((op16(), op16()),), what="rpm = 3")   # three rows per video
    assert np.array_equal(rows[1][0], rows[1][2]) and np.array_equal(rows[1][3], ref[1][1])


def test_the_last_two_windows_differ_from_the_shifted_rule(dev):
    """``rv_window_gather`` at stride 2 shifts its last windows back to full length; the clipped rule cuts them short: the earlier ones are the same
    windows under both rules, and rule 0 of the new entry is ``rv_window_gather`` itself."""
    from revisionllm_amd import hip, ops
    L, d, win, F = 47, 16, 11, 7
    video = features(1, L, d, 5)
    keep = SO.window_count(L, win)
    arange = np.arange(keep)[None]
    clipped = run_gather(dev, video, None, None, win, F, op16(), keep=keep)
    shifted = run_gather(dev, video, None, arange, win, F, op16(), rule=0)
    shifted_null = run_gather(dev, video, None, None, win, F, op16(), keep=keep, rule=0)
    assert keep == 9 and np.array_equal(shifted[1], shifted_null[1]) and torch.equal(bits(shifted[0]), bits(shifted_null[0]))
    assert np.array_equal(clipped[1][0, :keep - 2], shifted[1][0, :keep - 2]) and torch.equal(bits(clipped[0][0, :keep - 2]), bits(shifted[0][0, :keep - 2]))
    for n in (keep - 2, keep - 1):
        assert not np.array_equal(clipped[1][0, n], shifted[1][0, n]), n
        assert clipped[1][0, n, 0] == (n * win) // 2 and clipped[1][0, n, -1] == L - 1 and shifted[1][0, n, 0] == L - 1 - win
    old = ops.window_gather(video[0].to(dev), torch.from_numpy(arange[0].astype(np.int32)).to(dev), win=win, stride=2, num_frames=F, return_index=True)
    assert torch.equal(bits(old[0].cpu()), bits(shifted[0][0])) and np.array_equal(old[1].cpu().numpy(), shifted[1][0])
    five = run_gather(dev, video, None, None, 5, F, op16(), keep=SO.window_count(L, 5))             # odd win: (i * 5) // 2, not i * 2
    assert five[1][0, :4, 0].tolist() == [0, 2, 5, 7]


def test_public_calls_against_the_host_route(dev):
    """``ops.window_gather_clipped``, ``stage1.gather_windows`` and ``stage_resident_clipped`` against ``stage_windows(features, cut_windows(...))``."""
    from revisionllm_amd import ops
    from revisionllm_amd.data.feature_store import ResidentFeatures, WindowStager
    from revisionllm_amd.eval import stage1
    ctx_l, d, F = 1303, 24, 25
    geometry = dict(debug_window=20, feature_fps=5.0, num_frames=F)
    feats = features(1, ctx_l, d, 2)[0]
    frame_idx = stage1.cut_windows(ctx_l, **geometry)
    stager = WindowStager(dev, op_dtype=fl())
    cache = ResidentFeatures(dev, 64 << 20, op_dtype=fl(), stream=stager.stream)
    for name, array in (("f32", feats.numpy()), ("f16", feats.numpy().astype(np.float16))):
        want = stager.stage_windows(array, frame_idx).wait()
        resident = cache.get(name, array)
        got = stager.stage_resident_clipped(resident, **geometry).wait()
        torch.cuda.synchronize()
        assert got.dtype == want.dtype == op16() and got.shape == want.shape == (frame_idx.shape[0], F, d) and frame_idx.shape[0] == 26
        assert torch.equal(bits(got.cpu()), bits(want.cpu())), name
        direct = stage1.gather_windows(resident, dtype=op16(), **geometry)
        assert torch.equal(bits(direct.cpu()), bits(want.cpu()))
    fd = feats.to(dev)
    out, idx = ops.window_gather_clipped(fd, win=100, num_frames=F, out_dtype=F32, return_index=True)
    assert np.array_equal(idx.cpu().numpy(), frame_idx) and torch.equal(out.cpu(), feats[torch.from_numpy(frame_idx.astype(np.int64))])
    strided = torch.full((2, ctx_l, d + 3), NAN, device=dev)
    strided[:, :, :d] = fd
    both = ops.window_gather_clipped(strided[:, :, :d], win=100, num_frames=F, out_dtype=F32, mask=torch.ones(2, ctx_l, device=dev))   # [B, L, d], a view
    assert both.shape == (2, 26, F, d) and torch.equal(both[0], out) and torch.equal(both[1], out)
    sel = torch.tensor([25, -1, 0], dtype=torch.int32, device=dev)
    some = ops.window_gather_clipped(fd, win=100, num_frames=F, out_dtype=F32, select=sel)
    assert torch.equal(some[0], out[25]) and torch.equal(some[2], out[0]) and not bool(some[1].any())
    with pytest.raises(ValueError, match="take the host route"):
        stage1.gather_windows(fd[:99], **geometry)


# ------------------------------------------------------------------ the proposal score ------------------------------------------------------------------
def window_tensor(W, T, d, seed, dtype):
    return features(W, T, d, seed).to(dtype)


def run_proposals(dev, feat, q, props, k):
    """The C entry on a CPU window tensor whose frames outside every valid slice are NaN -> out CPU [P] after the sentinel checks."""
    from revisionllm_amd import hip
    W, T, d = feat.shape
    props = np.ascontiguousarray(props, dtype=np.int32).reshape(-1, 3)
    hidden = feat.clone()
    readable = torch.zeros(W, T, dtype=torch.bool)
    for w, a, b in props:
        if not SO.is_void(int(w), int(a), int(b), W, T):
            lo, hi = SO.slice_bounds(int(a), int(b), T)
            readable[w, lo:hi] = True
    hidden[~readable] = NAN
    f, p = hidden.to(dev), torch.from_numpy(props).to(dev)
    out = _Guarded(len(props), F32, dev)
    lib = hip.lib(None if feat.dtype == F32 else feat)
    rc = lib.rv_proposal_cosine(hip.ptr(f), hip.dtype_code(f), hip.ptr(q.to(dev)), hip.ptr(p), len(props), W, T, d, k, out.ptr, hip.stream())
    hip.check(rc, "rv_proposal_cosine")
    torch.cuda.synchronize()
    return out.take((len(props),))


def check_proposals(dev, feat, q, props, k, what=""):
    """out against ``ops.topk_cosine`` on each contiguous slice bit for bit, against the float64 oracle within 1e-4, NaN where the oracle has NaN."""
    from revisionllm_amd import ops
    W, T, d = feat.shape
    got = run_proposals(dev, feat, q, props, k)
    want = SO.proposal_scores(feat, q, props, k)
    fd, qd = feat.to(dev), q.to(dev)
    for p, (w, a, b) in enumerate(np.asarray(props).reshape(-1, 3)):
        w, a, b = int(w), int(a), int(b)
        if SO.is_void(w, a, b, W, T):
            assert bits(got[p:p + 1]).item() == 0x7fc00000, (what, p, "a void proposal stores the quiet NaN")
            continue
        if np.isnan(want[p]):
            assert bool(torch.isnan(got[p])), (what, p, (w, a, b))
        else:
            print(f"{what} p={p} {(w, a, b)} k={k}: got {float(got[p])!r} oracle {want[p]!r} err {abs(float(got[p]) - want[p]):.3g}")
            assert abs(float(got[p]) - want[p]) <= 1e-4, (what, p, (w, a, b), float(got[p]), want[p])
        each = ops.topk_cosine(fd[w, a:b + 1][None].contiguous(), qd, k).cpu()
        assert bits(each).item() == bits(got[p:p + 1]).item(), (what, p, (w, a, b), float(each), float(got[p]))
    return got, want


LENGTHS = [(0, 0, 0), (1, 3, 4), (2, 9, 11), (3, 2, 5), (4, 0, 11), (0, 5, 40), (1, 11, 11), (2, 0, 2 ** 31 - 1)]      # lengths 1, 2, 3, 4, T; b >= T clamps


@pytest.mark.parametrize("d", [16, 24, 18])
@pytest.mark.parametrize("k", [0, 1, 3, 20])
def test_proposal_scores(dev, d, k):
    """d = 16 and 24 take the 16-byte form, d = 18 the generic one; slices of 1, 2, 3, 4 and T frames, ends past
    T; k = 0 (mean), 1, 3 and above every length; f32 and 16-bit features."""
    W, T = 5, 12
    q = torch.randn(d, generator=torch.Generator().manual_seed(d + k))
    for dtype in (F32, op16()):
        feat = window_tensor(W, T, d, 10 * d + k, dtype)
        got, want = check_proposals(dev, feat, q, LENGTHS, k, what=f"d={d} k={k} {dtype}")
        assert not np.isnan(want).any() and not bool(torch.isnan(got).any())


def test_ties_nans_zero_columns_and_void_proposals(dev):
    W, T, d = 5, 12, 16
    q = torch.randn(d, generator=torch.Generator().manual_seed(3))
    for dtype in (F32, op16()):
        feat = window_tensor(W, T, d, 77, dtype)
        feat[0, 2] = feat[0, 5] = feat[0, 7] = feat[0, 3]                      # four equal frames: ties go to the smaller index, the sum does not care
        feat[1, 4, 3] = NAN                                                    # a NaN feature inside one slice
        feat[2, 3:7, 5] = 0.0                                                  # a column that is zero in every frame of one slice (0 / 0 in its norm)
        props = [(0, 1, 8), (0, 2, 7), (1, 2, 6), (1, 5, 9), (2, 3, 6), (2, 2, 6), (3, 0, 11),
                 (-1, 0, 3), (5, 0, 3), (2 ** 31 - 1, 0, 3), (-2 ** 31, 0, 3), (0, -1, 3), (0, -2 ** 31, 3), (0, 12, 14), (0, 2 ** 31 - 1, 2 ** 31 - 1),
                 (0, 5, 4), (0, 5, -1), (0, 0, -2 ** 31), (4, 11, 11)]
        for k in (0, 2, 3):
            got, want = check_proposals(dev, feat, q, props, k, what=f"edges k={k} {dtype}")
            isnan = torch.isnan(got).tolist()
            assert isnan == [False, False, True, False, True, False, False] + [True] * 11 + [False], (k, dtype, isnan)


@pytest.mark.parametrize("P", [1, 300])
def test_proposal_counts_and_the_public_call(dev, P):
    from revisionllm_amd import ops
    W, T, d = 5, 12, 16
    rng = np.random.default_rng(P)
    a = rng.integers(0, T, P)
    props = np.stack([rng.integers(0, W, P), a, a + rng.integers(0, T, P)], 1)
    if P > 1:
        props[rng.random(P) < 0.1, 0] = W                                      # void proposals among valid ones
        props[0], props[-1] = (0, 0, 0), (W - 1, T - 1, T - 1)                  # every frame of the tensor's two ends is some slice's only frame
    q = torch.randn(d, generator=torch.Generator().manual_seed(P))
    feat = window_tensor(W, T, d, P, op16())
    got, _ = check_proposals(dev, feat, q, props, 3, what=f"P={P}")
    fd, qd = feat.to(dev), q.to(dev)
    as_list = ops.proposal_cosine(fd, qd, [tuple(int(v) for v in row) for row in props], k=3)
    pt = torch.from_numpy(props.astype(np.int32)).to(dev)
    as_tensor = ops.proposal_cosine(fd, qd, pt, k=3)
    assert as_list.shape == (P,) and torch.equal(bits(as_list.cpu()), bits(as_tensor.cpu()))
    valid = ~torch.isnan(got)
    assert torch.equal(as_list.cpu()[valid], got[valid]) and torch.equal(torch.isnan(as_list.cpu()), torch.isnan(got))
    if P > 1:
        whole = torch.empty(W + 1, T, d, dtype=feat.dtype, device=dev)[1:]      # a view that is contiguous but starts inside a buffer
        whole.copy_(fd)
        assert torch.equal(bits(ops.proposal_cosine(whole, qd, pt, k=3).cpu()), bits(as_list.cpu()))


def test_the_form_switch_at_768_columns(dev):
    """d = 768 in 16 bits, W = 1: T = 7936 is the last window length with the 16-byte form, T = 7937 runs the generic form.  Each against the float64
    oracle; bit equality with ``rv_topk_cosine`` on a slice whose own call takes the same form: any slice at 7936, the whole window at 7937 (a
    shorter slice's own call would take the 16-byte form there: the same definition, another order of the sums)."""
    d = 768
    q = torch.randn(d, generator=torch.Generator().manual_seed(8))
    for T, props in ((7936, [(0, 0, 7935), (0, 100, 139), (0, 7930, 9000)]), (7937, [(0, 0, 7936)])):
        feat = window_tensor(1, T, d, T, op16())
        check_proposals(dev, feat, q, props, 3, what=f"T={T}")
    feat = window_tensor(1, 7937, d, 7937, op16())
    got = run_proposals(dev, feat, q, [(0, 100, 139), (0, 0, 7936)], 3)         # a short slice under the generic form: the oracle's bound
    want = SO.proposal_scores(feat, q, [(0, 100, 139), (0, 0, 7936)], 3)
    print("T=7937 generic form, slice of 40:", float(got[0]), want[0], abs(float(got[0]) - want[0]))
    assert abs(float(got[0]) - want[0]) <= 1e-4 and abs(float(got[1]) - want[1]) <= 1e-4


# ------------------------------------------------------------------ the epilogue ------------------------------------------------------------------
def test_score_query_device_equals_score_query(dev):
    from revisionllm_amd.eval import stage1
    W, T, d = 7, 24, 32
    q = torch.randn(d, generator=torch.Generator().manual_seed(4)).to(dev)
    answers = ["From 3 to 9.", "Not Present", "From 5 to 5.", "From 23 to 23.", "Between 2 and 30", "From 0 to 23.", "From 22 to 22."]
    ent = [0.5, 0.7, 0.2, 0.9, 0.4, 0.6, 0.8]
    for dtype in (F32, op16()):
        feats = window_tensor(W, T, d, 9, dtype).to(dev)
        for topk_pool in (True, False):
            for score, merge in (("mean_entropy", "multiply"), ("max_entropy", "add"), ("cosine_sim", "multiply")):
                for normalize in (True, False):
                    for plus in (False, True):
                        kw = dict(num_frames=T, debug_window=125, score=score, score_merge=merge, normalize=normalize, topk_pool=topk_pool, plus_baseline=plus)
                        e = [] if score == "cosine_sim" else ent
                        want = stage1.score_query(feats, answers, e, q, (10.0, 30.0), 300.0, **kw)
                        got = stage1.score_query_device(feats, answers, e, q, (10.0, 30.0), 300.0, **kw)
                        assert got == want, (dtype, kw, got, want)
                        assert len(got[1]["scores"]) == (4 if plus else 5) and len(got[1]["iou"]) == 5
    frames = stage1.iou(answers, (0.1, 0.2), T, 57, [])[0]
    assert frames == {0: (3, 9), 2: (4, 6), 4: (2, 30), 5: (0, 23), 6: (21, 23)}
    with pytest.raises(Exception, match="rv_topk_cosine") as host:
        stage1.score_query(feats, ["From 30 to 40."], [], q, (10.0, 30.0), 300.0, num_frames=T)      # an empty slice: the host route's refusal
    with pytest.raises(type(host.value), match="rv_topk_cosine"):
        stage1.score_query_device(feats, ["From 30 to 40."], [], q, (10.0, 30.0), 300.0, num_frames=T)


def test_the_calls_do_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the two ``ops`` calls: with the stream kept busy by work queued before them, an event recorded just
    before a call has not completed when the call returns."""
    from revisionllm_amd import ops
    feats = features(1, 1300, 64, 77)[0].to(dev)
    windows = ops.window_gather_clipped(feats, win=100, num_frames=25)
    q = torch.randn(64, device=dev)
    props = torch.tensor([[0, 3, 9], [5, 0, 24], [24, 7, 7], [30, 0, 3]], dtype=torch.int32, device=dev)
    mask = torch.ones(1300, device=dev)
    calls = (lambda: ops.window_gather_clipped(feats, win=100, num_frames=25, mask=mask, return_index=True),
             lambda: (ops.proposal_cosine(windows, q, props, k=3),),
             lambda: (ops.proposal_cosine(windows, q, [(0, 3, 9), (5, 0, 24), (24, 7, 7), (30, 0, 3)], k=0),))
    for which, call in enumerate(calls):
        want = call()                                                                          # (warm: library loaded, allocator blocks cached)
        a = torch.ones(8192, 8192, device=dev)
        c = torch.empty_like(a)
        torch.mm(a, a, out=c)
        torch.cuda.synchronize()
        for _ in range(12):                                                                    # ~1.1 TFLOP of f32 each: tens of milliseconds of queued work
            torch.mm(a, a, out=c)
        ev = torch.cuda.Event()
        ev.record()
        got = call()
        still_busy = not ev.query()
        torch.cuda.synchronize()
        assert still_busy, f"call {which} returned only after the work queued before it had finished: it synchronised"
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(got, want))


# ------------------------------------------------------------------ the driver ------------------------------------------------------------------
def test_the_driver_writes_the_same_records_with_device_features(dev, tmp_path, monkeypatch):
    """``eval_nlq_negative.eval`` on a tiny dense model: ``--device_features`` writes the records of the run without it, in the reference's loop and with
    ``--in_flight 3``, and the movie is uploaded once for its four queries."""
    from revisionllm_amd.data import feature_store
    from revisionllm_amd.eval import eval_nlq_negative as drv
    from revisionllm_amd.model import ReVisionLlamaForCausalLM
    from revisionllm_amd.utils import synth
    rs = np.random.RandomState(7)
    feat_dir, q_dir = tmp_path / "feats", tmp_path / "qfeats"
    os.makedirs(feat_dir), os.makedirs(q_dir)
    np.save(feat_dir / "movieA.npy", rs.randn(2500, 768).astype(np.float16))        # 8 half-overlapping windows of 625 frames, the last two clipped
    ann = {}
    for i in range(4):
        ann[f"q{i}"] = {"movie": "movieA", "sentence": f"A man opens door {i}.", "timestamps": [40.0 * i, 40.0 * i + 12], "movie_duration": 500.0}
        np.savez_compressed(q_dir / f"q{i}.npz", token_features=rs.randn(5 + i, 768).astype(np.float32), cls_features=rs.randn(768).astype(np.float32))
    with open(tmp_path / "ann.json", "w") as f:
        json.dump(ann, f)
    shape = synth.TINY
    tok = synth.FakeTokenizer(vocab=shape.vocab)
    dense = ReVisionLlamaForCausalLM(shape, device="cuda:0")
    dense.get_model().initialize_vision_modules(SimpleNamespace(clip_adapter=False, cross_attn=False, pretrain_clip_adapter=None, pretrain_mm_mlp_adapter=None,
                                                                clip_adapter_text=False, clip_adapter_feature="temporal", hierarchy=False, adapter_input_dim=768))
    dense.engine.init_synthetic(seed=SEED, llm=True, clip=False, linear=True)
    dense.generation_config.eos_token_id = 2
    real = dense.generate_steps
    dense.generate_steps = lambda *a, **kw: real(*a, **{**kw, "max_new_tokens": 6})
    dense.generate = lambda *a, **kw: __import__("revisionllm_amd.sched", fromlist=["drive"]).drive(dense.generate_steps(*a, **kw))
    dense.uniform_fn = lambda step, B: torch.full((B,), 0.37 + 0.05 * (step % 3))   # a fixed uniform per (step, row): every run draws the same numbers
    uploads, staged = [], []
    real_upload = feature_store.ResidentFeatures._upload
    real_clipped = feature_store.WindowStager.stage_resident_clipped
    monkeypatch.setattr(feature_store.ResidentFeatures, "_upload", lambda self, array: (uploads.append(array.shape), real_upload(self, array))[1])
    monkeypatch.setattr(feature_store.WindowStager, "stage_resident_clipped",
                        lambda self, features_dev, **kw: (staged.append(tuple(features_dev.shape)), real_clipped(self, features_dev, **kw))[1])
    base = ["--data_path", str(tmp_path / "ann.json"), "--feat_folder", str(feat_dir), "--q_feat_dir", str(q_dir), "--batch", "4",
            "--vis_feat_storage", "npy", "--num_frames", "24", "--debug", "True"]
    for mode, flags in (("seq", []), ("flight", ["--in_flight", "3", "--pool_rows", "16", "--max_new_tokens", "6"])):
        records = {}
        for on in (False, True):
            del uploads[:], staged[:]
            args = drv.parse_args(base + flags + ["--log_path", str(tmp_path / f"{mode}{on}")] + (["--device_features"] if on else []))
            assert drv.eval(args, tokenizer=tok, model=dense) == (4, [])
            records[on] = [json.loads(line) for line in open(tmp_path / f"{mode}{on}" / "predictions_streaming_0.txt")]
            assert uploads == ([(2500, 768)] if on else []) and staged == ([(2500, 768)] * 4 if on else [])
        assert records[True] == records[False], mode
        assert [r["query_id"] for r in records[True]] == ["q0", "q1", "q2", "q3"] and all(len(r["answer"]) == 8 for r in records[True])
