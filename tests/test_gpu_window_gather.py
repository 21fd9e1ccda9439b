"""rv_window_gather (the kernel behind ``ops.window_gather`` / ``eval.stage2.gather_windows`` / ``clip_stage_windows`` /
``WindowStager.stage_resident``: the recursion's window tensor cut from features that stay on the device) against tests/gather_oracle.py, the rule
restated with Python loops.  The oracle IS the rule: ``frame_idx`` must be equal and ``out`` must have the oracle's bits; the one exception is a NaN made
by a converting path (f32 -> 16 bits), which must be a NaN.  tests/test_gather_host_logic.py holds the oracle's indices to ``np.linspace`` and to
``stage2.cut_windows``.

Every direct call writes into buffers with 64 sentinel elements on either side of each output; the surroundings are compared bitwise.  The video holds
a sentinel from each row's duration on and in the ``ldv - d`` padding columns: a read past the duration or past a row would show in the output.  The
module runs in both builds: each library carries its own copy of the kernel and its own 16-bit type."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import gather_oracle as GO
import window_oracle as WO
from helpers import fl

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")
PAD = 64
FENCE = -776.0                       # exact in f32, fp16 and bf16
BEYOND = 12288.0                     # what the video holds past a duration and between rows (exact in all three)
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
F32 = torch.float32


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


# ------------------------------------------------------------------ running the entry ------------------------------------------------------------------
class _Guarded:
    """An output of ``n`` elements inside a sentinel-filled buffer, ``shift`` elements behind the 64-element front fence."""

    def __init__(self, n, dtype, dev, shift=0):
        self.n, self.at = n, PAD + shift
        self.sentinel = -12345 if dtype == torch.int32 else FENCE
        self.buf = torch.full((n + 2 * PAD + shift,), self.sentinel, dtype=dtype, device=dev)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + self.at * self.buf.element_size())

    def take(self, shape):
        b = self.buf.cpu()
        assert bool((b[:self.at] == self.sentinel).all()) and bool((b[self.at + self.n:] == self.sentinel).all()), "a write outside the output"
        return b[self.at:self.at + self.n].reshape(shape)


def durations(L, Ds):
    return (np.arange(L)[None, :] < np.asarray(Ds)[:, None]).astype(np.float32)


def features(M, L, d, seed, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, L, d, generator=g) * 3).to(dtype)


def fenced(video, mask):
    """The video with the sentinel from each row's duration on (mask [M, L] of 0 / 1 prefixes, or None)."""
    video = video.clone()
    if mask is not None:
        video[torch.from_numpy(mask) == 0] = BEYOND
    return video


def on_device(dev, video, pad=0, misalign=False):
    """[M, L, d] on the device as a view with a frame stride of d + pad elements, the padding columns holding the sentinel; ``misalign``: the view
    starts one element behind a 16-byte boundary."""
    M, L, d = video.shape
    ldv, off = d + pad, 1 if misalign else 0
    buf = torch.full((M * L * ldv + 8,), BEYOND, dtype=video.dtype, device=dev)
    view = buf[off:off + M * L * ldv].view(M, L, ldv)
    view[:, :, :d] = video.to(dev)
    assert (view.data_ptr() % 16 != 0) == misalign
    return view


def run(dev, video, mask, select, win, stride, F, out_dtype, pad=0, misalign=False, index=True):
    """The C entry on a CPU video [M, L, d], a numpy mask [M, L] or None and an integer select [R, keep] -> (out CPU [R, keep, F, d], frame_idx numpy
    [R, keep, F] or None), after the sentinel checks."""
    from revisionllm_amd import hip
    M, L, d = video.shape
    select = np.ascontiguousarray(select, dtype=np.int32)
    R, keep = select.shape
    v = on_device(dev, video, pad, misalign)
    m = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).to(dev) if mask is not None else None
    s = torch.from_numpy(select).to(dev)
    out = _Guarded(R * keep * F * d, out_dtype, dev, shift=1 if misalign else 0)
    idx = _Guarded(R * keep * F, torch.int32, dev) if index else None
    lib = hip.lib(None if video.dtype == F32 and out_dtype == F32 else op16())
    rc = lib.rv_window_gather(hip.ptr(v), hip.dtype_code(v), v.stride(1), hip.ptr(m), hip.ptr(s), R, R // M, L, d, win, stride, keep, F, out.ptr,
                              hip._DT[out_dtype], idx.ptr if idx else None, hip.stream())
    hip.check(rc, "rv_window_gather")
    torch.cuda.synchronize()
    return out.take((R, keep, F, d)), (idx.take((R, keep, F)).numpy() if idx else None)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same(got, ref, converting, what=""):
    """Bit equality; where a converting path made a NaN, a NaN."""
    out, idx = got
    want, want_idx = ref[0], ref[1]
    if idx is not None:
        assert np.array_equal(idx, want_idx), (what, "frame_idx", np.argwhere(idx != want_idx)[:4].tolist())
    assert out.dtype == want.dtype and out.shape == want.shape
    differ = bits(out) != bits(want)
    if converting:
        differ &= ~(torch.isnan(out) & torch.isnan(want))
    assert not bool(differ.any()), (what, "out", differ.nonzero()[:4].tolist())


def check(dev, video, mask, select, win, stride, F, dtypes=None, pad=0, misalign=False, what=""):
    """Fence, run in every dtype pair (default: all four), compare with the oracle -> the oracle's (out, idx, D) of the last pair."""
    ref = None
    for vd, od in dtypes or ((F32, op16()), (F32, F32), (op16(), op16()), (op16(), F32)):
        v = fenced(video.to(vd), mask)
        ref = GO.gather(v, mask, select, win, stride, F, od, saturate=fl() == "f16")
        same(run(dev, v, mask, select, win, stride, F, od, pad, misalign), ref, vd != od, f"{what} {vd} -> {od}")
    return ref


def some_select(R, keep, W, seed):
    """Rows of window indices: mostly valid, unsorted, with repeats and a few entries outside [0, W)."""
    rng = np.random.default_rng(seed)
    sel = rng.integers(0, max(W, 1), (R, keep))
    sel[rng.random((R, keep)) < 0.15] = -1
    sel[rng.random((R, keep)) < 0.05] = W
    return sel


# ------------------------------------------------------------------ sizes and layouts ------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("d", [1, 4, 5, 8, 770, 768])
def test_columns_strides_and_alignment(dev, d, pad):
    """d below, at and off the 16-byte pieces (768 and 770: several steps of a wave over a row, and a last partial one), a frame stride of d and d + 3,
    and the same view one element off 16-byte alignment: the vector path where it applies, one element per lane elsewhere, the same bits."""
    L, win, stride, F = 90, 20, 5, 7
    mask = durations(L, [L, 61])
    sel = some_select(2, 5, 21, d)
    for misalign in (False, True):
        ref = check(dev, features(2, L, d, d), mask, sel, win, stride, F, pad=pad, misalign=misalign, what=f"d={d} pad={pad} off={misalign}")
    assert ref[2] == [L, 61] and (ref[1][ref[1] >= 0].max() < L)


@pytest.mark.parametrize("F", [1, 2, 3, 31, 250, 251])
def test_num_frames(dev, F):
    """F = 1 (the start), 2 (start and end), and row counts that are and are not a multiple of a workgroup's 16 rows and a wave's 4."""
    L, win, stride = 700, 130, 5
    mask = durations(L, [L, 500])
    ref = check(dev, features(2, L, 8, F), mask, some_select(2, 4, 25, F), win, stride, F, dtypes=((F32, op16()), (op16(), F32)), what=f"F={F}")
    table = GO.frame_indices(L, win, stride, F)
    assert table[:, 0].tolist() == [lo for _, _, lo, _ in WO.windows(L, win, stride)]
    if F > 1:
        assert table[:, -1].tolist() == [e for _, e, _, _ in WO.windows(L, win, stride)]
    assert ref[1].shape == (2, 4, F)


def test_the_window_where_an_integer_rule_gives_other_frames(dev):
    """win = 130, stride = 1, L = D = 391, F = 31: window 0 is (0, 130); np.linspace's float64 operations give frame 116 at j = 27, s + j * 130 / 30 gives 117."""
    L, win, F = 391, 130, 31
    video = features(1, L, 8, 5)
    ref = check(dev, video, None, np.array([[0, 1, 2]]), win, 1, F, what="(0, 130, 31)")
    assert ref[1][0, 0].tolist() == np.linspace(0, 130, 31, dtype=np.int32).tolist() != GO.integer_shortcut(0, 130, 31)
    assert ref[1][0, 0, 27] == 116 and len(WO.windows(L, win, 1)) == 3


def test_the_last_frame_is_the_windows_end(dev):
    """win = 61, stride = 1, F = 8: 7 * (61 / 7) falls short of 61 in float64, so without ``y_{F-1} = e`` the last frame of window 0 would be 60."""
    L, win, F = 200, 61, 8
    ref = check(dev, features(1, L, 8, 61), None, np.array([[0, 1, 2]]), win, 1, F, dtypes=((F32, op16()),), what="last frame")
    assert math.floor((F - 1) * (win / (F - 1)) + 0.0) == win - 1 and ref[1][0, :, -1].tolist() == [61, 122, 183]


def test_durations(dev):
    """D = L, L - 1, win + 1, win (one window, its start clamped at 0), 1 and 0 (no window: zeros and -1), and no mask against a mask of ones."""
    L, win, stride, F = 120, 20, 5, 9
    Ds = [L, L - 1, win + 1, win, 1, 0]
    mask = durations(L, Ds)
    sel = np.tile(np.array([[0, 1, 3, 4, 28, 29, -1]]), (6, 1))
    video = features(6, L, 8, 3)
    ref = check(dev, video, mask, sel, win, stride, F, dtypes=((F32, op16()), (op16(), op16())), what="durations")
    assert ref[2] == Ds and [len(WO.windows(D, win, stride)) for D in Ds] == [29, 29, 5, 4, 0, 0]
    assert (ref[1][4:] == -1).all() and not bool(ref[0][4:].any()) and (ref[1][0, 4] >= 0).all() and (ref[1][1, 5] == -1).all()
    assert ref[1][3, 0].tolist() == np.linspace(0, win - 1, F, dtype=np.int32).tolist()             # D = win: window 0 is [0, win - 1], clamped
    ones = run(dev, video, durations(L, [L] * 6), sel, win, stride, F, op16())
    none = run(dev, video, None, sel, win, stride, F, op16())
    assert torch.equal(bits(ones[0]), bits(none[0])) and np.array_equal(ones[1], none[1])


def test_select_entries(dev):
    """Ascending with -1 padding (rv_window_select's form), unsorted, a window twice, an index equal to W_r, INT32_MAX and INT32_MIN."""
    L, win, stride, F = 200, 20, 5, 6
    W = len(WO.windows(L, win, stride))
    sel = np.array([[0, 3, 7, 48, -1, -1], [48, 0, 17, 5, 30, 2], [9, 9, 9, 1, 1, 9], [W, W - 1, W + 1, 0, W, 5], [I32_MAX, 1, I32_MIN, 2, I32_MAX - 1, -2]])
    ref = check(dev, features(1, L, 8, 11), durations(L, [L]), sel, win, stride, F, what="select")
    assert W == 49 and (ref[1][3, 0] == -1).all() and (ref[1][3, 1] >= 0).all() and (ref[1][4, [0, 2, 4, 5]] == -1).all()
    assert np.array_equal(ref[1][2, 0], ref[1][2, 5]) and not bool(ref[0][4, 0].any())


@pytest.mark.parametrize("R", [1, 5, 260])
def test_row_counts(dev, R):
    L, win, stride, F = 90, 10, 4, 5
    rng = np.random.default_rng(R)
    check(dev, features(R, L, 4, R), durations(L, rng.integers(0, L + 1, R)), some_select(R, 3, 44, R), win, stride, F,
          dtypes=((F32, op16()),), what=f"R={R}")


def test_three_rows_per_video_and_the_bqk_form(dev):
    """rpm = 3: a video and its mask row serve three rows of select; ``ops.window_gather`` takes them as [B, Q, keep]."""
    from revisionllm_amd import ops
    B, Q, L, d, win, stride, F = 4, 3, 150, 8, 10, 4, 6
    Ds = [150, 129, 64, 0]
    mask = durations(L, Ds)
    video = fenced(features(B, L, d, 9), mask)
    sel = some_select(B * Q, 5, 74, 3)
    ref = check(dev, video, mask, sel, win, stride, F, dtypes=((F32, op16()),), what="rpm=3")
    assert ref[2] == [150] * 3 + [129] * 3 + [64] * 3 + [0] * 3
    s = torch.from_numpy(sel.astype(np.int32)).view(B, Q, 5).to(dev)
    out, idx = ops.window_gather(video.to(dev), s, win=win, stride=stride, num_frames=F, mask=torch.from_numpy(mask).to(dev).bool(), return_index=True)
    assert out.shape == (B, Q, 5, F, d) and idx.shape == (B, Q, 5, F) and out.dtype == op16()
    same((out.cpu().view(B * Q, 5, F, d), idx.cpu().numpy().reshape(B * Q, 5, F)), ref, True, "[B, Q, keep]")
    flat = ops.window_gather(video.to(dev), s.view(B * Q, 5), win=win, stride=stride, num_frames=F, mask=torch.from_numpy(mask).to(dev))
    assert torch.equal(bits(flat.cpu()), bits(out.cpu().view(B * Q, 5, F, d)))
    one = ops.window_gather(video[0].to(dev), s[0, 0], win=win, stride=stride, num_frames=F, out_dtype=F32)          # [L, d] and [keep]
    assert one.shape == (5, F, d) and torch.equal(one.cpu(), GO.gather(video[:1], None, sel[:1], win, stride, F, F32)[0][0])
    strided = torch.full((B, L, d + 3), BEYOND, device=dev)
    strided[:, :, :d] = video.to(dev)
    view = ops.window_gather(strided[:, :, :d], s, win=win, stride=stride, num_frames=F, mask=torch.from_numpy(mask).to(dev))   # a view: read in place
    assert torch.equal(bits(view.cpu()), bits(out.cpu()))


# ------------------------------------------------------------------ dtypes ------------------------------------------------------------------
def test_f32_to_16_bits_on_ties_subnormals_zeros_infinities_and_nans(dev):
    from revisionllm_amd import hip
    L, d, win, stride, F = 40, 16, 8, 4, 9
    specials = [1 + 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
                2.0 ** -14 - 2.0 ** -25, -0.0, 0.0, float("inf"), -float("inf"), float("nan"), 65504.0, 65519.0, -65519.0, 1e-40, 7e4, -7e4, 65520.0]
    video = features(1, L, d, 21)
    flat = video.view(-1)
    flat[:len(specials) * 7:7] = torch.tensor(specials)
    big = flat.abs() >= 65520
    status = hip.numeric_status(fl(), dev)
    before = int(status[0])
    ref = GO.gather(video, None, np.arange(8)[None], win, stride, F, op16(), saturate=fl() == "f16")
    got = run(dev, video, None, np.arange(8)[None], win, stride, F, op16())
    same(got, ref, True, "specials")
    for pad, misalign in ((3, False), (0, True)):                                                  # the element path converts the same way
        same(run(dev, video, None, np.arange(8)[None], win, stride, F, op16(), pad, misalign), ref, True, "specials, element path")
    out = got[0].float()
    assert bool(torch.isnan(out).any()) and bool(big.any())
    if fl() == "f16":
        assert float(out[~torch.isnan(out)].abs().max()) == 65504.0 and not bool(torch.isinf(out).any())
        assert int(status[0]) > before, "the saturation counter did not move"
    else:
        assert bool(torch.isinf(out).any()) and bool((out == 70144.0).any())                       # bf16 stores 7e4 as it rounds, and an infinity as it is
        assert int(status[0]) == before


def test_the_same_type_is_a_copy_of_the_bits_and_16_bits_to_f32_is_exact(dev):
    """NaN payloads, subnormals and both zeros go through the three paths that do not round."""
    L, win, stride, F = 40, 8, 4, 9
    g = torch.Generator().manual_seed(4)
    raw32 = torch.randint(-2 ** 31, 2 ** 31 - 1, (1, L, 12), generator=g, dtype=torch.int64).to(torch.int32)
    raw16 = torch.randint(-2 ** 15, 2 ** 15 - 1, (1, L, 16), generator=g, dtype=torch.int64).to(torch.int16)
    sel = np.array([[0, 5, 8, -1, 3]])
    for video, od in ((raw32.view(F32), F32), (raw16.view(op16()), op16())):
        for pad in (0, 3):
            ref = GO.gather(video, None, sel, win, stride, F, od)
            same(run(dev, video, None, sel, win, stride, F, od, pad), ref, False, f"copy {od} pad={pad}")
    video = raw16.view(op16())
    quiet = torch.where(torch.isnan(video), torch.zeros_like(video), video)                           # (a signalling NaN comes back quiet: left out here)
    for pad in (0, 3):
        same(run(dev, quiet, None, sel, win, stride, F, F32, pad), GO.gather(quiet, None, sel, win, stride, F, F32), False, f"16 -> f32 pad={pad}")
    got = run(dev, video, None, sel, win, stride, F, F32)[0]
    want = GO.gather(video, None, sel, win, stride, F, F32)[0]
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~torch.isnan(got)], want[~torch.isnan(want)])


# ------------------------------------------------------------------ large cases ------------------------------------------------------------------
def test_the_drivers_size(dev):
    """L = 36000 frames of 768, 100 of the 287 windows, 250 frames each: f32 features into the operand type, as the driver stages them."""
    L, d, F = 36000, 768, 250
    video = features(1, L, d, 36)
    W = len(WO.windows(L, 625, 5))
    sel = np.sort(np.append(np.random.default_rng(36).choice(W - 1, 99, replace=False), W - 1))[None]
    ref = GO.gather(video, None, sel, 625, 5, F, op16())
    same(run(dev, video, None, sel, 625, 5, F, op16()), ref, True, "driver size")
    assert W == 287 and ref[1].max() == L - 1


def test_a_source_offset_past_4_gib(dev):
    """[1, 2^20, 1040] f32, uninitialised except for the frames of the last window: its rows start 4.36e9 bytes into the video."""
    from revisionllm_amd import ops
    L, d, win, F = 1 << 20, 1040, 1000, 7
    W = len(WO.windows(L, win, 1))
    idx = GO.frame_indices(L, win, 1, F)[W - 1]
    assert int(idx[0]) * d * 4 > 2 ** 32 and W == 1048 and int(idx[-1]) < L
    video = torch.empty(1, L, d, dtype=F32, device=dev)
    rows = features(1, F, d, 8)[0]
    video[0, torch.from_numpy(idx.astype(np.int64)).to(dev)] = rows.to(dev)
    sel = torch.tensor([W - 1, -1], dtype=torch.int32, device=dev)
    out, got_idx = ops.window_gather(video[0], sel, win=win, stride=1, num_frames=F, out_dtype=F32, return_index=True)
    assert torch.equal(out[0].cpu(), rows) and not bool(out[1].any()) and got_idx.cpu().tolist() == [idx.tolist(), [-1] * F]
    half = ops.window_gather(video[0], sel, win=win, stride=1, num_frames=F)
    assert torch.equal(bits(half[0].cpu()), bits(rows.to(op16())))


# ------------------------------------------------------------------ the public calls ------------------------------------------------------------------
def _movie(ctx_l, d, seed, a=400, b=460):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(ctx_l, d, generator=g)
    query = torch.randn(d, generator=g)
    feats[a:b] += 2.0 * query
    return feats, query


def test_select_goes_from_window_select_to_the_gather_without_a_host_copy(dev):
    from revisionllm_amd import ops
    B, Q, L, d, win, stride, F = 2, 3, 300, 16, 20, 5, 11
    g = torch.Generator().manual_seed(12)
    video, text = torch.randn(B, L, d, generator=g), torch.randn(B, Q, d, generator=g)
    mask = durations(L, [300, 140])
    v, m = fenced(video, mask).to(dev), torch.from_numpy(mask).to(dev)
    sel = ops.window_select(ops.frame_cosine_multi(text.to(dev), v), m, win=win, stride=stride, keep=40, min_sep=2)
    out, idx = ops.window_gather(v, sel.select, win=win, stride=stride, num_frames=F, mask=m, return_index=True)
    ref = GO.gather(fenced(video, mask), mask, sel.select.cpu().numpy().reshape(B * Q, 40), win, stride, F, op16())
    same((out.cpu().view(B * Q, 40, F, d), idx.cpu().numpy().reshape(B * Q, 40, F)), ref, True, "chained")
    n = sel.n_select.cpu()
    assert n.tolist() == [[40] * Q, [34] * Q] and bool((idx[1, :, 34:] == -1).all()) and bool((idx[1, :, :34] >= 0).all())


def test_gather_windows_and_clip_stage_windows_against_the_host_route(dev):
    from revisionllm_amd.eval import stage2
    geometry = dict(debug_window=20, feature_fps=5, stride=5)
    ctx_l, d, F = 1300, 16, 25
    feats, query = _movie(ctx_l, d, 2)
    _, frame_idx = stage2.cut_windows(ctx_l, num_frames=F, **geometry)
    for fdt in (F32, op16()):
        f = feats.to(fdt)
        fd = f.to(dev)
        for windows in ([3, 4, 9, 60, 63], list(range(64)), [7], [-1, 0, 5]):
            want = f[torch.from_numpy(frame_idx[windows].astype(np.int64))].to(op16())
            got = stage2.gather_windows(fd, windows, num_frames=F, dtype=op16(), **geometry)
            assert got.shape == (len(windows), F, d) and torch.equal(bits(got.cpu()), bits(want))
        row = torch.tensor([5, 6, 63, -1], dtype=torch.int32, device=dev)
        got = stage2.gather_windows(fd, row, num_frames=F, dtype=F32, **geometry)
        assert torch.equal(got[:3].cpu(), f[torch.from_numpy(frame_idx[[5, 6, 63]].astype(np.int64))].float()) and not bool(got[3].any())
        with pytest.raises(IndexError):
            stage2.gather_windows(fd, [64], num_frames=F, **geometry)
        for batch, min_sep in ((8, 1), (40, 2), (100, 1)):
            gw, windows = stage2.clip_stage_windows(fd, query.numpy(), batch=batch, num_frames=F, dtype=op16(), min_sep=min_sep, **geometry)
            assert gw == stage2.clip_grounding_windows(f, query, batch=batch, min_sep=min_sep, **geometry) and len(gw) == min(batch, 64)
            assert torch.equal(bits(windows.cpu()), bits(f[torch.from_numpy(frame_idx[gw].astype(np.int64))].to(op16())))


def test_stage_resident_hands_over_stage_windows_tensor(dev):
    """ctx_l = 9000 at the driver's geometry: f32 and 16-bit features through ``ResidentFeatures`` and ``stage_resident`` against the host gather."""
    from revisionllm_amd.data.feature_store import ResidentFeatures, WindowStager
    from revisionllm_amd.eval import stage2
    ctx_l, d = 9000, 768
    feats, _ = _movie(ctx_l, d, 6)
    _, frame_idx = stage2.cut_windows(ctx_l)
    stager = WindowStager(dev, op_dtype=fl())
    cache = ResidentFeatures(dev, 256 << 20, op_dtype=fl(), stream=stager.stream)
    windows = [0, 1, 17, 40, 69, 70]
    for name, array in (("f32", feats.numpy()), ("f16", feats.numpy().astype(np.float16))):
        resident = cache.get(name, array)
        assert resident.dtype == (torch.float16 if name == "f16" and fl() == "f16" else F32) and cache.get(name, array) is resident
        got = stager.stage_resident(resident, windows, debug_window=125, feature_fps=5, stride=5, num_frames=250).wait()
        want = stager.stage_windows(array, frame_idx[windows]).wait()
        torch.cuda.synchronize()
        assert got.dtype == want.dtype == op16() and got.shape == want.shape == (6, 250, d)
        assert torch.equal(bits(got.cpu()), bits(want.cpu()))
    assert (cache.hits, cache.misses) == (2, 2) and frame_idx.shape[0] == 71


def test_a_row_does_not_depend_on_its_batch(dev):
    L, win, stride, F = 200, 10, 4, 6
    Ds = [200, 180, 77, 130, 200]
    mask = durations(L, Ds)
    video = fenced(features(5, L, 8, 23), mask)
    sel = some_select(5, 7, 99, 2)
    whole = run(dev, video, mask, sel, win, stride, F, op16())
    for r in (0, 2, 4):
        alone = run(dev, video[r:r + 1], mask[r:r + 1], sel[r:r + 1], win, stride, F, op16())
        assert torch.equal(bits(whole[0][r:r + 1]), bits(alone[0])) and np.array_equal(whole[1][r:r + 1], alone[1])
    for n in (0, 6):                                                                                # and an entry not on its place in the row
        alone = run(dev, video[3:4], mask[3:4], sel[3:4, n:n + 1], win, stride, F, op16())
        assert torch.equal(bits(whole[0][3:4, n:n + 1]), bits(alone[0]))


def test_the_calls_do_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the calls: with the stream kept busy by work queued before them, an event recorded just before a
    call has not completed when the call returns (a call that waited for its own kernel would have waited for that work first)."""
    from revisionllm_amd import ops
    from revisionllm_amd.eval import stage2
    feats, _ = _movie(1300, 64, 77)
    fd = feats.to(dev)
    sel = torch.tensor([[0, 5, 9, -1], [3, 4, 60, 63]], dtype=torch.int32, device=dev)
    mask = torch.ones(1, 1300, device=dev)
    row = sel[1].contiguous()
    calls = (lambda: ops.window_gather(fd, sel, win=100, stride=5, num_frames=25, mask=mask[0], return_index=True),
             lambda: (stage2.gather_windows(fd, row, debug_window=20, feature_fps=5, stride=5, num_frames=25),),
             lambda: (stage2.gather_windows(fd, [3, 4, 60, 63], debug_window=20, feature_fps=5, stride=5, num_frames=25),))
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
        assert all(torch.equal(x, y) for x, y in zip(got, want))
