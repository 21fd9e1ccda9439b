"""Separately allocated frames in one front-end launch (rv_frames_to_patches_scattered, rv_yuv_surfaces_to_patches, rv_packed_surfaces_to_patches) and the
layers above them (the list forms of ops.frames_to_patches / yuv_to_patches / yuv_surface_to_patches / packed_to_patches, ClipTowers.encode_* on lists,
ClipFeatureExtractor's ``scattered=True``).

The yardstick throughout is the CONTIGUOUS entry on a stacked copy of the same frames, compared by BITS (torch.equal on the raw words; no tolerance): the
header defines the values as that entry's, and the TAB = 1 instances keep its text behind the base pointer.  The scattered frames are slices at permuted,
non-uniform offsets of one large byte buffer filled with 0xFF, every frame with its own random content: a frame taken from the wrong slot, or a byte read
from outside a surface, changes the result.  Every list call is also replayed through the raw C entry into NaN-filled outputs with ldp > Kp and guards
around them: the same bits, pad columns +0, everything else still NaN.  One case (P010, PQ) is held against the float64 oracle of the definition as well, so
that bit equality with a sibling is not the only link to it."""
import os

import numpy as np
import pytest
import torch

import hdr_oracle as ho
from helpers import SEED
from test_gpu_orient_frontend import NAN_BITS, SPELL, bits, lib_error, same_bits
from test_scattered_host_logic import PACKED, RGB, YUV, call_packed, call_rgb, call_yuv

pytestmark = pytest.mark.gpu

R, PATCH, K, KP = 28, 14, 588, 640
N = 3
WANT = ("patches", "image")
_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")


@pytest.fixture(scope="module", params=[None] if _FORCED else ["f16", "bf16"])
def flav(request, op_flavour):
    """Both operand flavours, as the sibling front-end tests run them (REVISION_TEST_FLAVOURS narrows it)."""
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import hip
    f = request.param or op_flavour or hip.flavour()
    prev = hip.set_flavour(f)
    yield f
    hip.set_flavour(prev)


class Tap:
    """A library handle that records the name and the arguments of every call and passes it on."""

    def __init__(self, lib, calls):
        self.lib, self.calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*a):
            self.calls.append((name, a))
            return fn(*a)
        return call


@pytest.fixture
def tap(monkeypatch):
    from revisionllm_amd import hip
    calls, real = [], hip.lib
    monkeypatch.setattr(hip, "lib", lambda f=None: Tap(real(f), calls))
    return calls


# ---- scattered surfaces ----
def scatter(arrs, pad=0, dtype=torch.uint8, seed=0):
    """uint8 arrays [rows, row bytes] (one per surface, all of one shape) -> device views [rows, row elements] of ``dtype``, cut at permuted, non-uniform
    offsets (multiples of the element size only) out of ONE byte buffer filled with 0xFF; rows lie ``pad`` bytes further apart than they are long."""
    es = torch.empty(0, dtype=dtype).element_size()
    rows, rb = arrs[0].shape
    pitch = rb + pad
    assert all(a.dtype == np.uint8 and a.shape == (rows, rb) for a in arrs) and rb % es == 0 and pad % es == 0
    order = np.random.RandomState(SEED + seed).permutation(len(arrs))
    at, offs = 5 * es, {}
    for k, i in enumerate(order):
        offs[int(i)] = at
        at += rows * pitch + (3 + (k * 37) % 23) * es
    buf = np.full(at + 64, 0xFF, np.uint8)
    for i, a in enumerate(arrs):
        buf[offs[i]:offs[i] + rows * pitch].reshape(rows, pitch)[:, :rb] = a
    d = torch.from_numpy(buf).cuda()
    views = [d.as_strided((rows, rb), (pitch, 1), offs[i]) for i in range(len(arrs))]
    return [v if es == 1 else v.view(dtype) for v in views]


def stack_copy(arrs, dtype=torch.uint8, repeat=None):
    """The same surfaces as ONE contiguous device tensor [n, rows, row elements] (built on the host: the stacked copy a caller makes today)."""
    arrs = list(arrs)
    if repeat is not None:
        arrs[repeat[1]] = arrs[repeat[0]]
    t = torch.from_numpy(np.stack(arrs))
    return (t if dtype == torch.uint8 else t.view(dtype)).cuda()


def noise(seed, *shape, hi=256, dtype=np.uint8):
    return np.random.RandomState(SEED + seed).randint(0, hi, shape).astype(dtype)


def as_bytes(a):
    """[rows, samples] of uint8 / uint16 / uint32 -> uint8 [rows, row bytes]."""
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)


# ---- running a list form: through ops, then replayed into guarded NaN outputs; and the stacked tensor form ----
def replay_into_nan(flav, name, args, n, got, Rr=R, patch=PATCH):
    """The recorded C call once more, into NaN-filled buffers with ldp > Kp and guards: the bits ops returned, pad columns +0, nothing else written."""
    from revisionllm_amd import hip
    dt = hip.op_dtype(flav)
    k, kp = 3 * patch * patch, (3 * patch * patch + 127) // 128 * 128
    ldp, guard, rows = kp + 24, 1024, n * (Rr // patch) ** 2
    pbuf = torch.full((guard + rows * ldp + guard,), NAN_BITS, dtype=torch.int16, device="cuda").view(dt)
    ibuf = torch.full((guard + n * 3 * Rr * Rr + guard,), float("nan"), device="cuda")
    a = list(args)
    a[-4], a[-3], a[-2] = pbuf.data_ptr() + 2 * guard, ldp, ibuf.data_ptr() + 4 * guard
    rc = getattr(hip.lib(flav).lib, name)(*a)
    torch.cuda.synchronize()
    assert rc == 0, hip.last_error()
    prow = pbuf[guard:guard + rows * ldp].view(rows, ldp)
    assert torch.equal(bits(prow[:, :kp]), bits(got[0])) and torch.equal(bits(ibuf[guard:-guard].view(n, 3, Rr, Rr)), bits(got[1]))
    assert bool((bits(prow[:, k:kp]) == 0).all()) and bool((bits(prow[:, kp:]) == NAN_BITS).all())
    assert bool((bits(pbuf[:guard]) == NAN_BITS).all()) and bool((bits(pbuf[-guard:]) == NAN_BITS).all())
    assert bool(torch.isnan(ibuf[:guard]).all()) and bool(torch.isnan(ibuf[-guard:]).all())


def check_list_form(flav, tap, entry, contiguous, fn, list_args, stacked_args, n, Rr=R, patch=PATCH, **kw):
    """fn(*list_args) reaches ``entry`` once, fn(*stacked_args) one of ``contiguous``; both outputs, bit for bit; the replay into NaN."""
    from revisionllm_amd import hip
    kw = dict(kw, op_dtype=hip.op_dtype(flav), want=WANT)
    del tap[:]
    got = fn(*list_args, **kw)
    assert [c[0] for c in tap] == [entry], [c[0] for c in tap]
    name, args = tap[0]
    want = fn(*stacked_args, **kw)
    assert tap[1][0] in contiguous and len(tap) == 2, [c[0] for c in tap]
    assert tuple(got[0].shape) == (n * (Rr // patch) ** 2, (3 * patch * patch + 127) // 128 * 128) and tuple(got[1].shape) == (n, 3, Rr, Rr)
    assert bool(torch.isfinite(got[1]).all())
    assert same_bits(got, want), (entry, kw)
    replay_into_nan(flav, name, args, n, got, Rr, patch)
    return got


# ---- RGB ----
def rgb_case(layout, n, H, W, seed=0, pad=7, repeat=None):
    """-> (list of per-frame views, the stacked tensor, keywords).  layout: "NCHW" | "NHWC" | a pix_fmt of packed RGB."""
    pix = {"NCHW": 1, "NHWC": 3, "bgr24": 3, "bgra": 4}[layout]
    rows = 3 * H if layout == "NCHW" else H
    arrs = [noise(100 * seed + f, rows, W * pix) for f in range(n)]
    views = scatter(arrs, pad=pad, seed=seed)
    views = [v.unflatten(0, (3, H)) if layout == "NCHW" else v.unflatten(1, (W, pix)) for v in views]
    if repeat is not None:
        views[repeat[1]] = views[repeat[0]]
    kw = dict(pix_fmt=layout) if layout in ("bgr24", "bgra") else dict(layout=layout)
    st = stack_copy(arrs, repeat=repeat)
    return views, st.unflatten(1, (3, H)) if layout == "NCHW" else st.unflatten(2, (W, pix)), kw


def frames_fn(frames, **kw):
    from revisionllm_amd import ops
    return ops.frames_to_patches(frames, kw.pop("R", R), kw.pop("patch", PATCH), **kw)


RGB_CONTIGUOUS = ("rv_frames_to_patches", "rv_frames_to_patches_oriented", "rv_frames_to_patches_packed")
RGB_CASES = [(lay, g) for lay in ("NCHW", "NHWC") for g in ((36, 64), (64, 36), (20, 30), (37, 63))] + [(lay, g) for lay in ("bgr24", "bgra") for g in ((36, 64), (37, 63))]


@pytest.mark.parametrize("layout,geom", RGB_CASES, ids=["%s-%dx%d" % (c[0], *c[1]) for c in RGB_CASES])
def test_rgb_frames_are_the_contiguous_entry_on_a_stacked_copy(flav, tap, layout, geom):
    views, stacked, kw = rgb_case(layout, N, *geom)
    assert len({v.data_ptr() for v in views}) == N and not views[0].is_contiguous()
    check_list_form(flav, tap, RGB, RGB_CONTIGUOUS, frames_fn, (views,), (stacked,), N, **kw)


# ---- planar / semi-planar YCbCr ----
#: name -> (torch dtype, depth, value in the high bits, subsampling, chroma layout); written from the formats' definitions
FMTS = {"nv12": (torch.uint8, 8, False, "420", "cbcr"), "nv21": (torch.uint8, 8, False, "420", "crcb"), "i420": (torch.uint8, 8, False, "420", "planar"),
        "nv16": (torch.uint8, 8, False, "422", "cbcr"), "p010le": (torch.uint16, 10, True, "420", "cbcr"), "yuv444p10le": (torch.uint16, 10, False, "444", "planar")}
SUBS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}


def samples(seed, rows, cols, depth, msb):
    """Random samples as the stored bytes: uint8, or uint16 words with the value in the low or the high bits."""
    if depth == 8:
        return noise(seed, rows, cols)
    v = noise(seed, rows, cols, hi=1 << depth, dtype=np.uint16)
    return as_bytes(v << (16 - depth) if msb else v)


def yuv_case(name, n, H, W, seed=0, pad=0, repeat=None, values=None):
    """-> ((y, cb, cr) lists of per-frame views, (y, cb, cr) stacked, surface keywords).  Interleaved chroma lies in one slice per frame, planar Cb and Cr in
    slices of two further buffers, so that Cr - Cb differs from frame to frame.  values: per-frame (y, cb, cr) sample arrays in the place of noise."""
    dt, depth, msb, sub, lay = FMTS[name]
    sx, sy = SUBS[sub]
    h, w = H // sy, W // sx
    es = 1 if dt == torch.uint8 else 2

    def plane(f, which, rows, cols):
        if values is not None:
            v = values[f][which].astype(np.uint16 if es == 2 else np.uint8)
            return as_bytes(v << (16 - depth) if msb else v)
        return samples(1000 * seed + 10 * f + which, rows, cols, depth, msb)

    ya = [plane(f, 0, H, W) for f in range(n)]
    ys = scatter(ya, pad=pad * es, dtype=dt, seed=seed)
    if lay == "planar":
        ba, ra = [plane(f, 1, h, w) for f in range(n)], [plane(f, 2, h, w) for f in range(n)]
        cbs = scatter(ba, pad=pad * es, dtype=dt, seed=seed + 1)
        crs = scatter(ra, pad=pad * es, dtype=dt, seed=seed + 2)
        assert len({r.data_ptr() - b.data_ptr() for b, r in zip(cbs, crs)}) > 1 or n == 1      # Cr - Cb is no constant of the batch
        st = (stack_copy(ya, dt, repeat), stack_copy(ba, dt, repeat), stack_copy(ra, dt, repeat))
    else:
        first, second = (1, 2) if lay == "cbcr" else (2, 1)
        pairs = [np.stack((plane(f, first, h, w).reshape(h, w, es), plane(f, second, h, w).reshape(h, w, es)), 2).reshape(h, 2 * w * es) for f in range(n)]
        pv = [v.unflatten(1, (w, 2)) for v in scatter(pairs, pad=2 * pad * es, dtype=dt, seed=seed + 1)]
        sp = stack_copy(pairs, dt, repeat).unflatten(2, (w, 2))
        if lay == "cbcr":
            cbs, crs, st = pv, None, (stack_copy(ya, dt, repeat), sp, None)
        else:                                                                                # VU pairs: two views one sample apart, as split_yuv hands them over
            cbs, crs, st = [v[..., 1] for v in pv], [v[..., 0] for v in pv], (stack_copy(ya, dt, repeat), sp[..., 1], sp[..., 0])
    lists = [ys, cbs, crs]
    if repeat is not None:
        for l in lists:
            if l is not None:
                l[repeat[1]] = l[repeat[0]]
    return tuple(lists), st, dict(depth=depth, msb_aligned=msb, subsampling=sub)


def surface_fn(y, cb, cr, **kw):
    from revisionllm_amd import ops
    return ops.yuv_surface_to_patches(y, cb, cr, R=kw.pop("R", R), patch=kw.pop("patch", PATCH), **kw)


YUV_CONTIGUOUS = ("rv_yuv_to_patches", "rv_yuv_surface_to_patches", "rv_yuv_surface_to_patches_hdr", "rv_yuv_surface_to_patches_oriented")
HDR = dict(matrix="bt2020", chroma_loc="topleft")
#            format         pad  extra keywords            geometries
YUV_CASES = [("nv12", 0, {}, ((36, 64), (64, 36), (20, 30))),
             ("nv21", 5, dict(matrix="bt709", chroma_loc="centre"), ((36, 64), (20, 30))),        # rows on a padded pitch
             ("i420", 0, dict(full_range=True), ((36, 64), (64, 36), (20, 30))),
             ("p010le", 3, dict(HDR, transfer="pq"), ((36, 64), (20, 30))),
             ("p010le", 0, dict(HDR, transfer="hlg"), ((64, 36), (20, 30))),
             ("yuv444p10le", 1, {}, ((37, 63), (20, 30))),
             ("nv16", 0, {}, ((36, 64), (64, 36), (20, 30)))]
YUV_PARAMS = [(n, p, k, g) for n, p, k, gs in YUV_CASES for g in gs]


@pytest.mark.parametrize("name,pad,more,geom", YUV_PARAMS, ids=["%s%s-%dx%d" % (c[0], "-" + c[2]["transfer"] if "transfer" in c[2] else "", *c[3]) for c in YUV_PARAMS])
def test_surfaces_are_the_contiguous_entry_on_stacked_planes(flav, tap, name, pad, more, geom):
    lists, stacked, kw = yuv_case(name, N, *geom, pad=pad)
    check_list_form(flav, tap, YUV, YUV_CONTIGUOUS, surface_fn, lists, stacked, N, **kw, **more)


def test_the_8_bit_420_wrapper_takes_lists_too(flav, tap):
    from revisionllm_amd import ops

    def fn(y, cb, cr, **kw):
        return ops.yuv_to_patches(y, cb, cr, R=R, patch=PATCH, **kw)
    for name in ("nv12", "i420", "nv21"):
        lists, stacked, _ = yuv_case(name, N, 36, 64, seed=3)
        check_list_form(flav, tap, YUV, YUV_CONTIGUOUS, fn, lists, stacked, N, matrix="bt709")


# ---- packed YCbCr ----
#: name -> (bytes per pixel, torch dtype of a word); the bytes are random: every word is a legal unit of these formats
PACKED_FMTS = {"yuyv422": (2, torch.uint8), "y210le": (4, torch.uint16), "xv30le": (4, torch.int32), "vuya": (4, torch.uint8)}


def packed_case(name, n, H, W, seed=0, pad=3, repeat=None):
    bpp, word = PACKED_FMTS[name]
    es = torch.empty(0, dtype=word).element_size()
    arrs = [noise(500 * seed + f, H, W * bpp) for f in range(n)]
    views = scatter(arrs, pad=pad * es, dtype=word, seed=seed)
    views = [v.view(torch.uint8) if es > 1 else v for v in views]                            # word-aligned slices, handed over as bytes
    assert all(v.data_ptr() % es == 0 for v in views)
    if repeat is not None:
        views[repeat[1]] = views[repeat[0]]
    return views, stack_copy(arrs, repeat=repeat), dict(H=H, W=W, pix_fmt=name)


def packed_fn(buf, **kw):
    from revisionllm_amd import ops
    return ops.packed_to_patches(buf, R=kw.pop("R", R), patch=kw.pop("patch", PATCH), **kw)


PACKED_PARAMS = [("yuyv422", (36, 64)), ("yuyv422", (20, 30)), ("y210le", (36, 64)), ("y210le", (64, 36)), ("xv30le", (37, 63)), ("xv30le", (20, 30)), ("vuya", (37, 63)),
                 ("vuya", (64, 36))]


@pytest.mark.parametrize("name,geom", PACKED_PARAMS, ids=["%s-%dx%d" % (c[0], *c[1]) for c in PACKED_PARAMS])
def test_packed_surfaces_are_the_contiguous_entry_on_a_stacked_copy(flav, tap, name, geom):
    views, stacked, kw = packed_case(name, N, *geom)
    check_list_form(flav, tap, PACKED, ("rv_packed_to_patches",), packed_fn, (views,), (stacked,), N, **kw)
    if name == "y210le":
        check_list_form(flav, tap, PACKED, ("rv_packed_to_patches",), packed_fn, (views,), (stacked,), N, **kw, **HDR, transfer="pq")


# ---- orientations: the three orientation classes (none; mirrors: 2, 6; transpose: 3, 5) of one case per family ----
@pytest.mark.parametrize("code", [0, 2, 3, 5, 6])
def test_orientations(flav, tap, code):
    views, stacked, kw = rgb_case("NHWC", N, 37, 63, seed=1)
    a = check_list_form(flav, tap, RGB, RGB_CONTIGUOUS, frames_fn, (views,), (stacked,), N, **kw, **SPELL[code])
    lists, stacked, kw = yuv_case("nv12", N, 36, 64, seed=1)
    b = check_list_form(flav, tap, YUV, YUV_CONTIGUOUS, surface_fn, lists, stacked, N, **kw, **SPELL[code])
    views, stacked, kw = packed_case("yuyv422", N, 36, 64, seed=1)
    c = check_list_form(flav, tap, PACKED, ("rv_packed_to_patches",), packed_fn, (views,), (stacked,), N, **kw, **SPELL[code])
    assert tap[0][1][3] == {0: 0, 2: 2, 3: 3, 5: 5, 6: 6}[code]                             # the code reached the entry
    del a, b, c


# ---- batch sizes: one frame; a frame listed twice; across the launch boundary; 1080p ----
def test_one_frame_and_a_frame_listed_twice(flav, tap):
    for n, repeat in ((1, None), (3, (0, 2))):
        views, stacked, kw = rgb_case("NCHW", n, 36, 64, seed=2, repeat=repeat)
        got = check_list_form(flav, tap, RGB, RGB_CONTIGUOUS, frames_fn, (views,), (stacked,), n, **kw)
        lists, stacked, kw = yuv_case("i420", n, 36, 64, seed=2, repeat=repeat)
        goty = check_list_form(flav, tap, YUV, YUV_CONTIGUOUS, surface_fn, lists, stacked, n, **kw)
        views, stacked, kw = packed_case("y210le", n, 36, 64, seed=2, repeat=repeat)
        gotp = check_list_form(flav, tap, PACKED, ("rv_packed_to_patches",), packed_fn, (views,), (stacked,), n, **kw)
        if repeat:
            for g in (got, goty, gotp):
                assert torch.equal(bits(g[1][0]), bits(g[1][2])) and not torch.equal(bits(g[1][0]), bits(g[1][1]))


def test_across_the_launch_boundary(flav, tap):
    """RV_FRAME_TABLE_MAX + 1 frames are two launches: the table and the output pointers move on.  The frames on both sides of the boundary and the last one
    are where they always were, and they are the right frames (every frame has its own content)."""
    from revisionllm_amd import hip
    n = hip.FRAME_TABLE_MAX + 1
    edge = hip.FRAME_TABLE_MAX
    for case, entry, contiguous, fn in ((rgb_case("NCHW", n, 36, 64, seed=4), RGB, RGB_CONTIGUOUS, frames_fn),
                                        (yuv_case("nv12", n, 36, 64, seed=4), YUV, YUV_CONTIGUOUS, surface_fn),
                                        (packed_case("yuyv422", n, 36, 64, seed=4), PACKED, ("rv_packed_to_patches",), packed_fn)):
        lists, stacked, kw = case
        multi = entry == YUV
        got = check_list_form(flav, tap, entry, contiguous, fn, lists if multi else (lists,), stacked if multi else (stacked,), n, **kw)
        for f in (0, edge - 1, edge, n - 1):                                             # both sides of the boundary; the last frame is the one behind it
            one = fn(*([None if l is None else l[f:f + 1] for l in lists] if multi else (lists[f:f + 1],)), op_dtype=hip.op_dtype(flav), want=WANT, **kw)
            g2 = (R // PATCH) ** 2
            assert torch.equal(bits(one[1][0]), bits(got[1][f])) and torch.equal(bits(one[0]), bits(got[0][f * g2:(f + 1) * g2])), (entry, f)
        assert len({got[1][f].cpu().numpy().tobytes() for f in (0, edge - 1, edge)}) == 3


def test_1080p_to_224(flav, tap):
    lists, stacked, kw = yuv_case("nv12", 2, 1080, 1920, seed=5, pad=64)
    check_list_form(flav, tap, YUV, YUV_CONTIGUOUS, surface_fn, lists, stacked, 2, Rr=224, patch=14, R=224, **kw)


# ---- against the float64 oracle of the definition ----
def test_scattered_p010_pq_against_the_float64_oracle(flav, tap):
    """The P010 / PQ case of tests/test_gpu_hdr_frontend.py (hdr_oracle.GEOMS[1] = 30 x 50, noise, PQ, BT.2020 -> BT.709, 1000 / 203 nits; parametrised at its
    line 121) with the bound that test asserts for it at its line 102: ``err <= ho.image_bound()``."""
    case = (ho.GEOMS[1], "noise", "pq", 1, 1000.0, 203.0)
    H, W, Rr, patch, n, fmt = case[0]
    assert fmt == (2, 10, True, "420", True)                                                # P010
    y, cb, cr = ho.values(n, H, W, 10, "420", "noise")
    lists, stacked, kw = yuv_case("p010le", n, H, W, seed=6, pad=1, values=[(y[f], cb[f], cr[f]) for f in range(n)])
    got = check_list_form(flav, tap, YUV, YUV_CONTIGUOUS, surface_fn, lists, stacked, n, Rr=Rr, patch=patch, R=Rr, **kw, **HDR, full_range=False, transfer="pq",
                          gamut=True, peak_nits=1000.0, sdr_white_nits=203.0)
    want, bound = ho.case_oracle(case), ho.image_bound()
    err = float(np.abs(got[1].cpu().numpy().astype(np.float64) - want).max())
    print(f"scattered p010 pq {flav}: image err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound)


# ---- refusals on the device path leave the outputs untouched ----
def nan_outputs(flav, n):
    from revisionllm_amd import hip
    p = torch.full((n * (R // PATCH) ** 2, KP), NAN_BITS, dtype=torch.int16, device="cuda").view(hip.op_dtype(flav))
    return p, torch.full((n, 3, R, R), float("nan"), device="cuda")


def untouched(p, i):
    torch.cuda.synchronize()
    return bool((bits(p) == NAN_BITS).all()) and bool(torch.isnan(i).all())


def test_refusals_leave_the_outputs_untouched(flav):
    """A bad entry BEHIND the first RV_FRAME_TABLE_MAX frames refuses the whole call: nothing is launched for the chunk in front of it."""
    from revisionllm_amd import hip
    lib = hip.lib(flav)
    n = hip.FRAME_TABLE_MAX + 2
    src = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    at = src.data_ptr()
    # RGB: pt.RGB_BASE is bgra, 6 x 8, row stride 32
    p, i = nan_outputs(flav, n)
    outs = dict(n=n, patches=p.data_ptr(), image=i.data_ptr())
    assert call_rgb(lib, [at + 256 * f for f in range(n - 1)] + [None], outs) == -1 and "frame %d of %d" % (n - 1, n) in lib_error(flav) and untouched(p, i)
    assert call_rgb(lib, None, outs) == -1 and untouched(p, i)
    assert call_rgb(lib, [at] * n, dict(outs, ldp=KP - 1)) == -1 and untouched(p, i)
    # YCbCr: 96 x 64 yuv420p10le; a null plane, an odd pointer, and (as P010) a frame whose Cb and Cr are the other way round
    geom = dict(n=n, H=6, W=8, y_row_stride=16, c_row_stride=8)
    good = [(at + 512 * f, at + 512 * f + 128, at + 512 * f + 192) for f in range(n)]
    for bad, word in (((good[0][0], None, good[0][2]), "null plane"), ((good[0][0] + 1, good[0][1], good[0][2]), "aligned")):
        assert call_yuv(lib, hip, good[:-1] + [bad], surface=geom, args=dict(patches=p.data_ptr(), image=i.data_ptr())) == -1
        assert word in lib_error(flav) and "frame %d of %d" % (n - 1, n) in lib_error(flav) and untouched(p, i)
    inter = [(a, b, b + 2) for a, b, _ in good]
    inter[-1] = (inter[-1][0], inter[-1][1] + 2, inter[-1][1])
    assert call_yuv(lib, hip, inter, surface=dict(geom, c_pix=4, c_row_stride=16, msb_aligned=1), args=dict(patches=p.data_ptr(), image=i.data_ptr())) == -1
    assert "interleaved" in lib_error(flav) and "frame %d of %d" % (n - 1, n) in lib_error(flav) and untouched(p, i)
    # packed: pt.PACKED_BASE is y210le, 6 x 8, row stride 32
    assert call_packed(lib, hip, [at + 256 * f for f in range(n - 1)] + [at + 1], outs) == -1 and "frame %d of %d" % (n - 1, n) in lib_error(flav) and untouched(p, i)
    assert call_packed(lib, hip, [at + 256 * f for f in range(n - 1)] + [None], outs) == -1 and "null base" in lib_error(flav) and untouched(p, i)
    # ... and the good tables run
    for run in (lambda: call_rgb(lib, [at + 256 * f for f in range(n)], outs), lambda: call_packed(lib, hip, [at + 256 * f for f in range(n)], outs),
                lambda: call_yuv(lib, hip, good, surface=geom, args=dict(patches=p.data_ptr(), image=i.data_ptr()))):
        assert run() == 0, hip.last_error()                                                  # one call at a time: each must fill the image on its own
        torch.cuda.synchronize()
        assert not bool(torch.isnan(i).any())
        i.fill_(float("nan"))


# ---- end to end ----
def test_end_to_end_through_the_tiny_towers(flav):
    """ClipTowers on lists is ClipTowers on the stacked tensors; the extractor with scattered=True is the extractor, on chunks of 1 / 5 / 2 frames with bsz = 3."""
    from revisionllm_amd import ops
    from revisionllm_amd.data.clip_extractor import ClipFeatureExtractor
    from revisionllm_amd.data.clip_model import ClipTowers
    from revisionllm_amd.utils import synth
    c = synth.CLIP_TINY
    tw = ClipTowers(**c, t_heads=synth.CLIP_TINY_TEXT_HEADS, op_dtype=flav).init_synthetic(seed=SEED)
    ex = ClipFeatureExtractor(tw)
    n, H, W = 4, 46, 80
    views, stacked, kw = rgb_case("NCHW", n, H, W, seed=7)
    a = tw.encode_frames(views, **kw)
    assert tuple(a.shape) == (n, c["embed_dim"]) and torch.equal(bits(a), bits(tw.encode_frames(stacked, **kw)))
    lists, stacked, kw = yuv_case("nv12", n, H, W, seed=7)
    assert torch.equal(bits(tw.encode_surfaces_yuv(*lists, **kw)), bits(tw.encode_surfaces_yuv(*stacked, **kw)))
    views, stacked, kw = packed_case("yuyv422", n, H, W, seed=7)
    assert torch.equal(bits(tw.encode_surfaces_packed(views, **kw)), bits(tw.encode_surfaces_packed(stacked, **kw)))
    n = 8
    for fmt, fb in (("p010le", ops.yuv_frame_bytes(H, W, "p010le")), ("yuyv422", ops.packed_frame_bytes(H, W, "yuyv422"))):
        buf = torch.from_numpy(noise(8, n, fb))
        more = dict(transfer="pq") if fmt == "p010le" else {}
        want = ex.encode_video_pix_fmt(iter([buf[:1], buf[1:6], buf[6:]]), H, W, fmt, bsz=3, **more)
        got = ex.encode_video_pix_fmt(iter([buf[:1], buf[1:6], buf[6:]]), H, W, fmt, bsz=3, scattered=True, **more)
        assert tuple(got.shape) == (n, c["embed_dim"]) and torch.equal(bits(got), bits(want)), fmt
    rgb = torch.from_numpy(noise(9, n, 3, H, W))
    assert torch.equal(bits(ex.encode_video(iter([rgb[:1], rgb[1:6], rgb[6:]]), bsz=3, scattered=True)), bits(ex.encode_video(iter([rgb[:1], rgb[1:6], rgb[6:]]), bsz=3)))
    nv12 = torch.from_numpy(noise(10, n, H * 3 // 2, W))
    assert torch.equal(bits(ex.encode_video_yuv(iter([nv12[:1], nv12[1:6], nv12[6:]]), H, W, "nv12", bsz=3, scattered=True)),
                       bits(ex.encode_video_yuv(iter([nv12[:1], nv12[1:6], nv12[6:]]), H, W, "nv12", bsz=3)))
