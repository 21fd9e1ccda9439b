"""rv_yuv_surface_to_patches (decoded YCbCr planes of 8-bit or 16-bit samples, 4:2:0 / 4:2:2 / 4:4:4, planar or interleaved chroma -> antialiased bicubic
resize of every plane at its own resolution -> colour matrix -> centre crop -> normalise -> conv1 patch matrix) and the layers above it
(ops.yuv_surface_to_patches, ops.split_yuv, ClipTowers.encode_surfaces_yuv, ClipFeatureExtractor.encode_video_pix_fmt) against an oracle kept in this file:
the definition in include/revision_hip.h written out in float64 numpy - the sample extraction, one dense resampling matrix per plane and axis, the
depth-aware colour equations, the normalisation.

Planes are uniform integer noise over the whole of [0, 2^depth) with a fixed seed: resampled values leave the code range and colours leave the RGB cube, so
a clamp, an integer or RGB intermediate, a wrong shift or a wrong offset would be caught.  patch = 14 (K = 588 -> Kp = 640: the pad columns exist) unless a
case says otherwise.

Bounds.  image vs oracle: the front end's 2e-4 in normalised units, which both sibling tests assert.  It carries over to 16-bit samples because f32 holds
every 16-bit sample exactly and the rounding is relative: ~40 x 40 taps at 2^-24 on values below 2^17 is an absolute error around 0.1 on a 65535 scale,
~1e-5 after the normalisation (derived, not measured).  End to end through the tiny towers: the existing tests' 2e-2.  The equivalences are compared by
bits.  RV_LOG_ERR=<file>: the measured maxima per case are appended there (profiles/frames_frontend_surface_err.log is the place for one such run)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import SEED, T, rel_err

pytestmark = pytest.mark.gpu

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
IMAGE_BOUND = 2e-4
NAN_BITS = 0x7FFF            # a NaN in fp16 and in bf16
K_RB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
MATRIX_CODE = {"bt601": 0, "bt709": 1, "bt2020": 2}
LOC_CODE = {"left": 0, "centre": 1, "topleft": 2}
SUB = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}
DEFAULT_COLOUR = ("bt601", False, "left")


def surf(depth, sub="420", msb=False, interleaved=False):
    """A surface format: (sample bytes, depth, value in the high bits, subsampling, interleaved CbCr)."""
    return (1 if depth == 8 else 2, depth, msb, sub, interleaved)


P010, P016 = surf(10, msb=True, interleaved=True), surf(16, msb=True, interleaved=True)
#         H    W    R   patch n  surface
CASES = [(2, 2, 14, 14, 2, surf(10)),                           # 1 x 1 chroma plane, 10 bits in the low bits (yuv420p10le)
         (16, 16, 28, 14, 2, P010),                             # P010: interleaved, value in the high bits
         (30, 50, 28, 14, 2, surf(12)),                         # 4:2:0 12-bit: chroma dimensions 15 x 25
         (15, 16, 28, 14, 2, surf(8, "422")),                   # 4:2:2 8-bit: odd H on the axis that is not subsampled
         (15, 17, 28, 14, 2, surf(10, "444")),                  # 4:4:4 10-bit: both sides odd
         (32, 48, 28, 14, 2, surf(8, "422", interleaved=True)),  # nv16
         (240, 426, 28, 14, 2, P016),                           # noise up to 65535; many taps, several staging chunks at twice the bytes
         (180, 320, 224, 14, 2, surf(10)),                      # yuv420p10le at the towers' real output size
         (64, 64, 32, 16, 2, surf(16, "444"))]                  # K = 768 = Kp: ldp > Kp with a sentinel behind every row
IDS = ["%dx%d-R%d-%s%d%s" % (c[0], c[1], c[2], c[5][3], c[5][1], ("msb" if c[5][2] else "") + ("-il" if c[5][4] else "")) for c in CASES]
COLOUR_GEOM = (96, 64, 28, 14, 2)
COLOURS = [(m, fr, loc) for m in ("bt601", "bt709", "bt2020") for fr in (False, True) for loc in ("left", "centre", "topleft")]
OLD_COLOURS = [(m, fr, loc) for m in ("bt601", "bt709") for fr in (False, True) for loc in ("left", "centre")]

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")


@pytest.fixture(scope="module", params=[None] if _FORCED else ["f16", "bf16"])
def flav(request, op_flavour):
    """Both operand flavours (conftest's module list is fixed, so the module brings its own parameter; REVISION_TEST_FLAVOURS still narrows it)."""
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import hip
    f = request.param or op_flavour or hip.flavour()
    prev = hip.set_flavour(f)
    yield f
    hip.set_flavour(prev)


# ---- inputs and the float64 oracle (computed once per geometry, format and colour setting, shared, never modified) ----
@functools.lru_cache(maxsize=None)
def values(n, H, W, depth, sub):
    """Sample VALUES, uniform over [0, 2^depth): int64 y [n,H,W], cb and cr [n,H/sub_y,W/sub_x] (CPU)."""
    sx, sy = SUB[sub]
    g = torch.Generator().manual_seed(SEED + 1000 * H + W + 7 * depth)
    return tuple(torch.randint(0, 1 << depth, s, generator=g, dtype=torch.int64) for s in ((n, H, W), (n, H // sy, W // sx), (n, H // sy, W // sx)))


def words(v, fmt, garbage=None):
    """Values (int64, any shape) -> the stored samples: uint8, or uint16 words with the value in the low or (``msb``) the high bits; ``garbage``: what the
    low bits of an msb-aligned word hold besides."""
    sb, depth, msb, _, _ = fmt
    if sb == 1:
        return v.to(torch.uint8)
    if msb:
        v = v << (16 - depth)
        if garbage is not None:
            v = v | garbage
    return v.to(torch.int32).to(torch.uint16)


def dev_planes(n, H, W, fmt, garbage=False):
    """(y, cb, cr) on the device in the format's layout: three contiguous planes, or cb / cr as the two halves of one interleaved [n,h,w,2] tensor."""
    y, cb, cr = values(n, H, W, fmt[1], fmt[3])
    junk = (lambda t: torch.randint(0, 1 << (16 - fmt[1]), t.shape, generator=torch.Generator().manual_seed(11))) if garbage else (lambda t: None)
    if fmt[4]:
        c = torch.stack((cb, cr), -1)
        pairs = words(c, fmt, junk(c)).cuda()
        return words(y, fmt, junk(y)).cuda(), pairs[..., 0], pairs[..., 1]
    return tuple(words(t, fmt, junk(t)).cuda() for t in (y, cb, cr))


def packed(n, H, W, fmt, layout):
    """The frames as the bytes of a rawvideo pipe, uint8 [n, frame bytes]; layout "planar" | "cbcr" | "crcb"."""
    y, cb, cr = values(n, H, W, fmt[1], fmt[3])
    if layout == "planar":
        c = torch.cat([cb.reshape(n, -1), cr.reshape(n, -1)], 1)
    else:
        c = torch.stack((cb, cr) if layout == "cbcr" else (cr, cb), -1).reshape(n, -1)
    return words(torch.cat([y.reshape(n, -1), c], 1), fmt).contiguous().view(torch.uint8)


def resized_size(H, W, R):
    return (R, int(R * W / H)) if H <= W else (int(R * H / W), R)


def cubic(x):
    x = np.abs(x)
    return np.where(x < 1.0, (1.5 * x - 2.5) * x * x + 1.0, np.where(x < 2.0, ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0, 0.0))


def axis_matrix(n_in, scale, div, off, first, R):
    """float64 [R, n_in]: row o holds the normalised weights of output index first + o of an axis of n_in samples, ``div`` times coarser than the frame and
    shifted by ``off`` samples: centre = scale * (i + 0.5) / div + off, filter scale = scale / div (the header's definition; div = 1, off = 0 is luma)."""
    m = np.zeros((R, n_in))
    fs = max(scale / div, 1.0)
    support = 2.0 * fs
    for o in range(R):
        centre = scale * (first + o + 0.5) / div + off
        lo, hi = max(0, int(centre - support + 0.5)), min(n_in, int(centre + support + 0.5))
        w = cubic((np.arange(lo, hi) - centre + 0.5) / fs)
        m[o, lo:hi] = w / w.sum()
    return m


def normalise(rgb):
    out = (rgb / 255.0 - np.array(MEAN).reshape(1, 3, 1, 1)) / (np.array(STD).reshape(1, 3, 1, 1) + 1e-8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle64(n, H, W, R, depth, sub, matrix="bt601", full_range=False, loc="left"):
    """float64 numpy [n,3,R,R]: the definition of rv_yuv_surface_to_patches' image on ``values(n, H, W, depth, sub)``."""
    sx, sy = SUB[sub]
    hr, wr = resized_size(H, W, R)
    top, left = int(round((hr - R) / 2.0)), int(round((wr - R) / 2.0))
    fy, fx = H / hr, W / wr
    y, cb, cr = (t.numpy().astype(np.float64) for t in values(n, H, W, depth, sub))
    offx = 0.25 if sx == 2 and loc in ("left", "topleft") else 0.0
    offy = 0.25 if sy == 2 and loc == "topleft" else 0.0
    my, mx = axis_matrix(H, fy, 1.0, 0.0, top, R), axis_matrix(W, fx, 1.0, 0.0, left, R)
    cy, cx = axis_matrix(H // sy, fy, float(sy), offy, top, R), axis_matrix(W // sx, fx, float(sx), offx, left, R)
    yr, cbr, crr = my @ y @ mx.T, cy @ cb @ cx.T, cy @ cr @ cx.T
    kr, kb = K_RB[matrix]
    kg = 1.0 - kr - kb
    s = 2.0 ** (depth - 8)
    if full_range:
        top_code = 2.0 ** depth - 1.0
        yl, b, r = yr * 255.0 / top_code, (cbr - 128.0 * s) * 255.0 / top_code, (crr - 128.0 * s) * 255.0 / top_code
    else:
        yl, b, r = (yr - 16.0 * s) * 255.0 / (219.0 * s), (cbr - 128.0 * s) * 255.0 / (224.0 * s), (crr - 128.0 * s) * 255.0 / (224.0 * s)
    return normalise(np.stack([yl + 2.0 * (1.0 - kr) * r, yl - (2.0 * kb * (1.0 - kb) / kg) * b - (2.0 * kr * (1.0 - kr) / kg) * r, yl + 2.0 * (1.0 - kb) * b], 1))


def unfold(img, patch, kp):
    """[n,3,R,R] -> [n*g*g, kp]: rows (frame, gy, gx), columns (channel, py, px), zero-padded - ClipTowers.encode_image's own unfold + pad."""
    n, _, R, _ = img.shape
    g = R // patch
    p = img.reshape(n, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, 3 * patch * patch)
    return F.pad(p, (0, kp - p.shape[1]))


def bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def log_err(what, value):
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            fh.write(f"test_gpu_yuv_surface_frontend.py {what} {value:.3e}\n")


def lib_error(flavour):
    """The last error message of ONE flavour's library (hip.last_error joins those of every loaded library)."""
    from revisionllm_amd import hip
    buf = ctypes.create_string_buffer(512)
    hip.lib(flavour).rv_last_error(buf, 512)
    return buf.value.decode()


def raw_call(planes, fmt, R, patch, flavour, colour=DEFAULT_COLOUR, ldp=None, want_patches=True, want_image=True, over=None, null_struct=False):
    """rv_yuv_surface_to_patches through ctypes on the planes of ``dev_planes`` and buffers of this test's making: patches pre-filled with NaN bit patterns,
    image with NaN.  ``over``: struct fields / arguments to override (the refusal cases).  -> (status, patches [rows, ldp] or None, image or None)."""
    from revisionllm_amd import hip
    dt = hip.op_dtype(flavour)
    sb, depth, msb, sub, il = fmt
    y, cb, cr = planes
    n, H, W = y.shape
    h, w = cb.shape[1], cb.shape[2]
    g, kp = R // patch, (3 * patch * patch + 127) // 128 * 128
    ldp = kp if ldp is None else ldp
    patches = torch.full((n * g * g, max(ldp, 1)), NAN_BITS, dtype=torch.int16, device="cuda").view(dt) if want_patches else None
    image = torch.full((n, 3, R, R), float("nan"), device="cuda") if want_image else None
    cp = 2 if il else 1                                                                 # samples between neighbours of one chroma plane
    a = dict(y=y.data_ptr(), cb=cb.data_ptr(), cr=cr.data_ptr(), y_frame_stride=H * W * sb, y_row_stride=W * sb, c_frame_stride=h * w * cp * sb,
             c_row_stride=w * cp * sb, sample_bytes=sb, depth=depth, msb_aligned=int(msb), c_pix=cp * sb, sub_x=SUB[sub][0], sub_y=SUB[sub][1], n=n, H=H, W=W,
             matrix=MATRIX_CODE[colour[0]], full_range=int(colour[1]), chroma_loc=LOC_CODE[colour[2]], R=R, patch=patch, ldp=ldp)
    a.update(over or {})
    s = hip.RvYuvSurface(**{k: a[k] for k, _ in hip.RvYuvSurface._fields_})
    f3 = ctypes.c_float * 3
    rc = hip.lib(flavour).rv_yuv_surface_to_patches(None if null_struct else ctypes.byref(s), a["R"], a["patch"], f3(*MEAN), f3(*STD), hip.ptr(patches),
                                                    a["ldp"], hip.ptr(image), hip.stream())
    torch.cuda.synchronize()
    return rc, patches, image


def surface_kw(fmt):
    return dict(depth=fmt[1], msb_aligned=fmt[2], subsampling=fmt[3])


def test_oracle_luma_is_torchs_antialiased_bicubic():
    """The oracle's own check: its luma resampling of 10-bit values is torch's float64 ``interpolate(mode="bicubic", antialias=True)`` + centre crop (what
    the RGB front end is tested against), at a downscale, an upscale, an odd-sided frame and the towers' real output size."""
    for H, W, R in ((96, 64, 28), (16, 16, 28), (15, 17, 28), (180, 320, 224)):
        hr, wr = resized_size(H, W, R)
        top, left = int(round((hr - R) / 2.0)), int(round((wr - R) / 2.0))
        y = values(1, H, W, 10, "444")[0].double()
        want = F.interpolate(y[:, None], size=(hr, wr), mode="bicubic", align_corners=False, antialias=True)[0, 0, top:top + R, left:left + R].numpy()
        got = axis_matrix(H, H / hr, 1.0, 0.0, top, R) @ y[0].numpy() @ axis_matrix(W, W / wr, 1.0, 0.0, left, R).T
        assert np.abs(got - want).max() < 1e-8


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_image_and_patches_vs_oracle(flav, case):
    """Per geometry and surface: image within 2e-4 of the float64 oracle; patches = image rounded once, unfolded and zero-padded, bit for bit - pad columns
    zero in a buffer that held NaN patterns, columns behind Kp untouched; the wrapper on the same planes gives the same bits, one output or both."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n, fmt = case
    dt = hip.op_dtype(flav)
    kp = (3 * patch * patch + 127) // 128 * 128
    ldp = kp + 8 if 3 * patch * patch == kp else kp
    planes = dev_planes(n, H, W, fmt)
    rc, patches, image = raw_call(planes, fmt, R, patch, flav, ldp=ldp)
    assert rc == 0, hip.last_error()
    assert not bool(torch.isnan(image).any())                                          # every element was written
    err = float(np.abs(image.cpu().numpy().astype(np.float64) - oracle64(n, H, W, R, fmt[1], fmt[3])).max())
    log_err(f"image {IDS[CASES.index(case)]} {flav}", err)
    assert err <= IMAGE_BOUND, err
    expect = unfold(image.to(dt), patch, kp)
    assert torch.equal(bits(patches[:, :kp]), bits(expect))
    if kp > 3 * patch * patch:
        assert bool((bits(patches[:, 3 * patch * patch:kp]) == 0).all())             # +0, not -0, not NaN
    if ldp > kp:
        assert bool((bits(patches[:, kp:]) == NAN_BITS).all())                       # the sentinel behind every row is untouched
    kw = dict(R=R, patch=patch, op_dtype=dt, **surface_kw(fmt))
    p2, i2 = ops.yuv_surface_to_patches(*planes, want=("patches", "image"), **kw)
    assert torch.equal(bits(p2), bits(patches[:, :kp])) and torch.equal(bits(i2), bits(image))
    p3, i3 = ops.yuv_surface_to_patches(*planes, **kw)
    assert i3 is None and torch.equal(bits(p3), bits(p2))
    p4, i4 = ops.yuv_surface_to_patches(*planes, want=("image",), **kw)
    assert p4 is None and torch.equal(bits(i4), bits(i2))


def test_every_colour_setting_vs_oracle(flav):
    """matrix x range x siting on 96 x 64, 4:2:0 10-bit, and the horizontal sitings at 4:2:2, against the oracle; every switch changes the result, except
    where the definition says it does not (top-left = left on an axis that is not subsampled)."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = COLOUR_GEOM
    dt = hip.op_dtype(flav)

    def run(fmt, m, fr, loc):
        _, img = ops.yuv_surface_to_patches(*dev_planes(n, H, W, fmt), R=R, patch=patch, matrix=m, full_range=fr, chroma_loc=loc, op_dtype=dt, want=("image",),
                                            **surface_kw(fmt))
        got = img.cpu().numpy().astype(np.float64)
        err = float(np.abs(got - oracle64(n, H, W, R, fmt[1], fmt[3], m, fr, loc)).max())
        log_err(f"image {H}x{W}->{R} {fmt[3]} {fmt[1]}-bit {m} {'full' if fr else 'studio'} {loc} {flav}", err)
        assert err <= IMAGE_BOUND, (fmt, m, fr, loc, err)
        return got

    got = {c: run(surf(10), *c) for c in COLOURS}
    for m, fr, loc in COLOURS:
        for other in (l for l in LOC_CODE if l != loc):
            assert np.abs(got[m, fr, loc] - got[m, fr, other]).max() > 100 * IMAGE_BOUND
        assert np.abs(got[m, fr, loc] - got[m, not fr, loc]).max() > 100 * IMAGE_BOUND
        for other in (k for k in K_RB if k != m):
            assert np.abs(got[m, fr, loc] - got[other, fr, loc]).max() > 100 * IMAGE_BOUND
    for fmt in (surf(10, "422"), surf(8, "422", interleaved=True)):
        g422 = {loc: run(fmt, "bt709", False, loc) for loc in LOC_CODE}
        assert np.abs(g422["left"] - g422["centre"]).max() > 100 * IMAGE_BOUND
        assert np.array_equal(g422["left"], g422["topleft"])                           # the vertical axis is not subsampled


# ---- exact equivalences: compared by bits ----
@pytest.mark.parametrize("geom", [(30, 50, 28, 14, 2), (96, 64, 28, 14, 2)], ids=["30x50", "96x64"])
def test_depth_8_420_is_rv_yuv_to_patches_to_the_bit(flav, geom):
    """(a) The same NV12 / NV21 / I420 bytes through ops.split_yuv + the surface entry and through ops.split_yuv420 + rv_yuv_to_patches, in all eight colour
    settings the first entry has: identical bits."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = geom
    kw = dict(R=R, patch=patch, op_dtype=hip.op_dtype(flav), want=("patches", "image"))
    for old, new, layout in (("nv12", "nv12", "cbcr"), ("nv21", "nv21", "crcb"), ("i420", "yuv420p", "planar")):
        buf = packed(n, H, W, surf(8), layout).cuda()
        planes, skw = ops.split_yuv(buf, H, W, new)
        assert skw == dict(depth=8, msb_aligned=False, subsampling="420")
        old_planes = ops.split_yuv420(buf.view(n, H * 3 // 2, W), H, W, old)
        for m, fr, loc in OLD_COLOURS:
            c = dict(matrix=m, full_range=fr, chroma_loc=loc)
            assert same_bits(ops.yuv_surface_to_patches(*planes, **skw, **c, **kw), ops.yuv_to_patches(*old_planes, **c, **kw)), (old, c)


def test_p010_is_yuv420p10le_and_its_low_bits_do_not_matter(flav):
    """(b) P010 words v << 6 give the bits of yuv420p10le words v (interleaved or planar, high or low bits: one set of values); (c) so do P010 words with
    random garbage in their six low bits."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = 30, 50, 28, 14, 2
    kw = dict(R=R, patch=patch, op_dtype=hip.op_dtype(flav), want=("patches", "image"))
    lsb = ops.yuv_surface_to_patches(*dev_planes(n, H, W, surf(10)), **surface_kw(surf(10)), **kw)
    clean = dev_planes(n, H, W, P010)
    assert bool((clean[0].cpu().to(torch.int32) % 64 == 0).all()) and int(clean[0].cpu().to(torch.int32).max()) > 1023
    assert same_bits(ops.yuv_surface_to_patches(*clean, **surface_kw(P010), **kw), lsb)
    dirty = dev_planes(n, H, W, P010, garbage=True)
    assert all(bool((d.cpu().to(torch.int32) % 64 != 0).any()) for d in dirty)
    assert same_bits(ops.yuv_surface_to_patches(*dirty, **surface_kw(P010), **kw), lsb)
    # ... and through the packed rawvideo bytes
    for fmt, name, layout in ((P010, "p010le", "cbcr"), (surf(10), "yuv420p10le", "planar")):
        planes, skw = ops.split_yuv(packed(n, H, W, fmt, layout).cuda(), H, W, name)
        assert skw == surface_kw(fmt)
        assert same_bits(ops.yuv_surface_to_patches(*planes, **skw, **kw), lsb), name


def window(n, H, W, fmt):
    """The planes inside a larger decode surface: pitch W + 11 SAMPLES (61 / 122 bytes at W = 50: no multiple of 16), the window 3 samples into the
    allocation, 2 spare rows and 40 spare samples per frame, noise everywhere else.  -> (y, cb, cr or None) device views as the wrapper takes them."""
    sb, depth, msb, sub, il = fmt
    y, cb, cr = values(n, H, W, depth, sub)
    h, w = cb.shape[1], cb.shape[2]
    pitch = W + 11 if not (il and sub == "444") else 2 * W + 11
    side = 2 * w + 5 <= pitch
    y, pair, cb, cr = (words(t, fmt) for t in (y, torch.stack((cb, cr), -1), cb, cr))
    fs = (H + (h if il or side else 2 * h) + 2) * pitch + 40
    flat = torch.randint(0, 256 ** sb, (n * fs + 3,), dtype=torch.int32, generator=torch.Generator().manual_seed(7)).to(y.dtype)
    yv = flat.as_strided((n, H, W), (fs, pitch, 1), 3)
    yv.copy_(y)
    if il:
        pairs = flat.as_strided((n, h, w, 2), (fs, pitch, 2, 1), 3 + H * pitch)
        pairs.copy_(pair)
        views = (yv, pairs, None)
    else:                      # planar chroma: two windows in the rows below the luma, side by side where they fit, else one below the other
        cbv = flat.as_strided((n, h, w), (fs, pitch * (1 if side else 2), 1), 3 + H * pitch)
        crv = flat.as_strided((n, h, w), (fs, pitch * (1 if side else 2), 1), 3 + H * pitch + (w + 5 if side else pitch))
        cbv.copy_(cb)
        crv.copy_(cr)
        views = (yv, cbv, crv)
    dev = flat.cuda()
    return tuple(None if v is None else dev.as_strided(v.shape, v.stride(), v.storage_offset()) for v in views)


@pytest.mark.parametrize("fmt", [surf(8, "422"), surf(8, interleaved=True), P010, surf(12, "444"), surf(10, "422", msb=True, interleaved=True)],
                         ids=["yuv422p", "nv12", "p010", "yuv444p12", "p210"])
def test_a_window_of_a_larger_surface(flav, fmt):
    """(d) Planes that lie inside a larger surface - a start offset of an odd number of samples, a padded pitch that is no multiple of 16 bytes, a padded
    frame stride - give the bits of the same planes contiguous, 8-bit and 16-bit, planar and interleaved."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = 30, 50, 28, 14, 2
    kw = dict(R=R, patch=patch, op_dtype=hip.op_dtype(flav), want=("patches", "image"), **surface_kw(fmt))
    base = ops.yuv_surface_to_patches(*dev_planes(n, H, W, fmt), **kw)
    win = window(n, H, W, fmt)
    es = win[0].element_size()
    assert win[0].data_ptr() % 16 == 3 * es and not win[0].is_contiguous() and (win[0].stride(1) * es) % 16 != 0
    assert same_bits(ops.yuv_surface_to_patches(*win, **kw), base)


def test_batching_and_determinism(flav):
    """(e) Two identical calls give identical bits; n split into two calls gives the bits of the one call; n = 0 gives empty outputs."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, _, fmt = CASES[6]
    kw = dict(R=R, patch=patch, op_dtype=hip.op_dtype(flav), want=("patches", "image"), **surface_kw(fmt))
    planes = dev_planes(3, H, W, fmt)
    a = ops.yuv_surface_to_patches(*planes, **kw)
    assert same_bits(ops.yuv_surface_to_patches(*planes, **kw), a)
    g2 = (R // patch) ** 2
    p1, i1 = ops.yuv_surface_to_patches(*(t[:1] for t in planes), **kw)
    p2, i2 = ops.yuv_surface_to_patches(*(t[1:] for t in planes), **kw)
    assert torch.equal(bits(torch.cat([p1, p2])), bits(a[0])) and torch.equal(bits(torch.cat([i1, i2])), bits(a[1])) and len(p1) == g2
    p, i = ops.yuv_surface_to_patches(*(t[:0] for t in planes), **kw)
    assert tuple(p.shape) == (0, 640) and tuple(i.shape) == (0, 3, R, R)
    rc, patches, image = raw_call(planes, fmt, R, patch, flav, over=dict(n=0, y=None, cb=None, cr=None))
    assert rc == 0 and bool((bits(patches) == NAN_BITS).all()) and bool(torch.isnan(image).all())


@pytest.mark.parametrize("geom", [(15, 17, 28, 14, 2), (96, 64, 28, 14, 2)], ids=["15x17", "96x64"])
def test_grey_chroma_is_the_rgb_front_end_on_the_scaled_luma(flav, geom):
    """4:4:4 10-bit full range with Cb = Cr = 512 is the grey frame Y * 255 / 1023: the image is within 2e-4 of the RGB front end's oracle (torch's float64
    antialiased bicubic resize, centre crop, normalise) on that frame, built in float and replicated to three channels."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = geom
    fmt = surf(10, "444")
    y = dev_planes(n, H, W, fmt)[0]
    grey = torch.full((n, H, W), 512, dtype=torch.int32).to(torch.uint16).cuda()
    _, img = ops.yuv_surface_to_patches(y, grey, grey.clone(), R=R, patch=patch, full_range=True, op_dtype=hip.op_dtype(flav), want=("image",),
                                        **surface_kw(fmt))
    frame = (values(n, H, W, 10, "444")[0].double() * 255.0 / 1023.0)[:, None].expand(n, 3, H, W)
    hr, wr = resized_size(H, W, R)
    top, left = int(round((hr - R) / 2.0)), int(round((wr - R) / 2.0))
    ref = F.interpolate(frame, size=(hr, wr), mode="bicubic", align_corners=False, antialias=True)[:, :, top:top + R, left:left + R]
    err = float(np.abs(img.cpu().numpy().astype(np.float64) - normalise(ref.numpy())).max())
    log_err(f"grey-vs-rgb-oracle {H}x{W}->{R} {flav}", err)
    assert err <= IMAGE_BOUND, err


# ---- refusals ----
REFUSAL_FMT = surf(10)             # planar 4:2:0, 10 bits in the low bits of 16-bit words
S8 = dict(sample_bytes=1, depth=8, c_pix=1)
REFUSALS = [("null y", dict(y=None), "null plane"),
            ("null cb", dict(cb=None), "null plane"),
            ("null cr", dict(cr=None), "null plane"),
            ("sample_bytes 0", dict(sample_bytes=0), "sample_bytes"),
            ("sample_bytes 3", dict(sample_bytes=3), "sample_bytes"),
            ("sample_bytes 4", dict(sample_bytes=4), "sample_bytes"),
            ("depth 8 in 16-bit words", dict(depth=8), "depth"),
            ("depth 17", dict(depth=17), "depth"),
            ("depth 10 in bytes", dict(sample_bytes=1, c_pix=1), "depth"),
            ("depth 7 in bytes", dict(S8, depth=7), "depth"),
            ("msb_aligned 2", dict(msb_aligned=2), "msb_aligned"),
            ("msb_aligned -1", dict(msb_aligned=-1), "msb_aligned"),
            ("msb_aligned with bytes", dict(S8, msb_aligned=1), "msb_aligned"),
            ("sub 1,2", dict(sub_x=1, sub_y=2), "sub_x"),
            ("sub 4,1", dict(sub_x=4, sub_y=1), "sub_x"),
            ("sub 0,0", dict(sub_x=0, sub_y=0), "sub_x"),
            ("sub 2,4", dict(sub_x=2, sub_y=4), "sub_x"),
            ("odd H at 4:2:0", dict(H=95), "odd"),
            ("odd W at 4:2:0", dict(W=63), "odd"),
            ("odd W at 4:2:2", dict(W=63, sub_y=1), "odd"),
            ("H = 0", dict(H=0), "frame size"),
            ("W = 1 at 4:2:0", dict(W=1), "frame size"),
            ("H = 0 at 4:4:4", dict(H=0, sub_x=1, sub_y=1), "frame size"),
            ("W = 8194", dict(W=8194), "frame size"),
            ("H = 8193 at 4:4:4", dict(H=8193, sub_x=1, sub_y=1), "frame size"),
            ("c_pix 1 with 16-bit words", dict(c_pix=1), "c_pix"),
            ("c_pix 3", dict(c_pix=3), "c_pix"),
            ("c_pix 8", dict(c_pix=8), "c_pix"),
            ("c_pix 2 with bytes, separate planes", dict(S8, c_pix=2), "interleaved"),
            ("c_pix 4 on separate planes", dict(c_pix=4), "interleaved"),
            ("odd y pointer", "y+1", "aligned"),
            ("odd cb pointer", "cb+1", "aligned"),
            ("odd cr pointer", "cr+1", "aligned"),
            ("odd y row stride", dict(y_row_stride=129), "aligned"),
            ("odd y frame stride", dict(y_frame_stride=96 * 64 * 2 + 1), "aligned"),
            ("odd c row stride", dict(c_row_stride=65), "aligned"),
            ("odd c frame stride", dict(c_frame_stride=48 * 32 * 2 + 1), "aligned"),
            ("matrix 3", dict(matrix=3), "matrix"),
            ("matrix -1", dict(matrix=-1), "matrix"),
            ("full_range 2", dict(full_range=2), "full_range"),
            ("full_range -1", dict(full_range=-1), "full_range"),
            ("chroma_loc 3", dict(chroma_loc=3), "chroma_loc"),
            ("chroma_loc -1", dict(chroma_loc=-1), "chroma_loc"),
            ("R not a multiple of patch", dict(R=30), "multiple"),
            ("ldp < Kp", dict(ldp=639), "ldp"),
            ("taps beyond the LDS budget", dict(H=8192, W=8192, R=1, patch=1), "LDS"),
            ("more workgroups than a launch", dict(n=2 ** 30), "workgroups")]


@pytest.mark.parametrize("what,over,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(flav, what, over, msg):
    """Every refusal returns < 0 with a message that names the entry point and the offending argument, before any launch: the NaN-filled outputs stay as they
    were."""
    H, W, R, patch, n = COLOUR_GEOM
    planes = dev_planes(n, H, W, REFUSAL_FMT)
    if isinstance(over, str):
        k = over[:-2]
        over = {k: planes["y cb cr".split().index(k)].data_ptr() + 1}
    rc, patches, image = raw_call(planes, REFUSAL_FMT, R, patch, flav, over=over)
    assert rc < 0
    assert lib_error(flav).startswith("rv_yuv_surface_to_patches") and msg in lib_error(flav), lib_error(flav)
    assert bool((bits(patches) == NAN_BITS).all()) and bool(torch.isnan(image).all())


def test_refuses_a_null_struct_both_outputs_null_and_foreign_tensors(flav):
    """A null struct and both outputs null are refused; the wrapper refuses CPU tensors, other dtypes, mixed dtypes, planes of the wrong shape, unknown names."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = COLOUR_GEOM
    fmt = REFUSAL_FMT
    y, cb, cr = dev_planes(n, H, W, fmt)
    rc, patches, image = raw_call((y, cb, cr), fmt, R, patch, flav, null_struct=True)
    assert rc < 0 and lib_error(flav).startswith("rv_yuv_surface_to_patches") and "null surface" in lib_error(flav)
    assert bool((bits(patches) == NAN_BITS).all()) and bool(torch.isnan(image).all())
    rc, _, _ = raw_call((y, cb, cr), fmt, R, patch, flav, want_patches=False, want_image=False)
    assert rc < 0 and "both outputs null" in lib_error(flav)
    kw = dict(R=R, patch=patch, **surface_kw(fmt))
    with pytest.raises(hip.HipLibraryError, match="CPU"):
        ops.yuv_surface_to_patches(y.cpu(), cb.cpu(), cr.cpu(), **kw)
    with pytest.raises(hip.HipLibraryError):
        ops.yuv_surface_to_patches(y.float(), cb, cr, **kw)
    with pytest.raises(hip.HipLibraryError):
        ops.yuv_surface_to_patches(y, cb.to(torch.uint8), cr.to(torch.uint8), **kw)     # one dtype for all planes
    with pytest.raises(hip.HipLibraryError):
        ops.yuv_surface_to_patches(y, cb[:, :-1], cr[:, :-1], **kw)
    with pytest.raises(hip.HipLibraryError):
        ops.yuv_surface_to_patches(y, cb, None, **kw)                                   # cr=None announces interleaved [n,h,w,2]
    with pytest.raises(hip.HipLibraryError):
        ops.yuv_surface_to_patches(y, cb, cr, R=R, patch=patch, depth=10, subsampling="444")   # chroma planes of 4:2:0 size
    with pytest.raises(hip.HipLibraryError, match="depth"):
        ops.yuv_surface_to_patches(y, cb, cr, R=R, patch=patch, depth=8)                # 16-bit words hold 9 .. 16 bits
    with pytest.raises(hip.HipLibraryError, match="multiple"):
        ops.yuv_surface_to_patches(y, cb, cr, R=30, patch=patch, depth=10)
    for bad in (dict(matrix="bt2100"), dict(chroma_loc="top"), dict(subsampling="411")):
        with pytest.raises(ValueError):
            ops.yuv_surface_to_patches(y, cb, cr, **{**kw, **bad})


# ---- end to end ----
@pytest.fixture(scope="module")
def tiny_towers(flav):
    """The tiny CLIP of the sibling front-end tests (utils/synth.py) and the oracle's weights."""
    from revisionllm_amd.data.clip_extractor import ClipFeatureExtractor
    from revisionllm_amd.data.clip_model import ClipTowers
    from revisionllm_amd.utils import synth
    c = synth.CLIP_TINY
    m = ClipTowers(**c, t_heads=synth.CLIP_TINY_TEXT_HEADS, op_dtype=flav).init_synthetic(seed=SEED)
    w = {k[len("clip."):]: T(v) for k, v in synth.build_numpy(synth.clip_towers_spec(**c), SEED, prefix="clip.").items()}
    return ClipFeatureExtractor(m), w, c


def test_encode_video_pix_fmt(flav, tiny_towers):
    """encode_video_pix_fmt on p010le within the towers' bound (2e-2) of the oracle towers fed this file's float64 front end; chunks of 1, 5 and 2 frames with
    bsz = 3, on the CPU as a pipe hands them over, equal the single-buffer call bit for bit; encode_surfaces_yuv on the split planes likewise."""
    from oracle import clip_vit
    from revisionllm_amd import ops
    ex, w, c = tiny_towers
    n, H, W, R = 8, 46, 80, c["image_res"]
    buf = packed(n, H, W, P010, "cbcr")
    assert tuple(buf.shape) == (n, ops.yuv_frame_bytes(H, W, "p010le"))
    ref = clip_vit.encode_image(torch.from_numpy(oracle64(n, H, W, R, 10, "420").copy()).float(), w)   # H < 720: the defaults are DEFAULT_COLOUR
    one = ex.encode_video_pix_fmt(buf.cuda(), H, W, "p010le", bsz=3)
    assert tuple(one.shape) == (n, c["embed_dim"])
    err = rel_err(one.cpu(), ref)
    log_err(f"tiny-towers-features p010le {H}x{W}->{R} {flav}", float(err))
    assert err < 2e-2
    chunks = ex.encode_video_pix_fmt(iter([buf[:1], buf[1:6], buf[6:]]), H, W, "p010le", bsz=3)
    assert torch.equal(bits(chunks), bits(one))
    planes, kw = ops.split_yuv(buf.cuda(), H, W, "p010le")
    got = ex.clip_extractor.encode_surfaces_yuv(*planes, **kw)
    assert rel_err(got.cpu(), ref) < 2e-2
    lsb = ex.encode_video_pix_fmt(packed(n, H, W, surf(10), "planar"), H, W, "yuv420p10le", bsz=3)
    assert torch.equal(bits(lsb), bits(one))
    with pytest.raises(ValueError, match="uint8"):
        ex.encode_video_pix_fmt(buf.float(), H, W, "p010le")
