"""rv_yuv_to_patches (decoded 8-bit 4:2:0 YCbCr planes -> antialiased bicubic resize of Y at full and Cb / Cr at half resolution -> colour matrix -> centre
crop -> normalise -> conv1 patch matrix) and the layers above it (ops.yuv_to_patches, ops.split_yuv420, ClipTowers.encode_frames_yuv,
ClipFeatureExtractor.encode_video_yuv) against an oracle kept in this file: the definition in include/revision_hip.h written out in float64 numpy - one
dense resampling matrix per plane and axis, the colour equations, the normalisation.  Its luma matrix is checked here against torch's own
``F.interpolate(mode="bicubic", antialias=True)`` in float64 (the oracle of test_gpu_frames_frontend.py).

Planes are uniform uint8 noise with a fixed seed: the hardest input for a resampler, one whose resampled values leave 0..255 and whose colours leave the
RGB cube, so a clamp or a uint8 / RGB intermediate would be caught.  patch = 14 (K = 588 -> Kp = 640: the pad columns exist) unless a case says otherwise.

Bounds.  image vs oracle: the RGB front end's 2e-4 in normalised units (f32 sums of at most ~40 x 40 taps of values below 256, then five f32 colour
coefficients on values of a few hundred: ~1e-6 is expected; 2e-4 is what the RGB test asserts and the issue sets).  End to end through the tiny
towers: the existing test's 2e-2.  RV_LOG_ERR=<file>: the measured maxima per case are appended there (profiles/frames_frontend_yuv_err.log is the place for one such run)."""
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
K_RB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
MATRIX_CODE = {"bt601": 0, "bt709": 1}
LOC_CODE = {"left": 0, "centre": 1}

#        H    W    R   patch n
CASES = [(2, 2, 14, 14, 2),          # 1 x 1 chroma plane, pure upscale
         (16, 16, 28, 14, 2),        # upscale on both planes
         (32, 48, 28, 14, 2),        # luma downscale < 2, chroma interpolated
         (96, 64, 28, 14, 2),        # portrait, chroma scale just above 1
         (30, 50, 28, 14, 2),        # odd chroma dimensions 15 x 25
         (240, 426, 28, 14, 2),      # many taps, several staging chunks
         (180, 320, 224, 14, 2),     # the towers' real output size
         (64, 64, 32, 16, 2)]        # K = 768 = Kp: ldp > Kp with a sentinel behind every row
IDS = ["%dx%d-R%d" % c[:3] for c in CASES]
COLOUR_CASE = CASES[3]
DEFAULT_COLOUR = ("bt601", False, "left")
COLOURS = [(m, fr, loc) for m in ("bt601", "bt709") for fr in (False, True) for loc in ("left", "centre")]

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


# ---- inputs and the float64 oracle (computed once per geometry and colour setting, shared, never modified) ----
@functools.lru_cache(maxsize=None)
def planes_u8(n, H, W):
    """uint8 noise: y [n,H,W], cb and cr [n,H/2,W/2] (CPU)."""
    g = torch.Generator().manual_seed(SEED + 1000 * H + W)
    return tuple(torch.randint(0, 256, s, generator=g, dtype=torch.uint8) for s in ((n, H, W), (n, H // 2, W // 2), (n, H // 2, W // 2)))


def packed(n, H, W, fmt):
    """The planes as the bytes of a rawvideo pipe: uint8 [n, H*3//2, W]."""
    y, cb, cr = planes_u8(n, H, W)
    if fmt == "i420":
        c = torch.cat([cb.reshape(n, -1), cr.reshape(n, -1)], 1)
    else:
        c = torch.stack((cb, cr) if fmt == "nv12" else (cr, cb), -1).reshape(n, -1)
    return torch.cat([y.reshape(n, -1), c], 1).reshape(n, H * 3 // 2, W).contiguous()


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


@functools.lru_cache(maxsize=None)
def oracle64(n, H, W, R, matrix="bt601", full_range=False, loc="left"):
    """float64 numpy [n,3,R,R]: the definition of rv_yuv_to_patches' image."""
    hr, wr = resized_size(H, W, R)
    top, left = int(round((hr - R) / 2.0)), int(round((wr - R) / 2.0))
    sy, sx = H / hr, W / wr
    y, cb, cr = (t.numpy().astype(np.float64) for t in planes_u8(n, H, W))
    my, mx = axis_matrix(H, sy, 1.0, 0.0, top, R), axis_matrix(W, sx, 1.0, 0.0, left, R)
    cy, cx = axis_matrix(H // 2, sy, 2.0, 0.0, top, R), axis_matrix(W // 2, sx, 2.0, 0.25 if loc == "left" else 0.0, left, R)
    yr, cbr, crr = my @ y @ mx.T, cy @ cb @ cx.T, cy @ cr @ cx.T
    kr, kb = K_RB[matrix]
    kg = 1.0 - kr - kb
    if full_range:
        yl, b, r = yr, cbr - 128.0, crr - 128.0
    else:
        yl, b, r = (yr - 16.0) * 255.0 / 219.0, (cbr - 128.0) * 255.0 / 224.0, (crr - 128.0) * 255.0 / 224.0
    rgb = np.stack([yl + 2.0 * (1.0 - kr) * r, yl - (2.0 * kb * (1.0 - kb) / kg) * b - (2.0 * kr * (1.0 - kr) / kg) * r, yl + 2.0 * (1.0 - kb) * b], 1)
    out = (rgb / 255.0 - np.array(MEAN).reshape(1, 3, 1, 1)) / (np.array(STD).reshape(1, 3, 1, 1) + 1e-8)
    out.setflags(write=False)
    return out


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
            fh.write(f"test_gpu_yuv_frontend.py {what} {value:.3e}\n")


def lib_error(flavour):
    """The last error message of ONE flavour's library (hip.last_error joins those of every loaded library)."""
    from revisionllm_amd import hip
    buf = ctypes.create_string_buffer(512)
    hip.lib(flavour).rv_last_error(buf, 512)
    return buf.value.decode()


def raw_call(planes, R, patch, flavour, colour=DEFAULT_COLOUR, ldp=None, want_patches=True, want_image=True, over=None):
    """rv_yuv_to_patches through ctypes on contiguous planar device planes and buffers of this test's making: patches pre-filled with NaN bit patterns, image
    with NaN.  ``over``: arguments to override (the refusal cases).  -> (status, patches [rows, ldp] or None, image or None)."""
    from revisionllm_amd import hip
    dt = hip.op_dtype(flavour)
    y, cb, cr = planes
    n, H, W = y.shape
    g, kp = R // patch, (3 * patch * patch + 127) // 128 * 128
    ldp = kp if ldp is None else ldp
    patches = torch.full((n * g * g, max(ldp, 1)), NAN_BITS, dtype=torch.int16, device="cuda").view(dt) if want_patches else None
    image = torch.full((n, 3, R, R), float("nan"), device="cuda") if want_image else None
    f3 = ctypes.c_float * 3
    a = dict(y=hip.ptr(y), yfs=H * W, yrs=W, cb=hip.ptr(cb), cr=hip.ptr(cr), cfs=(H // 2) * (W // 2), crs=W // 2, c_pix=1, n=n, H=H, W=W,
             matrix=MATRIX_CODE[colour[0]], full_range=int(colour[1]), chroma_loc=LOC_CODE[colour[2]], R=R, patch=patch, ldp=ldp)
    a.update(over or {})
    rc = hip.lib(flavour).rv_yuv_to_patches(a["y"], a["yfs"], a["yrs"], a["cb"], a["cr"], a["cfs"], a["crs"], a["c_pix"], a["n"], a["H"], a["W"], a["matrix"],
                                            a["full_range"], a["chroma_loc"], a["R"], a["patch"], f3(*MEAN), f3(*STD), hip.ptr(patches), a["ldp"],
                                            hip.ptr(image), hip.stream())
    torch.cuda.synchronize()
    return rc, patches, image


def dev_planes(n, H, W):
    return tuple(t.cuda() for t in planes_u8(n, H, W))


def test_oracle_luma_is_torchs_antialiased_bicubic():
    """The oracle's own check: its luma resampling is torch's float64 ``interpolate(mode="bicubic", antialias=True)`` + centre crop (what the RGB front end
    is tested against), at a downscale, an upscale and a crop with a half-to-even offset."""
    for H, W, R in ((96, 64, 28), (16, 16, 28), (56, 106, 28), (180, 320, 224)):
        hr, wr = resized_size(H, W, R)
        top, left = int(round((hr - R) / 2.0)), int(round((wr - R) / 2.0))
        y = planes_u8(1, H, W)[0].double()
        want = F.interpolate(y[:, None], size=(hr, wr), mode="bicubic", align_corners=False, antialias=True)[0, 0, top:top + R, left:left + R].numpy()
        got = axis_matrix(H, H / hr, 1.0, 0.0, top, R) @ y[0].numpy() @ axis_matrix(W, W / wr, 1.0, 0.0, left, R).T
        assert np.abs(got - want).max() < 1e-9


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_image_and_patches_vs_oracle(flav, case):
    """Per geometry: image within 2e-4 of the float64 oracle; patches = image rounded once, unfolded and zero-padded, bit for bit - pad columns zero in a
    buffer that held NaN patterns, columns behind Kp untouched; asking for one output alone gives the same bits."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = case
    dt = hip.op_dtype(flav)
    kp = (3 * patch * patch + 127) // 128 * 128
    ldp = kp + 8 if 3 * patch * patch == kp else kp
    planes = dev_planes(n, H, W)
    rc, patches, image = raw_call(planes, R, patch, flav, ldp=ldp)
    assert rc == 0, hip.last_error()
    err = float(np.abs(image.cpu().numpy().astype(np.float64) - oracle64(n, H, W, R)).max())
    log_err(f"image {H}x{W}->{R} {flav}", err)
    assert err <= IMAGE_BOUND, err
    expect = unfold(image.to(dt), patch, kp)
    assert torch.equal(bits(patches[:, :kp]), bits(expect))
    if kp > 3 * patch * patch:
        assert bool((bits(patches[:, 3 * patch * patch:kp]) == 0).all())             # +0, not -0, not NaN
    if ldp > kp:
        assert bool((bits(patches[:, kp:]) == NAN_BITS).all())                       # the sentinel behind every row is untouched
    # the wrapper allocates its own outputs: both, patches alone, image alone - the same bits
    p2, i2 = ops.yuv_to_patches(*planes, R=R, patch=patch, op_dtype=dt, want=("patches", "image"))
    assert torch.equal(bits(p2), bits(patches[:, :kp])) and torch.equal(bits(i2), bits(image))
    p3, i3 = ops.yuv_to_patches(*planes, R=R, patch=patch, op_dtype=dt)
    assert i3 is None and torch.equal(bits(p3), bits(p2))
    p4, i4 = ops.yuv_to_patches(*planes, R=R, patch=patch, op_dtype=dt, want=("image",))
    assert p4 is None and torch.equal(bits(i4), bits(i2))


def test_every_colour_setting_vs_oracle(flav):
    """matrix x range x siting on 96 x 64 against the oracle; left and centre siting differ (the offset is not ignored), and so do the other two switches."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = COLOUR_CASE
    planes = dev_planes(n, H, W)
    got = {}
    for m, fr, loc in COLOURS:
        _, img = ops.yuv_to_patches(*planes, R=R, patch=patch, matrix=m, full_range=fr, chroma_loc=loc, op_dtype=hip.op_dtype(flav), want=("image",))
        got[m, fr, loc] = img.cpu().numpy().astype(np.float64)
        err = float(np.abs(got[m, fr, loc] - oracle64(n, H, W, R, m, fr, loc)).max())
        log_err(f"image {H}x{W}->{R} {m} {'full' if fr else 'studio'} {loc} {flav}", err)
        assert err <= IMAGE_BOUND, (m, fr, loc, err)
    for m, fr, loc in COLOURS:
        other_loc = "centre" if loc == "left" else "left"
        assert np.abs(got[m, fr, loc] - got[m, fr, other_loc]).max() > 100 * IMAGE_BOUND
        assert np.abs(got[m, fr, loc] - got[m, not fr, loc]).max() > 100 * IMAGE_BOUND
        assert np.abs(got[m, fr, loc] - got["bt709" if m == "bt601" else "bt601", fr, loc]).max() > 100 * IMAGE_BOUND


def surface(n, H, W, fmt):
    """The planes inside a larger decode surface: pitch W + 24, the window 3 bytes into the allocation (no 16-byte load edge falls where it does in a packed
    buffer), 2 spare rows and 40 spare bytes per frame, noise everywhere else.  -> (y, cb, cr or None) views as ops.yuv_to_patches takes them."""
    y, cb, cr = planes_u8(n, H, W)
    pitch, h2, w2 = W + 24, H // 2, W // 2
    fs = (H * 3 // 2 + 2) * pitch + 40
    flat = torch.randint(0, 256, (n * fs + 3,), dtype=torch.uint8, generator=torch.Generator().manual_seed(7))
    yv = flat.as_strided((n, H, W), (fs, pitch, 1), 3)
    yv.copy_(y)
    if fmt == "i420":          # planar chroma: two half-width windows side by side in the rows below the luma
        cbv = flat.as_strided((n, h2, w2), (fs, pitch, 1), 3 + H * pitch)
        crv = flat.as_strided((n, h2, w2), (fs, pitch, 1), 3 + H * pitch + w2 + 5)
        cbv.copy_(cb)
        crv.copy_(cr)
        views = (yv, cbv, crv)
    else:
        pairs = flat.as_strided((n, h2, w2, 2), (fs, pitch, 2, 1), 3 + H * pitch)
        pairs.copy_(torch.stack((cb, cr) if fmt == "nv12" else (cr, cb), -1))
        views = (yv, pairs, None) if fmt == "nv12" else (yv, pairs[..., 1], pairs[..., 0])
    dev = flat.cuda()
    return tuple(None if v is None else dev.as_strided(v.shape, v.stride(), v.storage_offset()) for v in views)


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[5]], ids=[IDS[0], IDS[4], IDS[5]])
def test_layout_independence(flav, case):
    """The same content as I420, NV12 and NV21 (packed rawvideo buffers through split_yuv420, no copy), and as windows of a larger surface with a padded
    pitch, a 3-byte base offset and a padded frame stride: the same bits as the contiguous planar call."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = case
    kw = dict(R=R, patch=patch, op_dtype=hip.op_dtype(flav), want=("patches", "image"))
    base = ops.yuv_to_patches(*dev_planes(n, H, W), **kw)
    for fmt in ("i420", "nv12", "nv21"):
        buf = packed(n, H, W, fmt).cuda()
        views = ops.split_yuv420(buf, H, W, fmt)
        for v in views:
            assert v is None or buf.data_ptr() <= v.data_ptr() < buf.data_ptr() + buf.numel()
        assert same_bits(ops.yuv_to_patches(*views, **kw), base), fmt
        win = surface(n, H, W, fmt)
        assert win[0].data_ptr() % 16 == 3 and not win[0].is_contiguous()
        assert same_bits(ops.yuv_to_patches(*win, **kw), base), fmt + " window"


@pytest.mark.parametrize("case", [CASES[3], CASES[5]], ids=[IDS[3], IDS[5]])
def test_grey_frames_match_the_rgb_kernel(flav, case):
    """Full range with Cb = Cr = 128 is a grey frame: image equals ops.frames_to_patches on the Y plane replicated to three channels, within 2e-4."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = case
    y = dev_planes(n, H, W)[0]
    grey = torch.full((n, H // 2, W // 2), 128, dtype=torch.uint8, device="cuda")
    _, img = ops.yuv_to_patches(y, grey, grey.clone(), R=R, patch=patch, full_range=True, op_dtype=hip.op_dtype(flav), want=("image",))
    _, ref = ops.frames_to_patches(y[:, None].expand(n, 3, H, W).contiguous(), R, patch, op_dtype=hip.op_dtype(flav), want=("image",))
    err = float((img - ref).abs().max())
    log_err(f"grey-vs-rgb-kernel {H}x{W}->{R} {flav}", err)
    assert err <= IMAGE_BOUND, err


def test_batching_and_determinism(flav):
    """Frame f of an n = 3 call equals the n = 1 call on that frame bit for bit; two identical calls give identical bits; n = 0 gives empty outputs."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, _ = CASES[5]
    kw = dict(R=R, patch=patch, op_dtype=hip.op_dtype(flav), want=("patches", "image"))
    planes = dev_planes(3, H, W)
    a = ops.yuv_to_patches(*planes, **kw)
    assert same_bits(ops.yuv_to_patches(*planes, **kw), a)
    g2 = (R // patch) ** 2
    for f in range(3):
        p1, i1 = ops.yuv_to_patches(*(t[f:f + 1] for t in planes), **kw)
        assert torch.equal(bits(p1), bits(a[0][f * g2:(f + 1) * g2])) and torch.equal(bits(i1), bits(a[1][f:f + 1]))
    p, i = ops.yuv_to_patches(*(t[:0] for t in planes), **kw)
    assert tuple(p.shape) == (0, 640) and tuple(i.shape) == (0, 3, R, R)
    f3 = ctypes.c_float * 3
    assert hip.lib(flav).rv_yuv_to_patches(None, 0, 0, None, None, 0, 0, 1, 0, H, W, 0, 0, 0, R, patch, f3(*MEAN), f3(*STD), None, 0, None, None) == 0


REFUSALS = [("odd H", dict(H=95), "odd"),
            ("odd W", dict(W=63), "odd"),
            ("c_pix 0", dict(c_pix=0), "c_pix"),
            ("c_pix 3", dict(c_pix=3), "c_pix"),
            ("c_pix 2 on separate planes", dict(c_pix=2), "interleaved"),
            ("matrix 2", dict(matrix=2), "matrix"),
            ("matrix -1", dict(matrix=-1), "matrix"),
            ("full_range 2", dict(full_range=2), "full_range"),
            ("chroma_loc 2", dict(chroma_loc=2), "chroma_loc"),
            ("chroma_loc -1", dict(chroma_loc=-1), "chroma_loc"),
            ("null y", dict(y=None), "null plane"),
            ("null cb", dict(cb=None), "null plane"),
            ("null cr", dict(cr=None), "null plane"),
            ("H = 0", dict(H=0), "frame size"),
            ("W = 8194", dict(W=8194), "frame size"),
            ("H = 8194", dict(H=8194), "frame size"),
            ("R not a multiple of patch", dict(R=30), "multiple"),
            ("ldp < Kp", dict(ldp=639), "ldp"),
            ("taps beyond the LDS budget", dict(H=8192, W=8192, R=1, patch=1), "LDS"),
            ("more workgroups than a launch", dict(n=2 ** 30), "workgroups")]


@pytest.mark.parametrize("what,over,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(flav, what, over, msg):
    """Every refusal returns < 0 with a message, before any launch: the NaN-filled outputs stay as they were."""
    H, W, R, patch, n = COLOUR_CASE
    rc, patches, image = raw_call(dev_planes(n, H, W), R, patch, flav, over=over)
    assert rc < 0
    assert lib_error(flav).startswith("rv_yuv_to_patches") and msg in lib_error(flav), lib_error(flav)
    assert bool((bits(patches) == NAN_BITS).all()) and bool(torch.isnan(image).all())


def test_refuses_both_outputs_null_and_foreign_tensors(flav):
    """Both outputs null is refused; the wrapper refuses CPU tensors, anything but uint8 and planes of the wrong shape."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = COLOUR_CASE
    y, cb, cr = dev_planes(n, H, W)
    rc, _, _ = raw_call((y, cb, cr), R, patch, flav, want_patches=False, want_image=False)
    assert rc < 0 and "both outputs null" in lib_error(flav)
    with pytest.raises(hip.HipLibraryError):
        ops.yuv_to_patches(*planes_u8(n, H, W), R=R, patch=patch)
    with pytest.raises(hip.HipLibraryError):
        ops.yuv_to_patches(y.float(), cb, cr, R=R, patch=patch)
    with pytest.raises(hip.HipLibraryError):
        ops.yuv_to_patches(y, cb[:, :-1], cr[:, :-1], R=R, patch=patch)
    with pytest.raises(hip.HipLibraryError):
        ops.yuv_to_patches(y, cb, None, R=R, patch=patch)                             # cr=None announces interleaved [n,H/2,W/2,2]
    with pytest.raises(hip.HipLibraryError):
        ops.yuv_to_patches(y, cb, cr, R=30, patch=patch)
    with pytest.raises(ValueError):
        ops.yuv_to_patches(y, cb, cr, R=R, patch=patch, matrix="bt2020")


@pytest.fixture(scope="module")
def tiny_towers(flav):
    """The tiny CLIP of test_gpu_frames_frontend.py (utils/synth.py) and the oracle's weights."""
    from revisionllm_amd.data.clip_extractor import ClipFeatureExtractor
    from revisionllm_amd.data.clip_model import ClipTowers
    from revisionllm_amd.utils import synth
    c = synth.CLIP_TINY
    m = ClipTowers(**c, t_heads=synth.CLIP_TINY_TEXT_HEADS, op_dtype=flav).init_synthetic(seed=SEED)
    w = {k[len("clip."):]: T(v) for k, v in synth.build_numpy(synth.clip_towers_spec(**c), SEED, prefix="clip.").items()}
    return ClipFeatureExtractor(m), w, c


def test_encode_frames_and_video_yuv(flav, tiny_towers):
    """encode_frames_yuv on NV12 within the towers' bound (2e-2) of the oracle towers fed this file's float64 front end; encode_video_yuv over chunks of
    1, 5 and 2 frames with bsz = 3 equals the single-buffer call bit for bit, on CPU chunks as a pipe hands them over."""
    from oracle import clip_vit
    ex, w, c = tiny_towers
    n, H, W, R = 8, 46, 80, c["image_res"]
    from revisionllm_amd import ops
    buf = packed(n, H, W, "nv12")
    ref = clip_vit.encode_image(torch.from_numpy(oracle64(n, H, W, R).copy()).float(), w)
    got = ex.clip_extractor.encode_frames_yuv(*ops.split_yuv420(buf.cuda(), H, W, "nv12"))
    assert tuple(got.shape) == (n, c["embed_dim"])
    err = rel_err(got.cpu(), ref)
    log_err(f"tiny-towers-features nv12 {H}x{W}->{R} {flav}", float(err))
    assert err < 2e-2
    one = ex.encode_video_yuv(buf.cuda(), H, W, "nv12", bsz=3)                        # H < 720: the defaults are this file's DEFAULT_COLOUR
    assert rel_err(one.cpu(), ref) < 2e-2
    chunks = ex.encode_video_yuv(iter([buf[:1], buf[1:6], buf[6:]]), H, W, "nv12", bsz=3)
    assert torch.equal(bits(chunks), bits(one))
    i420 = ex.encode_video_yuv(packed(n, H, W, "i420"), H, W, "i420", bsz=3)
    assert torch.equal(bits(i420), bits(one))
    with pytest.raises(ValueError, match="uint8"):
        ex.encode_video_yuv(buf.float(), H, W, "nv12")
