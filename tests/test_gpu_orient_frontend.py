"""Display orientation inside the CLIP front-end kernels (rv_frames_to_patches_oriented, rv_yuv_surface_to_patches_oriented) and the layers above them
(``rotate`` / ``hflip`` / ``vflip`` of ops.frames_to_patches, ops.yuv_to_patches, ops.yuv_surface_to_patches, ClipTowers.encode_*,
ClipFeatureExtractor.encode_video*) against the float64 oracle of tests/orient_oracle.py: the header's definition - the un-oriented entry on the picture
oriented with three NumPy steps - written out on its own.

Inputs: uniform integer noise over the whole code range with the suite's seed; every pixel is compared.

Bounds.  Image vs oracle: the sibling front-end tests' 2e-4 in normalised units - the oriented passes do the same number of f32 roundings per output as the
un-oriented ones (the same taps with the same f64-computed weights, summed in the other order along a mirrored axis), so their derivation carries over.
Patches: the image rounded once to the operand type (the kernel's own image: bit for bit; the oracle's: within the bound and one rounding).  HDR cases:
hdr_oracle.image_bound().  End to end through the tiny towers: the siblings' 2e-2.  Equivalences are compared by bits, except a mirror-only orientation against
the existing entry on a flipped copy: both lie within one bound of the same oracle, so within two of each other (the sums run in opposite orders; bit
equality is not claimed).  RV_LOG_ERR=<file>: the measured maxima are appended there (profiles/frontend_orient_err.log holds one such run)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import orient_oracle as oo
from helpers import SEED, T, rel_err

pytestmark = pytest.mark.gpu

ME = "test_gpu_orient_frontend.py"
NAN_BITS = 0x7FFF            # a NaN in fp16 and in bf16
HALF_ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # relative rounding error of one conversion (11 / 8 significant bits)
#: orientation code -> the keywords that spell it
SPELL = {0: dict(), 1: dict(rotate=90, hflip=True), 2: dict(hflip=True), 3: dict(rotate=90), 4: dict(vflip=True), 5: dict(rotate=270), 6: dict(rotate=180),
         7: dict(rotate=90, vflip=True)}
MATRIX_CODE = {"bt601": 0, "bt709": 1, "bt2020": 2}
LOC_CODE = {"left": 0, "centre": 1, "topleft": 2}


def surf(depth, sub="420", msb=False, interleaved=False):
    """A surface format: (sample bytes, depth, value in the high bits, subsampling, interleaved CbCr)."""
    return (1 if depth == 8 else 2, depth, msb, sub, interleaved)


P010 = surf(10, msb=True, interleaved=True)
#              H   W   R  patch n
RGB_GEOMS = [(30, 51, 28, 14, 2),                 # an odd crop margin; under transpose the long side changes axis
             (7, 5, 14, 14, 2)]                   # an upscale
#                H   W   R  patch n  surface                        siting
SURFACES = [(32, 54, 28, 14, 2, surf(8), "left"),
            (32, 54, 28, 14, 2, surf(8), "centre"),
            (32, 54, 28, 14, 2, surf(8), "topleft"),
            (32, 54, 28, 14, 2, P010, "left"),
            (2, 2, 14, 14, 2, surf(10), "left"),                    # yuv420p10le: a 1 x 1 chroma plane
            (15, 16, 28, 14, 2, surf(8, "422"), "left"),            # under transpose the 1,2 display subsampling
            (15, 17, 28, 14, 2, surf(10, "444"), "left"),
            (32, 48, 28, 14, 2, surf(8, "422", interleaved=True), "topleft")]     # nv16
SURFACE_IDS = ["%dx%d-%s%d%s-%s" % (c[0], c[1], c[5][3], c[5][1], ("msb" if c[5][2] else "") + ("-il" if c[5][4] else ""), c[6]) for c in SURFACES]
BIG = [(180, 320, 224, 14, 2, surf(10), "left"), (180, 320, 224, 14, 2, surf(8, interleaved=True), "left")]      # many tiles and staging chunks

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


def words(v, fmt):
    """Values (int64 tensor) -> the stored samples: uint8, or uint16 words with the value in the low or (msb) the high bits."""
    if fmt[0] == 1:
        return v.to(torch.uint8)
    return (v << (16 - fmt[1]) if fmt[2] else v).to(torch.int32).to(torch.uint16)


def dev_planes(n, H, W, fmt, flip=None):
    """(y, cb, cr) on the device in the format's layout: three contiguous planes, or cb / cr as the two halves of one interleaved [n,h,w,2] tensor.
    ``flip``: plane axes to reverse first (the copy a caller makes today)."""
    y, cb, cr = (torch.from_numpy(a.copy()) for a in oo.yuv_values(n, H, W, fmt[1], fmt[3]))
    if flip:
        y, cb, cr = (t.flip(flip).contiguous() for t in (y, cb, cr))
    if fmt[4]:
        pairs = words(torch.stack((cb, cr), -1), fmt).cuda()
        return words(y, fmt).cuda(), pairs[..., 0], pairs[..., 1]
    return tuple(words(t, fmt).cuda() for t in (y, cb, cr))


def surface_kw(fmt):
    return dict(depth=fmt[1], msb_aligned=fmt[2], subsampling=fmt[3])


def unfold(img, patch, kp):
    """[n,3,R,R] -> [n*g*g, kp]: rows (frame, gy, gx), columns (channel, py, px), zero-padded."""
    n, _, R, _ = img.shape
    g = R // patch
    p = img.reshape(n, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, 3 * patch * patch)
    return F.pad(p, (0, kp - p.shape[1]))


def bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def lib_error(flavour):
    from revisionllm_amd import hip
    buf = ctypes.create_string_buffer(512)
    hip.lib(flavour).rv_last_error(buf, 512)
    return buf.value.decode()


def check(patches, image, want, patch, dt, what, bound=oo.IMAGE_BOUND):
    """Image within the bound of the oracle, every pixel; patches = the image rounded once (the kernel's own image: bit for bit; the oracle's: within the
    bound and one rounding), pad columns +0."""
    n, _, R, _ = want.shape
    kp = (3 * patch * patch + 127) // 128 * 128
    assert tuple(image.shape) == (n, 3, R, R) and tuple(patches.shape) == (n * (R // patch) ** 2, kp)
    assert bool(torch.isfinite(image).all())
    err = float(np.abs(image.cpu().numpy().astype(np.float64) - want).max())
    print(f"{what}: image err {err:.3e} (bound {bound:.3e})")
    oo.log_err(ME, f"image {what}", err)
    assert err <= bound, (what, err, bound)
    assert torch.equal(bits(patches), bits(unfold(image.to(dt), patch, kp)))
    assert bool((bits(patches[:, 3 * patch * patch:]) == 0).all())                      # +0, not -0, not NaN
    wantp = unfold(torch.from_numpy(want.copy()), patch, kp)
    tol = bound + (wantp.abs() + bound) * HALF_ULP[dt] + 2.0 ** -25
    assert bool(((patches.cpu().double() - wantp).abs() <= tol).all())
    return image.cpu().numpy().astype(np.float64)


def run_surface(case, code, flav, planes=None, want=("patches", "image"), **more):
    from revisionllm_amd import hip, ops
    H, W, R, patch, n, fmt, loc = case
    planes = dev_planes(n, H, W, fmt) if planes is None else planes
    return ops.yuv_surface_to_patches(*planes, R=R, patch=patch, op_dtype=hip.op_dtype(flav), want=want, chroma_loc=loc, **surface_kw(fmt), **SPELL[code], **more)


def far_apart(results, what):
    """The results of the eight orientations differ pairwise by more than 100 x the bound."""
    codes = sorted(results)
    for i, a in enumerate(codes):
        for b in codes[i + 1:]:
            d = float(np.abs(results[a] - results[b]).max())
            assert d > 100 * oo.IMAGE_BOUND, (what, a, b, d)


# ---- 1: RGB ----
@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("geom", RGB_GEOMS, ids=["30x51", "7x5"])
def test_rgb_all_orientations_vs_oracle(flav, geom, layout):
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = geom
    dt = hip.op_dtype(flav)
    src = torch.from_numpy(oo.rgb_values(n, H, W).copy())
    src = (src if layout == "NCHW" else src.permute(0, 2, 3, 1).contiguous()).cuda()
    got = {}
    for code in oo.ORIENTS:
        p, i = ops.frames_to_patches(src, R, patch, layout=layout, op_dtype=dt, want=("patches", "image"), **SPELL[code])
        got[code] = check(p, i, oo.rgb_oracle64(n, H, W, R, code), patch, dt, f"rgb {H}x{W}->{R} {layout} orient {code} {flav}")
    far_apart(got, geom)                                                                # (5)


# ---- 2: surfaces ----
@pytest.mark.parametrize("case", SURFACES, ids=SURFACE_IDS)
def test_surfaces_all_orientations_vs_oracle(flav, case):
    from revisionllm_amd import hip
    H, W, R, patch, n, fmt, loc = case
    dt = hip.op_dtype(flav)
    planes = dev_planes(n, H, W, fmt)
    got = {}
    for code in oo.ORIENTS:
        p, i = run_surface(case, code, flav, planes)
        got[code] = check(p, i, oo.yuv_oracle64(n, H, W, R, fmt[1], fmt[3], code, loc=loc), patch, dt,
                          f"surface {SURFACE_IDS[SURFACES.index(case)]} orient {code} {flav}")
    if (H, W) != (2, 2):
        far_apart(got, case)                                                            # (5)


def test_yuv_to_patches_takes_the_orientation_too(flav):
    """The 8-bit 4:2:0 wrapper goes through the oriented surface entry: the bits of ops.yuv_surface_to_patches on the same planes."""
    from revisionllm_amd import hip, ops
    case = SURFACES[0]
    H, W, R, patch, n, fmt, loc = case
    planes = dev_planes(n, H, W, fmt)
    for code in (0, 3, 2, 5):
        a = ops.yuv_to_patches(*planes, R=R, patch=patch, chroma_loc="left", op_dtype=hip.op_dtype(flav), want=("patches", "image"), **SPELL[code])
        assert same_bits(a, run_surface(case, code, flav, planes)), code


# ---- 3: many tiles and staging chunks ----
@pytest.mark.parametrize("code", [3, 2], ids=["rotate90", "hflip"])
@pytest.mark.parametrize("case", BIG, ids=["yuv420p10le", "nv12"])
def test_many_tiles_and_staging_chunks(flav, case, code):
    from revisionllm_amd import hip
    H, W, R, patch, n, fmt, loc = case
    p, i = run_surface(case, code, flav)
    check(p, i, oo.yuv_oracle64(n, H, W, R, fmt[1], fmt[3], code, loc=loc), patch, hip.op_dtype(flav), f"big {H}x{W}->{R} {fmt[3]}{fmt[1]} orient {code} {flav}")


# ---- 4: HDR ----
@pytest.mark.parametrize("code", [3, 6], ids=["rotate90", "rotate180"])
@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_hdr_surfaces_vs_hdr_oracle(flav, transfer, code):
    import hdr_oracle as ho
    from revisionllm_amd import hip
    H, W, R, patch, n = 32, 54, 28, 14, 2
    case = (H, W, R, patch, n, P010, "topleft")
    p, i = run_surface(case, code, flav, matrix="bt2020", transfer=transfer)
    got = check(p, i, oo.hdr_oracle64(n, H, W, R, 10, "420", code, transfer), patch, hip.op_dtype(flav), f"hdr {transfer} orient {code} {flav}", bound=ho.image_bound())
    assert float(np.abs(got - oo.hdr_oracle64(n, H, W, R, 10, "420", 0, transfer)).max()) > 100 * oo.IMAGE_BOUND


# ---- 6: exact and near equivalences ----
def test_orient_zero_through_the_new_entries_is_the_existing_entries(flav):
    from revisionllm_amd import hip, ops
    dt = hip.op_dtype(flav)
    f3 = ctypes.c_float * 3
    H, W, R, patch, n = RGB_GEOMS[0]
    src = torch.from_numpy(oo.rgb_values(n, H, W).copy()).cuda()
    base = ops.frames_to_patches(src, R, patch, op_dtype=dt, want=("patches", "image"))
    p, i = torch.empty_like(base[0]), torch.empty_like(base[1])
    rc = hip.lib(flav).rv_frames_to_patches_oriented(hip.ptr(src), 0, 3 * H * W, W, n, H, W, 0, R, patch, f3(*oo.MEAN), f3(*oo.STD), hip.ptr(p), 640, hip.ptr(i),
                                                     hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, hip.last_error()
    assert same_bits((p, i), base)
    for case, hdr in ((SURFACES[3], None), (SURFACES[5], None), (SURFACES[3], hip.RvHdrMap(1, 1, 1000.0, 203.0))):
        H, W, R, patch, n, fmt, loc = case
        y, cb, cr = dev_planes(n, H, W, fmt)
        base = run_surface(case, 0, flav, (y, cb, cr), **(dict(transfer="pq", gamut=True) if hdr else {}))
        sb, cp = fmt[0], (2 if fmt[4] else 1)
        h, w = cb.shape[1:]
        s = hip.RvYuvSurface(y.data_ptr(), cb.data_ptr(), cr.data_ptr(), H * W * sb, W * sb, h * w * cp * sb, w * cp * sb, sb, fmt[1], int(fmt[2]), cp * sb,
                             *oo.SUB[fmt[3]], n, H, W, 0, 0, LOC_CODE[loc])
        p, i = torch.empty_like(base[0]), torch.empty_like(base[1])
        rc = hip.lib(flav).rv_yuv_surface_to_patches_oriented(ctypes.byref(s), ctypes.byref(hdr) if hdr else None, 0, R, patch, f3(*oo.MEAN), f3(*oo.STD),
                                                              hip.ptr(p), 640, hip.ptr(i), hip.stream())
        torch.cuda.synchronize()
        assert rc == 0, hip.last_error()
        assert same_bits((p, i), base)


@pytest.mark.parametrize("code,axes", [(2, (2,)), (4, (1,)), (6, (1, 2))], ids=["hflip", "vflip", "rotate180"])
def test_a_mirror_is_the_existing_entry_on_a_flipped_copy(flav, code, axes):
    """RGB, and centre-sited or 4:4:4 surfaces (no siting offset that would change side): the oriented call against what a caller does today - flip every
    plane, make it contiguous, call the existing entry - within 2 x the bound (both lie within one bound of the same oracle; the tap sums run in opposite
    orders, so bit equality is not claimed)."""
    from revisionllm_amd import hip, ops
    dt = hip.op_dtype(flav)
    H, W, R, patch, n = RGB_GEOMS[0]
    src = torch.from_numpy(oo.rgb_values(n, H, W).copy()).cuda()
    _, a = ops.frames_to_patches(src, R, patch, op_dtype=dt, want=("image",), **SPELL[code])
    _, b = ops.frames_to_patches(src.flip([x + 1 for x in axes]).contiguous(), R, patch, op_dtype=dt, want=("image",))
    d = float((a - b).abs().max())
    oo.log_err(ME, f"mirror-vs-flipped-copy rgb orient {code} {flav}", d)
    assert d <= 2 * oo.IMAGE_BOUND
    for case in (SURFACES[1], SURFACES[6]):
        Hs, Ws, _, _, ns, fmt, _ = case
        _, a = run_surface(case, code, flav, want=("image",))
        _, b = run_surface(case, 0, flav, dev_planes(ns, Hs, Ws, fmt, flip=list(axes)), want=("image",))
        d = float((a - b).abs().max())
        oo.log_err(ME, f"mirror-vs-flipped-copy {fmt[3]} orient {code} {flav}", d)
        assert d <= 2 * oo.IMAGE_BOUND


# ---- 7: a window of a larger surface ----
def test_a_window_of_a_larger_padded_p010_surface_under_rotate_270(flav):
    """A P010 window inside a larger surface (start 3 samples in, pitch W + 11 samples: no multiple of 16 bytes, padded frame stride, noise around it) through
    ctypes with orient 5 into outputs inside NaN-filled buffers with ldp > Kp: the bits of the contiguous planes; the columns behind Kp of every patch row
    and the guard bands around both outputs still hold their NaN; the pad columns are +0."""
    from revisionllm_amd import hip
    case = SURFACES[3]
    H, W, R, patch, n, fmt, loc = case
    dt = hip.op_dtype(flav)
    base_p, base_i = run_surface(case, 5, flav)
    y, cb, cr = (torch.from_numpy(a.copy()) for a in oo.yuv_values(n, H, W, fmt[1], fmt[3]))
    h, w = cb.shape[1:]
    pitch = W + 11
    fs = (H + h + 2) * pitch + 40                                                       # samples per frame of the big surface
    flat = torch.randint(0, 65536, (n * fs + 3,), dtype=torch.int32, generator=torch.Generator().manual_seed(7)).to(torch.uint16)
    flat.as_strided((n, H, W), (fs, pitch, 1), 3).copy_(words(y, fmt))
    flat.as_strided((n, h, w, 2), (fs, pitch, 2, 1), 3 + H * pitch).copy_(words(torch.stack((cb, cr), -1), fmt))
    dev = flat.cuda()
    at = dev.data_ptr() + 2 * 3
    assert at % 16 == 6 and (2 * pitch) % 16 != 0
    g, kp = R // patch, 640
    ldp, guard = kp + 24, 1024
    rows = n * g * g
    pbuf = torch.full((guard + rows * ldp + guard,), NAN_BITS, dtype=torch.int16, device="cuda").view(dt)
    ibuf = torch.full((guard + n * 3 * R * R + guard,), float("nan"), device="cuda")
    s = hip.RvYuvSurface(at, at + 2 * H * pitch, at + 2 * H * pitch + 2, 2 * fs, 2 * pitch, 2 * fs, 2 * pitch, 2, 10, 1, 4, 2, 2, n, H, W, 0, 0, LOC_CODE[loc])
    f3 = ctypes.c_float * 3
    rc = hip.lib(flav).rv_yuv_surface_to_patches_oriented(ctypes.byref(s), None, 5, R, patch, f3(*oo.MEAN), f3(*oo.STD), ctypes.c_void_p(pbuf.data_ptr() + 2 * guard),
                                                          ldp, ctypes.c_void_p(ibuf.data_ptr() + 4 * guard), hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, hip.last_error()
    prow = pbuf[guard:guard + rows * ldp].view(rows, ldp)
    assert torch.equal(bits(prow[:, :kp]), bits(base_p)) and torch.equal(bits(ibuf[guard:-guard].view(n, 3, R, R)), bits(base_i))
    assert bool((bits(prow[:, 3 * patch * patch:kp]) == 0).all())
    assert bool((bits(prow[:, kp:]) == NAN_BITS).all())
    assert bool((bits(pbuf[:guard]) == NAN_BITS).all()) and bool((bits(pbuf[-guard:]) == NAN_BITS).all())
    assert bool(torch.isnan(ibuf[:guard]).all()) and bool(torch.isnan(ibuf[-guard:]).all())


# ---- 8: batching and determinism ----
def test_batching_and_determinism(flav):
    """n = 5 equals five calls of n = 1, bit for bit; two runs give equal bits; n = 0 gives empty outputs - RGB and P010, rotate=90 and hflip."""
    from revisionllm_amd import hip, ops
    dt = hip.op_dtype(flav)
    case = (32, 54, 28, 14, 5, P010, "left")
    planes = dev_planes(5, 32, 54, P010)
    src = torch.from_numpy(oo.rgb_values(5, 30, 51).copy()).cuda()
    for code in (3, 2):
        calls = (lambda sl: run_surface(case, code, flav, tuple(t[sl] for t in planes)),
                 lambda sl: ops.frames_to_patches(src[sl], 28, 14, op_dtype=dt, want=("patches", "image"), **SPELL[code]))
        for call in calls:
            a = call(slice(None))
            assert same_bits(call(slice(None)), a)
            ones = [call(slice(k, k + 1)) for k in range(5)]
            assert torch.equal(bits(torch.cat([p for p, _ in ones])), bits(a[0])) and torch.equal(bits(torch.cat([i for _, i in ones])), bits(a[1]))
            p, i = call(slice(0, 0))
            assert tuple(p.shape) == (0, 640) and tuple(i.shape) == (0, 3, 28, 28)


# ---- 9: refusals ----
def raw_surface(flav, orient, over=None, null_struct=False, want_patches=True, want_image=True):
    """rv_yuv_surface_to_patches_oriented through ctypes on the sibling surface test's refusal surface (96 x 64 yuv420p10le) and NaN-filled outputs."""
    import test_gpu_yuv_surface_frontend as ys
    from revisionllm_amd import hip
    H, W, R, patch, n = ys.COLOUR_GEOM
    fmt = ys.REFUSAL_FMT
    y, cb, cr = dev_planes(n, H, W, fmt)
    if isinstance(over, str):
        k = over[:-2]
        over = {k: (y, cb, cr)["y cb cr".split().index(k)].data_ptr() + 1}
    dt = hip.op_dtype(flav)
    h, w = cb.shape[1:]
    a = dict(y=y.data_ptr(), cb=cb.data_ptr(), cr=cr.data_ptr(), y_frame_stride=H * W * 2, y_row_stride=W * 2, c_frame_stride=h * w * 2, c_row_stride=w * 2,
             sample_bytes=2, depth=10, msb_aligned=0, c_pix=2, sub_x=2, sub_y=2, n=n, H=H, W=W, matrix=0, full_range=0, chroma_loc=0, R=R, patch=patch, ldp=640)
    a.update(over or {})
    patches = torch.full((n * (R // patch) ** 2, 640), NAN_BITS, dtype=torch.int16, device="cuda").view(dt) if want_patches else None
    image = torch.full((n, 3, R, R), float("nan"), device="cuda") if want_image else None
    s = hip.RvYuvSurface(**{k: a[k] for k, _ in hip.RvYuvSurface._fields_})
    f3 = ctypes.c_float * 3
    rc = hip.lib(flav).rv_yuv_surface_to_patches_oriented(None if null_struct else ctypes.byref(s), None, orient, a["R"], a["patch"], f3(*oo.MEAN), f3(*oo.STD),
                                                          hip.ptr(patches), a["ldp"], hip.ptr(image), hip.stream())
    torch.cuda.synchronize()
    return rc, patches, image


def untouched(patches, image):
    return bool((bits(patches) == NAN_BITS).all()) and bool(torch.isnan(image).all())


def test_refusals_of_the_surface_entry(flav):
    """orient 8 and -1; every refusal of rv_yuv_surface_to_patches (the sibling test's list) reached through the oriented entry under rotate=90; a null struct;
    both outputs null: < 0, a message that names the new entry and the argument, and the NaN-filled outputs as they were."""
    import test_gpu_yuv_surface_frontend as ys
    name = "rv_yuv_surface_to_patches_oriented"
    for bad in (8, -1):
        rc, p, i = raw_surface(flav, bad)
        assert rc < 0 and lib_error(flav).startswith(name + ": orient") and untouched(p, i)
    for what, over, msg in ys.REFUSALS:
        rc, p, i = raw_surface(flav, 3, over)
        assert rc < 0, what
        assert lib_error(flav).startswith(name + ":") and msg in lib_error(flav), (what, lib_error(flav))
        assert untouched(p, i), what
    rc, p, i = raw_surface(flav, 3, null_struct=True)
    assert rc < 0 and lib_error(flav) == name + ": null surface" and untouched(p, i)
    rc, _, _ = raw_surface(flav, 3, want_patches=False, want_image=False)
    assert rc < 0 and "both outputs null" in lib_error(flav)
    rc, p, i = raw_surface(flav, 3)                                                     # ... and the same call without an override runs
    assert rc == 0 and not bool(torch.isnan(i).any())


def test_refusals_of_the_rgb_entry(flav):
    import test_gpu_frames_frontend as fr
    from revisionllm_amd import hip, ops
    name = "rv_frames_to_patches_oriented"
    H, W, R, patch, n = RGB_GEOMS[0]
    dt = hip.op_dtype(flav)
    src = torch.from_numpy(oo.rgb_values(n, H, W).copy()).cuda()
    f3 = ctypes.c_float * 3

    def raw(orient, over=None, outputs=True):
        a = dict(frames=hip.ptr(src), layout=0, fs=3 * H * W, rs=W, n=n, H=H, W=W, R=R, patch=patch, ldp=640)
        a.update(over or {})
        p = torch.full((n * (R // patch) ** 2, 640), NAN_BITS, dtype=torch.int16, device="cuda").view(dt)
        i = torch.full((n, 3, R, R), float("nan"), device="cuda")
        rc = hip.lib(flav).rv_frames_to_patches_oriented(a["frames"], a["layout"], a["fs"], a["rs"], a["n"], a["H"], a["W"], orient, a["R"], a["patch"], f3(*oo.MEAN),
                                                         f3(*oo.STD), hip.ptr(p) if outputs else None, a["ldp"], hip.ptr(i) if outputs else None, hip.stream())
        torch.cuda.synchronize()
        return rc, p, i

    for bad in (8, -1):
        rc, p, i = raw(bad)
        assert rc < 0 and lib_error(flav).startswith(name + ": orient") and untouched(p, i)
    for what, over, msg in fr.REFUSALS:
        rc, p, i = raw(3, over)
        assert rc < 0 and lib_error(flav).startswith(name + ":") and msg in lib_error(flav) and untouched(p, i), (what, lib_error(flav))
    rc, p, i = raw(3, outputs=False)
    assert rc < 0 and "both outputs null" in lib_error(flav) and untouched(p, i)
    with pytest.raises(ValueError, match="rotate"):
        ops.frames_to_patches(src, R, patch, rotate=45)


# ---- 10: end to end ----
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


def test_encode_video_pix_fmt_and_encode_video_under_rotate_90(flav, tiny_towers):
    """encode_video_pix_fmt(..., rotate=90) on p010le and encode_video(..., rotate=90) on uint8 NHWC chunks through the tiny towers: within the towers' 2e-2
    of the oracle towers fed the oriented float64 front end, further than that from rotate=0, the same bits however the frames are chunked; float frames at
    the towers' resolution refuse an orientation."""
    from oracle import clip_vit
    from revisionllm_amd import ops
    ex, w, c = tiny_towers
    n, H, W, R = 8, 46, 80, c["image_res"]
    y, cb, cr = (torch.from_numpy(a.copy()) for a in oo.yuv_values(n, H, W, 10, "420"))
    buf = words(torch.cat([y.reshape(n, -1), torch.stack((cb, cr), -1).reshape(n, -1)], 1), P010).contiguous().view(torch.uint8)
    assert tuple(buf.shape) == (n, ops.yuv_frame_bytes(H, W, "p010le"))
    ref = clip_vit.encode_image(torch.from_numpy(oo.yuv_oracle64(n, H, W, R, 10, "420", 3).copy()).float(), w)      # H < 720: BT.601, studio, left
    one = ex.encode_video_pix_fmt(buf.cuda(), H, W, "p010le", bsz=3, rotate=90)
    assert tuple(one.shape) == (n, c["embed_dim"])
    err = rel_err(one.cpu(), ref)
    oo.log_err(ME, f"tiny-towers-features p010le rotate=90 {H}x{W}->{R} {flav}", float(err))
    assert err < 2e-2
    assert torch.equal(bits(ex.encode_video_pix_fmt(iter([buf[:1], buf[1:6], buf[6:]]), H, W, "p010le", bsz=3, rotate=90)), bits(one))
    assert rel_err(ex.encode_video_pix_fmt(buf.cuda(), H, W, "p010le", bsz=3).cpu(), ref) > 2e-2
    planes, kw = ops.split_yuv(buf.cuda(), H, W, "p010le")
    assert rel_err(ex.clip_extractor.encode_surfaces_yuv(*planes, **kw, rotate=90).cpu(), ref) < 2e-2
    with pytest.raises(ValueError, match="rotate"):
        ex.encode_video_pix_fmt(buf, H, W, "p010le", rotate=30)
    # decoded uint8 frames
    n, H, W = 5, 45, 80
    nhwc = torch.from_numpy(oo.rgb_values(n, H, W).copy()).permute(0, 2, 3, 1).contiguous()
    ref = clip_vit.encode_image(torch.from_numpy(oo.rgb_oracle64(n, H, W, R, 3).copy()).float(), w)
    one = ex.encode_video(nhwc.cuda(), bsz=2, rotate=90)
    err = rel_err(one.cpu(), ref)
    oo.log_err(ME, f"tiny-towers-features rgb rotate=90 {H}x{W}->{R} {flav}", float(err))
    assert err < 2e-2
    assert torch.equal(bits(ex.encode_video(iter([nhwc[:2], nhwc[2:]]), bsz=2, rotate=90)), bits(one))
    assert rel_err(ex.encode_video(nhwc.cuda(), bsz=2).cpu(), ref) > 2e-2
    assert torch.equal(bits(ex.clip_extractor.encode_frames(nhwc.cuda(), rotate=90)), bits(ex.encode_video(nhwc.cuda(), bsz=5, rotate=90)))
    # 8-bit 4:2:0 through encode_video_yuv
    y8, cb8, cr8 = (torch.from_numpy(a.copy()).to(torch.uint8) for a in oo.yuv_values(4, 46, 80, 8, "420"))
    nv12 = torch.cat([y8.reshape(4, -1), torch.stack((cb8, cr8), -1).reshape(4, -1)], 1).view(4, 46 * 3 // 2, 80)
    ref = clip_vit.encode_image(torch.from_numpy(oo.yuv_oracle64(4, 46, 80, R, 8, "420", 2).copy()).float(), w)
    assert rel_err(ex.encode_video_yuv(nv12, 46, 80, "nv12", bsz=3, hflip=True).cpu(), ref) < 2e-2
    # frames that are past the front end
    native = torch.zeros(2, 3, R, R)
    with pytest.raises(ValueError, match="past the front end"):
        ex.encode_video(native, rotate=90)
    with pytest.raises(ValueError, match="past the front end"):
        ex.encode_video(native, hflip=True)
    assert tuple(ex.encode_video(native.to(torch.uint8), rotate=180).shape) == (2, c["embed_dim"])      # uint8 frames of that size are decoded frames
