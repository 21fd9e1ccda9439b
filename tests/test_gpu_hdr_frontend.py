"""rv_yuv_surface_to_patches_hdr (an HDR surface -> the surface front end's resampling and colour matrix -> PQ / HLG to display light -> BT.2390 tone mapping ->
BT.2020 to BT.709 primaries -> BT.709 OETF -> normalise -> conv1 patch matrix, one kernel) and the layers above it (ops.yuv_surface_to_patches(transfer=...),
ClipTowers.encode_surfaces_yuv, ClipFeatureExtractor.encode_video_pix_fmt) against the float64 oracle of tests/hdr_oracle.py: the definition in
include/revision_hip.h written out in NumPy.

Inputs: uniform integer noise over the whole of [0, 2^depth) (resampled values leave the code range and colours the RGB cube: both clamps work), and one
smooth ramp frame whose luma runs from code 0 to the code of peak_nits.  Every pixel is compared, none excluded.

Image bound (hdr_oracle.image_bound): the float32 transcription of the HDR steps is 2.7e-4 away from the float64 oracle on these inputs (``f32_model``,
tests/test_hdr_host_logic.py measures and logs it), which is not below a quarter of the SDR front end's 2e-4, so the bound is four times the model: about
1.1e-3 in normalised units.  Patches: the image rounded once to the operand type (bit for bit against the kernel's own image, and within the image bound plus
half a unit in the last place of the oracle's).  End to end through the tiny towers: the SDR tests' 2e-2.  Equivalences are compared by bits.
RV_LOG_ERR=<file>: the bound and the measured maxima are appended there (profiles/hdr_frontend_err.log holds one such run)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hdr_oracle as ho
from helpers import SEED, T, rel_err

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FFF            # a NaN in fp16 and in bf16
HDR_COLOUR = dict(matrix="bt2020", full_range=False, chroma_loc="topleft")
HALF_ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}     # relative rounding error of one conversion (11 / 8 significant bits)

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")


@pytest.fixture(scope="module", params=[None] if _FORCED else ["f16", "bf16"])
def flav(request, op_flavour):
    """Both operand flavours, as the surface test runs them (REVISION_TEST_FLAVOURS narrows it)."""
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import hip
    f = request.param or op_flavour or hip.flavour()
    prev = hip.set_flavour(f)
    yield f
    hip.set_flavour(prev)


def words(v, fmt):
    """Values (int64 tensor) -> the stored 16-bit words, the value in the low or (msb) the high bits."""
    return (v << (16 - fmt[1]) if fmt[2] else v).to(torch.int32).to(torch.uint16)


def dev_planes(n, H, W, fmt, kind="noise"):
    """(y, cb, cr) on the device in the format's layout: three contiguous planes, or cb / cr as the two halves of one interleaved [n,h,w,2] tensor."""
    y, cb, cr = (torch.from_numpy(a.copy()) for a in ho.values(n, H, W, fmt[1], fmt[3], kind))
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


def run(case, flav, want=("patches", "image"), planes=None):
    from revisionllm_amd import hip, ops
    (H, W, R, patch, n, fmt), kind, transfer, gamut, peak, white = case
    planes = dev_planes(n, H, W, fmt, kind) if planes is None else planes
    return ops.yuv_surface_to_patches(*planes, R=R, patch=patch, op_dtype=hip.op_dtype(flav), want=want, transfer=transfer, gamut=bool(gamut), peak_nits=peak,
                                      sdr_white_nits=white, **HDR_COLOUR, **surface_kw(fmt))


def check_against_oracle(case, flav, what):
    """Image within the bound of the oracle, every pixel; patches = the image rounded once (the kernel's own image: bit for bit; the oracle's: within the image
    bound and one rounding), pad columns +0."""
    from revisionllm_amd import hip
    (H, W, R, patch, n, fmt) = case[0]
    dt = hip.op_dtype(flav)
    kp = (3 * patch * patch + 127) // 128 * 128
    patches, image = run(case, flav)
    assert tuple(image.shape) == (n, 3, R, R) and tuple(patches.shape) == (n * (R // patch) ** 2, kp)
    assert bool(torch.isfinite(image).all())
    want = ho.case_oracle(case)
    bound = ho.image_bound()
    err = float(np.abs(image.cpu().numpy().astype(np.float64) - want).max())
    print(f"{what} {flav}: image err {err:.3e} (bound {bound:.3e})")
    ho.log_err("test_gpu_hdr_frontend.py", f"image {what} {flav}", err)
    assert err <= bound, (what, err, bound)
    assert torch.equal(bits(patches), bits(unfold(image.to(dt), patch, kp)))
    assert bool((bits(patches[:, 3 * patch * patch:]) == 0).all())                      # +0, not -0, not NaN
    wantp = unfold(torch.from_numpy(want.copy()), patch, kp)
    tol = bound + (wantp.abs() + bound) * HALF_ULP[dt] + 2.0 ** -25
    assert bool(((patches.cpu().double() - wantp).abs() <= tol).all())
    return image


def test_the_bound_is_derived_from_the_f32_model():
    m, bound = ho.f32_model(), ho.image_bound()
    ho.log_err("test_gpu_hdr_frontend.py", "f32_model", m)
    ho.log_err("test_gpu_hdr_frontend.py", "image_bound", bound)
    assert bound == (ho.SDR_IMAGE_BOUND if m < ho.SDR_IMAGE_BOUND / 4 else 4 * m)


@pytest.mark.parametrize("gamut", [1, 0], ids=["to709", "nogamut"])
@pytest.mark.parametrize("transfer", ["pq", "hlg"])
@pytest.mark.parametrize("geom", ho.GEOMS, ids=ho.GEOM_IDS)
def test_image_and_patches_vs_oracle(flav, geom, transfer, gamut):
    img = check_against_oracle((geom, "noise", transfer, gamut, 1000.0, 203.0), flav, f"{ho.GEOM_IDS[ho.GEOMS.index(geom)]} {transfer} gamut{gamut}")
    # the HDR steps did something: far from the SDR entry on the same bytes, and inside the range of a BT.709-coded value
    from revisionllm_amd import hip, ops
    H, W, R, patch, n, fmt = geom
    _, sdr = ops.yuv_surface_to_patches(*dev_planes(n, H, W, fmt), R=R, patch=patch, op_dtype=hip.op_dtype(flav), want=("image",), **HDR_COLOUR, **surface_kw(fmt))
    assert float((img - sdr).abs().max()) > 0.1
    lo, hi = ((v - np.array(ho.MEAN)) / (np.array(ho.STD) + 1e-8) for v in (0.0, 1.0))
    for c in range(3):
        assert float(img[:, c].min()) >= lo[c] - 1e-5 and float(img[:, c].max()) <= hi[c] + 1e-5


@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_a_smooth_ramp_from_code_0_to_the_code_of_the_peak(flav, transfer):
    img = check_against_oracle((ho.RAMP_GEOM, "ramp-" + transfer, transfer, 1, 1000.0, 203.0), flav, f"ramp {transfer}")
    assert abs(float(img[:, 1].min()) - (0.0 - ho.MEAN[1]) / (ho.STD[1] + 1e-8)) < 1e-5                   # code 0 is below black: clamped to it


@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_peak_and_sdr_white_levels_vs_oracle(flav, transfer):
    """peak_nits 400 / 1000 / 4000 x sdr_white_nits 100 / 203 on the P010 geometry; every pair gives another picture."""
    got = {}
    for peak, white in ho.LEVELS:
        got[peak, white] = check_against_oracle((ho.LEVELS_GEOM, "noise", transfer, 1, peak, white), flav, f"levels {transfer} {peak:g}/{white:g}")
    keys = list(got)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert float((got[a] - got[b]).abs().max()) > 100 * ho.SDR_IMAGE_BOUND, (a, b)


def test_aliases_defaults_and_the_sdr_entry_is_untouched(flav):
    """ffmpeg's color_trc names are the short ones; gamut=None follows the matrix; transfer=None is the SDR entry bit for bit whatever the other three say."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n, fmt = ho.GEOMS[1]
    planes = dev_planes(n, H, W, fmt)
    kw = dict(R=R, patch=patch, op_dtype=hip.op_dtype(flav), want=("patches", "image"), **surface_kw(fmt))
    for short, long in (("pq", "smpte2084"), ("hlg", "arib-std-b67")):
        a = ops.yuv_surface_to_patches(*planes, transfer=short, **HDR_COLOUR, **kw)
        assert same_bits(ops.yuv_surface_to_patches(*planes, transfer=long, gamut=True, peak_nits=1000.0, sdr_white_nits=203.0, **HDR_COLOUR, **kw), a)
        b = ops.yuv_surface_to_patches(*planes, transfer=short, matrix="bt709", **kw)
        assert same_bits(ops.yuv_surface_to_patches(*planes, transfer=short, matrix="bt709", gamut=False, **kw), b)
        assert not same_bits(ops.yuv_surface_to_patches(*planes, transfer=short, matrix="bt709", gamut=True, **kw), b)
    sdr = ops.yuv_surface_to_patches(*planes, **HDR_COLOUR, **kw)
    assert same_bits(ops.yuv_surface_to_patches(*planes, transfer=None, peak_nits=4000.0, sdr_white_nits=100.0, gamut=True, **HDR_COLOUR, **kw), sdr)
    with pytest.raises(ValueError, match="transfer"):
        ops.yuv_surface_to_patches(*planes, transfer="bt709", **HDR_COLOUR, **kw)
    with pytest.raises(hip.HipLibraryError, match="peak_nits"):
        ops.yuv_surface_to_patches(*planes, transfer="pq", peak_nits=20000.0, **HDR_COLOUR, **kw)


@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_a_window_of_a_larger_p010_surface_and_nothing_outside_the_outputs_is_touched(flav, transfer):
    """A P010 window inside a larger surface (start 3 samples in, pitch W + 11 samples = 122 bytes: no multiple of 16, padded frame stride, noise around it)
    through ctypes into outputs that sit inside NaN-filled buffers: the bits of the contiguous planes, and every element around the outputs - the columns
    behind Kp of each patch row, the guard bands in front of and behind both outputs - still holds its NaN."""
    from revisionllm_amd import hip
    H, W, R, patch, n, fmt = ho.GEOMS[1]
    dt = hip.op_dtype(flav)
    case = (ho.GEOMS[1], "noise", transfer, 1, 1000.0, 203.0)
    base_p, base_i = run(case, flav)
    y, cb, cr = (torch.from_numpy(a.copy()) for a in ho.values(n, H, W, fmt[1], fmt[3]))
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
    s = hip.RvYuvSurface(at, at + 2 * H * pitch, at + 2 * H * pitch + 2, 2 * fs, 2 * pitch, 2 * fs, 2 * pitch, 2, 10, 1, 4, 2, 2, n, H, W, 2, 0, 2)
    m = hip.RvHdrMap(ho.TRANSFER_CODE[transfer], 1, 1000.0, 203.0)
    f3 = ctypes.c_float * 3
    rc = hip.lib(flav).rv_yuv_surface_to_patches_hdr(ctypes.byref(s), ctypes.byref(m), R, patch, f3(*ho.MEAN), f3(*ho.STD),
                                                     ctypes.c_void_p(pbuf.data_ptr() + 2 * guard), ldp, ctypes.c_void_p(ibuf.data_ptr() + 4 * guard), hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, hip.last_error()
    prow = pbuf[guard:guard + rows * ldp].view(rows, ldp)
    assert torch.equal(bits(prow[:, :kp]), bits(base_p)) and torch.equal(bits(ibuf[guard:-guard].view(n, 3, R, R)), bits(base_i))
    assert bool((bits(prow[:, kp:]) == NAN_BITS).all())
    assert bool((bits(pbuf[:guard]) == NAN_BITS).all()) and bool((bits(pbuf[-guard:]) == NAN_BITS).all())
    assert bool(torch.isnan(ibuf[:guard]).all()) and bool(torch.isnan(ibuf[-guard:]).all())
    # a refusal leaves everything as it was
    pbuf.view(torch.int16).fill_(NAN_BITS)
    m.peak_nits = float("nan")
    rc = hip.lib(flav).rv_yuv_surface_to_patches_hdr(ctypes.byref(s), ctypes.byref(m), R, patch, f3(*ho.MEAN), f3(*ho.STD),
                                                     ctypes.c_void_p(pbuf.data_ptr() + 2 * guard), ldp, None, hip.stream())
    torch.cuda.synchronize()
    assert rc < 0 and bool((bits(pbuf) == NAN_BITS).all())


@pytest.mark.parametrize("transfer", ["pq", "hlg"])
def test_batching_and_determinism(flav, transfer):
    """n = 3 equals three calls of n = 1, bit for bit; two runs give equal bits; n = 0 gives empty outputs."""
    case = ((96, 64, 28, 14, 3, ho.GEOMS[2][5]), "noise", transfer, 1, 1000.0, 203.0)
    planes = dev_planes(3, 96, 64, case[0][5])
    a = run(case, flav, planes=planes)
    assert same_bits(run(case, flav, planes=planes), a)
    ones = [run(case, flav, planes=tuple(t[i:i + 1] for t in planes)) for i in range(3)]
    assert torch.equal(bits(torch.cat([p for p, _ in ones])), bits(a[0])) and torch.equal(bits(torch.cat([i for _, i in ones])), bits(a[1]))
    p, i = run(case, flav, planes=tuple(t[:0] for t in planes))
    assert tuple(p.shape) == (0, 640) and tuple(i.shape) == (0, 3, 28, 28)


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


def test_encode_video_pix_fmt_on_pq_p010(flav, tiny_towers):
    """encode_video_pix_fmt(pix_fmt="p010le", transfer="pq") - the HDR10 defaults: BT.2020, top-left siting, peak 1000, white 203, BT.709 primaries - within the
    towers' bound (2e-2, the SDR end-to-end tests') of the oracle towers fed the float64 HDR oracle's image; chunks regrouped by bsz give the same bits; it is
    not the SDR call, and encode_surfaces_yuv on the split planes is the same thing."""
    from oracle import clip_vit
    from revisionllm_amd import ops
    ex, w, c = tiny_towers
    n, H, W, R = 8, 46, 80, c["image_res"]
    fmt = ho.GEOMS[1][5]
    y, cb, cr = (torch.from_numpy(a.copy()) for a in ho.values(n, H, W, 10, "420"))
    buf = words(torch.cat([y.reshape(n, -1), torch.stack((cb, cr), -1).reshape(n, -1)], 1), fmt).contiguous().view(torch.uint8)
    assert tuple(buf.shape) == (n, ops.yuv_frame_bytes(H, W, "p010le"))
    ref = clip_vit.encode_image(torch.from_numpy(ho.oracle64(n, H, W, R, 10, "420", "noise", "pq", 1).copy()).float(), w)
    one = ex.encode_video_pix_fmt(buf.cuda(), H, W, "p010le", bsz=3, transfer="pq")
    assert tuple(one.shape) == (n, c["embed_dim"])
    err = rel_err(one.cpu(), ref)
    ho.log_err("test_gpu_hdr_frontend.py", f"tiny-towers-features p010le pq {H}x{W}->{R} {flav}", float(err))
    assert err < 2e-2
    chunks = ex.encode_video_pix_fmt(iter([buf[:1], buf[1:6], buf[6:]]), H, W, "p010le", bsz=3, transfer="smpte2084")
    assert torch.equal(bits(chunks), bits(one))
    planes, kw = ops.split_yuv(buf.cuda(), H, W, "p010le")
    got = ex.clip_extractor.encode_surfaces_yuv(*planes, **kw, **HDR_COLOUR, transfer="pq")
    assert rel_err(got.cpu(), ref) < 2e-2
    sdr = ex.encode_video_pix_fmt(buf.cuda(), H, W, "p010le", bsz=3, matrix="bt2020")
    assert rel_err(sdr.cpu(), ref) > 2e-2
