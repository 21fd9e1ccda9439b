"""rv_frames_to_patches (decoded uint8 frames -> antialiased bicubic resize -> centre crop -> normalise -> conv1 patch matrix) and the layers above it
(ops.frames_to_patches, ClipTowers.encode_frames, ClipFeatureExtractor.encode_video on decoded frames) against an oracle kept in this file:
torch's own ``F.interpolate(mode="bicubic", align_corners=False, antialias=True)`` on the CPU in float64, then crop and normalise in float64.

Frames are uniform uint8 noise with a fixed seed: the hardest input for a resampler, and one whose resampled values leave 0..255, so a clamp or a uint8
intermediate would be caught.  R = 28, patch = 14 (K = 588 -> Kp = 640: the pad columns exist) unless a case says otherwise.

Bounds.  image vs oracle: 2e-4 in normalised units - torch's f32 path of the same call sits 3.7e-3 grey levels (5.6e-5 normalised) from its float64 path at
360 x 640 -> 224; 2e-4 leaves ~4 x for another summation order.  patches vs oracle: that plus half an ulp of the operand type (2^-11 / 2^-8 relative).
RV_LOG_ERR=<file>: the measured maxima per case are appended there (profiles/frames_frontend_err.log holds one such run)."""
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
HALF_ULP = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
NAN_BITS = 0x7FFF            # a NaN in fp16 and in bf16

#        H    W    R   patch n
CASES = [(45, 80, 28, 14, 3),        # landscape, downscale ~1.6: antialias taps
         (80, 45, 28, 14, 3),        # portrait
         (28, 28, 28, 14, 3),        # identity
         (20, 33, 28, 14, 3),        # upscale: support stays 2
         (56, 106, 28, 14, 3),       # resized width 53, (53 - 28) / 2 = 12.5 -> left 12 (half to even)
         (29, 57, 28, 14, 3),        # resized width int(28 * 57 / 29) = 55 (truncated), left = round(13.5) = 14
         (261, 470, 28, 14, 3),      # scale 9.3, ~38 taps per axis
         (40, 70, 32, 16, 3),        # K = 768 = Kp: no pad columns; ldp > Kp with a sentinel behind every row
         (360, 640, 224, 14, 2)]     # ViT-L/14's own geometry
IDS = ["%dx%d-R%d" % c[:3] for c in CASES]
SMALL = CASES[0]

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


# ---- inputs and the float64 oracle (computed once per geometry, shared, never modified) ----
@functools.lru_cache(maxsize=None)
def frames_u8(n, H, W):
    """uint8 noise [n,3,H,W] (CPU)."""
    return torch.randint(0, 256, (n, 3, H, W), generator=torch.Generator().manual_seed(SEED + 1000 * H + W), dtype=torch.uint8)


def resized_size(H, W, R):
    """torchvision's Resize(int): shorter side -> R, longer side -> int(R * long / short)."""
    return (R, int(R * W / H)) if H <= W else (int(R * H / W), R)


def crop_offsets(hr, wr, R):
    """CenterCrop: Python's round (half to even)."""
    return int(round((hr - R) / 2.0)), int(round((wr - R) / 2.0))


@functools.lru_cache(maxsize=None)
def oracle64(n, H, W, R):
    """float64 [n,3,R,R]: resize (antialiased bicubic), centre crop, (v / 255 - mean) / (std + 1e-8)."""
    hr, wr = resized_size(H, W, R)
    y = F.interpolate(frames_u8(n, H, W).double(), size=(hr, wr), mode="bicubic", align_corners=False, antialias=True)
    top, left = crop_offsets(hr, wr, R)
    y = y[:, :, top:top + R, left:left + R]
    mean = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    return ((y / 255.0 - mean) / (std + 1e-8)).contiguous()


def unfold(img, patch, kp):
    """[n,3,R,R] -> [n*g*g, kp]: rows (frame, gy, gx), columns (channel, py, px), zero-padded - ClipTowers.encode_image's own unfold + pad."""
    n, _, R, _ = img.shape
    g = R // patch
    p = img.reshape(n, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, 3 * patch * patch)
    return F.pad(p, (0, kp - p.shape[1]))


def bits(t):
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous().view(torch.int32)


def log_err(what, value):
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            fh.write(f"test_gpu_frames_frontend.py {what} {value:.3e}\n")


def lib_error(flavour):
    """The last error message of ONE flavour's library (hip.last_error joins those of every loaded library)."""
    from revisionllm_amd import hip
    buf = ctypes.create_string_buffer(512)
    hip.lib(flavour).rv_last_error(buf, 512)
    return buf.value.decode()


def raw_call(frames, layout, R, patch, flavour, ldp=None, want_patches=True, want_image=True, mean=MEAN, std=STD, over=None):
    """rv_frames_to_patches through ctypes on buffers of this test's making: patches pre-filled with NaN bit patterns, image with NaN.
    ``frames``: a device tensor (strides taken from it) or None.  ``over``: arguments to override (the refusal cases).
    -> (status, patches [rows, ldp] or None, image or None)."""
    from revisionllm_amd import hip
    dt = hip.op_dtype(flavour)
    if layout == 0:
        n, _, H, W = frames.shape
        fs, rs = 3 * frames.stride(1), frames.stride(2)
    else:
        n, H, W, _ = frames.shape
        fs, rs = frames.stride(0), frames.stride(1)
    g, kp = R // patch, (3 * patch * patch + 127) // 128 * 128
    ldp = kp if ldp is None else ldp
    patches = torch.full((n * g * g, max(ldp, 1)), NAN_BITS, dtype=torch.int16, device="cuda").view(dt) if want_patches else None
    image = torch.full((n, 3, R, R), float("nan"), device="cuda") if want_image else None
    f3 = ctypes.c_float * 3
    a = dict(frames=hip.ptr(frames), layout=layout, fs=fs, rs=rs, n=n, H=H, W=W, R=R, patch=patch, ldp=ldp)
    a.update(over or {})
    rc = hip.lib(flavour).rv_frames_to_patches(a["frames"], a["layout"], a["fs"], a["rs"], a["n"], a["H"], a["W"], a["R"], a["patch"], f3(*mean), f3(*std),
                                               hip.ptr(patches), a["ldp"], hip.ptr(image), hip.stream())
    torch.cuda.synchronize()
    return rc, patches, image


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_image_and_patches_vs_oracle(flav, case):
    """(1) image within 2e-4 of the float64 oracle; (2) patches = image rounded once, unfolded and zero-padded, bit for bit - pad columns zero in a buffer
    that held NaN patterns, columns behind Kp untouched; the identity geometry reproduces the f32 normalisation of the source to 1 ulp."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = case
    dt = hip.op_dtype(flav)
    kp = (3 * patch * patch + 127) // 128 * 128
    ldp = kp + 8 if 3 * patch * patch == kp else kp
    src = frames_u8(n, H, W).cuda()
    rc, patches, image = raw_call(src, 0, R, patch, flav, ldp=ldp)
    assert rc == 0, hip.last_error()
    want = oracle64(n, H, W, R)
    err = float((image.cpu().double() - want).abs().max())
    log_err(f"image {H}x{W}->{R} {flav}", err)
    assert err <= IMAGE_BOUND, err
    # patches: the same f32 value rounded once to the operand type
    expect = unfold(image.to(dt), patch, kp)
    assert torch.equal(bits(patches[:, :kp]), bits(expect))
    if kp > 3 * patch * patch:
        assert bool((bits(patches[:, 3 * patch * patch:kp]) == 0).all())             # +0, not -0, not NaN
    if ldp > kp:
        assert bool((bits(patches[:, kp:]) == NAN_BITS).all())                       # the sentinel behind every row is untouched
    w64 = unfold(want, patch, kp)
    perr = (patches[:, :kp].cpu().double() - w64).abs() - w64.abs() * HALF_ULP[flav]
    log_err(f"patches-minus-half-ulp {H}x{W}->{R} {flav}", float(perr.max()))
    assert float(perr.max()) <= IMAGE_BOUND
    if (H, W) == (R, R):
        x = frames_u8(n, H, W).float() / 255.0
        ref = ((x - torch.tensor(MEAN).view(1, 3, 1, 1)) / (torch.tensor(STD).view(1, 3, 1, 1) + 1e-8)).numpy()
        assert bool((np.abs(image.cpu().numpy() - ref) <= np.spacing(np.abs(ref))).all())
    # the wrapper allocates its own outputs and returns the same bits
    p2, i2 = ops.frames_to_patches(src, R, patch, op_dtype=dt, want=("patches", "image"))
    assert torch.equal(bits(p2), bits(patches[:, :kp])) and torch.equal(bits(i2), bits(image))
    p3, i3 = ops.frames_to_patches(src, R, patch, op_dtype=dt)
    assert i3 is None and torch.equal(bits(p3), bits(p2))


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[6]], ids=[IDS[0], IDS[4], IDS[6]])      # even widths: W + 5 is odd
def test_layout_and_stride_independence(flav, case):
    """(3) NHWC and NCHW of the same frames, a window of a larger buffer (7 rows and 5 columns more: an odd row stride, so no row segment is 16-byte
    aligned like its neighbour) and its contiguous copy, one frame alone and the same frame among three: the same bits."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = case
    dt = hip.op_dtype(flav)
    src = frames_u8(n, H, W).cuda()
    want = ("patches", "image")
    p0, i0 = ops.frames_to_patches(src, R, patch, op_dtype=dt, want=want)
    nhwc = src.permute(0, 2, 3, 1).contiguous()
    p1, i1 = ops.frames_to_patches(nhwc, R, patch, layout="NHWC", op_dtype=dt, want=want)
    assert torch.equal(bits(p1), bits(p0)) and torch.equal(bits(i1), bits(i0))
    big = torch.randint(0, 256, (n, 3, H + 7, W + 5), dtype=torch.uint8, generator=torch.Generator().manual_seed(7)).cuda()
    big[:, :, 2:2 + H, 3:3 + W] = src
    view = big[:, :, 2:2 + H, 3:3 + W]
    assert not view.is_contiguous() and view.stride(2) % 2 == 1
    p2, i2 = ops.frames_to_patches(view, R, patch, op_dtype=dt, want=want)
    assert torch.equal(bits(p2), bits(p0)) and torch.equal(bits(i2), bits(i0))
    big_l = torch.randint(0, 256, (n, H + 7, W + 5, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(8)).cuda()
    big_l[:, 2:2 + H, 3:3 + W] = nhwc
    view_l = big_l[:, 2:2 + H, 3:3 + W]
    assert not view_l.is_contiguous() and view_l.stride(1) % 2 == 1
    p3, i3 = ops.frames_to_patches(view_l, R, patch, layout="NHWC", op_dtype=dt, want=want)
    assert torch.equal(bits(p3), bits(p0)) and torch.equal(bits(i3), bits(i0))
    g2 = (R // patch) ** 2
    for layout, t in (("NCHW", src), ("NHWC", nhwc)):
        p4, i4 = ops.frames_to_patches(t[1:2], R, patch, layout=layout, op_dtype=dt, want=want)
        assert torch.equal(bits(p4), bits(p0[g2:2 * g2])) and torch.equal(bits(i4), bits(i0[1:2]))


def test_repeatable_and_empty(flav):
    """(4) two launches give the same bits; n = 0 gives empty outputs and launches nothing."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = CASES[6]
    dt = hip.op_dtype(flav)
    src = frames_u8(n, H, W).cuda()
    a = ops.frames_to_patches(src, R, patch, op_dtype=dt, want=("patches", "image"))
    b = ops.frames_to_patches(src, R, patch, op_dtype=dt, want=("patches", "image"))
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    p, i = ops.frames_to_patches(src[:0], R, patch, op_dtype=dt, want=("patches", "image"))
    assert tuple(p.shape) == (0, 640) and tuple(i.shape) == (0, 3, R, R)
    assert hip.lib(flav).rv_frames_to_patches(None, 1, 0, 0, 0, H, W, R, patch, (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD), None, 0, None, None) == 0


REFUSALS = [("R not a multiple of patch", dict(R=30), "multiple"),
            ("H = 0", dict(H=0), "frame size"),
            ("W = 8193", dict(W=8193), "frame size"),
            ("H = 8193", dict(H=8193), "frame size"),
            ("null frames", dict(frames=None), "null frames"),
            ("ldp < Kp", dict(ldp=639), "ldp"),
            ("layout 2", dict(layout=2), "layout"),
            ("layout -1", dict(layout=-1), "layout")]


@pytest.mark.parametrize("what,over,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(flav, what, over, msg):
    """(5) every refusal returns < 0 with a message, before any launch: the NaN-filled outputs stay as they were."""
    H, W, R, patch, n = SMALL
    rc, patches, image = raw_call(frames_u8(n, H, W).cuda(), 0, R, patch, flav, over=over)
    assert rc < 0
    assert lib_error(flav).startswith("rv_frames_to_patches") and msg in lib_error(flav), lib_error(flav)
    assert bool((bits(patches) == NAN_BITS).all()) and bool(torch.isnan(image).all())


def test_refuses_both_outputs_null_and_foreign_tensors(flav):
    """(5) both outputs null is refused; the wrapper refuses CPU tensors and anything but uint8."""
    from revisionllm_amd import hip, ops
    H, W, R, patch, n = SMALL
    src = frames_u8(n, H, W)
    rc, _, _ = raw_call(src.cuda(), 0, R, patch, flav, want_patches=False, want_image=False)
    assert rc < 0 and "both outputs null" in lib_error(flav)
    with pytest.raises(hip.HipLibraryError):
        ops.frames_to_patches(src, R, patch)
    with pytest.raises(hip.HipLibraryError):
        ops.frames_to_patches(src.cuda().float(), R, patch)
    with pytest.raises(ValueError):
        ops.frames_to_patches(torch.zeros(2, 3, 40, 3, dtype=torch.uint8, device="cuda"), R, patch)       # NCHW or NHWC?
    with pytest.raises(hip.HipLibraryError):
        ops.frames_to_patches(src.cuda(), 30, patch)


@pytest.fixture(scope="module")
def tiny_towers(flav):
    """The tiny CLIP of test_clip_towers_vs_reference_golden_and_oracle (utils/synth.py) and the oracle's weights."""
    from revisionllm_amd.data.clip_extractor import ClipFeatureExtractor
    from revisionllm_amd.data.clip_model import ClipTowers
    from revisionllm_amd.utils import synth
    c = synth.CLIP_TINY
    m = ClipTowers(**c, t_heads=synth.CLIP_TINY_TEXT_HEADS, op_dtype=flav).init_synthetic(seed=SEED)
    w = {k[len("clip."):]: T(v) for k, v in synth.build_numpy(synth.clip_towers_spec(**c), SEED, prefix="clip.").items()}
    return ClipFeatureExtractor(m), w, c


def test_encode_video_on_decoded_frames(flav, tiny_towers):
    """(6) uint8 NHWC frames of another size through encode_video, bsz = 2 (batches 2 + 2 + 1), as one tensor and as chunks of 2 / 3 frames: within the
    towers' bound of the oracle towers fed this file's float64 front end, and the same bits either way."""
    from oracle import clip_vit
    ex, w, c = tiny_towers
    n, H, W, R = 5, 45, 80, c["image_res"]
    nhwc = frames_u8(n, H, W).permute(0, 2, 3, 1).contiguous()
    ref = clip_vit.encode_image(oracle64(n, H, W, R).float(), w)
    one = ex.encode_video(nhwc.cuda(), bsz=2)
    assert tuple(one.shape) == (n, c["embed_dim"])
    assert rel_err(one.cpu(), ref) < 2e-2
    chunks = ex.encode_video(iter([nhwc[:2], nhwc[2:]]), bsz=2)               # CPU chunks, as a decoder hands them over
    assert torch.equal(bits(chunks), bits(one))
    nchw = ex.encode_video(frames_u8(n, H, W).cuda(), bsz=2)                   # [T,3,H,W] of another size: the same path
    assert torch.equal(bits(nchw), bits(one))
    with pytest.raises(ValueError, match="uint8"):
        ex.encode_video(frames_u8(n, H, W).float())


def test_encode_video_native_path_untouched(flav, tiny_towers):
    """(7) float [T,3,R,R] frames: encode_video = encode_image(preprocess(frames)), bit for bit."""
    from revisionllm_amd.data.clip_extractor import preprocess
    ex, _, c = tiny_towers
    R = c["image_res"]
    frames = frames_u8(3, R, R).float()
    assert torch.equal(bits(ex.encode_video(frames)), bits(ex.clip_extractor.encode_image(preprocess(frames))))
    assert torch.equal(bits(ex.encode_video(frames_u8(3, R, R))), bits(ex.clip_extractor.encode_image(preprocess(frames))))
