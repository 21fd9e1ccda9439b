"""Packed YCbCr surfaces (rv_packed_to_patches: YUY2 / UYVY / Y210, AYUV / VUYA / Y410 / XV36 ...) and packed RGB in any byte order
(rv_frames_to_patches_packed: bgr24, bgra, argb ...) inside the CLIP front-end kernels, and the layers above them (ops.packed_to_patches,
ops.frames_to_patches(pix_fmt=), ClipTowers.encode_surfaces_packed, ClipFeatureExtractor.encode_video_pix_fmt / encode_video(pix_fmt=)).

The formats are packed and unpacked by tests/packed_table.py, written from the published layouts; ops.PACKED_PIX_FMTS is never imported here.

Bounds.  A packed surface against its planar twin (the planar 4:2:2 / 4:4:4 surface that holds the same samples), and packed RGB against the NHWC entry on a
contiguous RGB copy: BITS, image and patches - the header defines the values as the twin's and the kernels keep its tap order and fmaf chains.  Against the
float64 oracle of the definition (tests/orient_oracle.py fed this file's own unpack): the sibling front-end tests' IMAGE_BOUND = 2e-4 in normalised units - the
same number of f32 roundings per output as the planar kernel; patches: the image rounded once to the operand type.  RV_LOG_ERR=<file>: the measured maxima are
appended there (profiles/packed_frontend_err.log is the place for one such run)."""
import functools
import os

import numpy as np
import pytest
import torch

import orient_oracle as oo
import packed_table as pt
from helpers import SEED
from test_gpu_orient_frontend import HALF_ULP, NAN_BITS, SPELL, bits, lib_error, same_bits, unfold

pytestmark = pytest.mark.gpu

ME = "test_gpu_packed_frontend.py"
#          H    W    R  patch
GEOMS = [(1, 2, 14, 14),            # one unit, pure upscale
         (3, 6, 14, 14),            # small odd H
         (37, 50, 28, 14),          # odd H, staged segments start off a 16-byte line
         (96, 64, 28, 14),          # downscale
         (180, 320, 224, 14),       # the towers' own size
         (250, 428, 28, 14)]        # about 9x downscale: many taps per output, several staging chunks
ODD_W = (5, 7, 14, 14)              # 1 px / unit formats only
CASES = [(name, g) for name in pt.NAMES for g in GEOMS + ([ODD_W] if pt.ppu(name) == 1 else [])]
CASE_IDS = ["%s-%dx%d" % (name, g[0], g[1]) for name, g in CASES]
N = 2
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


@functools.lru_cache(maxsize=None)
def planes_of(n, H, W, name):
    """Seeded sample values (y, cb, cr) for a format; never modified."""
    return oo.yuv_values(n, H, W, pt.depth(name), pt.sub(name))


@functools.lru_cache(maxsize=None)
def packed_of(n, H, W, name, fill_seed=0):
    out = pt.pack(name, *planes_of(n, H, W, name), np.random.RandomState(SEED + 17 + fill_seed))
    out.setflags(write=False)
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def twin_planes(name, planes):
    """The planar surface that holds the same samples: uint8, or uint16 words msb-aligned where the packed words are."""
    _, sb, d, shift = pt.TABLE[name]
    if sb == 1:
        return tuple(dev(p.astype(np.uint8)) for p in planes), dict(depth=8, msb_aligned=False, subsampling=pt.sub(name))
    return tuple(dev((p << shift).astype(np.uint16)) for p in planes), dict(depth=d, msb_aligned=shift > 0, subsampling=pt.sub(name))


def run_packed(buf, H, W, name, R, patch, flav, **kw):
    from revisionllm_amd import hip, ops
    return ops.packed_to_patches(buf, H=H, W=W, pix_fmt=name, R=R, patch=patch, op_dtype=hip.op_dtype(flav), want=("patches", "image"), **kw)


def run_twin(name, planes, R, patch, flav, **kw):
    from revisionllm_amd import hip, ops
    t, fmt = twin_planes(name, planes)
    return ops.yuv_surface_to_patches(*t, R=R, patch=patch, op_dtype=hip.op_dtype(flav), want=("patches", "image"), **fmt, **kw)


def finite_and_padded(out, patch):
    p, i = out
    assert bool(torch.isfinite(i).all()) and bool((bits(p[:, 3 * patch * patch:]) == 0).all())


# ---- 1: every packed format is its planar twin to the bit ----
@pytest.mark.parametrize("name,geom", CASES, ids=CASE_IDS)
def test_packed_is_its_planar_twin_to_the_bit(flav, name, geom):
    H, W, R, patch = geom
    got = run_packed(dev(packed_of(N, H, W, name)), H, W, name, R, patch, flav)
    finite_and_padded(got, patch)
    assert same_bits(got, run_twin(name, planes_of(N, H, W, name), R, patch, flav)), (name, geom)


@pytest.mark.parametrize("transfer", ["pq", "hlg"])
@pytest.mark.parametrize("name", ["y210le", "xv30le"])
def test_hdr_packed_is_the_planar_hdr_entry_to_the_bit(flav, name, transfer):
    H, W, R, patch = GEOMS[2]
    kw = dict(matrix="bt2020", chroma_loc="topleft", transfer=transfer)
    got = run_packed(dev(packed_of(N, H, W, name)), H, W, name, R, patch, flav, **kw)
    finite_and_padded(got, patch)
    assert same_bits(got, run_twin(name, planes_of(N, H, W, name), R, patch, flav, **kw))
    assert not same_bits(got, run_packed(dev(packed_of(N, H, W, name)), H, W, name, R, patch, flav, matrix="bt2020", chroma_loc="topleft"))


@pytest.mark.parametrize("name", ["yuyv422", "y210le"])
def test_all_orientations_are_the_planar_oriented_entry_to_the_bit(flav, name):
    H, W, R, patch = GEOMS[2]
    buf, planes = dev(packed_of(N, H, W, name)), planes_of(N, H, W, name)
    seen = set()
    for code in oo.ORIENTS:
        got = run_packed(buf, H, W, name, R, patch, flav, **SPELL[code])
        assert same_bits(got, run_twin(name, planes, R, patch, flav, **SPELL[code])), (name, code)
        seen.add(got[1].cpu().numpy().tobytes())
    assert len(seen) == 8


# ---- 2: against an independent float64 oracle of the definition ----
ORACLE_GEOMS = [GEOMS[2], GEOMS[3]]


@pytest.mark.parametrize("name", ["uyvy422", "y212le", "ayuv", "xv30le"])
def test_against_the_float64_oracle(flav, name):
    from revisionllm_amd import hip
    dt = hip.op_dtype(flav)
    worst = 0.0
    for H, W, R, patch in ORACLE_GEOMS:
        packed = packed_of(N, H, W, name)
        buf, planes = dev(packed), pt.unpack(name, packed, W)
        kp = (3 * patch * patch + 127) // 128 * 128
        for matrix in ("bt601", "bt709", "bt2020"):
            for full in (False, True):
                for loc in ("left", "centre"):
                    want = oo.normalise(oo.yuv_rgb_of(planes, H, W, R, pt.depth(name), pt.sub(name), 0, matrix, full, loc))
                    p, i = run_packed(buf, H, W, name, R, patch, flav, matrix=matrix, full_range=full, chroma_loc=loc)
                    err = float(np.abs(i.cpu().numpy().astype(np.float64) - want).max())
                    worst = max(worst, err)
                    assert err <= oo.IMAGE_BOUND, (name, H, W, matrix, full, loc, err)
                    assert torch.equal(bits(p), bits(unfold(i.to(dt), patch, kp)))          # patches: the image rounded once
                    wantp = unfold(torch.from_numpy(want.copy()), patch, kp)
                    tol = oo.IMAGE_BOUND + (wantp.abs() + oo.IMAGE_BOUND) * HALF_ULP[dt] + 2.0 ** -25
                    assert bool(((p.cpu().double() - wantp).abs() <= tol).all())
    print(f"{name} {flav}: worst image err {worst:.3e} (bound {oo.IMAGE_BOUND:.1e})")
    oo.log_err(ME, f"image-vs-float64-oracle {name} {flav}", worst)


# ---- 3: bytes that carry no value change nothing ----
@pytest.mark.parametrize("name", ["ayuv", "vuyx", "uyva", "ayuv64le", "xv48le", "xv30le", "y210le", "xv36le"])
def test_bytes_that_carry_no_value_change_nothing(flav, name):
    H, W, R, patch = GEOMS[2]
    a, b = packed_of(N, H, W, name, 0), packed_of(N, H, W, name, 1)
    assert not np.array_equal(a, b) and all(np.array_equal(x, y) for x, y in zip(pt.unpack(name, a, W), pt.unpack(name, b, W)))
    assert same_bits(run_packed(dev(a), H, W, name, R, patch, flav), run_packed(dev(b), H, W, name, R, patch, flav))


# ---- 4: a window of a larger surface ----
@pytest.mark.parametrize("name", ["yuyv422", "y210le"])
def test_a_window_of_a_larger_padded_surface(flav, name):
    """The window starts 3 units into the rows of a surface with a padded pitch (no multiple of 16 bytes) and a padded frame stride, inside noise; outputs
    inside NaN-filled buffers with ldp > Kp: the bits of the contiguous call, pad columns +0, everything else still NaN; other noise around it: the same bits."""
    from revisionllm_amd import hip
    H, W, R, patch = GEOMS[2]
    dt = hip.op_dtype(flav)
    unit, rb = pt.unit_bytes(name), pt.frame_bytes(1, W, name)
    base_p, base_i = run_packed(dev(packed_of(N, H, W, name)), H, W, name, R, patch, flav)
    pitch, x0 = rb + 5 * unit + (4 if unit == 4 else 8), 3 * unit
    fs = (H + 3) * pitch
    assert x0 % 16 and pitch % 16 and x0 % unit == 0
    kp = 640
    ldp, guard, rows = kp + 24, 1024, N * (R // patch) ** 2
    outs = []
    for seed in (7, 8):
        big = np.random.RandomState(seed).randint(0, 256, (N, fs)).astype(np.uint8)
        for f in range(N):
            big[f, 2 * pitch:(2 + H) * pitch].reshape(H, pitch)[:, x0:x0 + rb] = packed_of(N, H, W, name)[f]
        d = dev(big)
        view = d[:, 2 * pitch:(2 + H) * pitch].view(N, H, pitch)[:, :, x0:x0 + rb]
        assert view.data_ptr() % 16 and not view.is_contiguous() and np.array_equal(view.cpu().numpy(), packed_of(N, H, W, name))
        outs.append(run_packed(view, H, W, name, R, patch, flav))                          # through ops: passed by its strides
        pbuf = torch.full((guard + rows * ldp + guard,), NAN_BITS, dtype=torch.int16, device="cuda").view(dt)
        ibuf = torch.full((guard + N * 3 * R * R + guard,), float("nan"), device="cuda")
        rc = pt.call_packed(hip.lib(flav), hip, view.data_ptr(), pbuf.data_ptr() + 2 * guard, ibuf.data_ptr() + 4 * guard,
                            dict(PACKED_ARGS[name], frame_stride=fs, row_stride=pitch, n=N, H=H, W=W, R=R, patch=patch, ldp=ldp))
        torch.cuda.synchronize()
        assert rc == 0, hip.last_error()
        prow = pbuf[guard:guard + rows * ldp].view(rows, ldp)
        assert torch.equal(bits(prow[:, :kp]), bits(base_p)) and torch.equal(bits(ibuf[guard:-guard].view(N, 3, R, R)), bits(base_i))
        assert bool((bits(prow[:, 3 * patch * patch:kp]) == 0).all()) and bool((bits(prow[:, kp:]) == NAN_BITS).all())
        assert bool((bits(pbuf[:guard]) == NAN_BITS).all()) and bool((bits(pbuf[-guard:]) == NAN_BITS).all())
        assert bool(torch.isnan(ibuf[:guard]).all()) and bool(torch.isnan(ibuf[-guard:]).all())
    assert same_bits(outs[0], (base_p, base_i)) and same_bits(outs[1], (base_p, base_i))


#: the struct fields of the two formats the raw calls use, written from the layouts above
PACKED_ARGS = {"yuyv422": pt.YUYV, "y210le": dict(unit_bytes=8, pix_per_unit=2, sample_bytes=2, y_off=0, cb_off=2, cr_off=6, depth=10, msb_aligned=1)}


# ---- 5: batching and determinism ----
def test_batching_and_determinism(flav):
    H, W, R, patch = GEOMS[2]
    for name in ("uyvy422", "xv36le"):
        buf = dev(packed_of(4, H, W, name))
        a = run_packed(buf, H, W, name, R, patch, flav)
        assert same_bits(run_packed(buf, H, W, name, R, patch, flav), a)
        one, three = run_packed(buf[:1], H, W, name, R, patch, flav), run_packed(buf[1:], H, W, name, R, patch, flav)
        assert same_bits((torch.cat([one[0], three[0]]), torch.cat([one[1], three[1]])), a)
        assert same_bits(run_packed(buf.reshape(4, -1), H, W, name, R, patch, flav), a)     # [n, frame bytes]
        p, i = run_packed(buf[:0], H, W, name, R, patch, flav)
        assert tuple(p.shape) == (0, 640) and tuple(i.shape) == (0, 3, R, R)


# ---- 6: RGB orders ----
RGB_GEOMS = [(1, 1, 14, 14), (37, 50, 28, 14), (180, 320, 224, 14)]


@pytest.mark.parametrize("geom", RGB_GEOMS, ids=["1x1", "37x50", "180x320"])
@pytest.mark.parametrize("name", list(pt.RGB_ORDERS))
def test_rgb_orders_are_the_nhwc_entry_on_an_rgb_copy(flav, name, geom):
    from revisionllm_amd import hip, ops
    H, W, R, patch = geom
    dt = hip.op_dtype(flav)
    rgb = oo.rgb_values(N, H, W)
    want = ops.frames_to_patches(dev(rgb.transpose(0, 2, 3, 1)), R, patch, layout="NHWC", op_dtype=dt, want=("patches", "image"))
    for fill in (0, 1):
        src = dev(pt.pack_rgb(name, rgb, np.random.RandomState(SEED + fill)))
        assert same_bits(ops.frames_to_patches(src, R, patch, op_dtype=dt, want=("patches", "image"), pix_fmt=name), want), (name, geom, fill)
    if geom == RGB_GEOMS[1]:
        pix = src.shape[3]
        big = torch.randint(0, 256, (N, H + 2, W * pix + 13), dtype=torch.uint8, device="cuda")      # a padded row stride, a window 5 bytes in
        win = big[:, 1:1 + H, 5:5 + W * pix].unflatten(2, (W, pix))
        win.copy_(src)
        assert not win.is_contiguous() and win.stride(1) == W * pix + 13
        assert same_bits(ops.frames_to_patches(win, R, patch, op_dtype=dt, want=("patches", "image"), pix_fmt=name), want)


def test_bgra_turned_by_90_degrees(flav):
    from revisionllm_amd import hip, ops
    H, W, R, patch = RGB_GEOMS[1]
    dt = hip.op_dtype(flav)
    rgb = oo.rgb_values(N, H, W)
    want = ops.frames_to_patches(dev(rgb.transpose(0, 2, 3, 1)), R, patch, layout="NHWC", op_dtype=dt, want=("patches", "image"), rotate=90)
    got = ops.frames_to_patches(dev(pt.pack_rgb("bgra", rgb, np.random.RandomState(SEED))), R, patch, op_dtype=dt, want=("patches", "image"), pix_fmt="bgra", rotate=90)
    assert same_bits(got, want)
    assert not same_bits(got, ops.frames_to_patches(dev(rgb.transpose(0, 2, 3, 1)), R, patch, layout="NHWC", op_dtype=dt, want=("patches", "image")))


# ---- 7: 1080p / 2160p geometries are accepted ----
BIG = [(name, 1080, 1920) for name in pt.NAMES] + [(name, 2160, 3840) for name in ("yuyv422", "y210le", "xv30le")]


@pytest.mark.parametrize("name,H,W", BIG, ids=["%s-%d" % (c[0], c[1]) for c in BIG])
def test_1080p_and_2160p_are_accepted_and_are_the_planar_twin(flav, name, H, W):
    planes = planes_of(1, H, W, name)
    got = run_packed(dev(pt.pack(name, *planes, np.random.RandomState(SEED))), H, W, name, 224, 14, flav)
    finite_and_padded(got, 14)
    assert same_bits(got, run_twin(name, planes, 224, 14, flav))


# ---- 8: refusals through the raw C entries ----
def nan_outputs(flav, n=2, R=28, patch=14):
    from revisionllm_amd import hip
    p = torch.full((n * (R // patch) ** 2, 640), NAN_BITS, dtype=torch.int16, device="cuda").view(hip.op_dtype(flav))
    return p, torch.full((n, 3, R, R), float("nan"), device="cuda")


def untouched(p, i):
    torch.cuda.synchronize()
    return bool((bits(p) == NAN_BITS).all()) and bool(torch.isnan(i).all())


def test_refusals_of_the_packed_entry(flav):
    from revisionllm_amd import hip
    name = "rv_packed_to_patches"
    src = torch.zeros(2 * 6 * 32 + 64, dtype=torch.uint8, device="cuda")
    for what, over, word in pt.PACKED_REFUSALS:
        p, i = nan_outputs(flav)
        over = dict(over)
        outs = (over.pop("patches", p.data_ptr()), over.pop("image", i.data_ptr()))
        rc = pt.call_packed(hip.lib(flav), hip, src.data_ptr(), *outs, over)
        assert rc == -1, what                                                                # RV_ERR_ARG
        assert lib_error(flav).startswith(name + ":") and word in lib_error(flav), (what, lib_error(flav))
        assert untouched(p, i), what
    p, i = nan_outputs(flav)
    assert pt.call_packed(hip.lib(flav), hip, src.data_ptr(), p.data_ptr(), i.data_ptr(), {}, null_struct=True) == -1
    assert lib_error(flav) == name + ": null surface" and untouched(p, i)
    assert pt.call_packed(hip.lib(flav), hip, None, p.data_ptr(), i.data_ptr(), dict(n=0)) == 0 and untouched(p, i)       # nothing to do: no launch
    assert pt.call_packed(hip.lib(flav), hip, src.data_ptr(), p.data_ptr(), i.data_ptr(), {}) == 0                         # ... and the baseline runs
    torch.cuda.synchronize()
    assert not bool(torch.isnan(i).any())


def test_refusals_of_the_packed_rgb_entry(flav):
    from revisionllm_amd import hip
    name = "rv_frames_to_patches_packed"
    src = torch.zeros(2 * 6 * 32, dtype=torch.uint8, device="cuda")
    for what, over, word in pt.RGB_REFUSALS:
        p, i = nan_outputs(flav)
        over = dict(over)
        frames = over.pop("frames", src.data_ptr())
        outs = (over.pop("patches", p.data_ptr()), over.pop("image", i.data_ptr()))
        rc = pt.call_rgb(hip.lib(flav), frames, *outs, over)
        assert rc == -1, what
        assert lib_error(flav).startswith(name + ":") and word in lib_error(flav), (what, lib_error(flav))
        assert untouched(p, i), what
    p, i = nan_outputs(flav)
    assert pt.call_rgb(hip.lib(flav), None, p.data_ptr(), i.data_ptr(), dict(n=0)) == 0 and untouched(p, i)
    assert pt.call_rgb(hip.lib(flav), src.data_ptr(), p.data_ptr(), i.data_ptr(), {}) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(i).any())


# ---- 9: end to end ----
def test_end_to_end_through_the_tiny_towers(flav):
    """encode_video_pix_fmt on yuyv422 chunks of 1 / 5 / 2 frames with bsz = 3 is, to the bit, encode_video_pix_fmt on the same samples repacked as yuv422p;
    encode_video(bgr frames, pix_fmt="bgr24") is encode_video(rgb frames, layout="NHWC")."""
    from revisionllm_amd.data.clip_extractor import ClipFeatureExtractor
    from revisionllm_amd.data.clip_model import ClipTowers
    from revisionllm_amd.utils import synth
    c = synth.CLIP_TINY
    ex = ClipFeatureExtractor(ClipTowers(**c, t_heads=synth.CLIP_TINY_TEXT_HEADS, op_dtype=flav).init_synthetic(seed=SEED))
    n, H, W = 8, 46, 80
    planes = planes_of(n, H, W, "yuyv422")
    packed = torch.from_numpy(packed_of(n, H, W, "yuyv422").reshape(n, -1).copy())
    planar = torch.from_numpy(np.concatenate([p.reshape(n, -1) for p in planes], 1).astype(np.uint8))
    want = ex.encode_video_pix_fmt(planar, H, W, "yuv422p", bsz=3)
    got = ex.encode_video_pix_fmt(iter([packed[:1], packed[1:6], packed[6:]]), H, W, "yuyv422", bsz=3)
    assert tuple(got.shape) == (n, c["embed_dim"]) and torch.equal(bits(got), bits(want))
    assert torch.equal(bits(ex.encode_video_pix_fmt(packed.cuda(), H, W, "yuyv422", bsz=3, rotate=90)), bits(ex.encode_video_pix_fmt(planar, H, W, "yuv422p", bsz=3, rotate=90)))
    rgb = oo.rgb_values(5, 45, 80)
    nhwc = torch.from_numpy(np.ascontiguousarray(rgb.transpose(0, 2, 3, 1)))
    bgr = torch.from_numpy(pt.pack_rgb("bgr24", rgb, np.random.RandomState(SEED)))
    want = ex.encode_video(nhwc, bsz=2, layout="NHWC")
    assert torch.equal(bits(ex.encode_video(iter([bgr[:2], bgr[2:]]), bsz=2, pix_fmt="bgr24")), bits(want))
    assert not torch.equal(bits(ex.encode_video(bgr, bsz=2, layout="NHWC")), bits(want))      # the bytes read as RGB are another picture
