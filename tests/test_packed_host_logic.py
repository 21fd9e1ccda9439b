"""The host side of the packed front end (rv_packed_to_patches, rv_frames_to_patches_packed; ops.PACKED_PIX_FMTS / packed_frame_bytes / packed_to_patches,
ops.frames_to_patches(pix_fmt=), ClipFeatureExtractor.encode_video_pix_fmt / encode_video(pix_fmt=)), without a GPU: the sizes, the test's own format table
(tests/packed_table.py) against the library's after the fact, its pack / unpack round trip, the sensitivity of the float64 oracle the GPU test uses, the two
symbols in the header, the ctypes table and both libraries, every refusal that is decided before a launch, and the neighbours that must not have changed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import orient_oracle as oo
import packed_table as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAVOURS = ("f16", "bf16")
PACKED, RGB = "rv_packed_to_patches", "rv_frames_to_patches_packed"


def lib_error(flavour):
    from revisionllm_amd import hip
    buf = ctypes.create_string_buffer(512)
    hip.lib(flavour).rv_last_error(buf, 512)
    return buf.value.decode()


# ---- sizes and the two tables ----
@pytest.mark.parametrize("name", pt.NAMES)
def test_packed_frame_bytes(name):
    from revisionllm_amd import ops
    bpp = {"yuyv422": 2, "uyvy422": 2, "yvyu422": 2, "y210le": 4, "y212le": 4, "ayuv": 4, "vuya": 4, "vuyx": 4, "uyva": 4, "ayuv64le": 8, "xv36le": 8, "xv48le": 8,
           "xv30le": 4}[name]                                                            # bytes per pixel, from the formats' definitions
    for H, W in ((1, 2), (37, 50), (1080, 1920)):
        assert ops.packed_frame_bytes(H, W, name) == H * W * bpp == pt.frame_bytes(H, W, name)
    if pt.ppu(name) == 2:
        with pytest.raises(ValueError, match="multiple of 2"):
            ops.packed_frame_bytes(4, 7, name)
    else:
        assert ops.packed_frame_bytes(5, 7, name) == 35 * bpp
    with pytest.raises(ValueError):
        ops.packed_frame_bytes(0, 8, name)


def test_the_tests_table_and_the_librarys_agree_after_the_fact():
    """Same names; per name the library's fields (unit bytes, pixels per unit, sample bytes, offsets, depth, msb) are what this file's slots say."""
    from revisionllm_amd import ops
    assert sorted(ops.PACKED_PIX_FMTS) == sorted(pt.NAMES)
    for name, (unit, ppu, sb, oy, ocb, ocr, depth, msb) in ops.PACKED_PIX_FMTS.items():
        slots, tsb, tdepth, shift = pt.TABLE[name]
        assert (unit, ppu, sb, depth, bool(msb)) == (pt.unit_bytes(name), pt.ppu(name), tsb, tdepth, shift > 0), name
        if tsb == 4:
            assert (oy, ocb, ocr) == (slots["Y"], slots["Cb"], slots["Cr"]), name
        else:
            assert (oy, ocb, ocr) == tuple(slots.index(c) * tsb for c in ("Y0" if ppu == 2 else "Y", "Cb", "Cr")), name
            assert ppu == 1 or slots.index("Y1") - slots.index("Y0") == 2                # the second Y sample lies half a unit behind the first
        assert depth + shift == (8 * tsb if tsb < 4 else 10)
    assert not set(ops.PACKED_PIX_FMTS) & set(ops.PIX_FMTS)
    assert {n: (len(o), o.index("R"), o.index("G"), o.index("B")) for n, o in pt.RGB_ORDERS.items()} == ops.RGB_PIX_FMTS


@pytest.mark.parametrize("name", pt.NAMES)
def test_pack_unpack_round_trip(name):
    H, W = 5, 6
    planes = oo.yuv_values(2, H, W, pt.depth(name), pt.sub(name))
    a, b = (pt.pack(name, *planes, np.random.RandomState(s)) for s in (1, 2))
    assert a.dtype == np.uint8 and a.shape == (2, H, pt.frame_bytes(1, W, name))
    for buf in (a, b):
        assert all(np.array_equal(x, y) for x, y in zip(pt.unpack(name, buf, W), planes))
    if name not in ("yuyv422", "uyvy422", "yvyu422"):
        assert not np.array_equal(a, b)                                                  # the fill bits differ, the values do not
    # a hand-written unit per family
    if name == "yuyv422":
        assert pt.pack(name, np.array([[[1, 2]]]), np.array([[[3]]]), np.array([[[4]]]), np.random.RandomState(0)).tolist() == [[[1, 3, 2, 4]]]
    if name == "uyvy422":
        assert pt.pack(name, np.array([[[1, 2]]]), np.array([[[3]]]), np.array([[[4]]]), np.random.RandomState(0)).tolist() == [[[3, 1, 4, 2]]]
    if name == "xv30le":
        w = pt.pack(name, np.array([[[0x155]]]), np.array([[[0x001]]]), np.array([[[0x3FF]]]), np.random.RandomState(0)).view("<u4")
        assert int(w[0, 0, 0]) & 0x3FFFFFFF == 0x001 | 0x155 << 10 | 0x3FF << 20
    if name == "y210le":
        w = pt.pack(name, np.array([[[1, 2]]]), np.array([[[3]]]), np.array([[[4]]]), np.random.RandomState(0)).view("<u2")
        assert (w[0, 0] >> 6).tolist() == [1, 3, 2, 4]


def test_the_oracle_is_sensitive_to_a_swap_and_to_a_shift():
    """Swapping Cb and Cr, or shifting Y by one sample, moves the float64 oracle by far more than the bound the GPU test holds the kernel to."""
    H, W, R = 37, 50, 28
    for name in ("uyvy422", "xv30le"):
        d, sub = pt.depth(name), pt.sub(name)
        y, cb, cr = pt.unpack(name, pt.pack(name, *oo.yuv_values(2, H, W, d, sub), np.random.RandomState(3)), W)
        base = oo.normalise(oo.yuv_rgb_of((y, cb, cr), H, W, R, d, sub, 0))
        swapped = oo.normalise(oo.yuv_rgb_of((y, cr, cb), H, W, R, d, sub, 0))
        shifted = oo.normalise(oo.yuv_rgb_of((np.roll(y, 1, axis=2), cb, cr), H, W, R, d, sub, 0))
        assert float(np.abs(swapped - base).max()) > 1000 * oo.IMAGE_BOUND
        assert float(np.abs(shifted - base).max()) > 1000 * oo.IMAGE_BOUND


# ---- the symbols ----
C_TYPES = {"const uint8_t*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "void*": ctypes.c_void_p,
           "float*": ctypes.c_void_p}


@pytest.mark.parametrize("name", [PACKED, RGB])
def test_header_ctypes_table_and_both_libraries_carry_the_symbol(name):
    from revisionllm_amd import hip
    header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    m = re.search(r"^(\w+)\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
    assert m and m.group(1) == "int"
    params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in " ".join(m.group(2).split()).split(",")]
    res, args = hip.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(params)
    for written, a in zip(params, args):
        if re.match(r"const float \w+\[3\]$", written):
            assert a._type_ is ctypes.c_float
        elif written.startswith("const rv_packed_surface*"):
            assert a._type_ is hip.RvPackedSurface
        elif written.startswith("const rv_hdr_map*"):
            assert a._type_ is hip.RvHdrMap
        else:
            assert C_TYPES[written.rsplit(" ", 1)[0]] is a, (written, a)
    assert "#define RV_ABI_VERSION 5" in header
    for flavour in FLAVOURS:
        assert hasattr(hip.lib(flavour), name) and hip.lib(flavour).rv_abi_version() == 5
    # the struct, field by field, as the header declares it
    body = re.search(r"typedef struct rv_packed_surface \{(.*?)\} rv_packed_surface;", header, re.S).group(1)
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            ctype = "const void*" if decl.startswith("const void*") else decl.split(" ", 1)[0]
            for n in decl[len(ctype):].split(","):
                fields.append((n.strip(), {"const void*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[ctype]))
    assert fields == list(hip.RvPackedSurface._fields_)


# ---- refusals of the C entries: validation runs before any launch, so no device is needed ----
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refusals_of_the_c_entries(flavour):
    from revisionllm_amd import hip
    lib = hip.lib(flavour)
    for what, over, word in pt.PACKED_REFUSALS:
        over = dict(over)
        outs = (over.pop("patches", 0x40000), over.pop("image", 0x50000))
        assert pt.call_packed(lib, hip, 0x10000, *outs, over) == -1, what
        assert lib_error(flavour).startswith(PACKED + ":") and word in lib_error(flavour), (what, lib_error(flavour))
    assert pt.call_packed(lib, hip, 0x10000, 0x40000, 0x50000, {}, null_struct=True) == -1 and lib_error(flavour) == PACKED + ": null surface"
    for over in (dict(n=0), dict(n=0, base=None), dict(pt.XV30, n=0), dict(pt.YUYV, n=0, H=5), dict(n=0, orient=3, hdr=(1, 1, 1000.0, 203.0))):
        assert pt.call_packed(lib, hip, 0x10000, 0x40000, 0x50000, over) == 0, over       # nothing to do: validated, not launched
    assert pt.call_packed(lib, hip, 0x10000, 0x40000, 0x50000, dict(pt.XV30, n=0, W=7)) == 0   # odd W is legal with one pixel per unit
    for what, over, word in pt.RGB_REFUSALS:
        over = dict(over)
        frames = over.pop("frames", 0x10000)
        outs = (over.pop("patches", 0x40000), over.pop("image", 0x50000))
        assert pt.call_rgb(lib, frames, *outs, over) == -1, what
        assert lib_error(flavour).startswith(RGB + ":") and word in lib_error(flavour), (what, lib_error(flavour))
    assert pt.call_rgb(lib, None, 0x40000, 0x50000, dict(n=0)) == 0


# ---- refusals of the Python layer: before anything is read or launched ----
def test_host_side_refusals_of_packed_to_patches():
    from revisionllm_amd import hip, ops
    kw = dict(H=4, W=8, R=14, patch=14)
    good = torch.zeros(2, 4, 16, dtype=torch.uint8)
    with pytest.raises(ValueError) as e:
        ops.packed_to_patches(good, pix_fmt="v210", **kw)
    assert "yuyv422" in str(e.value) and "nv12" in str(e.value)                          # both tables are listed
    with pytest.raises(ValueError, match="pix_fmt"):
        ops.packed_to_patches(good, pix_fmt="nv12", **kw)                               # a planar name is not a packed one
    with pytest.raises(ValueError, match="multiple of 2"):
        ops.packed_to_patches(good, pix_fmt="yuyv422", H=4, W=7, R=14, patch=14)
    for bad in (good.to(torch.int16), good[:, :3], good[..., :15], torch.zeros(2, 4, 8, 2, dtype=torch.uint8), torch.zeros(2, 63, dtype=torch.uint8), "bytes"):
        with pytest.raises(ValueError, match="uint8 tensor"):
            ops.packed_to_patches(bad, pix_fmt="yuyv422", **kw)
    with pytest.raises(ValueError, match="rotate"):
        ops.packed_to_patches(good, pix_fmt="yuyv422", rotate=45, **kw)
    with pytest.raises(ValueError, match="transfer"):
        ops.packed_to_patches(good, pix_fmt="yuyv422", transfer="gamma", **kw)
    with pytest.raises(ValueError, match="matrix"):
        ops.packed_to_patches(good, pix_fmt="yuyv422", matrix="bt470", **kw)
    # 16 / 32-bit words off their boundary: an odd byte offset, an odd pitch
    flat = torch.zeros(2 * 4 * 40 + 8, dtype=torch.uint8)
    for name, rb in (("y210le", 32), ("xv30le", 32)):
        for off, pitch in ((1, 40), (2 if name == "xv30le" else 1, 36), (0, 33)):
            view = flat.as_strided((2, 4, rb), (4 * pitch, pitch, 1), off)
            with pytest.raises(ValueError, match="multiples of"):
                ops.packed_to_patches(view, pix_fmt=name, **kw)
    for name in ("yuyv422", "y210le"):                                                   # everything else is in order: the tensor is on the CPU
        with pytest.raises(hip.HipLibraryError, match="device tensor"):
            ops.packed_to_patches(torch.zeros(2, 4, ops.packed_frame_bytes(1, 8, name), dtype=torch.uint8), pix_fmt=name, **kw)


def test_host_side_refusals_of_the_rgb_orders():
    from revisionllm_amd import hip, ops
    bgra = torch.zeros(2, 4, 8, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="pix_fmt"):
        ops.frames_to_patches(bgra, 14, 14, pix_fmt="rgb48le")
    with pytest.raises(ValueError, match="layout"):
        ops.frames_to_patches(torch.zeros(2, 3, 4, 8, dtype=torch.uint8), 14, 14, layout="NCHW", pix_fmt="bgr24")       # pix_fmt with NCHW frames
    with pytest.raises(ValueError, match="uint8 tensor"):
        ops.frames_to_patches(torch.zeros(2, 3, 4, 8, dtype=torch.uint8), 14, 14, pix_fmt="bgr24")                       # [n,3,H,W] is not [n,H,W,3]
    with pytest.raises(ValueError, match="uint8 tensor"):
        ops.frames_to_patches(bgra, 14, 14, pix_fmt="bgr24")
    with pytest.raises(ValueError, match="uint8 tensor"):
        ops.frames_to_patches(bgra.float(), 14, 14, pix_fmt="bgra")
    with pytest.raises(ValueError, match="rotate"):
        ops.frames_to_patches(bgra, 14, 14, pix_fmt="bgra", rotate=1)
    with pytest.raises(hip.HipLibraryError, match="device tensor"):
        ops.frames_to_patches(bgra, 14, 14, pix_fmt="bgra")


def test_the_extractor_refuses_before_it_reads():
    from revisionllm_amd.data.clip_extractor import ClipFeatureExtractor

    class Towers:                                                                        # never reached
        device, cfg = "cpu", dict(image_res=14, patch=14, embed_dim=8)

    ex = ClipFeatureExtractor(Towers())

    def chunks():
        raise AssertionError("read before the refusal")
        yield

    with pytest.raises(ValueError) as e:
        ex.encode_video_pix_fmt(chunks(), 4, 8, "v210")
    assert "yuyv422" in str(e.value) and "nv12" in str(e.value)
    with pytest.raises(ValueError, match="multiple of 2"):
        ex.encode_video_pix_fmt(chunks(), 4, 7, "uyvy422")
    with pytest.raises(ValueError, match="rotate"):
        ex.encode_video_pix_fmt(chunks(), 4, 8, "uyvy422", rotate=10)
    with pytest.raises(ValueError, match="transfer"):
        ex.encode_video_pix_fmt(chunks(), 4, 8, "y210le", transfer="gamma")
    with pytest.raises(ValueError, match="pix_fmt"):
        ex.encode_video(chunks(), pix_fmt="rgb48le")
    with pytest.raises(ValueError, match="layout"):
        ex.encode_video(chunks(), layout="NCHW", pix_fmt="bgr24")
    with pytest.raises(ValueError, match="uint8 tensors"):
        ex.encode_video_pix_fmt(torch.zeros(2, 4, 16, dtype=torch.uint8), 4, 8, "uyvy422")      # chunks are [t, frame bytes]


# ---- the neighbours are what they were ----
def test_the_planar_table_and_its_helpers_are_unchanged():
    from revisionllm_amd import ops
    assert sorted(ops.PIX_FMTS) == sorted(["nv12", "nv21", "nv16", "nv24", "yuv420p", "yuv422p", "yuv444p", "yuv420p10le", "yuv422p10le", "yuv444p10le", "yuv420p12le",
                                           "yuv444p12le", "yuv420p16le", "p010le", "p016le", "p210le", "p410le"])
    assert ops.PIX_FMTS["p010le"] == (2, 10, True, "420", "cbcr") and ops.PIX_FMTS["yuv422p"] == (1, 8, False, "422", "planar")
    with pytest.raises(ValueError, match="pix_fmt"):
        ops.split_yuv(torch.zeros(1, 64, dtype=torch.uint8), 4, 8, "yuyv422")
    with pytest.raises(ValueError, match="pix_fmt"):
        ops.yuv_frame_bytes(4, 8, "yuyv422")
    assert ops.yuv_frame_bytes(4, 8, "yuv422p") == 64 and ops.yuv_frame_bytes(4, 8, "p010le") == 96
    (y, cb, cr), kw = ops.split_yuv(torch.arange(64, dtype=torch.uint8).view(1, 64), 4, 8, "yuv422p")
    assert tuple(y.shape) == (1, 4, 8) and tuple(cb.shape) == (1, 4, 4) and int(cb[0, 0, 0]) == 32 and int(cr[0, 0, 0]) == 48
    assert kw == dict(depth=8, msb_aligned=False, subsampling="422")
