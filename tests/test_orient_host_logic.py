"""The host side of display orientation in the CLIP front end (rv_frames_to_patches_oriented, rv_yuv_surface_to_patches_oriented), without a GPU:
ops.orientation against the NumPy definition of the header; the two symbols in the header, the export map, the ctypes table and both libraries; the refusals
that are decided before any launch; and the sensitivity of the float64 oracle of tests/orient_oracle.py, so that the GPU test cannot pass with the siting
sign or the crop parity wrong."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import orient_oracle as oo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB, YUV = "rv_frames_to_patches_oriented", "rv_yuv_surface_to_patches_oriented"
FLAVOURS = ("f16", "bf16")


def lib_error(flavour):
    from revisionllm_amd import hip
    buf = ctypes.create_string_buffer(512)
    hip.lib(flavour).rv_last_error(buf, 512)
    return buf.value.decode()


# ---- ops.orientation ----
def test_orientation_maps_onto_exactly_the_eight_codes_of_the_definition():
    """Every rotate x hflip x vflip gives the code whose three NumPy steps (transpose, mirror x, mirror y) are: turn clockwise by ``rotate``, then flip."""
    from revisionllm_amd import ops
    A = np.random.RandomState(oo.SEED).randint(0, 1000, (3, 5, 7))
    seen = {}
    for rotate, hflip, vflip in itertools.product((0, 90, 180, 270), (False, True), (False, True)):
        code = ops.orientation(rotate, hflip, vflip)
        assert isinstance(code, int) and 0 <= code <= 7
        want = np.rot90(A, -(rotate // 90), axes=(-2, -1))                                # np.rot90 turns counter-clockwise
        want = want[..., ::-1] if hflip else want
        want = want[..., ::-1, :] if vflip else want
        assert np.array_equal(oo.orient(A, code), want), (rotate, hflip, vflip, code)
        seen.setdefault(code, []).append((rotate, hflip, vflip))
    assert sorted(seen) == list(range(8)) and all(len(v) == 2 for v in seen.values())     # 16 spellings, 8 orientations, each met twice
    assert {r: ops.orientation(r) for r in oo.ROTATE_CODE} == oo.ROTATE_CODE
    assert ops.orientation() == 0 and ops.orientation(0, True, False) == 2 and ops.orientation(0, False, True) == 4
    assert ops.orientation(hflip=True, vflip=True) == ops.orientation(180)


def test_the_codes_compose_like_the_numpy_definition():
    from revisionllm_amd import ops
    A = np.random.RandomState(oo.SEED + 1).randint(0, 1000, (5, 7))
    q, h, u, t = (ops.orientation(r) for r in (90, 180, 270, 0))
    assert np.array_equal(oo.orient(oo.orient(A, q), q), oo.orient(A, h))                  # twice by 90 degrees = code 6
    assert np.array_equal(oo.orient(oo.orient(A, q), h), oo.orient(A, u))
    assert np.array_equal(oo.orient(oo.orient(A, q), u), A) and np.array_equal(oo.orient(oo.orient(A, h), h), A)
    assert np.array_equal(oo.orient(oo.orient(A, q), 2), oo.orient(A, ops.orientation(90, hflip=True)))
    assert np.array_equal(oo.orient(oo.orient(A, u), 4), oo.orient(A, ops.orientation(270, vflip=True)))
    assert np.array_equal(oo.orient(A, 1), A.T) and np.array_equal(oo.orient(A, 7), A[::-1, ::-1].T)     # the two diagonal flips
    for c in oo.ORIENTS:
        assert oo.orient(A, c).shape == ((7, 5) if c & 1 else (5, 7))
    assert len({oo.orient(A, c).tobytes() + bytes(oo.orient(A, c).shape) for c in oo.ORIENTS}) == 8


@pytest.mark.parametrize("bad", [dict(rotate=45), dict(rotate=-90), dict(rotate=360), dict(rotate=90.0), dict(rotate="90"), dict(rotate=None), dict(rotate=True),
                                 dict(hflip=1), dict(vflip="yes"), dict(hflip=None)], ids=lambda b: "-".join(f"{k}={v!r}" for k, v in b.items()))
def test_bad_orientations_are_refused(bad):
    from revisionllm_amd import ops
    with pytest.raises(ValueError):
        ops.orientation(**bad)
    # ... by every wrapper, before it looks at a tensor
    z8 = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.frames_to_patches(torch.zeros(1, 3, 4, 4, dtype=torch.uint8), 14, 14, **bad)
    with pytest.raises(ValueError):
        ops.yuv_to_patches(z8, z8[:, :2, :2], z8[:, :2, :2], R=14, patch=14, **bad)
    with pytest.raises(ValueError):
        ops.yuv_surface_to_patches(z8, z8[:, :2, :2], z8[:, :2, :2], R=14, patch=14, **bad)


# ---- the symbols ----
C_TYPES = {"const uint8_t*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "void*": ctypes.c_void_p,
           "float*": ctypes.c_void_p}


def header_signature(name):
    """(restype word, [parameter types as written]) of a prototype in the header."""
    header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    m = re.search(r"^(\w+)\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
    assert m, name
    params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in " ".join(m.group(2).split()).split(",")]
    return m.group(1), params


@pytest.mark.parametrize("name", [RGB, YUV])
def test_header_export_map_ctypes_table_and_both_libraries_carry_the_symbol(name):
    from revisionllm_amd import hip
    ret, params = header_signature(name)
    res, args = hip.SIGNATURES[name]
    assert ret == "int" and res is ctypes.c_int and len(args) == len(params)
    for written, a in zip(params, args):
        if re.match(r"const float \w+\[3\]$", written):
            assert a._type_ is ctypes.c_float
        elif written.startswith("const rv_yuv_surface*"):
            assert a._type_ is hip.RvYuvSurface
        elif written.startswith("const rv_hdr_map*"):
            assert a._type_ is hip.RvHdrMap
        else:
            ctype = written.rsplit(" ", 1)[0]
            assert C_TYPES[ctype] is a, (written, a)
    # the un-oriented prototype with one int32_t orient in front of R
    base, base_params = header_signature(name[:-len("_oriented")])
    names = [p.split()[-1] for p in params]
    assert names[names.index("orient") + 1] == "R" and "int32_t orient" in params
    assert [p for p in params if p != "int32_t orient" and "rv_hdr_map" not in p] == base_params
    assert "#define RV_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    emap = open(os.path.join(ROOT, "revisionllm_amd", "csrc", "exports.map")).read()
    assert "global: rv_*;" in emap and name in emap
    for flavour in FLAVOURS:
        assert hasattr(hip.lib(flavour), name), flavour


# ---- refusals that need no device: validation runs before any launch ----
def rgb_call(flavour, orient, **over):
    from revisionllm_amd import hip
    a = dict(frames=0x10000, layout=0, fs=3 * 30 * 51, rs=51, n=2, H=30, W=51, R=28, patch=14, patches=0x40000, ldp=640, image=0x50000)
    a.update(over)
    f3 = ctypes.c_float * 3
    return hip.lib(flavour).rv_frames_to_patches_oriented(a["frames"], a["layout"], a["fs"], a["rs"], a["n"], a["H"], a["W"], orient, a["R"], a["patch"],
                                                          f3(*oo.MEAN), f3(*oo.STD), a["patches"], a["ldp"], a["image"], None)


def yuv_call(flavour, orient, surface=None, hdr=None, null_surface=False, **over):
    from revisionllm_amd import hip
    H, W = 32, 54
    s = dict(y=0x10000, cb=0x20000, cr=0x30000, y_frame_stride=H * W, y_row_stride=W, c_frame_stride=H * W // 4, c_row_stride=W // 2, sample_bytes=1, depth=8,
             msb_aligned=0, c_pix=1, sub_x=2, sub_y=2, n=2, H=H, W=W, matrix=0, full_range=0, chroma_loc=0)
    s.update(surface or {})
    a = dict(R=28, patch=14, patches=0x40000, ldp=640, image=0x50000)
    a.update(over)
    f3 = ctypes.c_float * 3
    return hip.lib(flavour).rv_yuv_surface_to_patches_oriented(None if null_surface else ctypes.byref(hip.RvYuvSurface(**s)),
                                                               None if hdr is None else ctypes.byref(hip.RvHdrMap(**hdr)), orient, a["R"], a["patch"],
                                                               f3(*oo.MEAN), f3(*oo.STD), a["patches"], a["ldp"], a["image"], None)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refusals_decided_on_the_host(flavour):
    for bad in (8, -1, 16, 1 << 30):
        assert rgb_call(flavour, bad) < 0
        assert lib_error(flavour).startswith(RGB + ": orient"), lib_error(flavour)
        assert yuv_call(flavour, bad) < 0
        assert lib_error(flavour).startswith(YUV + ": orient"), lib_error(flavour)
    for orient in oo.ORIENTS:
        # everything the un-oriented entries refuse, under the new name
        for over, msg in ((dict(layout=2), "layout"), (dict(R=30), "multiple"), (dict(H=0), "frame size"), (dict(W=8193), "frame size"), (dict(frames=None), "null frames"),
                          (dict(patches=None, image=None), "both outputs null"), (dict(ldp=639), "ldp"), (dict(layout=0, fs=3 * 30 * 51 + 1), "frame_stride"),
                          (dict(H=8192, W=8192, R=1, patch=1), "LDS"), (dict(n=-1), "n = -1")):
            assert rgb_call(flavour, orient, **over) < 0, (orient, over)
            assert lib_error(flavour).startswith(RGB + ":") and msg in lib_error(flavour), lib_error(flavour)
        for surface, over, msg in ((dict(y=None), {}, "null plane"), (dict(sub_x=1, sub_y=2), {}, "sub_x"), (dict(H=31), {}, "odd"), (dict(W=53), {}, "odd"),
                                   (dict(chroma_loc=3), {}, "chroma_loc"), (dict(depth=10), {}, "depth"), ({}, dict(R=30), "multiple"), ({}, dict(ldp=639), "ldp"),
                                   ({}, dict(patches=None, image=None), "both outputs null"), (dict(H=8192, W=8192), dict(R=1, patch=1), "LDS"),
                                   (dict(n=2 ** 30), {}, "workgroups")):
            assert yuv_call(flavour, orient, surface=surface, **over) < 0, (orient, surface, over)
            assert lib_error(flavour).startswith(YUV + ":") and msg in lib_error(flavour), lib_error(flavour)
        assert yuv_call(flavour, orient, null_surface=True) < 0 and lib_error(flavour) == YUV + ": null surface"
        assert yuv_call(flavour, orient, hdr=dict(transfer=3, gamut=1, peak_nits=1000.0, sdr_white_nits=203.0)) < 0 and "transfer" in lib_error(flavour)
        # nothing to do: 0, and no launch
        assert rgb_call(flavour, orient, n=0, frames=None) == 0
        assert yuv_call(flavour, orient, surface=dict(n=0, y=None, cb=None, cr=None)) == 0
        assert yuv_call(flavour, orient, surface=dict(n=0), hdr=dict(transfer=2, gamut=0, peak_nits=1000.0, sdr_white_nits=203.0)) == 0
    # parity is checked along the CODED subsampled axes: an odd H is legal at 4:2:2 whatever the orientation (n = 0: validated, not launched)
    assert yuv_call(flavour, 3, surface=dict(n=0, H=15, W=16, sub_y=1)) == 0
    assert yuv_call(flavour, 3, surface=dict(n=0, H=16, W=15, sub_y=1)) < 0 and "odd" in lib_error(flavour)


# ---- the oracle can tell ----
def test_the_oracle_is_sensitive_to_the_siting_sign_and_to_the_crop_parity(capsys):
    """On the 32 x 54 4:2:0 case (resized to 28 x 47: the crop takes 10 columns off the left and 9 off the right), from the oracle alone:
    the definition with the siting offset NOT negated on a mirrored axis, and the un-oriented result mirrored afterwards, are both more than 100 x the image
    bound away from the definition."""
    n, H, W, R = 2, 32, 54, 28
    Hd, Wd, _, fx, top, left = oo.display_geometry(H, W, R, 2)
    assert (Hd, Wd, top, left) == (32, 54, 0, 10) and int(R * W / H) - R - left == 9
    # (3, "left") would show nothing: under transpose the offset of the coded x axis lands on display y, which a turn by 90 degrees does not mirror
    for code, loc in ((2, "left"), (6, "topleft"), (3, "topleft"), (5, "left"), (4, "topleft")):
        right = oo.yuv_oracle64(n, H, W, R, 8, "420", code, loc=loc)
        wrong = oo.yuv_oracle64(n, H, W, R, 8, "420", code, loc=loc, negate=False)
        d = float(np.abs(right - wrong).max())
        with capsys.disabled():
            print(f"\norient {code} {loc}: siting offset not negated differs from the definition by {d:.3e} ({d / oo.IMAGE_BOUND:.0f} x the bound)")
        assert d > 100 * oo.IMAGE_BOUND
    assert np.array_equal(oo.yuv_oracle64(n, H, W, R, 8, "420", 3, loc="left"), oo.yuv_oracle64(n, H, W, R, 8, "420", 3, loc="left", negate=False))
    # centre siting has no offset to negate
    assert np.array_equal(oo.yuv_oracle64(n, H, W, R, 8, "420", 2, loc="centre"), oo.yuv_oracle64(n, H, W, R, 8, "420", 2, loc="centre", negate=False))
    for code, flip in ((2, lambda a: a[..., ::-1]), (6, lambda a: a[..., ::-1, ::-1])):
        for loc in ("centre", "left"):
            d = float(np.abs(flip(oo.yuv_oracle64(n, H, W, R, 8, "420", 0, loc=loc)) - oo.yuv_oracle64(n, H, W, R, 8, "420", code, loc=loc)).max())
            with capsys.disabled():
                print(f"orient {code} {loc}: the un-oriented result mirrored differs from the definition by {d:.3e} ({d / oo.IMAGE_BOUND:.0f} x the bound)")
            assert d > 100 * oo.IMAGE_BOUND
    d = float(np.abs(oo.rgb_oracle64(2, 30, 51, 28, 0)[..., ::-1] - oo.rgb_oracle64(2, 30, 51, 28, 2)).max())
    assert d > 100 * oo.IMAGE_BOUND                                                       # 30 x 51 -> 28 x 47 too: an odd crop margin
    # ... while a vertical flip of this geometry (no crop along y, centre siting) IS the mirrored result, up to the order of the sums
    assert np.abs(oo.yuv_oracle64(n, H, W, R, 8, "420", 0, loc="centre")[..., ::-1, :] - oo.yuv_oracle64(n, H, W, R, 8, "420", 4, loc="centre")).max() < 1e-9


def test_orientation_zero_is_the_sibling_oracles_definition():
    """Code 0 of this oracle restates the un-oriented definition: its resampling matrix is the one tests/hdr_oracle.py keeps."""
    import hdr_oracle as ho
    assert np.array_equal(oo.axis_matrix(27, 54 / 47, 2.0, 0.25, 10, 28), ho.axis_matrix(27, 54 / 47, 2.0, 0.25, 10, 28))
    planes = oo.yuv_values(2, 32, 54, 10, "420")
    assert np.array_equal(oo.yuv_rgb_of(planes, 32, 54, 28, 10, "420", 0, "bt2020", False, "topleft"), ho.sdr_rgb_of(planes, 32, 54, 28, 10, "420"))
