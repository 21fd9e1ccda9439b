"""The host side of the scattered front end (rv_frames_to_patches_scattered, rv_yuv_surfaces_to_patches, rv_packed_surfaces_to_patches; the list forms of
ops.frames_to_patches / yuv_to_patches / yuv_surface_to_patches / packed_to_patches; ClipFeatureExtractor's ``scattered=True``), without a GPU: the three
symbols and RV_FRAME_TABLE_MAX in the header, the ctypes table and both libraries; the pointer tables the list forms build, on CPU tensors with a recorder in
the place of the library (the device check, hip.ptr and hip.stream are stood in for as well: they are what keeps a CPU address from a kernel); every ValueError
of the list forms; the tensor forms, which must not have moved; every refusal of the C entries that is decided before a launch - validation covers the whole
table first, so nothing here needs a device -; and the batching of the extractor in both modes."""
import ctypes
import os
import re

import pytest
import torch

import packed_table as pt
from test_hdr_host_logic import MAP_REFUSALS, SURFACE_REFUSALS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAVOURS = ("f16", "bf16")
RGB, YUV, PACKED = "rv_frames_to_patches_scattered", "rv_yuv_surfaces_to_patches", "rv_packed_surfaces_to_patches"
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def lib_error(flavour):
    from revisionllm_amd import hip
    buf = ctypes.create_string_buffer(512)
    hip.lib(flavour).rv_last_error(buf, 512)
    return buf.value.decode()


# ---- the symbols ----
def test_header_ctypes_table_and_both_libraries_carry_the_symbols():
    from revisionllm_amd import hip
    header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    assert "#define RV_ABI_VERSION 5" in header
    m = re.search(r"^#define RV_FRAME_TABLE_MAX (\d+)$", header, re.M)
    assert m and int(m.group(1)) == 64 == hip.FRAME_TABLE_MAX
    # three pointers per frame and the largest parameter block stay under the 4 KiB of a kernel's argument segment
    assert 64 * ctypes.sizeof(hip.RvSurfacePlanes) + 1024 < 4096 and ctypes.sizeof(hip.RvSurfacePlanes) == 24
    assert re.search(r"typedef struct rv_surface_planes \{ const void \*y, \*cb, \*cr; \} rv_surface_planes;", header)
    assert [f for f, _ in hip.RvSurfacePlanes._fields_] == ["y", "cb", "cr"]
    first = {RGB: "const uint8_t* const* frames", YUV: "const rv_yuv_surface* s", PACKED: "const rv_packed_surface* s"}
    for name in (RGB, YUV, PACKED):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M)
        assert m, name
        params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in " ".join(m.group(1).split()).split(",")]
        res, args = hip.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, params)
        assert params[0] == first[name] and params[-1] == "void* stream"
        for flavour in FLAVOURS:
            assert hasattr(hip.lib(flavour), name) and hip.lib(flavour).rv_abi_version() == 5
    assert hip.SIGNATURES[YUV][1][1]._type_ is hip.RvSurfacePlanes and hip.SIGNATURES[YUV][1][2]._type_ is hip.RvHdrMap
    assert hip.SIGNATURES[PACKED][1][0]._type_ is hip.RvPackedSurface and hip.SIGNATURES[RGB][1][0]._type_ is ctypes.c_void_p
    assert "rv_*" in open(os.path.join(ROOT, "revisionllm_amd", "csrc", "exports.map")).read()
    # the header says what the issue asks it to say
    for phrase in ("HOST arrays", "read at the call", "a null pointer in any entry", "is validated before the first launch", "names the frame"):
        assert phrase in header, phrase


# ---- the pointer tables of the list forms, on CPU tensors ----
class Recorder:
    """Stands in for a library handle: records the name and the arguments of every entry that is called."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def rec(monkeypatch):
    from revisionllm_amd import hip, ops
    r = Recorder()
    monkeypatch.setattr(hip, "lib", lambda f=None: r)
    monkeypatch.setattr(hip, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(hip, "stream", lambda: None)
    monkeypatch.setattr("revisionllm_amd.frontend._require_device", lambda tensors, who: None)
    return r


def struct_of(byref_arg):
    return byref_arg._obj


def test_rgb_list_forms_build_the_table(rec):
    from revisionllm_amd import ops
    H, W = 6, 10
    # NCHW frames as windows of larger, separately allocated buffers: a padded pitch, an offset, another order than the allocation order
    big = [torch.zeros(3, H + 3, W + 7, dtype=torch.uint8) for _ in range(4)]
    frames = [big[i][:, 2:2 + H, 5:5 + W] for i in (2, 0, 3, 0)]                           # frame 0 of the pool is listed twice
    p, i = ops.frames_to_patches(frames, 28, 14, want=("patches", "image"))
    assert tuple(p.shape) == (4 * 4, 640) and tuple(i.shape) == (4, 3, 28, 28)
    (name, a), = rec.calls
    assert name == RGB
    assert list(a[0]) == [f.data_ptr() for f in frames] and frames[0].data_ptr() == big[2].data_ptr() + 2 * (W + 7) + 5      # the view's offset is honoured
    assert a[1:12] == (0, 3, 0, 1, 2, (H + 3) * (W + 7), W + 7, 4, H, W, 0)                   # layout, pix, offsets, channel / row stride of frame 0, n, H, W, orient
    assert a[12:14] == (28, 14) and list(a[14]) == pytest.approx(MEAN) and a[16] == p.data_ptr() and a[17] == 640 and a[18] == i.data_ptr()
    # NHWC, bgra with a rotation, tuples
    rec.calls.clear()
    bgra = tuple(torch.zeros(H, W + 2, 4, dtype=torch.uint8)[:, 1:1 + W] for _ in range(3))
    ops.frames_to_patches(bgra, 28, 14, pix_fmt="bgra", rotate=90)
    (name, a), = rec.calls
    assert name == RGB and list(a[0]) == [f.data_ptr() for f in bgra]
    assert a[1:12] == (1, 4, 2, 1, 0, 0, 4 * (W + 2), 3, H, W, 3) and a[18] is None
    rec.calls.clear()
    nhwc = [torch.zeros(H, W, 3, dtype=torch.uint8) for _ in range(2)]
    ops.frames_to_patches(nhwc, 28, 14)
    assert rec.calls[0][0] == RGB and rec.calls[0][1][1:8] == (1, 3, 0, 1, 2, 0, 3 * W)
    # a view that cannot be passed by strides is copied frame by frame, as the tensor form copies the batch
    rec.calls.clear()
    ops.frames_to_patches([f.permute(2, 0, 1) for f in nhwc], 28, 14, layout="NCHW")
    assert rec.calls[0][1][1] == 0 and rec.calls[0][1][6:8] == (H * W, W) and list(rec.calls[0][1][0]) != [f.data_ptr() for f in nhwc]


def test_yuv_list_forms_build_the_table(rec):
    from revisionllm_amd import hip, ops
    H, W = 8, 12
    # i420-like: Y, Cb and Cr of every frame in three unrelated allocations; the Y planes on a padded pitch
    y = [torch.zeros(H, W + 4, dtype=torch.uint8)[:, :W] for _ in range(3)]
    cb = [torch.zeros(H // 2, W // 2, dtype=torch.uint8) for _ in range(3)]
    cr = [torch.zeros(H // 2, W // 2, dtype=torch.uint8) for _ in range(3)]
    ops.yuv_to_patches(y, cb, cr, R=28, patch=14, matrix="bt709", chroma_loc="centre", rotate=180)
    (name, a), = rec.calls
    s = struct_of(a[0])
    assert name == YUV and [(t.y, t.cb, t.cr) for t in a[1]] == [(p.data_ptr(), q.data_ptr(), r.data_ptr()) for p, q, r in zip(y, cb, cr)]
    assert (s.y, s.cb, s.cr, s.y_frame_stride, s.c_frame_stride) == (None, None, None, 0, 0)
    assert (s.y_row_stride, s.c_row_stride, s.sample_bytes, s.depth, s.msb_aligned, s.c_pix, s.sub_x, s.sub_y) == (W + 4, W // 2, 1, 8, 0, 1, 2, 2)
    assert (s.n, s.H, s.W, s.matrix, s.full_range, s.chroma_loc) == (3, H, W, 1, 0, 1) and a[2] is None and a[3:6] == (6, 28, 14)
    # P010-like: 16-bit words, interleaved CbCr as [h,w,2] with cr=None, PQ; strides are passed in bytes
    rec.calls.clear()
    y16 = [torch.zeros(H, W, dtype=torch.uint16) for _ in range(2)]
    c16 = [torch.zeros(H // 2, W // 2 + 1, 2, dtype=torch.uint16)[:, :W // 2] for _ in range(2)]
    ops.yuv_surface_to_patches(y16, c16, R=28, patch=14, depth=10, msb_aligned=True, matrix="bt2020", chroma_loc="topleft", transfer="pq", peak_nits=600.0)
    (name, a), = rec.calls
    s, m = struct_of(a[0]), struct_of(a[2])
    assert name == YUV and [(t.y, t.cb, t.cr) for t in a[1]] == [(p.data_ptr(), q.data_ptr(), q.data_ptr() + 2) for p, q in zip(y16, c16)]
    assert (s.y_row_stride, s.c_row_stride, s.sample_bytes, s.depth, s.msb_aligned, s.c_pix, s.sub_x, s.sub_y) == (2 * W, 2 * (W + 2), 2, 10, 1, 4, 2, 2)
    assert (m.transfer, m.gamut, m.peak_nits, m.sdr_white_nits) == (1, 1, 600.0, 203.0) and a[3] == 0
    # NV21 as two views one byte apart: the interleaved surface it is
    rec.calls.clear()
    vu = [torch.zeros(H // 2, W // 2, 2, dtype=torch.uint8) for _ in range(2)]
    ops.yuv_surface_to_patches(y[:2], [t[..., 1] for t in vu], [t[..., 0] for t in vu], R=28, patch=14)
    s = struct_of(rec.calls[0][1][0])
    assert s.c_pix == 2 and [(t.cb - t.cr) for t in rec.calls[0][1][1]] == [1, 1] and isinstance(rec.calls[0][1][1], ctypes.Array)
    assert rec.calls[0][1][1]._type_ is hip.RvSurfacePlanes


def test_packed_list_form_builds_the_table(rec):
    from revisionllm_amd import ops
    H, W = 4, 8
    rb = ops.packed_frame_bytes(1, W, "y210le")
    big = [torch.zeros(H + 2, rb + 24, dtype=torch.uint8) for _ in range(3)]
    views = [b[1:1 + H, 8:8 + rb] for b in big[::-1]]
    ops.packed_to_patches(views, H=H, W=W, pix_fmt="y210le", R=28, patch=14, matrix="bt709", hflip=True)
    (name, a), = rec.calls
    s = struct_of(a[0])
    assert name == PACKED and list(a[1]) == [v.data_ptr() for v in views] and views[0].data_ptr() == big[2].data_ptr() + rb + 24 + 8
    assert (s.base, s.frame_stride, s.row_stride, s.unit_bytes, s.pix_per_unit, s.sample_bytes, s.y_off, s.cb_off, s.cr_off) == (None, 0, rb + 24, 8, 2, 2, 0, 2, 6)
    assert (s.depth, s.msb_aligned, s.n, s.H, s.W, s.matrix) == (10, 1, 3, H, W, 1) and a[2] is None and a[3] == 2
    rec.calls.clear()
    flat = [torch.zeros(H * rb, dtype=torch.uint8) for _ in range(2)]                      # [frame bytes] per frame
    ops.packed_to_patches(flat, H=H, W=W, pix_fmt="y210le", R=28, patch=14)
    assert list(rec.calls[0][1][1]) == [f.data_ptr() for f in flat] and struct_of(rec.calls[0][1][0]).row_stride == rb


def test_value_errors_of_the_list_forms(rec):
    from revisionllm_amd import ops
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt)                                # noqa: E731
    kw = dict(R=28, patch=14)
    bad_lists = [([], "empty"),
                 ([z(3, 4, 6), "frame"], "not a tensor"),
                 ([z(3, 4, 6), z(3, 4, 8)], "disagrees"),                                   # shape
                 ([z(3, 4, 6), z(3, 4, 6, dt=torch.int16)], "disagrees"),                   # dtype
                 ([z(3, 4, 6), z(3, 4, 12)[:, :, ::2]], "disagrees"),                       # strides
                 ([z(3, 4, 6), torch.zeros(3, 4, 6, dtype=torch.uint8, device="meta")], "disagrees")]                    # device
    for frames, word in bad_lists:
        with pytest.raises(ValueError, match=word):
            ops.frames_to_patches(frames, 28, 14)
    with pytest.raises(ValueError, match="uint8 tensors"):
        ops.frames_to_patches([z(3, 4, 6).float()], 28, 14)
    with pytest.raises(ValueError, match="NCHW and as NHWC"):
        ops.frames_to_patches([z(3, 4, 3)], 28, 14)
    with pytest.raises(ValueError, match="layout"):
        ops.frames_to_patches([z(3, 4, 6)], 28, 14, layout="NHWC")
    with pytest.raises(ValueError, match="pix_fmt"):
        ops.frames_to_patches([z(4, 6, 4)], 28, 14, pix_fmt="rgb48le")
    with pytest.raises(ValueError, match="uint8 tensors"):
        ops.frames_to_patches([z(4, 6, 3)], 28, 14, pix_fmt="bgra")
    with pytest.raises(ValueError, match="rotate"):
        ops.frames_to_patches([z(3, 4, 6)], 28, 14, rotate=45)
    y, c = [z(4, 8), z(4, 8)], [z(2, 4), z(2, 4)]
    for args, word in ((([], [], []), "empty"), ((y, c[:1], c), "same frames"), ((y, c, c[:1]), "same frames"), ((y, torch.zeros(2, 2, 4), c), "must be one too"),
                       ((y, c, [c[0], None]), "not a tensor"), ((y, [z(2, 4), z(2, 5)], c), "disagrees"), ((y, [t.to(torch.uint16) for t in c], c), "one dtype"),
                       ((y, [z(2, 4, 2), z(2, 4, 2)], c), r"\[2,4\] per frame"), ((y, c), r"\[2,4,2\] per frame"), (([z(5, 8)], [z(2, 4)], [z(2, 4)]), "multiple of 2"),
                       (([z(2, 4, 8)], c[:1], c[:1]), r"\[H,W\]")):
        for fn in (ops.yuv_to_patches, ops.yuv_surface_to_patches):
            with pytest.raises(ValueError, match=word):
                fn(*args, **kw)
    with pytest.raises(ValueError, match="matrix"):
        ops.yuv_to_patches(y, c, c, matrix="bt2020", **kw)                                  # the 8-bit entry's own two matrices
    with pytest.raises(ValueError, match="uint8 planes"):
        ops.yuv_to_patches([t.to(torch.uint16) for t in y], c, c, **kw)
    with pytest.raises(ValueError, match="subsampling"):
        ops.yuv_surface_to_patches(y, c, c, subsampling="411", **kw)
    with pytest.raises(ValueError, match="transfer"):
        ops.yuv_surface_to_patches(y, c, c, transfer="gamma", **kw)
    pk = dict(H=4, W=8, pix_fmt="y210le", **kw)
    for bufs, word in (([], "empty"), ([z(4, 32), z(4, 16)], "disagrees"), ([z(4, 16)], "uint8 tensors"), ([z(4, 32).short()], "uint8 tensors"), ([z(4, 32), 7], "not a tensor"),
                       ([z(4, 33)[:, 1:]], "multiples of 2"), ([z(4, 35)[:, :32]], "multiples of 2")):
        with pytest.raises(ValueError, match=word):
            ops.packed_to_patches(bufs, **pk)
    with pytest.raises(ValueError, match="pix_fmt"):
        ops.packed_to_patches([z(4, 32)], **dict(pk, pix_fmt="nv12"))
    assert rec.calls == []                                                                    # the library was never touched


def test_the_list_forms_need_device_tensors_and_the_tensor_forms_have_not_moved():
    """Without the stand-ins: a list of CPU tensors is refused like a CPU tensor (the table would hold host addresses); a TENSOR still takes today's path - its
    own refusal, worded as before, from the code in front of the contiguous entry."""
    from revisionllm_amd import hip, ops
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8)                                       # noqa: E731
    with pytest.raises(hip.HipLibraryError, match="device tensors"):
        ops.frames_to_patches([z(3, 4, 6)], 28, 14)
    with pytest.raises(hip.HipLibraryError, match="device tensors"):
        ops.yuv_surface_to_patches([z(4, 8)], [z(2, 4)], [z(2, 4)], R=28, patch=14)
    with pytest.raises(hip.HipLibraryError, match="device tensors"):
        ops.packed_to_patches([z(4, 16)], H=4, W=8, pix_fmt="yuyv422", R=28, patch=14)
    with pytest.raises(hip.HipLibraryError, match="frames_to_patches needs a device tensor"):
        ops.frames_to_patches(z(1, 3, 4, 6), 28, 14)
    with pytest.raises(hip.HipLibraryError, match="yuv_to_patches needs device tensors"):
        ops.yuv_to_patches(z(1, 4, 8), z(1, 2, 4), z(1, 2, 4), R=28, patch=14)
    with pytest.raises(hip.HipLibraryError, match="yuv_surface_to_patches needs device tensors"):
        ops.yuv_surface_to_patches(z(1, 4, 8), z(1, 2, 4), z(1, 2, 4), R=28, patch=14)
    with pytest.raises(hip.HipLibraryError, match="packed_to_patches needs a device tensor"):
        ops.packed_to_patches(z(1, 4, 16), H=4, W=8, pix_fmt="yuyv422", R=28, patch=14)


def test_tensor_arguments_still_reach_the_contiguous_entries(rec, monkeypatch):
    """The tensor forms decide ``is_cuda`` themselves, in code this change does not touch; with that one property answered for a CPU tensor, the recorder sees the
    entries, and the arguments, of the parent commit."""
    from revisionllm_amd import ops
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    H, W = 6, 10
    f = torch.zeros(2, 3, H, W, dtype=torch.uint8)
    p, _ = ops.frames_to_patches(f, 28, 14)
    ops.frames_to_patches(f, 28, 14, rotate=90)
    ops.frames_to_patches(torch.zeros(2, H, W, 4, dtype=torch.uint8), 28, 14, pix_fmt="bgra")
    y, c = torch.zeros(2, H, W, dtype=torch.uint8), torch.zeros(2, H // 2, W // 2, dtype=torch.uint8)
    ops.yuv_to_patches(y, c, c.clone(), R=28, patch=14)
    ops.yuv_surface_to_patches(y, c, c.clone(), R=28, patch=14)
    ops.yuv_surface_to_patches(y, c, c.clone(), R=28, patch=14, transfer="hlg")
    ops.yuv_surface_to_patches(y, c, c.clone(), R=28, patch=14, vflip=True)
    ops.packed_to_patches(torch.zeros(2, H, 2 * W, dtype=torch.uint8), H=H, W=W, pix_fmt="yuyv422", R=28, patch=14)
    assert [n for n, _ in rec.calls] == ["rv_frames_to_patches", "rv_frames_to_patches_oriented", "rv_frames_to_patches_packed", "rv_yuv_to_patches",
                                         "rv_yuv_surface_to_patches", "rv_yuv_surface_to_patches_hdr", "rv_yuv_surface_to_patches_oriented", "rv_packed_to_patches"]
    a = rec.calls[0][1]
    assert a[:9] == (f.data_ptr(), 0, 3 * H * W, W, 2, H, W, 28, 14) and a[11:14] == (p.data_ptr(), 640, None)
    a = rec.calls[3][1]
    assert a[:3] == (y.data_ptr(), H * W, W) and a[3] == c.data_ptr() and a[5:11] == (H * W // 4, W // 2, 1, 2, H, W)
    s = struct_of(rec.calls[7][1][0])
    assert (s.frame_stride, s.row_stride, s.n) == (H * 2 * W, 2 * W, 2) and s.base is not None


# ---- refusals of the C entries: validation runs before any launch, so no device is needed ----
def call_rgb(lib, frames, over):
    """rv_frames_to_patches_scattered with pt.RGB_BASE's arguments (bgra, 2 frames of 6 x 8) and ``over``; frames: a list of addresses, or None."""
    a = dict(pt.RGB_BASE, layout=1, channel_stride=0, patches=0x40000, image=0x50000)
    a.update(over)
    tab = None if frames is None else (ctypes.c_void_p * len(frames))(*frames)
    f3 = ctypes.c_float * 3
    return lib.rv_frames_to_patches_scattered(tab, a["layout"], a["pix_bytes"], a["r_off"], a["g_off"], a["b_off"], a["channel_stride"], a["row_stride"], a["n"], a["H"], a["W"],
                                              a["orient"], a["R"], a["patch"], f3(*MEAN), f3(*STD), a["patches"], a["ldp"], a["image"], None)


def call_yuv(lib, hip, planes, surface=None, hdr=None, args=None, null_surface=False):
    """rv_yuv_surfaces_to_patches on test_hdr_host_logic's 96 x 64 yuv420p10le baseline; planes: a list of (y, cb, cr) addresses, or None."""
    H, W = 96, 64
    s = dict(y=None, cb=None, cr=None, y_frame_stride=1, y_row_stride=W * 2, c_frame_stride=1, c_row_stride=W, sample_bytes=2, depth=10, msb_aligned=0, c_pix=2, sub_x=2,
             sub_y=2, n=2, H=H, W=W, matrix=2, full_range=0, chroma_loc=2)                  # odd frame strides: they are not read
    s.update(surface or {})
    a = dict(R=28, patch=14, ldp=640, patches=0x40000, image=0x50000, orient=0)
    a.update(args or {})
    tab = None if planes is None else (hip.RvSurfacePlanes * len(planes))(*planes)
    m = None if hdr is None else ctypes.byref(hip.RvHdrMap(**dict(dict(transfer=1, gamut=1, peak_nits=1000.0, sdr_white_nits=203.0), **hdr)))
    f3 = ctypes.c_float * 3
    return lib.rv_yuv_surfaces_to_patches(None if null_surface else ctypes.byref(hip.RvYuvSurface(**s)), tab, m, a["orient"], a["R"], a["patch"], f3(*MEAN), f3(*STD),
                                          a["patches"], a["ldp"], a["image"], None)


def call_packed(lib, hip, bases, over, null_struct=False):
    """rv_packed_surfaces_to_patches with pt.PACKED_BASE's arguments (y210le, 2 frames of 6 x 8) and ``over``; bases: a list of addresses, or None."""
    a = dict(pt.PACKED_BASE, base=None, patches=0x40000, image=0x50000, hdr=None)
    a.update(over)
    a["frame_stride"] = 1                                                                   # not read
    s = hip.RvPackedSurface(**{k: a[k] for k, _ in hip.RvPackedSurface._fields_})
    m = hip.RvHdrMap(*a["hdr"]) if a["hdr"] else None
    tab = None if bases is None else (ctypes.c_void_p * len(bases))(*bases)
    f3 = ctypes.c_float * 3
    return lib.rv_packed_surfaces_to_patches(None if null_struct else ctypes.byref(s), tab, ctypes.byref(m) if m else None, a["orient"], a["R"], a["patch"], f3(*MEAN),
                                             f3(*STD), a["patches"], a["ldp"], a["image"], None)


GOOD3 = [(0x10000, 0x20000, 0x30000), (0x90000, 0x70000, 0x80000), (0x50000, 0x60000, 0x40000)]


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_refusals_of_the_tables(flavour):
    from revisionllm_amd import hip
    lib = hip.lib(flavour)
    err = lambda: lib_error(flavour)                                                        # noqa: E731
    # RGB
    assert call_rgb(lib, None, {}) == -1 and err() == RGB + ": null frames"
    assert call_rgb(lib, [0x10000, 0x20000, None, 0x30000], dict(n=4)) == -1 and err().startswith(RGB + ":") and "frame 2 of 4" in err()
    assert call_rgb(lib, None, dict(n=0)) == 0 and call_rgb(lib, [None], dict(n=0)) == 0
    assert call_rgb(lib, [0x10000], dict(layout=0, n=1)) == -1 and "layout 0" in err()      # NCHW takes pix_bytes 3 and offsets 0, 1, 2
    assert call_rgb(lib, [0x10000], dict(layout=2, n=1)) == -1 and "layout 2" in err()
    # the table is validated whole before the first launch: a null entry behind RV_FRAME_TABLE_MAX refuses the call with nothing launched for the first chunk
    # (a launch without a device would not return RV_ERR_ARG)
    n = hip.FRAME_TABLE_MAX + 3
    assert call_rgb(lib, [0x10000] * (n - 1) + [None], dict(n=n)) == -1 and "frame %d of %d" % (n - 1, n) in err()
    # YCbCr
    assert call_yuv(lib, hip, None) == -1 and err().startswith(YUV + ": null array")
    assert call_yuv(lib, hip, None, surface=dict(n=0)) == 0 and call_yuv(lib, hip, [(None, None, None)], surface=dict(n=0)) == 0
    assert call_yuv(lib, hip, GOOD3, surface=dict(n=3), null_surface=True) == -1 and err() == YUV + ": null surface"
    for k in (1, 2):
        for plane in range(3):
            tab = [tuple(None if (f, c) == (k, plane) else v for c, v in enumerate(t)) for f, t in enumerate(GOOD3)]
            assert call_yuv(lib, hip, tab, surface=dict(n=3)) == -1 and "null plane in frame %d of 3" % k in err(), err()
    for plane in range(3):                                                                  # a misaligned 16-bit pointer in frame 1
        tab = [tuple(v + 1 if (f, c) == (1, plane) else v for c, v in enumerate(t)) for f, t in enumerate(GOOD3)]
        assert call_yuv(lib, hip, tab, surface=dict(n=3)) == -1 and "aligned" in err() and "frame 1 of 3" in err(), err()
    assert call_yuv(lib, hip, tab, surface=dict(n=0)) == 0                                  # nothing to do: the table is not looked at
    # interleaved chroma: frame 0 sets the relation (cr = cb + 2), frame 2 has it the other way round, frame 1 has none
    inter = [(0x10000, 0x20000, 0x20002), (0x30000, 0x40000, 0x40002), (0x50000, 0x60002, 0x60000)]
    assert call_yuv(lib, hip, inter, surface=dict(n=3, c_pix=4)) == -1 and "interleaved" in err() and "frame 2 of 3" in err(), err()
    inter[2], inter[1] = (0x50000, 0x60000, 0x60002), (0x30000, 0x40000, 0x48000)
    assert call_yuv(lib, hip, inter, surface=dict(n=3, c_pix=4)) == -1 and "interleaved" in err() and "frame 1 of 3" in err(), err()
    assert call_yuv(lib, hip, [(0x10000, 0x20000, 0x20004)], surface=dict(n=1, c_pix=4)) == -1 and "interleaved" in err() and "frame 0" in err()
    # packed
    assert call_packed(lib, hip, None, {}) == -1 and err().startswith(PACKED + ": null array")
    assert call_packed(lib, hip, None, dict(n=0)) == 0
    assert call_packed(lib, hip, [0x10000, 0x20000], {}, null_struct=True) == -1 and err() == PACKED + ": null surface"
    assert call_packed(lib, hip, [0x10000, 0x20000, None], dict(n=3)) == -1 and "null base pointer for frame 2 of 3" in err()
    assert call_packed(lib, hip, [0x10000, 0x20001], {}) == -1 and "frame 1 of 2" in err() and "aligned" in err()
    assert call_packed(lib, hip, [0x10000, 0x20002], dict(pt.XV30)) == -1 and "frame 1 of 2" in err() and "32-bit" in err()


#: refusals of the contiguous entries that do not exist for a table: a frame stride is not read, and 2^30 frames would need a table of that length
NOT_FOR_TABLES = ("odd frame stride with 16-bit words", "more workgroups than a launch")


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_each_familys_own_refusals_through_the_new_entries(flavour):
    from revisionllm_amd import hip
    lib = hip.lib(flavour)
    for what, over, word in pt.RGB_REFUSALS:
        over = dict(over)
        frames = [0x10000, 0x20000] if "frames" not in over else over.pop("frames")
        assert call_rgb(lib, frames, over) == -1, what
        assert lib_error(flavour).startswith(RGB + ":") and word in lib_error(flavour), (what, lib_error(flavour))
    for what, over, word in pt.PACKED_REFUSALS:
        if what in NOT_FOR_TABLES:
            continue
        over = dict(over)
        base = over.pop("base", 0)
        bases = [None, None] if base is None else [0x10000 + int(base), 0x20000 + int(base)]
        assert call_packed(lib, hip, bases, over) == -1, what
        assert lib_error(flavour).startswith(PACKED + ":") and word in lib_error(flavour), (what, lib_error(flavour))
    for what, surface, args, word in SURFACE_REFUSALS:
        if what in NOT_FOR_TABLES:
            continue
        surface = dict(surface)
        planes = [tuple(surface.pop(k, v) for k, v in zip(("y", "cb", "cr"), t)) for t in GOOD3[:2]]
        for hdr in (None, dict(transfer=2)):
            assert call_yuv(lib, hip, planes, surface=surface, args=args, hdr=hdr) == -1, what
            assert lib_error(flavour).startswith(YUV + ":") and word in lib_error(flavour), (what, lib_error(flavour))
    for what, hdr, word in MAP_REFUSALS:
        assert call_yuv(lib, hip, GOOD3[:2], hdr=hdr) == -1, what
        assert lib_error(flavour).startswith(YUV + ":") and word in lib_error(flavour), (what, lib_error(flavour))
    for orient in (-1, 8):
        assert call_yuv(lib, hip, GOOD3[:2], args=dict(orient=orient)) == -1 and "orient" in lib_error(flavour)


# ---- the extractor's batching in both modes ----
class Towers:
    """Stands in for ClipTowers: records the frames every front-end call is handed, by their first byte."""
    device, cfg = "cpu", dict(image_res=14, patch=14, embed_dim=4)

    def __init__(self):
        self.batches = []

    def _take(self, x):
        self.batches.append(("list" if isinstance(x, (list, tuple)) else "tensor", [int(f.reshape(-1)[0]) & 255 for f in x]))
        return torch.zeros(len(x), 4)

    def encode_frames(self, frames, **kw):
        return self._take(frames)

    def encode_frames_yuv(self, y, cb, cr=None, **kw):
        assert isinstance(y, (list, tuple)) == isinstance(cb, (list, tuple)) and (cr is None or isinstance(cr, type(cb)))
        return self._take(y)

    def encode_surfaces_yuv(self, y, cb, cr=None, **kw):
        assert isinstance(y, (list, tuple)) == isinstance(cb, (list, tuple)) and (cr is None or isinstance(cr, type(cb)))
        if isinstance(y, (list, tuple)):                                                     # per-frame views of the decoder's chunks, not copies
            assert all(p.dim() == 2 for p in y) and len(cb) == len(y)
        return self._take(y)

    def encode_surfaces_packed(self, buf, **kw):
        return self._take(buf)


def numbered(n, *shape):
    """n frames of ``shape`` whose bytes all hold the frame's number."""
    return torch.arange(n, dtype=torch.uint8).view(n, *([1] * len(shape))).expand(n, *shape).contiguous()


@pytest.mark.parametrize("cuts", [(1, 5, 2), (3, 3, 3, 1), (10,), (2, 2, 2, 2, 2), (7, 3)])
def test_scattered_batches_are_the_default_batches_without_a_cat(cuts, monkeypatch):
    from revisionllm_amd import ops
    from revisionllm_amd.data.clip_extractor import ClipFeatureExtractor
    n, H, W, bsz = sum(cuts), 4, 8, 3
    runs = {"rgb": (numbered(n, 3, H, W), lambda ex, ch, **kw: ex.encode_video(ch, bsz=bsz, **kw)),
            "bgra": (numbered(n, H, W, 4), lambda ex, ch, **kw: ex.encode_video(ch, bsz=bsz, pix_fmt="bgra", **kw)),
            "nv12": (numbered(n, H * 3 // 2, W), lambda ex, ch, **kw: ex.encode_video_yuv(ch, H, W, "nv12", bsz=bsz, **kw)),
            "i420": (numbered(n, H * 3 // 2, W), lambda ex, ch, **kw: ex.encode_video_yuv(ch, H, W, "i420", bsz=bsz, **kw)),
            "p010le": (numbered(n, ops.yuv_frame_bytes(H, W, "p010le")), lambda ex, ch, **kw: ex.encode_video_pix_fmt(ch, H, W, "p010le", bsz=bsz, **kw)),
            "yuv444p10le": (numbered(n, ops.yuv_frame_bytes(H, W, "yuv444p10le")), lambda ex, ch, **kw: ex.encode_video_pix_fmt(ch, H, W, "yuv444p10le", bsz=bsz, **kw)),
            "yuyv422": (numbered(n, ops.packed_frame_bytes(H, W, "yuyv422")), lambda ex, ch, **kw: ex.encode_video_pix_fmt(ch, H, W, "yuyv422", bsz=bsz, **kw))}
    # same batch lengths, same frame order, and no torch.cat of frames (the features of the batches are still joined by one)
    for name, (frames, run) in runs.items():
        def chunks():
            at = 0
            for c in cuts:
                yield frames[at:at + c]
                at += c
        default, scattered = Towers(), Towers()
        run(ClipFeatureExtractor(default), chunks())
        real_cat = torch.cat

        def no_cat(tensors, *a, **k):
            if len(tensors) and tensors[0].dtype == torch.uint8:
                raise AssertionError("torch.cat of frames in scattered mode")
            return real_cat(tensors, *a, **k)
        monkeypatch.setattr(torch, "cat", no_cat)
        out = run(ClipFeatureExtractor(scattered), chunks(), scattered=True)
        monkeypatch.setattr(torch, "cat", real_cat)
        assert tuple(out.shape) == (n, 4)
        assert [b for _, b in scattered.batches] == [b for _, b in default.batches] == [list(range(i, min(i + bsz, n))) for i in range(0, n, bsz)], name
        assert all(kind == "list" for kind, _ in scattered.batches) and all(kind == "tensor" for kind, _ in default.batches), name
    ex = ClipFeatureExtractor(Towers())
    held = list(ex._batches(iter([frames[:2], frames[2:]]), bsz, ndim=frames.dim(), scattered=True))
    assert all(f.data_ptr() == frames[i].data_ptr() for i, f in enumerate(f for b in held for f in b))      # views: nothing was copied
    with pytest.raises(ValueError, match="uint8 tensors"):
        list(ex._batches(iter([frames.float()]), bsz, ndim=frames.dim(), scattered=True))
