"""The CLIP front end's bindings: decoded frames - RGB, planar / semi-planar YCbCr, packed YCbCr; one tensor, or a list of separately allocated frames - ->
the conv1 GEMM's patch matrix and / or the normalised image, in one launch of a fused kernel.  ``ops`` re-exports every public name.

One body per surface family serves the tensor form and the list form: a tensor of frames is taken as a list of ONE tensor whose leading axis counts the
frames, so the geometry checks, the pass-by-strides rule and the copy fallback read the same dimensions one axis further in; a list has a pointer per frame
where the tensor has ``base + f * frame_stride`` (frame stride 0, null base).  Every refusal comes before the library is touched.  ``_launch`` is the one place
that allocates the outputs and spells the entries' common tail.
"""
import torch

from . import hip

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_LAYOUTS = {"NCHW": 0, "NHWC": 1}


#: clockwise degrees by which the coded picture is turned to be displayed -> the orientation code of include/revision_hip.h (bit 0 transpose, bit 1 mirror
#: display x, bit 2 mirror display y, applied in that order)
_ROTATIONS = {0: 0, 90: 3, 180: 6, 270: 5}


def orientation(rotate=0, hflip=False, vflip=False):
    """The ``orient`` code (0 .. 7) of rv_frames_to_patches_oriented / rv_yuv_surface_to_patches_oriented.  ``rotate`` 0 | 90 | 180 | 270: the clockwise degrees
    by which the coded picture must be turned to be displayed (mp4's ``rotate`` tag; the NEGATIVE of ffprobe's display-matrix ``rotation``); ``hflip`` /
    ``vflip``: mirror the turned picture left-right / top-bottom.  Anything else is refused."""
    if isinstance(rotate, bool) or not isinstance(rotate, int) or rotate not in _ROTATIONS:
        raise ValueError(f"rotate {rotate!r}: one of {sorted(_ROTATIONS)} (clockwise degrees; ffprobe's display-matrix rotation is the negative)")
    if not isinstance(hflip, bool) or not isinstance(vflip, bool):
        raise ValueError(f"hflip {hflip!r} / vflip {vflip!r}: True or False")
    return _ROTATIONS[rotate] ^ (2 if hflip else 0) ^ (4 if vflip else 0)      # the mirrors come last in the code and commute: a flip toggles its bit


#: ffmpeg's pix_fmt names of packed 8-bit RGB -> (bytes per pixel, byte offsets of R, G, B inside it); a fourth byte (alpha or padding) is never read
RGB_PIX_FMTS = {
    "rgb24": (3, 0, 1, 2), "bgr24": (3, 2, 1, 0), "rgba": (4, 0, 1, 2), "bgra": (4, 2, 1, 0), "argb": (4, 1, 2, 3), "abgr": (4, 3, 2, 1),
    "rgb0": (4, 0, 1, 2), "bgr0": (4, 2, 1, 0), "0rgb": (4, 1, 2, 3), "0bgr": (4, 3, 2, 1),
}


# ---- what the families share ----
def _frame_list(frames, who, what="frames"):
    """The checks every list form shares: a list / tuple of per-frame tensors (separately allocated surfaces, or views of larger ones) that agree in dtype,
    device, shape and strides, so that one geometry and one set of pitches serve the whole batch.  ValueError otherwise, before the library is touched."""
    if len(frames) == 0:
        raise ValueError(f"{who}: an empty list of {what} has no frame to take the shape, the dtype and the device from")
    for i, t in enumerate(frames):
        if not torch.is_tensor(t):
            raise ValueError(f"{who}: {what}[{i}] is a {type(t).__name__}, not a tensor")
    e = frames[0]
    for i, t in enumerate(frames):
        if t.dtype != e.dtype or t.device != e.device or t.shape != e.shape or t.stride() != e.stride():
            raise ValueError(f"{who}: {what}[{i}] ({t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}) disagrees with {what}[0] ({e.dtype} {tuple(e.shape)} "
                             f"strides {e.stride()} on {e.device}): the frames of a list share dtype, device, shape and strides")
    return list(frames)


def _no_cpu_path(who, what):
    return hip.HipLibraryError(f"{who} needs {what} (got a CPU tensor); there is no CPU path")


def _require_device(tensors, who):
    """The list forms' device check: the pointer tables hold device addresses, there is no CPU path."""
    if not all(t.is_cuda for t in tensors):
        raise _no_cpu_path(who, "device tensors")


def _device_tensor(t, who, what):
    """The tensor forms' device check."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _no_cpu_path(who, what)


#: how the tensor form (False) and the list form (True) of one refusal differ: (the frame axis inside a shape, "in a list", what the frames come as)
_WORDS = {False: ("n,", "", "a uint8 tensor"), True: ("", " in a list", "uint8 tensors")}


def _dims(shape):
    return "[" + ",".join(str(d) for d in shape) + "]"


def _got(t):
    return f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(t).__name__


def _rows_of_samples(t, a, n, rows, cols, pix):
    """Can a plane [rows,cols] (``a`` = 0), or the planes [n,rows,cols] of a batch (``a`` = 1), be passed by strides?  Samples of a row ``pix`` apart, rows
    and frames in ascending order (a dimension of extent 1 has no stride to speak of)."""
    return (cols == 1 or t.stride(a + 1) == pix) and (rows == 1 or t.stride(a) >= pix * cols) and (a == 0 or n <= 1 or t.stride(0) > 0)


def _plane_strides(t, a, n, rows, cols, pix):
    """(frame stride, row stride) of a plane ``_rows_of_samples`` accepted; the frames of a list (``a`` = 0) have a pointer each and no frame stride."""
    rs = t.stride(a) if rows > 1 else pix * cols
    return (0 if a == 0 else t.stride(0) if n > 1 else rs * rows), rs


def _copies(frames):
    return [t.contiguous() for t in frames]


def _ref(struct):
    return None if struct is None else hip.C.byref(struct)


def _launch(entry, head, n, device, out):
    """The one call site of the front end's entries: allocates the outputs of ``n`` frames and calls ``entry`` with its own leading arguments ``head`` and the
    tail all eleven share.  ``out``: the wrappers' (R, patch, mean, std, op_dtype, want) -> (patches, image)."""
    R, patch, mean, std, op_dtype, want = out
    dt = hip.op_dtype(op_dtype)
    g = R // max(patch, 1)
    kp = (3 * patch * patch + 127) // 128 * 128
    patches = torch.empty(n * g * g, kp, dtype=dt, device=device) if "patches" in want else None
    image = torch.empty(n, 3, R, R, dtype=torch.float32, device=device) if "image" in want else None
    f3 = hip.C.c_float * 3
    hip.check(getattr(hip.lib(dt), entry)(*head, R, patch, f3(*mean), f3(*std), hip.ptr(patches), kp, hip.ptr(image), hip.stream()), entry)
    return patches, image


# ---- RGB ----
def _rgb_format(pix_fmt, layout, ax="n,"):
    """(bytes per pixel, offsets of R, G, B) of a packed RGB ``pix_fmt``, which goes with NHWC alone; ``ax``: the frame axis in the shape the refusal names."""
    if pix_fmt not in RGB_PIX_FMTS:
        raise ValueError(f"pix_fmt {pix_fmt!r}: one of {sorted(RGB_PIX_FMTS)} (packed 8-bit RGB)")
    if layout not in (None, "NHWC"):
        raise ValueError(f"pix_fmt {pix_fmt!r} names the byte order of packed pixels [{ax}H,W,{RGB_PIX_FMTS[pix_fmt][0]}]: layout {layout!r} does not go with it")
    return RGB_PIX_FMTS[pix_fmt]


def frames_to_patches(frames, R, patch, layout=None, mean=CLIP_MEAN, std=CLIP_STD, op_dtype=None, want=("patches",), *, rotate=0, hflip=False, vflip=False,
                      pix_fmt=None):
    """Decoded uint8 frames -> the CLIP front end in one launch (rv_frames_to_patches): Resize(R, antialiased bicubic) / CenterCrop(R) /
    (x / 255 - mean) / (std + 1e-8), then -> (patches, image): ``patches`` [n*g*g, Kp] of the operand type (the conv1 GEMM's A matrix: rows (frame, gy, gx),
    columns (channel, py, px), zero-padded from 3 * patch^2 to a multiple of 128), ``image`` f32 [n,3,R,R]; the one ``want`` does not name is None.
    frames: uint8 device tensor [n,3,H,W] ("NCHW") or [n,H,W,3] ("NHWC"); ``layout`` is inferred when only one reading fits.  A window of a larger buffer
    is passed by its strides (pixels of a row adjacent, NCHW channel planes a third of the frame stride apart); any other view is copied first.
    ``rotate`` / ``hflip`` / ``vflip`` (``orientation``): the frames are CODED sideways or upside down (a ``-noautorotate`` pipe, a hardware decoder) and are
    turned and flipped inside the same launch (rv_frames_to_patches_oriented) - resize and crop are those of the displayed picture, no copy is made.
    ``pix_fmt`` (one of ``RGB_PIX_FMTS``: "bgr24" is what ``cv2.VideoCapture`` hands over, "bgra" / "rgba" / "argb" ... what screen capture and colour converters
    do): the frames are [n,H,W,3] or [n,H,W,4] in that byte order and are read as they lie (rv_frames_to_patches_packed) - the bits of the call on a contiguous
    RGB copy, without the copy; a fourth byte is ignored.  ``None`` is the call as it always was.
    ``frames`` may also be a LIST (or tuple) of per-frame tensors [3,H,W] / [H,W,3] (with ``pix_fmt`` [H,W,3|4]) - the surfaces of a decoder's pool, the slots
    of a capture ring, views of larger buffers: separately allocated frames that agree in dtype, device, shape and strides go through ONE launch per 64 frames
    by a table of their pointers (rv_frames_to_patches_scattered), with no ``torch.stack`` in front; the bits are those of the call on the stacked tensor."""
    who = "frames_to_patches"
    orient = orientation(rotate, hflip, vflip)
    listed = isinstance(frames, (list, tuple))
    frames, a = (_frame_list(frames, who), 0) if listed else ([frames], 1)
    e = frames[0]
    if pix_fmt is not None:
        pix, r, g, b = _rgb_format(pix_fmt, layout, _WORDS[listed][0])
        layout = "NHWC"
    else:
        pix, r, g, b = 3, 0, 1, 2
        if not listed:                                                      # the plain tensor form asks for the device before it looks at the shape
            _device_tensor(e, who, "a device tensor")
    if not torch.is_tensor(e) or e.dtype != torch.uint8 or e.dim() != a + 3 or (pix_fmt is not None and e.shape[a + 2] != pix):
        ax, in_a_list, tensors = _WORDS[listed]
        if pix_fmt is not None:
            raise ValueError(f"{pix_fmt} frames{in_a_list} come as {tensors} [{ax}H,W,{pix}], got {_got(e)}")
        raise (ValueError if listed else hip.HipLibraryError)(f"frames{in_a_list} come as {tensors} [{ax}3,H,W] or [{ax}H,W,3], got {_got(e)}")
    if pix_fmt is None:
        nchw, nhwc = e.shape[a] == 3, e.shape[a + 2] == 3
        if layout is None:
            if nchw == nhwc:
                raise ValueError(f"frames of shape {tuple(e.shape)} read as " + ("NCHW and as NHWC: pass layout=" if nchw else "neither NCHW nor NHWC"))
            layout = "NCHW" if nchw else "NHWC"
        if layout not in _LAYOUTS or not (nchw if layout == "NCHW" else nhwc):
            raise ValueError(f"layout {layout!r} does not fit frames of shape {tuple(e.shape)}")
    if listed:
        _require_device(frames, who)
    elif pix_fmt is not None:
        _device_tensor(e, who, "a device tensor")
    n = len(frames) if listed else e.shape[0]
    if layout == "NCHW":                    # channel planes a channel stride apart, and in a tensor the frames three of those
        H, W = e.shape[a + 1:]
        if not (e.stride(a + 2) == 1 and e.stride(a + 1) >= W and e.stride(a) > 0 and (listed or n <= 1 or e.stride(0) == 3 * e.stride(1))):
            frames = _copies(frames)
        cs, rs = frames[0].stride(a), frames[0].stride(a + 1)
        fs = 3 * cs
    else:                                   # pixels of ``pix`` adjacent bytes
        H, W = e.shape[a:a + 2]
        if not (e.stride(a + 2) == 1 and e.stride(a + 1) == pix and e.stride(a) >= pix * W and (listed or n <= 1 or e.stride(0) > 0)):
            frames = _copies(frames)
        cs, rs = 0, frames[0].stride(a)
        fs = frames[0].stride(0) if n > 1 else rs * H
    out = (R, patch, mean, std, op_dtype, want)
    if listed:
        table = (hip.C.c_void_p * n)(*[t.data_ptr() for t in frames])
        return _launch("rv_frames_to_patches_scattered", (table, _LAYOUTS[layout], pix, r, g, b, cs, rs, n, H, W, orient), n, e.device, out)
    if pix_fmt is not None:
        return _launch("rv_frames_to_patches_packed", (hip.ptr(frames[0]), pix, r, g, b, fs, rs, n, H, W, orient), n, e.device, out)
    if orient:
        return _launch("rv_frames_to_patches_oriented", (hip.ptr(frames[0]), _LAYOUTS[layout], fs, rs, n, H, W, orient), n, e.device, out)
    return _launch("rv_frames_to_patches", (hip.ptr(frames[0]), _LAYOUTS[layout], fs, rs, n, H, W), n, e.device, out)


# ---- planar / semi-planar YCbCr ----
_MATRICES = {"bt601": 0, "bt709": 1}
_CHROMA_LOCS = {"left": 0, "centre": 1}
_YUV_FORMATS = ("nv12", "nv21", "i420")
_SURFACE_MATRICES = {"bt601": 0, "bt709": 1, "bt2020": 2}
_SURFACE_LOCS = {"left": 0, "centre": 1, "topleft": 2}
_SUBSAMPLINGS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}


def _plane_tensors(who, y, cb, cr, dtypes, takes):
    """The tensor forms' first look at their planes: device tensors of one of ``dtypes``, all of Y's."""
    for t in (y, cb) + (() if cr is None else (cr,)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _no_cpu_path(who, "device tensors")
        if t.dtype not in dtypes or t.dtype != y.dtype:
            raise hip.HipLibraryError(f"{who} takes {takes}, got {t.dtype} {tuple(t.shape)}")


def _yuv_planes(who, y, cb, cr, listed, sx, sy):
    """The planes of a surface subsampled by ``sx`` x ``sy``, tensors [n,..] or lists of per-frame planes, checked and made passable by strides ->
    (y, cb, cr, y frame stride, y row stride, chroma frame stride, chroma row stride, c_pix, n, H, W, sample bytes): lists of planes (of one tensor for the
    tensor form), Cb and Cr as [..,h,w] views that one stride pair serves, strides in samples, c_pix 2 where they are the halves of interleaved pairs."""
    refuse = ValueError if listed else hip.HipLibraryError
    if listed:
        lists = [("y", y), ("cb", cb)] + ([] if cr is None else [("cr", cr)])
        for name, l in lists:
            if not isinstance(l, (list, tuple)):
                raise ValueError(f"{who}: y is a list of per-frame planes, so {name} must be one too (got a {type(l).__name__})")
        y, cb = _frame_list(y, who, "y"), _frame_list(cb, who, "cb")
        cr = None if cr is None else _frame_list(cr, who, "cr")
        n, e = len(y), y[0]
        if len(cb) != n or (cr is not None and len(cr) != n):
            raise ValueError(f"{who}: {n} Y planes, {len(cb)} Cb planes" + ("" if cr is None else f", {len(cr)} Cr planes") + ": the lists name the same frames")
        for name, l in lists[1:]:
            if l[0].dtype != e.dtype or l[0].device != e.device:
                raise ValueError(f"{who}: {name} planes are {l[0].dtype} on {l[0].device}, Y planes {e.dtype} on {e.device}: one dtype, one device")
        if e.dtype not in (torch.uint8, torch.uint16):
            raise ValueError(f"{who} takes planes of one dtype, uint8 or uint16, got {e.dtype}")
    else:
        y, cb, cr, e = [y], [cb], None if cr is None else [cr], y
    a = 0 if listed else 1
    if e.dim() != a + 2 or e.shape[a] % sy or e.shape[a + 1] % sx:
        raise refuse(f"{who}: Y planes{_WORDS[listed][1]} are [{_WORDS[listed][0]}H,W] with H a multiple of {sy} and W of {sx}, got {tuple(e.shape)}")
    if not listed:
        n = e.shape[0]
    H, W = e.shape[a:]
    h, w, es = H // sy, W // sx, e.element_size()
    frames = () if listed else (n,)
    if cr is None:
        if tuple(cb[0].shape) != frames + (h, w, 2):
            raise refuse(f"{who}: interleaved CbCr of frames {H} x {W} is {_dims(frames + (h, w, 2))}{' per frame' if listed else ''}, got {tuple(cb[0].shape)}")
        if not (cb[0].stride(a + 2) == 1 and _rows_of_samples(cb[0], a, n, h, w, 2)):
            cb = _copies(cb)
        cb, cr = [t[..., 0] for t in cb], [t[..., 1] for t in cb]
    elif tuple(cb[0].shape) != frames + (h, w) or tuple(cr[0].shape) != frames + (h, w):
        raise refuse(f"{who}: Cb and Cr of frames {H} x {W} are {_dims(frames + (h, w))}{' per frame' if listed else ''}, got {tuple(cb[0].shape)} and {tuple(cr[0].shape)}")
    if not _rows_of_samples(e, a, n, H, W, 1):
        y = _copies(y)
    b, r = cb[0], cr[0]
    if abs(b.data_ptr() - r.data_ptr()) == es and b.stride() == r.stride() and _rows_of_samples(b, a, n, h, w, 2):
        c_pix = 2                           # two views one sample apart: the interleaved surface they are
    else:
        c_pix = 1
        if not (b.stride() == r.stride() and _rows_of_samples(b, a, n, h, w, 1)):
            cb, cr = _copies(cb), _copies(cr)
    if listed:
        _require_device(y + cb + cr, who)
    return (y, cb, cr) + _plane_strides(y[0], a, n, H, W, 1) + _plane_strides(cb[0], a, n, h, w, c_pix) + (c_pix, n, H, W, es)


def _yuv_surface_launch(planes, listed, depth, msb_aligned, sx, sy, matrix, full_range, chroma_loc, hdr, orient, out):
    """``_yuv_planes`` and the surface's tags -> the rv_yuv_surface and the entry that goes with the form, the orientation and the HDR map."""
    y, cb, cr, yfs, yrs, cfs, crs, c_pix, n, H, W, es = planes
    base = (None, None, None) if listed else (y[0].data_ptr(), cb[0].data_ptr(), cr[0].data_ptr())
    s = hip.RvYuvSurface(*base, yfs * es, yrs * es, cfs * es, crs * es, es, int(depth), int(bool(msb_aligned)), c_pix * es, sx, sy, n, H, W, matrix,
                         int(bool(full_range)), chroma_loc)
    if listed:
        table = (hip.RvSurfacePlanes * n)(*[(p.data_ptr(), q.data_ptr(), r.data_ptr()) for p, q, r in zip(y, cb, cr)])
        return _launch("rv_yuv_surfaces_to_patches", (hip.C.byref(s), table, _ref(hdr), orient), n, y[0].device, out)
    if orient:
        return _launch("rv_yuv_surface_to_patches_oriented", (hip.C.byref(s), _ref(hdr), orient), n, y[0].device, out)
    if hdr is not None:
        return _launch("rv_yuv_surface_to_patches_hdr", (hip.C.byref(s), hip.C.byref(hdr)), n, y[0].device, out)
    return _launch("rv_yuv_surface_to_patches", (hip.C.byref(s),), n, y[0].device, out)


def yuv_to_patches(y, cb, cr=None, *, R, patch, matrix="bt601", full_range=False, chroma_loc="left", mean=CLIP_MEAN, std=CLIP_STD, op_dtype=None,
                   want=("patches",), rotate=0, hflip=False, vflip=False):
    """Decoded 8-bit 4:2:0 YCbCr frames -> the CLIP front end in one launch (rv_yuv_to_patches; the header has the definition of the values): Y resampled at
    full, Cb / Cr at half resolution, colour matrix per output pixel, then everything ``frames_to_patches`` does -> (patches, image) as it returns them.
    y: uint8 device tensor [n,H,W] (H, W even).  Chroma, either of
      * ``cb`` [n,H/2,W/2,2] with ``cr=None``: interleaved CbCr (NV12);
      * ``cb`` and ``cr`` [n,H/2,W/2] each: two planes (I420), or two views one byte apart with a sample stride of 2 (NV21 / NV12 as ``split_yuv420``
        hands them over): those are read as the interleaved surface they are.
    Planes are passed by their strides when each row's bytes are adjacent (a window of a larger decode surface, a padded pitch); any other view is copied first.
    matrix "bt601" | "bt709"; full_range False = studio; chroma_loc "left" (MPEG-2 / H.264) | "centre" (JPEG / MPEG-1).
    ``rotate`` / ``hflip`` / ``vflip`` (``orientation``): the planes are the CODED surface of a stream that is displayed turned or flipped; they go through
    rv_yuv_surface_to_patches_oriented as the 8-bit 4:2:0 surface they are (``yuv_surface_to_patches`` says what orientation does to the siting).
    ``y`` / ``cb`` / ``cr`` may also be LISTS of per-frame planes (y [H,W]; cb [H/2,W/2,2], or cb and cr [H/2,W/2]) of equal length, as
    ``yuv_surface_to_patches`` takes them: separately allocated surfaces in one launch, without a stacking copy."""
    who = "yuv_to_patches"
    orient = orientation(rotate, hflip, vflip)
    listed = isinstance(y, (list, tuple))
    if not listed:
        _plane_tensors(who, y, cb, cr, (torch.uint8,), "uint8 planes")
    if matrix not in _MATRICES or chroma_loc not in _CHROMA_LOCS:
        raise ValueError(f"matrix {matrix!r} / chroma_loc {chroma_loc!r}: one of {sorted(_MATRICES)} / {sorted(_CHROMA_LOCS)}")
    if listed and y and torch.is_tensor(y[0]) and y[0].dtype != torch.uint8:
        raise ValueError(f"{who} takes uint8 planes, got {y[0].dtype}")
    planes = _yuv_planes(who, y, cb, cr, listed, 2, 2)
    out = (R, patch, mean, std, op_dtype, want)
    if listed or orient:                    # as the 8-bit 4:2:0 surface they are
        return _yuv_surface_launch(planes, listed, 8, False, 2, 2, _MATRICES[matrix], full_range, _CHROMA_LOCS[chroma_loc], None, orient, out)
    y, cb, cr, yfs, yrs, cfs, crs, c_pix, n, H, W, _ = planes
    return _launch("rv_yuv_to_patches", (hip.ptr(y[0]), yfs, yrs, hip.ptr(cb[0]), hip.ptr(cr[0]), cfs, crs, c_pix, n, H, W, _MATRICES[matrix], int(bool(full_range)),
                                         _CHROMA_LOCS[chroma_loc]), n, y[0].device, out)


def split_yuv420(buf, H, W, fmt):
    """The bytes of a rawvideo pipe (``ffmpeg -f rawvideo -pix_fmt nv12 | nv21 | yuv420p``) -> zero-copy views ``(y, cb, cr_or_None)`` that ``yuv_to_patches``
    takes without a copy.  buf: uint8 [n, H*3//2, W] (CPU or device; each frame's H * W * 3 / 2 bytes adjacent), H and W even.
      nv12: y [n,H,W], cbcr [n,H/2,W/2,2], None        nv21: y, cb = vu[..., 1], cr = vu[..., 0] (sample stride 2, one byte apart)
      i420: y, cb [n,H/2,W/2] at byte H * W of each frame, cr at H * W * 5 / 4"""
    if fmt not in _YUV_FORMATS:
        raise ValueError(f"fmt {fmt!r}: one of {_YUV_FORMATS}")
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"4:2:0 frames have even sides of at least 2, got {H} x {W}")
    if not torch.is_tensor(buf) or buf.dtype != torch.uint8 or buf.dim() != 3 or tuple(buf.shape[1:]) != (H * 3 // 2, W):
        raise ValueError(f"{fmt} frames of {H} x {W} come as a uint8 tensor [n,{H * 3 // 2},{W}], got {_got(buf)}")
    if buf.stride(2) != 1 or buf.stride(1) != W:
        raise ValueError("split_yuv420 returns views: the bytes of each frame must be adjacent (a padded surface is passed to yuv_to_patches plane by plane)")
    n, h2, w2 = buf.shape[0], H // 2, W // 2
    y = buf[:, :H]
    if fmt == "i420":
        fs, at = buf.stride(0), buf.storage_offset()
        cb = buf.as_strided((n, h2, w2), (fs, w2, 1), at + H * W)
        cr = buf.as_strided((n, h2, w2), (fs, w2, 1), at + H * W + h2 * w2)
        return y, cb, cr
    pairs = buf[:, H:].unflatten(2, (w2, 2))
    return (y, pairs, None) if fmt == "nv12" else (y, pairs[..., 1], pairs[..., 0])


#: ffmpeg's pix_fmt names -> (bytes per sample, depth, value in the high bits, subsampling, chroma layout: "planar" Cb plane then Cr plane | "cbcr" | "crcb"
#: interleaved pairs)
PIX_FMTS = {
    "nv12": (1, 8, False, "420", "cbcr"), "nv21": (1, 8, False, "420", "crcb"), "nv16": (1, 8, False, "422", "cbcr"), "nv24": (1, 8, False, "444", "cbcr"),
    "yuv420p": (1, 8, False, "420", "planar"), "yuv422p": (1, 8, False, "422", "planar"), "yuv444p": (1, 8, False, "444", "planar"),
    "yuv420p10le": (2, 10, False, "420", "planar"), "yuv422p10le": (2, 10, False, "422", "planar"), "yuv444p10le": (2, 10, False, "444", "planar"),
    "yuv420p12le": (2, 12, False, "420", "planar"), "yuv444p12le": (2, 12, False, "444", "planar"), "yuv420p16le": (2, 16, False, "420", "planar"),
    "p010le": (2, 10, True, "420", "cbcr"), "p016le": (2, 16, True, "420", "cbcr"), "p210le": (2, 10, True, "422", "cbcr"), "p410le": (2, 10, True, "444", "cbcr"),
}


#: transfer characteristics of an HDR surface -> rv_hdr_map.transfer; ffmpeg's ``color_trc`` names are aliases
_TRANSFERS = {"pq": 1, "smpte2084": 1, "hlg": 2, "arib-std-b67": 2}


def hdr_map(transfer, matrix="bt2020", gamut=None, peak_nits=1000.0, sdr_white_nits=203.0):
    """The ``hip.RvHdrMap`` that ``yuv_surface_to_patches`` hands to rv_yuv_surface_to_patches_hdr, or None for ``transfer=None`` (an SDR surface).
    transfer "pq" | "hlg" ("smpte2084" | "arib-std-b67", ffmpeg's ``color_trc`` names, are aliases); ``gamut`` None = BT.2020 -> BT.709 primaries exactly
    when ``matrix == "bt2020"``, else True / False.  The range of ``peak_nits`` / ``sdr_white_nits`` (1 .. 10000) is the library's check."""
    if transfer is None:
        return None
    if transfer not in _TRANSFERS:
        raise ValueError(f"transfer {transfer!r}: None or one of {sorted(_TRANSFERS)}")
    return hip.RvHdrMap(_TRANSFERS[transfer], int(matrix == "bt2020" if gamut is None else bool(gamut)), float(peak_nits), float(sdr_white_nits))


def yuv_surface_to_patches(y, cb, cr=None, *, R, patch, depth=8, msb_aligned=False, subsampling="420", matrix="bt601", full_range=False, chroma_loc="left",
                           mean=CLIP_MEAN, std=CLIP_STD, op_dtype=None, want=("patches",), transfer=None, peak_nits=1000.0, sdr_white_nits=203.0, gamut=None,
                           rotate=0, hflip=False, vflip=False):
    """Decoded YCbCr frames of any planar / semi-planar surface -> the CLIP front end in one launch (rv_yuv_surface_to_patches; the header has the definition of
    the values) -> (patches, image) as ``frames_to_patches`` returns them.
    Planes are ``torch.uint8`` (depth 8) or ``torch.uint16`` (depth 9 .. 16; ``msb_aligned``: the value sits in the high bits of the word, as in P010 /
    P016) device tensors, all of one dtype.  y [n,H,W]; with ``subsampling`` "420" | "422" | "444" the chroma planes hold h x w = H/2 x W/2 | H x W/2 | H x W
    samples (H, W even along a halved axis only), either of
      * ``cb`` [n,h,w,2] with ``cr=None``: interleaved CbCr (NV12, NV16, P010 ...);
      * ``cb`` and ``cr`` [n,h,w] each: two planes, or two views one sample apart with a sample stride of 2 (as ``split_yuv`` hands over NV21): those are
        read as the interleaved surface they are.
    Planes are passed by their strides when each row's samples are adjacent (a window of a larger decode surface, a padded pitch); any other view is copied
    first.  matrix "bt601" | "bt709" | "bt2020" (the non-constant-luminance matrix alone: no transfer conversion); full_range False = studio; chroma_loc
    "left" (MPEG-2 / H.264) | "centre" (JPEG / MPEG-1) | "topleft" (BT.2020 / HEVC 4:2:0).
    HDR surfaces: ``transfer`` "pq" | "hlg" (``hdr_map`` has the aliases) converts the values to BT.709-coded SDR per output pixel inside the same kernel
    (rv_yuv_surface_to_patches_hdr: transfer to display light with ``peak_nits`` as the display peak, BT.2390 tone mapping with ``sdr_white_nits`` becoming
    SDR white, BT.2020 -> BT.709 primaries when ``gamut`` - None: exactly when ``matrix == "bt2020"`` -, BT.709 OETF).  No metadata is read: ``peak_nits`` is
    the caller's number.  ``transfer=None`` is the SDR entry, which ignores the other three.
    Orientation: ``rotate`` 0 | 90 | 180 | 270 (clockwise degrees to display: mp4's ``rotate`` tag), then ``hflip`` / ``vflip`` (``orientation``).  The planes,
    ``subsampling`` and ``chroma_loc`` describe the CODED surface; it is turned and flipped inside the same kernel (rv_yuv_surface_to_patches_oriented), SDR or
    HDR: resize and crop are those of the displayed picture, the siting follows its axis and changes side where that axis is mirrored, and a turned 4:2:2
    surface (4:4:0 on the display) is taken as the 4:2:2 surface it is.  The identity is the un-oriented entry.
    Surface pools: ``y`` / ``cb`` / ``cr`` may also be LISTS (or tuples) of per-frame planes of equal length - y [H,W]; cb [h,w,2] with ``cr=None``, or cb and
    cr [h,w] each, which may be three unrelated allocations per frame.  The frames of a list agree in dtype, device, shape and strides (one pitch for the
    pool); each may be a view of a larger surface.  They go through one launch per 64 frames by a table of their pointers (rv_yuv_surfaces_to_patches): no
    ``torch.stack``, and the bits of the call on the stacked planes.  Every other keyword behaves as it does for tensors."""
    who = "yuv_surface_to_patches"
    orient = orientation(rotate, hflip, vflip)
    hdr = hdr_map(transfer, matrix, gamut, peak_nits, sdr_white_nits)
    listed = isinstance(y, (list, tuple))
    if not listed:
        _plane_tensors(who, y, cb, cr, (torch.uint8, torch.uint16), "planes of one dtype, uint8 or uint16")
    if matrix not in _SURFACE_MATRICES or chroma_loc not in _SURFACE_LOCS or subsampling not in _SUBSAMPLINGS:
        raise ValueError(f"matrix {matrix!r} / chroma_loc {chroma_loc!r} / subsampling {subsampling!r}: one of {sorted(_SURFACE_MATRICES)} / "
                         f"{sorted(_SURFACE_LOCS)} / {sorted(_SUBSAMPLINGS)}")
    sx, sy = _SUBSAMPLINGS[subsampling]
    return _yuv_surface_launch(_yuv_planes(who, y, cb, cr, listed, sx, sy), listed, depth, msb_aligned, sx, sy, _SURFACE_MATRICES[matrix], full_range,
                               _SURFACE_LOCS[chroma_loc], hdr, orient, (R, patch, mean, std, op_dtype, want))


def yuv_frame_bytes(H, W, pix_fmt):
    """Bytes of one ``H`` x ``W`` frame of a rawvideo pipe in ffmpeg's ``pix_fmt`` (one of ``PIX_FMTS``)."""
    if pix_fmt not in PIX_FMTS:
        raise ValueError(f"pix_fmt {pix_fmt!r}: one of {sorted(PIX_FMTS)}")
    sb, _, _, sub, _ = PIX_FMTS[pix_fmt]
    sx, sy = _SUBSAMPLINGS[sub]
    if H < sy or W < sx or H % sy or W % sx:
        raise ValueError(f"{pix_fmt} frames ({sub}) have H a multiple of {sy} and W a multiple of {sx}, got {H} x {W}: odd along a subsampled axis")
    return (H * W + 2 * (H // sy) * (W // sx)) * sb


def split_yuv(buf, H, W, pix_fmt):
    """The bytes of a rawvideo pipe (``ffmpeg -f rawvideo -pix_fmt <one of PIX_FMTS>``) -> ``((y, cb, cr_or_None), kw)``: zero-copy views of the planes (uint8,
    or uint16 for the 16-bit formats) and the keyword arguments (``depth``, ``msb_aligned``, ``subsampling``) that go with them, so that
    ``yuv_surface_to_patches(*planes, R=R, patch=patch, **kw, **colour)`` reads the buffer as it lies.  buf: uint8 [n, yuv_frame_bytes(H, W, pix_fmt)], CPU
    or device, each frame's bytes adjacent.  Interleaved CbCr comes as ``cb`` [n,h,w,2] with ``cr`` None; CrCb (nv21) as two views one sample apart."""
    fb = yuv_frame_bytes(H, W, pix_fmt)
    sb, depth, msb, sub, layout = PIX_FMTS[pix_fmt]
    if not torch.is_tensor(buf) or buf.dtype != torch.uint8 or buf.dim() != 2 or buf.shape[1] != fb:
        raise ValueError(f"{pix_fmt} frames of {H} x {W} come as a uint8 tensor [n,{fb}], got {_got(buf)}")
    if buf.stride(1) != 1:
        raise ValueError("split_yuv returns views: the bytes of each frame must be adjacent (a padded surface is passed to yuv_surface_to_patches plane by plane)")
    if sb == 2:
        if buf.stride(0) % 2 or buf.storage_offset() % 2:
            raise ValueError(f"{pix_fmt}: 16-bit words must be adjacent bytes at an even offset (frame stride {buf.stride(0)}, offset {buf.storage_offset()})")
        buf = buf.view(torch.uint16)
    sx, sy = _SUBSAMPLINGS[sub]
    n, h, w = buf.shape[0], H // sy, W // sx
    fs, at = buf.stride(0), buf.storage_offset()
    y = buf.as_strided((n, H, W), (fs, W, 1), at)
    kw = dict(depth=depth, msb_aligned=msb, subsampling=sub)
    if layout == "planar":
        return (y, buf.as_strided((n, h, w), (fs, w, 1), at + H * W), buf.as_strided((n, h, w), (fs, w, 1), at + H * W + h * w)), kw
    pairs = buf.as_strided((n, h, w, 2), (fs, 2 * w, 2, 1), at + H * W)
    return ((y, pairs, None) if layout == "cbcr" else (y, pairs[..., 1], pairs[..., 0])), kw


# ---- packed YCbCr ----
#: ffmpeg's pix_fmt names of PACKED YCbCr surfaces -> (unit bytes, pixels per unit, sample bytes, offset of Y / Cb / Cr inside the unit, depth, value in the high
#: bits): the fields of rv_packed_surface (include/revision_hip.h has the layouts).  Offsets are bytes (the first Y sample's; with 2 pixels per unit the second one
#: lies half a unit behind it), or bit shifts for the 32-bit word of three 10-bit fields (sample bytes 4).
PACKED_PIX_FMTS = {
    "yuyv422": (4, 2, 1, 0, 1, 3, 8, False), "uyvy422": (4, 2, 1, 1, 0, 2, 8, False), "yvyu422": (4, 2, 1, 0, 3, 1, 8, False),
    "y210le": (8, 2, 2, 0, 2, 6, 10, True), "y212le": (8, 2, 2, 0, 2, 6, 12, True),
    "ayuv": (4, 1, 1, 1, 2, 3, 8, False), "vuya": (4, 1, 1, 2, 1, 0, 8, False), "vuyx": (4, 1, 1, 2, 1, 0, 8, False), "uyva": (4, 1, 1, 1, 0, 2, 8, False),
    "ayuv64le": (8, 1, 2, 2, 4, 6, 16, False), "xv36le": (8, 1, 2, 2, 0, 4, 12, True), "xv48le": (8, 1, 2, 2, 0, 4, 16, False),
    "xv30le": (4, 1, 4, 10, 0, 20, 10, False),
}


def _packed_fmt(pix_fmt):
    if pix_fmt not in PACKED_PIX_FMTS:
        raise ValueError(f"pix_fmt {pix_fmt!r}: one of {sorted(PACKED_PIX_FMTS)} (packed) or of {sorted(PIX_FMTS)} (planar / semi-planar: split_yuv)")
    return PACKED_PIX_FMTS[pix_fmt]


def packed_frame_bytes(H, W, pix_fmt):
    """Bytes of one ``H`` x ``W`` frame of a rawvideo pipe in a packed ``pix_fmt`` (one of ``PACKED_PIX_FMTS``)."""
    unit, ppu = _packed_fmt(pix_fmt)[:2]
    if isinstance(H, bool) or isinstance(W, bool) or not isinstance(H, int) or not isinstance(W, int) or H < 1 or W < ppu or W % ppu:
        raise ValueError(f"{pix_fmt} frames have W a multiple of {ppu} (a unit of {unit} bytes covers {ppu} pixels) and H >= 1, got {H} x {W}")
    return H * (W // ppu) * unit


def packed_to_patches(buf, *, H, W, pix_fmt, R, patch, matrix="bt601", full_range=False, chroma_loc="left", transfer=None, peak_nits=1000.0, sdr_white_nits=203.0,
                      gamut=None, rotate=0, hflip=False, vflip=False, mean=CLIP_MEAN, std=CLIP_STD, op_dtype=None, want=("patches",)):
    """Frames of a PACKED YCbCr surface (``PACKED_PIX_FMTS``: yuyv422 / uyvy422 from capture cards and webcams, y210le / ayuv / vuya / xv30le (Y410) / xv36le from
    VAAPI / D3D11 / QSV decoders) -> the CLIP front end in one launch (rv_packed_to_patches) -> (patches, image) as ``frames_to_patches`` returns them.  The
    values are the bits of ``yuv_surface_to_patches`` on the planar 4:2:2 / 4:4:4 surface that holds the same samples; no de-interleave pass is made and every
    source row is read once.  A / X bytes, the top bits of xv30le and the low bits of y210le / xv36le words never matter.
    buf: uint8 device tensor [n, H, row_bytes] with row_bytes = ``packed_frame_bytes(1, W, pix_fmt)``, passed by its strides - a padded pitch, or a window of a
    larger surface that starts on a unit boundary, is passed as it lies - or [n, ``packed_frame_bytes(H, W, pix_fmt)``].  With 16 / 32-bit words the address and
    the strides are multiples of the word size.  Colour tags, ``transfer`` / ``peak_nits`` / ``sdr_white_nits`` / ``gamut`` and ``rotate`` / ``hflip`` / ``vflip``
    as in ``yuv_surface_to_patches`` (``chroma_loc`` matters for the 4:2:2 formats only).  Every refusal comes before anything is read or launched.
    ``buf`` may also be a LIST (or tuple) of per-frame tensors [H, row_bytes] or [frame bytes] that agree in dtype, device, shape and strides: separately
    allocated surfaces in one launch per 64 frames by a table of their base pointers (rv_packed_surfaces_to_patches), without a stacking copy."""
    who = "packed_to_patches"
    unit, ppu, sb, oy, ocb, ocr, depth, msb = _packed_fmt(pix_fmt)
    orient = orientation(rotate, hflip, vflip)
    hdr = hdr_map(transfer, matrix, gamut, peak_nits, sdr_white_nits)
    if matrix not in _SURFACE_MATRICES or chroma_loc not in _SURFACE_LOCS:
        raise ValueError(f"matrix {matrix!r} / chroma_loc {chroma_loc!r}: one of {sorted(_SURFACE_MATRICES)} / {sorted(_SURFACE_LOCS)}")
    rb, fb = packed_frame_bytes(1, W, pix_fmt), packed_frame_bytes(H, W, pix_fmt)
    listed = isinstance(buf, (list, tuple))
    bufs, a = (_frame_list(buf, who), 0) if listed else ([buf], 1)
    e = bufs[0]
    if not torch.is_tensor(e) or e.dtype != torch.uint8 or not ((e.dim() == a + 2 and tuple(e.shape[a:]) == (H, rb)) or (e.dim() == a + 1 and e.shape[a] == fb)):
        ax, in_a_list, tensors = _WORDS[listed]
        raise ValueError(f"{pix_fmt} frames of {H} x {W}{in_a_list} come as {tensors} [{ax}{H},{rb}] or [{ax}{fb}], got {_got(e)}")
    n = len(bufs) if listed else e.shape[0]
    if e.dim() == a + 1:                    # [frame bytes]: rows of ``rb`` adjacent bytes
        if e.stride(a) != 1:
            bufs = _copies(bufs)
        bufs = [t.as_strided(t.shape[:a] + (H, rb), t.stride()[:a] + (rb, 1), t.storage_offset()) for t in bufs]
    elif not _rows_of_samples(e, a, n, H, rb, 1):
        bufs = _copies(bufs)
    fs, rs = _plane_strides(bufs[0], a, n, H, rb, 1)
    for i, t in enumerate(bufs if sb > 1 else ()):
        if t.storage_offset() % sb or rs % sb or fs % sb or (t.is_cuda and t.data_ptr() % sb):
            raise ValueError(f"{pix_fmt}: {8 * sb}-bit words must lie at multiples of {sb} bytes (" + (f"frame {i}: " if listed else "")
                             + f"offset {t.storage_offset()}, row stride {rs}" + ("" if listed else f", frame stride {fs}") + ")")
    if listed:
        _require_device(bufs, who)
    else:
        _device_tensor(bufs[0], who, "a device tensor")
    s = hip.RvPackedSurface(None if listed else bufs[0].data_ptr(), fs, rs, unit, ppu, sb, oy, ocb, ocr, depth, int(msb), n, H, W, _SURFACE_MATRICES[matrix],
                            int(bool(full_range)), _SURFACE_LOCS[chroma_loc])
    out = (R, patch, mean, std, op_dtype, want)
    if listed:
        table = (hip.C.c_void_p * n)(*[t.data_ptr() for t in bufs])
        return _launch("rv_packed_surfaces_to_patches", (hip.C.byref(s), table, _ref(hdr), orient), n, e.device, out)
    return _launch("rv_packed_to_patches", (hip.C.byref(s), _ref(hdr), orient), n, e.device, out)
