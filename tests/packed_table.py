"""The packed pixel formats of rv_packed_to_patches / rv_frames_to_patches_packed as THIS file reads their published layouts (ffmpeg's pixfmt.h / pixdesc, Microsoft's
"10-bit and 16-bit YUV video formats"), the pack / unpack pair the packed front-end tests share, and the refusal lists of the two C entries.  NumPy only; nothing here
imports the library's own table (ops.PACKED_PIX_FMTS), so a swapped Cb / Cr or a wrong offset there cannot cancel out.

A format is a repeating unit of four slots (memory order, little-endian words): "Y0" / "Y1" the two luma samples of a 4:2:2 unit, "Y" the one of a 4:4:4 unit, "Cb",
"Cr", and "A" / "X" for a slot that carries no value.  ``shift``: the value sits in the high bits of its word, ``shift`` low bits carry nothing.  xv30le is one 32-bit
word of bit fields instead."""
import numpy as np

#        name        slots (memory order)        bytes per slot, depth, shift
TABLE = {
    "yuyv422": (("Y0", "Cb", "Y1", "Cr"), 1, 8, 0),
    "uyvy422": (("Cb", "Y0", "Cr", "Y1"), 1, 8, 0),
    "yvyu422": (("Y0", "Cr", "Y1", "Cb"), 1, 8, 0),
    "y210le": (("Y0", "Cb", "Y1", "Cr"), 2, 10, 6),
    "y212le": (("Y0", "Cb", "Y1", "Cr"), 2, 12, 4),
    "ayuv": (("A", "Y", "Cb", "Cr"), 1, 8, 0),
    "vuya": (("Cr", "Cb", "Y", "A"), 1, 8, 0),
    "vuyx": (("Cr", "Cb", "Y", "X"), 1, 8, 0),
    "uyva": (("Cb", "Y", "Cr", "A"), 1, 8, 0),
    "ayuv64le": (("A", "Y", "Cb", "Cr"), 2, 16, 0),
    "xv36le": (("Cb", "Y", "Cr", "X"), 2, 12, 4),
    "xv48le": (("Cb", "Y", "Cr", "X"), 2, 16, 0),
    "xv30le": ({"Cb": 0, "Y": 10, "Cr": 20}, 4, 10, 0),         # bit positions inside the one 32-bit word; bits 30, 31 carry nothing
}
NAMES = tuple(TABLE)


def ppu(name):
    """Pixels per unit: 2 for the 4:2:2 formats."""
    return 2 if "Y0" in TABLE[name][0] else 1


def sub(name):
    return "422" if ppu(name) == 2 else "444"


def depth(name):
    return TABLE[name][2]


def unit_bytes(name):
    slots, sb, _, _ = TABLE[name]
    return 4 if sb == 4 else 4 * sb


def frame_bytes(H, W, name):
    return H * (W // ppu(name)) * unit_bytes(name)


def pack(name, y, cb, cr, fill):
    """Sample values (int arrays y [n,H,W], cb / cr [n,H,W/ppu]) -> uint8 [n, H, row bytes].  ``fill``: a RandomState whose bits go wherever no value lives (A / X
    slots, the low bits of msb-aligned words, the top 2 bits of xv30le)."""
    slots, sb, d, shift = TABLE[name]
    n, H, W = y.shape
    if sb == 4:
        w = np.zeros((n, H, W), np.uint32)
        for comp, v in (("Y", y), ("Cb", cb), ("Cr", cr)):
            w |= v.astype(np.uint32) << np.uint32(slots[comp])
        w |= fill.randint(0, 4, w.shape).astype(np.uint32) << np.uint32(30)
        return np.ascontiguousarray(w).view(np.uint8).reshape(n, H, -1)
    dt = np.uint8 if sb == 1 else np.dtype("<u2")
    src = {"Y0": y[..., 0::2], "Y1": y[..., 1::2], "Y": y, "Cb": cb, "Cr": cr}
    units = np.zeros((n, H, W // ppu(name), 4), dt)
    for k, slot in enumerate(slots):
        if slot in src:
            units[..., k] = (src[slot].astype(np.int64) << shift) | (fill.randint(0, 1 << shift, src[slot].shape) if shift else 0)
        else:
            units[..., k] = fill.randint(0, 1 << (8 * sb), units.shape[:3])
    return np.ascontiguousarray(units).view(np.uint8).reshape(n, H, -1)


def unpack(name, buf, W):
    """uint8 [n, H, row bytes] -> the sample values (int64 y [n,H,W], cb, cr [n,H,W/ppu])."""
    slots, sb, d, shift = TABLE[name]
    n, H = buf.shape[:2]
    if sb == 4:
        w = np.ascontiguousarray(buf).view(np.dtype("<u4")).reshape(n, H, W).astype(np.int64)
        return tuple((w >> slots[c]) & 1023 for c in ("Y", "Cb", "Cr"))
    units = np.ascontiguousarray(buf).view(np.uint8 if sb == 1 else np.dtype("<u2")).reshape(n, H, W // ppu(name), 4).astype(np.int64) >> shift
    at = {slot: units[..., k] for k, slot in enumerate(slots)}
    if ppu(name) == 2:
        y = np.stack((at["Y0"], at["Y1"]), -1).reshape(n, H, W)
    else:
        y = at["Y"]
    return y, at["Cb"], at["Cr"]


#: packed RGB: name -> the bytes of a pixel in memory order ("A" / "0": a byte that carries no value)
RGB_ORDERS = {"rgb24": "RGB", "bgr24": "BGR", "rgba": "RGBA", "bgra": "BGRA", "argb": "ARGB", "abgr": "ABGR", "rgb0": "RGB0", "bgr0": "BGR0", "0rgb": "0RGB",
              "0bgr": "0BGR"}


def pack_rgb(name, rgb, fill):
    """uint8 [n,3,H,W] -> uint8 [n,H,W,3|4] in the name's byte order, the fourth byte from ``fill``."""
    order = RGB_ORDERS[name]
    n, _, H, W = rgb.shape
    out = np.zeros((n, H, W, len(order)), np.uint8)
    for k, ch in enumerate(order):
        out[..., k] = rgb[:, "RGB".index(ch)] if ch in "RGB" else fill.randint(0, 256, (n, H, W))
    return out


# ---- refusals of the raw C entries: (what, overrides of the baseline arguments, a word of the message that names the argument) ----
#: baseline: y210le, 2 frames of 6 x 8, R 28, patch 14 (the callers supply base / outputs); "base+1" etc. are resolved by the caller
PACKED_BASE = dict(frame_stride=6 * 32, row_stride=32, unit_bytes=8, pix_per_unit=2, sample_bytes=2, y_off=0, cb_off=2, cr_off=6, depth=10, msb_aligned=1, n=2, H=6, W=8,
                   matrix=0, full_range=0, chroma_loc=0, orient=0, R=28, patch=14, ldp=640)
YUYV = dict(unit_bytes=4, sample_bytes=1, y_off=0, cb_off=1, cr_off=3, depth=8, msb_aligned=0, row_stride=16, frame_stride=96)
XV30 = dict(unit_bytes=4, pix_per_unit=1, sample_bytes=4, y_off=10, cb_off=0, cr_off=20, depth=10, msb_aligned=0)
PACKED_REFUSALS = [
    ("null base", dict(base=None), "null base"),
    ("sample bytes 3", dict(sample_bytes=3), "sample_bytes"),
    ("unit of 6 bytes", dict(unit_bytes=6), "unit_bytes"),
    ("unit of 4 bytes with 16-bit words", dict(unit_bytes=4), "unit_bytes"),
    ("3 pixels per unit", dict(pix_per_unit=3), "pix_per_unit"),
    ("2 pixels in a bit-field word", dict(XV30, pix_per_unit=2), "pix_per_unit"),
    ("cb on y", dict(cb_off=0), "cb_off"),
    ("cb on the second y", dict(cb_off=4), "cb_off"),
    ("cr on cb", dict(cr_off=2), "cr_off"),
    ("cr outside the unit", dict(cr_off=8), "cr_off"),
    ("negative offset", dict(y_off=-2), "y_off"),
    ("second y outside the unit", dict(y_off=4, cb_off=0, cr_off=2), "y_off"),
    ("offset off a word boundary", dict(cb_off=3), "cb_off"),
    ("yuyv: cb on the second y", dict(YUYV, cb_off=2), "cb_off"),
    ("bit field at shift 5", dict(XV30, y_off=5), "y_off"),
    ("two bit fields at one shift", dict(XV30, cb_off=20), "cb_off"),
    ("odd W with 2 pixels per unit", dict(W=7), "W = 7"),
    ("odd base with 16-bit words", dict(base="+1"), "base"),
    ("base off a 32-bit word", dict(XV30, base="+2"), "base"),
    ("odd row stride with 16-bit words", dict(row_stride=33), "row_stride"),
    ("odd frame stride with 16-bit words", dict(frame_stride=193), "frame_stride"),
    ("row stride off a 32-bit word", dict(XV30, row_stride=34), "row_stride"),
    ("depth 8 with 16-bit words", dict(depth=8), "depth"),
    ("depth 10 with bytes", dict(YUYV, depth=10), "depth"),
    ("depth 12 with the bit-field word", dict(XV30, depth=12), "depth"),
    ("msb_aligned with bytes", dict(YUYV, msb_aligned=1), "msb_aligned"),
    ("msb_aligned with the bit-field word", dict(XV30, msb_aligned=1), "msb_aligned"),
    ("msb_aligned 2", dict(msb_aligned=2), "msb_aligned"),
    ("matrix 3", dict(matrix=3), "matrix"),
    ("full_range 2", dict(full_range=2), "full_range"),
    ("chroma_loc 3", dict(chroma_loc=3), "chroma_loc"),
    ("orient 8", dict(orient=8), "orient"),
    ("orient -1", dict(orient=-1), "orient"),
    ("transfer 3", dict(hdr=(3, 1, 1000.0, 203.0)), "transfer"),
    ("gamut 2", dict(hdr=(1, 2, 1000.0, 203.0)), "gamut"),
    ("peak_nits 0", dict(hdr=(1, 1, 0.0, 203.0)), "peak_nits"),
    ("sdr_white_nits above 10000", dict(hdr=(2, 1, 1000.0, 20000.0)), "sdr_white_nits"),
    ("R no multiple of patch", dict(R=30), "multiple"),
    ("H = 0", dict(H=0), "frame size"),
    ("W above 8192", dict(W=8194), "frame size"),
    ("n = -1", dict(n=-1), "n = -1"),
    ("both outputs null", dict(patches=None, image=None), "both outputs null"),
    ("ldp below Kp", dict(ldp=639), "ldp"),
    ("a geometry beyond the LDS", dict(H=8192, W=8192, R=1, patch=1), "LDS"),
    ("more workgroups than a launch", dict(n=2 ** 30), "workgroups"),
]
#: baseline: bgra, 2 frames of 6 x 8
RGB_BASE = dict(pix_bytes=4, r_off=2, g_off=1, b_off=0, frame_stride=6 * 32, row_stride=32, n=2, H=6, W=8, orient=0, R=28, patch=14, ldp=640)
RGB_REFUSALS = [
    ("2 bytes per pixel", dict(pix_bytes=2), "pix_bytes"),
    ("5 bytes per pixel", dict(pix_bytes=5), "pix_bytes"),
    ("r on g", dict(r_off=1), "r_off"),
    ("g on b", dict(g_off=0), "g_off"),
    ("b outside a 3-byte pixel", dict(pix_bytes=3, b_off=3, g_off=0), "b_off"),
    ("negative offset", dict(r_off=-1), "r_off"),
    ("orient 8", dict(orient=8), "orient"),
    ("null frames", dict(frames=None), "null frames"),
    ("R no multiple of patch", dict(R=30), "multiple"),
    ("H = 0", dict(H=0), "frame size"),
    ("W above 8192", dict(W=8193), "frame size"),
    ("n = -1", dict(n=-1), "n = -1"),
    ("both outputs null", dict(patches=None, image=None), "both outputs null"),
    ("ldp below Kp", dict(ldp=639), "ldp"),
    ("a geometry beyond the LDS", dict(H=8192, W=8192, R=1, patch=1), "LDS"),
]


def call_packed(lib, hip, base, patches, image, over, null_struct=False):
    """rv_packed_to_patches through ctypes with the baseline arguments and ``over``; base / patches / image: addresses (or None)."""
    import ctypes
    a = dict(PACKED_BASE, base=base, patches=patches, image=image, hdr=None)
    a.update(over)
    if isinstance(a["base"], str):
        a["base"] = base + int(a["base"])
    s = hip.RvPackedSurface(**{k: a[k] for k, _ in hip.RvPackedSurface._fields_})
    m = hip.RvHdrMap(*a["hdr"]) if a["hdr"] else None
    f3 = ctypes.c_float * 3
    mean, std = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
    return lib.rv_packed_to_patches(None if null_struct else ctypes.byref(s), ctypes.byref(m) if m else None, a["orient"], a["R"], a["patch"], f3(*mean), f3(*std),
                                    a["patches"], a["ldp"], a["image"], None)


def call_rgb(lib, frames, patches, image, over):
    import ctypes
    a = dict(RGB_BASE, frames=frames, patches=patches, image=image)
    a.update(over)
    f3 = ctypes.c_float * 3
    mean, std = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
    return lib.rv_frames_to_patches_packed(a["frames"], a["pix_bytes"], a["r_off"], a["g_off"], a["b_off"], a["frame_stride"], a["row_stride"], a["n"], a["H"], a["W"],
                                           a["orient"], a["R"], a["patch"], f3(*mean), f3(*std), a["patches"], a["ldp"], a["image"], None)
