"""SHA-256 digests of what the CLIP front end's C entries write, for a fixed, seeded case list: the check that a change of csrc/frames.hip,
csrc/frames_yuv.hip or csrc/frames_common.h leaves every output bit where it was.

    REVISION_HIP_LIB=... REVISION_HIP_LIB_BF16=... python tools/frontend_digest.py [--out FILE]     (default: profiles/frontend_digest.json)

Run it once on a build of the parent commit (the two variables name its libraries) and once on this tree's build, in a fresh process each on the same
machine; the two files must hold the same digests.  Both operand flavours run.  A case is one source format, transfer, orientation and form at one geometry: it
is called twice, for patches + image and for the image alone, and its digest is the SHA-256 of the patches, the image and the second call's image, in that
order.  The outputs are pre-filled with NaN, so a pad column left untouched or a store outside the written region shows.

The cases reach every kernel instance at least once - frames_to_patches_kernel<ORI, PK, TAB> (12), yuv_to_patches_kernel<S, TRC, ORI, TAB> (36),
packed_to_patches_kernel<S, TRC, ORI, TAB> (54):
  sources       RGB as NCHW, NHWC and bgra; planar YCbCr 4:2:0 with 8-bit (yuv420p / nv12) and 16-bit samples (yuv420p10le / p010le: the planar and the
                interleaved layout alternate over the other axes); packed yuyv422 (1-byte samples), y210le (2) and xv30le (4)
  transfer      SDR, PQ, HLG (YCbCr)
  orientation   codes 0, 2 (mirror x) and 1 (transpose)
  form          contiguous frames and a list of separately allocated frames
  geometry      n = 3 frames of 360 x 640 -> R = 224, patch 14 (downscale, several tiles per axis with a ragged last one, pad columns K = 588 < Kp = 640);
                n = 3 frames of 90 x 160 -> R = 64, patch 32 (a source below 2R: the chroma planes are interpolated; K = Kp); list form only: 65 frames of 32 x 32 -> R = 16, patch 8 (more than the 64
                frames of one launch).  The cases of a form take the geometries in turn, so each geometry sees every kernel, orientation class and transfer
"""
import argparse
import ctypes as C
import hashlib
import itertools
import json
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from revisionllm_amd import frontend, hip  # noqa: E402

GEOMETRIES = (("360x640", 3, 360, 640, 224, 14, (False, True)), ("90x160", 3, 90, 160, 64, 32, (False, True)), ("65x32x32", 65, 32, 32, 16, 8, (True,)))
ORIENTS = (0, 2, 1)
RGB = ("nchw", "nhwc", "bgra")
PLANAR = (("yuv420p", "nv12"), ("yuv420p10le", "p010le"))          # per sample size: the planar and the interleaved format
PACKED = ("yuyv422", "y210le", "xv30le")
TRANSFERS = (0, 1, 2)


def noise(name, n, nbytes, depth=8, msb=True):
    """[n, nbytes] seeded bytes on the device; 16-bit words with the value in the low bits stay below 2^depth, as a decoder writes them."""
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    buf = torch.randint(0, 256, (n, nbytes), dtype=torch.uint8, generator=g)
    if depth > 8 and not msb:
        buf[:, 1::2] &= (1 << (depth - 8)) - 1
    return buf.cuda()


def frames_of(buf, listed, keep):
    """Base pointers of the frames: those of the contiguous buffer, or of one allocation per frame with another allocation between two of them."""
    if not listed:
        return [buf[i].data_ptr() for i in range(buf.shape[0])]
    out = []
    for i in range(buf.shape[0]):
        keep.append(buf[i].clone())
        out.append(keep[-1].data_ptr())
        keep.append(torch.empty(256 * (1 + i % 3), dtype=torch.uint8, device="cuda"))
    return out


def hdr(transfer):
    return None if transfer == 0 else hip.RvHdrMap(transfer, 1, 1000.0, 203.0)


def run(lib, entry, head, n, R, patch, dt, both):
    """One call into NaN-filled outputs -> their bytes (patches, then image)."""
    g, kp = R // patch, (3 * patch * patch + 127) // 128 * 128
    patches = torch.full((n * g * g, kp), float("nan"), dtype=dt, device="cuda") if both else None
    image = torch.full((n, 3, R, R), float("nan"), dtype=torch.float32, device="cuda")
    f3 = C.c_float * 3
    hip.check(getattr(lib, entry)(*head, R, patch, f3(*frontend.CLIP_MEAN), f3(*frontend.CLIP_STD), hip.ptr(patches), kp, hip.ptr(image), hip.stream()), entry)
    torch.cuda.synchronize()
    return b"".join(t.cpu().contiguous().view(torch.uint8).numpy().tobytes() for t in (patches, image) if t is not None)


def cases(gi):
    """(name, entry, head of the argument list, objects to keep alive) of every case of geometry gi."""
    gname, n, H, W, R, patch, forms = GEOMETRIES[gi]
    for listed in forms:
        form = "list" if listed else "contig"
        count = itertools.count()

        def mine():     # the cases of a form take its geometries in turn (18 cases per orientation: shifted by one from one orientation to the next)
            k = next(count)
            return (k + k // 18) % (3 if listed else 2) == gi
        for orient in ORIENTS:
            for fmt in RGB:
                if not mine():
                    continue
                keep = []
                pix = 4 if fmt == "bgra" else 3
                buf = noise("rgb%d%s" % (pix, gname), n, 3 * H * W if pix == 3 else 4 * H * W)
                ptrs = frames_of(buf, listed, keep)
                layout, cs, rs = (0, H * W, W) if fmt == "nchw" else (1, 0, pix * W)
                off = (2, 1, 0) if fmt == "bgra" else (0, 1, 2)
                name = "%s/%s/%s/orient%d" % (gname, fmt, form, orient)
                if listed:
                    tab = (C.c_void_p * n)(*ptrs)
                    yield name, "rv_frames_to_patches_scattered", (tab, layout, pix, *off, cs, rs, n, H, W, orient), (buf, keep, tab)
                elif fmt == "bgra":
                    yield name, "rv_frames_to_patches_packed", (C.c_void_p(ptrs[0]), pix, *off, buf.stride(0), rs, n, H, W, orient), (buf,)
                elif orient:
                    yield name, "rv_frames_to_patches_oriented", (C.c_void_p(ptrs[0]), layout, buf.stride(0), rs, n, H, W, orient), (buf,)
                else:
                    yield name, "rv_frames_to_patches", (C.c_void_p(ptrs[0]), layout, buf.stride(0), rs, n, H, W), (buf,)
            for ti, transfer in enumerate(TRANSFERS):
                matrix, loc = (1, 0) if transfer == 0 else (2, 2)
                m = hdr(transfer)
                for si, pair in enumerate(PLANAR):
                    if not mine():
                        continue
                    fmt = pair[(ti + ORIENTS.index(orient) + listed) % 2]
                    sb, depth, msb, _, chroma = frontend.PIX_FMTS[fmt]
                    keep = []
                    ysz, csz = H * W * sb, (H // 2) * (W // 2) * sb
                    buf = noise(fmt + gname, n, ysz + 2 * csz, depth, msb)
                    ptrs = frames_of(buf, listed, keep)
                    inter = chroma != "planar"
                    planes = [(p, p + ysz, p + ysz + (sb if inter else csz)) for p in ptrs]
                    s = hip.RvYuvSurface(*((None,) * 3 if listed else planes[0]), buf.stride(0), W * sb, buf.stride(0), (W if inter else W // 2) * sb, sb, depth, int(msb),
                                         (2 if inter else 1) * sb, 2, 2, n, H, W, matrix, 0, loc)
                    name = "%s/%s/%s/trc%d/orient%d" % (gname, fmt, form, transfer, orient)
                    if listed:
                        tab = (hip.RvSurfacePlanes * n)(*planes)
                        yield name, "rv_yuv_surfaces_to_patches", (C.byref(s), tab, m and C.byref(m), orient), (buf, keep, tab, s, m)
                    elif orient:
                        yield name, "rv_yuv_surface_to_patches_oriented", (C.byref(s), m and C.byref(m), orient), (buf, s, m)
                    elif m:
                        yield name, "rv_yuv_surface_to_patches_hdr", (C.byref(s), C.byref(m)), (buf, s, m)
                    else:
                        yield name, "rv_yuv_surface_to_patches", (C.byref(s),), (buf, s)
                        if sb == 1:     # the first entry point: the same 8-bit 4:2:0 surface as plain arguments
                            yield name + "/plain", "rv_yuv_to_patches", (planes[0][0], s.y_frame_stride, s.y_row_stride, planes[0][1], planes[0][2], s.c_frame_stride,
                                                                         s.c_row_stride, s.c_pix, n, H, W, matrix, 0, loc), (buf,)
                for fmt in PACKED:
                    if not mine():
                        continue
                    unit, ppu, sb, oy, ocb, ocr, depth, msb = frontend.PACKED_PIX_FMTS[fmt]
                    keep = []
                    buf = noise(fmt + gname, n, H * (W // ppu) * unit)
                    ptrs = frames_of(buf, listed, keep)
                    s = hip.RvPackedSurface(None if listed else ptrs[0], buf.stride(0), (W // ppu) * unit, unit, ppu, sb, oy, ocb, ocr, depth, int(msb), n, H, W, matrix, 0, loc)
                    name = "%s/%s/%s/trc%d/orient%d" % (gname, fmt, form, transfer, orient)
                    if listed:
                        tab = (C.c_void_p * n)(*ptrs)
                        yield name, "rv_packed_surfaces_to_patches", (C.byref(s), tab, m and C.byref(m), orient), (buf, keep, tab, s, m)
                    else:
                        yield name, "rv_packed_to_patches", (C.byref(s), m and C.byref(m), orient), (buf, s, m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend_digest.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "frontend_digest needs the GPU"
    res = {}
    for fl in ("f16", "bf16"):
        lib, dt = hip.lib(fl), hip.op_dtype(fl)
        res[fl] = {}
        for gi, geo in enumerate(GEOMETRIES):
            for name, entry, head, keep in cases(gi):
                res[fl][name] = hashlib.sha256(b"".join(run(lib, entry, head, geo[1], geo[4], geo[5], dt, both) for both in (True, False))).hexdigest()
                del keep
    out = dict(abi=hip.lib("f16").rv_abi_version(), cases=len(res["f16"]), digests=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(dict(out=a.out, cases=out["cases"], sha256_of_digests=hashlib.sha256(json.dumps(res, sort_keys=True).encode()).hexdigest())))


if __name__ == "__main__":
    main()
