"""CLIP front end at 1080p on decoder output: rv_yuv_to_patches on NV12 against rv_frames_to_patches on the same frames as NCHW RGB, and against the torch
composition (colour conversion + resize) a user would otherwise write on the GPU.

60 NV12 frames of 1080 x 1920 (noise) -> R = 224, patch = 14 (one encode_video_yuv batch).  The RGB frames are the NV12 frames converted once, outside the
timed region (nearest chroma, BT.709 studio, rounded to uint8): the RGB entry is timed on bytes a conversion pass would have had to write first.  The three
forms run in one process, alternating, each launch between two device events: 5 warm-up + 20 timed launches per form.  Reported: median, min .. max per form,
yuv / rgb (the yardstick: the RGB entry on the same box; the YUV entry reads half the bytes and filters half the plane area), and the source bytes the crop
uses over the YUV call's median as a fraction of the 8 TB/s HBM figure.  Writes one JSON object to --out (default profiles/frontend_yuv_1080p.json).

--pix-fmt NAME (one of ops.PIX_FMTS: p010le, yuv444p10le, nv16 ...) times rv_yuv_surface_to_patches on noise frames of that format instead, alone, with the
same warm-up and launch counts: median, min .. max, and the source bytes the crop uses over the median.  ``--pix-fmt nv12`` is the same bytes as the default
run through the surface entry, for a like-for-like figure next to P010.

--transfer pq|hlg times rv_yuv_surface_to_patches_hdr on P010 noise (BT.2020, top-left siting, peak 1000 / white 203 nits, BT.709 primaries) at 1080 x 1920
and 2160 x 3840 against the SDR entry on the same bytes, alternating in one process with the same warm-up and launch counts: median, min .. max per form and
hdr / sdr per size.  The extra work is R x R pixels against a whole source frame read, so the expectation is "within noise".  Default --out:
profiles/frontend_hdr.json.

--rotate N [--hflip] [--vflip] times the display orientation inside the kernel (rv_yuv_surface_to_patches_oriented) on NV12 and P010 noise at 1080 x 1920
against what a caller does without it on the same bytes - torch.rot90 / flip + .contiguous() of every plane, then the un-oriented entry - and, as information,
against the un-oriented entry alone (another picture, the same bytes): three forms alternating in one process, the same warm-up and launch counts.  Centre
siting, so that the one-call and the two-step form compute the same picture (a flip cannot carry left siting through the two-step form); their largest patch
difference is reported.  The goal: oriented <= two-step.  The run is ADDED to --out (default profiles/frontend_orient.json) under its orientation.

    python tools/frontend_yuv_prof.py [--frames 60] [--height 1080] [--width 1920] [--pix-fmt NAME | --transfer pq|hlg | --rotate N [--hflip] [--vflip] |
                                      --scattered] [--out FILE] [--once]
    (--once: one launch, for a kernel trace)

--pix-fmt <packed name> (yuyv422 / y210le / xv30le / ayuv ...) and --rgb-order <bgra / bgr24 ...>: the packed entries (rv_packed_to_patches,
rv_frames_to_patches_packed) against the planar / NHWC entry on the same samples and against the two-step path they replace (a torch de-interleave or channel
swap over every full-resolution frame, then the existing entry), alternating on the same bytes.  The expectation: packed <= planar (each source row is staged
once), and the two-step path costs the extra pass.  Each run is ADDED to --out (default profiles/frontend_packed.json) under its name.

--scattered: the list forms (rv_yuv_surfaces_to_patches, rv_frames_to_patches_scattered: one pointer per frame in the kernel arguments) on --frames separately
allocated 1080p surfaces, for NV12, P010 + PQ and bgra, against the contiguous entry on a pre-stacked copy of the same bytes and against the two-step path a
surface pool forces without them (torch.stack of every plane, then the contiguous entry): three forms alternating in one process, each launch between two device
events, the same warm-up and launch counts.  No ratio is fixed in advance; the expectation is list / contiguous about 1 and list / two-step below 1 by about the
cost of the copy.  Writes the three runs to --out (default profiles/frontend_scattered.json).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from revisionllm_amd import hip, ops  # noqa: E402

HBM_PEAK = 8.0e12
KR, KB = 0.2126, 0.0722          # BT.709, studio range, as encode_video_yuv assumes at 1080 lines


def to_rgb_float(y, cbcr):
    """NV12 planes -> float RGB [n,3,H,W] in 0..255 (unclamped): nearest chroma, BT.709 studio range."""
    n, H, W = y.shape
    c = cbcr.permute(0, 3, 1, 2).float().repeat_interleave(2, 2).repeat_interleave(2, 3)
    yl = (y.float() - 16.0) * (255.0 / 219.0)
    cb, cr = (c[:, 0] - 128.0) * (255.0 / 224.0), (c[:, 1] - 128.0) * (255.0 / 224.0)
    kg = 1.0 - KR - KB
    return torch.stack([yl + 2 * (1 - KR) * cr, yl - (2 * KB * (1 - KB) / kg) * cb - (2 * KR * (1 - KR) / kg) * cr, yl + 2 * (1 - KB) * cb], 1)


def torch_composition(y, cbcr, R, patch, dt):
    """convert -> antialiased bicubic resize -> centre crop -> normalise -> unfold -> pad -> operand type."""
    n, H, W = y.shape
    x = to_rgb_float(y, cbcr)
    hr, wr = (R, int(R * W / H)) if H <= W else (int(R * H / W), R)
    x = F.interpolate(x, size=(hr, wr), mode="bicubic", align_corners=False, antialias=True)
    top, left = int(round((hr - R) / 2.0)), int(round((wr - R) / 2.0))
    x = x[:, :, top:top + R, left:left + R]
    mean = torch.tensor(ops.CLIP_MEAN, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(ops.CLIP_STD, device=x.device).view(1, 3, 1, 1)
    x = (x / 255.0 - mean) / (std + 1e-8)
    g = R // patch
    p = x.reshape(n, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, 3 * patch * patch)
    kp = (p.shape[1] + 127) // 128 * 128
    return F.pad(p, (0, kp - p.shape[1])).to(dt)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def surface_run(a, dt):
    """--pix-fmt: the surface entry alone on one format."""
    n, H, W, R = a.frames, a.height, a.width, a.res
    fb = ops.yuv_frame_bytes(H, W, a.pix_fmt)
    buf = torch.randint(0, 256, (n, fb), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    sb, depth, msb, sub, _ = ops.PIX_FMTS[a.pix_fmt]
    if sb == 2 and not msb and depth < 16:      # value in the low bits: keep the words inside [0, 2^depth) as a decoder would
        buf[:, 1::2] &= (1 << (depth - 8)) - 1
    planes, kw = ops.split_yuv(buf.cuda(), H, W, a.pix_fmt)
    colour = dict(matrix="bt709", full_range=False, chroma_loc="left")
    call = lambda: ops.yuv_surface_to_patches(*planes, R=R, patch=a.patch, op_dtype=dt, **kw, **colour)[0]
    if a.once:
        call()
        torch.cuda.synchronize()
        return
    t = []
    for i in range(a.warmup + a.iters):
        s, _ = timed(call)
        if i >= a.warmup:
            t.append(s)
    med = statistics.median(t)
    sx, sy = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}[sub]
    used = n * (min(H, W) ** 2 + 2 * (min(H, W) // sx) * (min(H, W) // sy)) * sb      # the centred square of every plane
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), pix_fmt=a.pix_fmt, frames=n, height=H, width=W, res=R, patch=a.patch,
               warmup=a.warmup, iters=a.iters, yuv_ms=dict(median=med * 1e3, min=min(t) * 1e3, max=max(t) * 1e3), used_source_bytes=used,
               yuv_bytes_per_s=used / med, yuv_fraction_of_8TBps=used / med / HBM_PEAK)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def hdr_run(a, dt):
    """--transfer: the HDR entry against the SDR entry on the same P010 bytes, at 1080p and 2160p."""
    n, R = a.frames, a.res
    colour = dict(matrix="bt2020", full_range=False, chroma_loc="topleft")
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), pix_fmt="p010le", transfer=a.transfer, peak_nits=1000.0, sdr_white_nits=203.0,
               frames=n, res=R, patch=a.patch, warmup=a.warmup, iters=a.iters, sizes={})
    for H, W in ((1080, 1920), (2160, 3840)):
        buf = torch.randint(0, 256, (n, ops.yuv_frame_bytes(H, W, "p010le")), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
        planes, kw = ops.split_yuv(buf.cuda(), H, W, "p010le")
        forms = (("sdr", lambda: ops.yuv_surface_to_patches(*planes, R=R, patch=a.patch, op_dtype=dt, **kw, **colour)[0]),
                 ("hdr", lambda: ops.yuv_surface_to_patches(*planes, R=R, patch=a.patch, op_dtype=dt, transfer=a.transfer, **kw, **colour)[0]))
        if a.once:
            forms[1][1]()
            torch.cuda.synchronize()
            continue
        t = {k: [] for k, _ in forms}
        for i in range(a.warmup + a.iters):
            for name, fn in forms:
                s, _ = timed(fn)
                if i >= a.warmup:
                    t[name].append(s)
        med = {k: statistics.median(v) for k, v in t.items()}
        ms = lambda k: dict(median=med[k] * 1e3, min=min(t[k]) * 1e3, max=max(t[k]) * 1e3)
        res["sizes"][f"{H}x{W}"] = dict(sdr_ms=ms("sdr"), hdr_ms=ms("hdr"), hdr_over_sdr=med["hdr"] / med["sdr"])
        del planes, buf
    if a.once:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def orient_run(a, dt):
    """--rotate / --hflip / --vflip: the oriented call against flip / rot90 + contiguous + the un-oriented entry, and against the un-oriented entry alone."""
    n, H, W, R = a.frames, a.height, a.width, a.res
    spell = dict(rotate=a.rotate, hflip=a.hflip, vflip=a.vflip)
    colour = dict(matrix="bt709", full_range=False, chroma_loc="centre")
    run = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), orient=ops.orientation(**spell), frames=n, height=H, width=W, res=R, patch=a.patch,
               warmup=a.warmup, iters=a.iters, formats={})

    def turned(t):
        """What a caller does today with one plane [n,rows,cols] or [n,rows,cols,2]: a copy in display orientation."""
        t = torch.rot90(t, -(a.rotate // 90), (1, 2))                                     # rot90 turns counter-clockwise
        t = t.flip(2) if a.hflip else t
        t = t.flip(1) if a.vflip else t
        return t.contiguous()

    for pix_fmt in ("nv12", "p010le"):
        buf = torch.randint(0, 256, (n, ops.yuv_frame_bytes(H, W, pix_fmt)), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
        (y, cbcr, _), kw = ops.split_yuv(buf.cuda(), H, W, pix_fmt)
        call = lambda yy, cc, **o: ops.yuv_surface_to_patches(yy, cc, None, R=R, patch=a.patch, op_dtype=dt, **kw, **colour, **o)[0]
        forms = (("oriented", lambda: call(y, cbcr, **spell)), ("two_step", lambda: call(turned(y), turned(cbcr))), ("unoriented", lambda: call(y, cbcr)))
        if a.once:
            forms[0][1]()
            torch.cuda.synchronize()
            continue
        t, first = {k: [] for k, _ in forms}, {}
        for i in range(a.warmup + a.iters):
            for name, fn in forms:
                s, out = timed(fn)
                if i >= a.warmup:
                    t[name].append(s)
                if i == 0:
                    first[name] = out
        med = {k: statistics.median(v) for k, v in t.items()}
        ms = lambda k: dict(median=med[k] * 1e3, min=min(t[k]) * 1e3, max=max(t[k]) * 1e3)
        run["formats"][pix_fmt] = dict(oriented_ms=ms("oriented"), two_step_ms=ms("two_step"), unoriented_ms=ms("unoriented"),
                                       oriented_over_two_step=med["oriented"] / med["two_step"], oriented_over_unoriented=med["oriented"] / med["unoriented"],
                                       goal_met=bool(med["oriented"] <= med["two_step"]),
                                       max_abs_patch_diff_oriented_vs_two_step=float((first["oriented"].float() - first["two_step"].float()).abs().max()))
        del y, cbcr, buf, first
    if a.once:
        return
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res["rotate=%d hflip=%d vflip=%d" % (a.rotate, a.hflip, a.vflip)] = run
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(run))


def deinterleave(buf, H, W, pix_fmt):
    """What a caller does today with a packed surface: a torch pass over every frame into the planar planes ``ops.yuv_surface_to_patches`` takes."""
    unit, ppu, sb, oy, ocb, ocr, depth, msb = ops.PACKED_PIX_FMTS[pix_fmt]
    n = buf.shape[0]
    if sb == 4:
        w = buf.view(torch.int32).view(n, H, W)
        planes = tuple(((w >> o) & 1023).to(torch.int16).view(torch.uint16) for o in (oy, ocb, ocr))
        return planes, dict(depth=depth, msb_aligned=False, subsampling="444")
    u = (buf if sb == 1 else buf.view(torch.int16)).view(n, H, W // ppu, 4)
    y = torch.stack((u[..., oy // sb], u[..., oy // sb + 2]), -1).view(n, H, W) if ppu == 2 else u[..., oy // sb].contiguous()
    planes = (y, u[..., ocb // sb].contiguous(), u[..., ocr // sb].contiguous())
    planes = planes if sb == 1 else tuple(t.view(torch.uint16) for t in planes)
    return planes, dict(depth=depth, msb_aligned=msb, subsampling="422" if ppu == 2 else "444")


def alternate(forms, a):
    """Median / min / max seconds per form, the forms alternating inside every iteration; the first outputs."""
    t, first = {k: [] for k, _ in forms}, {}
    for i in range(a.warmup + a.iters):
        for name, fn in forms:
            s, out = timed(fn)
            if i >= a.warmup:
                t[name].append(s)
            if i == 0:
                first[name] = out
    med = {k: statistics.median(v) for k, v in t.items()}
    return med, {k: dict(median=med[k] * 1e3, min=min(v) * 1e3, max=max(v) * 1e3) for k, v in t.items()}, first


def add_to(out, key, run):
    res = {}
    if os.path.exists(out):
        with open(out) as f:
            res = json.load(f)
    res[key] = run
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(run))


def packed_run(a, dt):
    """--pix-fmt <a packed name>: rv_packed_to_patches against the planar entry on the same samples (already de-interleaved) and against the two-step path it
    replaces (torch de-interleave + the planar entry), alternating on the same bytes.  The run is ADDED to --out under the format's name."""
    n, H, W, R = a.frames, a.height, a.width, a.res
    buf = torch.randint(0, 256, (n, ops.packed_frame_bytes(H, W, a.pix_fmt)), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    colour = dict(matrix="bt709", full_range=False, chroma_loc="left")
    planes, kw = deinterleave(buf, H, W, a.pix_fmt)
    planar = lambda pl: ops.yuv_surface_to_patches(*pl, R=R, patch=a.patch, op_dtype=dt, **kw, **colour)[0]
    forms = (("packed", lambda: ops.packed_to_patches(buf, H=H, W=W, pix_fmt=a.pix_fmt, R=R, patch=a.patch, op_dtype=dt, **colour)[0]),
             ("planar", lambda: planar(planes)), ("two_step", lambda: planar(deinterleave(buf, H, W, a.pix_fmt)[0])))
    if a.once:
        forms[0][1]()
        torch.cuda.synchronize()
        return
    med, ms, first = alternate(forms, a)
    add_to(a.out, a.pix_fmt, dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), pix_fmt=a.pix_fmt, frames=n, height=H, width=W, res=R, patch=a.patch,
                                  warmup=a.warmup, iters=a.iters, packed_ms=ms["packed"], planar_ms=ms["planar"], two_step_ms=ms["two_step"],
                                  packed_over_planar=med["packed"] / med["planar"], packed_over_two_step=med["packed"] / med["two_step"],
                                  packed_not_slower_than_planar=bool(med["packed"] <= med["planar"]),
                                  same_bits_as_planar=bool(torch.equal(first["packed"].view(torch.int16), first["planar"].view(torch.int16)))))


def rgb_order_run(a, dt):
    """--rgb-order: rv_frames_to_patches_packed against the NHWC entry on an RGB copy and against channel-index ``.contiguous()`` + the NHWC entry."""
    n, H, W, R = a.frames, a.height, a.width, a.res
    pix, r, g, b = ops.RGB_PIX_FMTS[a.rgb_order]
    src = torch.randint(0, 256, (n, H, W, pix), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    swap = lambda: src[..., [r, g, b]].contiguous()
    rgb = swap()
    nhwc = lambda t: ops.frames_to_patches(t, R, a.patch, layout="NHWC", op_dtype=dt)[0]
    forms = (("packed", lambda: ops.frames_to_patches(src, R, a.patch, op_dtype=dt, pix_fmt=a.rgb_order)[0]), ("rgb24", lambda: nhwc(rgb)),
             ("two_step", lambda: nhwc(swap())))
    if a.once:
        forms[0][1]()
        torch.cuda.synchronize()
        return
    med, ms, first = alternate(forms, a)
    add_to(a.out, a.rgb_order, dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), rgb_order=a.rgb_order, frames=n, height=H, width=W, res=R,
                                    patch=a.patch, warmup=a.warmup, iters=a.iters, packed_ms=ms["packed"], rgb24_ms=ms["rgb24"], two_step_ms=ms["two_step"],
                                    packed_over_rgb24=med["packed"] / med["rgb24"], packed_over_two_step=med["packed"] / med["two_step"],
                                    same_bits_as_rgb24=bool(torch.equal(first["packed"].view(torch.int16), first["rgb24"].view(torch.int16)))))


def scattered_run(a, dt):
    """--scattered: the list entry on separately allocated surfaces against the contiguous entry on a stacked copy and against torch.stack + that entry."""
    n, H, W, R = a.frames, a.height, a.width, a.res
    gen = torch.Generator().manual_seed(0)

    def surfaces(*shape):
        """n separate allocations of one plane, with another allocation between two of them so that they are not neighbours."""
        out, spacers = [], []
        for i in range(n):
            t = torch.randint(0, 256, shape, dtype=torch.uint8, generator=gen).cuda()
            out.append(t)
            spacers.append(torch.empty(4096 * (1 + i % 3), dtype=torch.uint8, device="cuda"))
        return out, spacers

    res = {}
    for name in ("nv12", "p010le_pq", "bgra"):
        if name == "bgra":
            frames, keep = surfaces(H, W, 4)
            call = lambda f: ops.frames_to_patches(f, R, a.patch, op_dtype=dt, pix_fmt="bgra")[0]
            stack = lambda: torch.stack(frames)
        else:
            wide = name != "nv12"
            es, dtype = (2, torch.uint16) if wide else (1, torch.uint8)
            yb, keep = surfaces(H, W * es)                       # bytes: the stack below is a plain byte copy
            cb, keep2 = surfaces(H // 2, W * es)
            y, c = [t.view(dtype) for t in yb], [t.view(dtype).view(H // 2, W // 2, 2) for t in cb]
            kw = dict(depth=10, msb_aligned=True, matrix="bt2020", chroma_loc="topleft", transfer="pq") if wide else dict(matrix="bt709")
            frames = (y, c)
            call = lambda f: ops.yuv_surface_to_patches(f[0], f[1], R=R, patch=a.patch, op_dtype=dt, **kw)[0]
            stack = lambda: (torch.stack(yb).view(dtype), torch.stack(cb).view(dtype).view(n, H // 2, W // 2, 2))
        stacked = stack()
        forms = (("list", lambda: call(frames)), ("contiguous", lambda: call(stacked)), ("two_step", lambda: call(stack())))
        if a.once:
            forms[0][1]()
            torch.cuda.synchronize()
            continue
        med, ms, first = alternate(forms, a)
        res[name] = dict(frames=n, height=H, width=W, res=R, patch=a.patch, warmup=a.warmup, iters=a.iters, list_ms=ms["list"], contiguous_ms=ms["contiguous"],
                         two_step_ms=ms["two_step"], list_over_contiguous=med["list"] / med["contiguous"], list_over_two_step=med["list"] / med["two_step"],
                         same_bits_as_contiguous=bool(torch.equal(first["list"].view(torch.int16), first["contiguous"].view(torch.int16))))
        del keep
    if a.once:
        return
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), **res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--res", type=int, default=224)
    ap.add_argument("--patch", type=int, default=14)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend_yuv_1080p.json"))
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--pix-fmt", default=None, help="time rv_yuv_surface_to_patches on this ffmpeg pix_fmt instead (ops.PIX_FMTS); a packed name "
                    "(ops.PACKED_PIX_FMTS: yuyv422, y210le, xv30le, ayuv ...) times rv_packed_to_patches against the planar entry and the two-step path")
    ap.add_argument("--rgb-order", default=None, help="time rv_frames_to_patches_packed on this byte order (ops.RGB_PIX_FMTS: bgra, bgr24 ...) against a channel "
                    "swap + the NHWC entry")
    ap.add_argument("--transfer", default=None, choices=("pq", "hlg"), help="time rv_yuv_surface_to_patches_hdr on P010 at 1080p and 2160p against the SDR entry")
    ap.add_argument("--rotate", type=int, default=0, choices=(0, 90, 180, 270), help="time the oriented entry (clockwise degrees) against rot90 + the un-oriented entry")
    ap.add_argument("--hflip", action="store_true")
    ap.add_argument("--vflip", action="store_true")
    ap.add_argument("--scattered", action="store_true", help="time the list entries on separately allocated surfaces (NV12, P010 + PQ, bgra) against the contiguous "
                    "entry on a stacked copy and against torch.stack + that entry")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "frontend_yuv_prof needs the GPU: a CPU run says nothing about time"
    dt = hip.op_dtype()
    if a.scattered:
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "frontend_scattered.json")
        return scattered_run(a, dt)
    if a.rgb_order is not None or a.pix_fmt in ops.PACKED_PIX_FMTS:
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "frontend_packed.json")
        return rgb_order_run(a, dt) if a.rgb_order is not None else packed_run(a, dt)
    if a.rotate or a.hflip or a.vflip:
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "frontend_orient.json")
        return orient_run(a, dt)
    if a.transfer is not None:
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "frontend_hdr.json")
        return hdr_run(a, dt)
    if a.pix_fmt is not None:
        return surface_run(a, dt)
    n, H, W, R = a.frames, a.height, a.width, a.res
    buf = torch.randint(0, 256, (n, H * 3 // 2, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    y, cbcr, _ = ops.split_yuv420(buf, H, W, "nv12")
    colour = dict(matrix="bt709", full_range=False, chroma_loc="left")
    yuv = lambda: ops.yuv_to_patches(y, cbcr, R=R, patch=a.patch, op_dtype=dt, **colour)[0]
    if a.once:
        yuv()
        torch.cuda.synchronize()
        return
    rgb_u8 = torch.cat([to_rgb_float(y[i:i + 4], cbcr[i:i + 4]).round().clamp(0, 255).to(torch.uint8) for i in range(0, n, 4)], 0)
    rgb = lambda: ops.frames_to_patches(rgb_u8, R, a.patch, layout="NCHW", op_dtype=dt)[0]
    comp = lambda: torch_composition(y, cbcr, R, a.patch, dt)
    forms = (("yuv", yuv), ("rgb", rgb), ("torch", comp))
    t, first = {k: [] for k, _ in forms}, {}
    for i in range(a.warmup + a.iters):
        for name, fn in forms:
            s, out = timed(fn)
            if i >= a.warmup:
                t[name].append(s)
            if i == 0:
                first[name] = out
    # source bytes the crop uses: the centred square (the shorter side) of every frame, 1.5 bytes a pixel (3 for the RGB entry)
    used = n * min(H, W) ** 2 * 3 // 2
    med = {k: statistics.median(v) for k, v in t.items()}
    ms = lambda k: dict(median=med[k] * 1e3, min=min(t[k]) * 1e3, max=max(t[k]) * 1e3)
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), frames=n, height=H, width=W, res=R, patch=a.patch, warmup=a.warmup, iters=a.iters,
               yuv_ms=ms("yuv"), rgb_ms=ms("rgb"), torch_ms=ms("torch"), yuv_over_rgb=med["yuv"] / med["rgb"], speedup_vs_torch=med["torch"] / med["yuv"],
               used_source_bytes=used, yuv_bytes_per_s=used / med["yuv"], yuv_fraction_of_8TBps=used / med["yuv"] / HBM_PEAK,
               # not an error figure: the composition upsamples chroma (nearest) before it filters, the kernel filters the chroma planes themselves
               max_abs_diff_yuv_vs_torch=float((first["yuv"].float() - first["torch"].float()).abs().max()),
               max_abs_diff_yuv_vs_rgb_entry_on_rounded_rgb=float((first["yuv"].float() - first["rgb"].float()).abs().max()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
