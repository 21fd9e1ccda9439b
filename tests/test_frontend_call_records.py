"""The CLIP front-end bindings (ops.frames_to_patches / yuv_to_patches / yuv_surface_to_patches / packed_to_patches, their splitters and byte counters, and the
extractor's pix_fmt refusal) against the call records of commit 9e7cd56, on the CPU: every wrapper is driven on small CPU tensors with the stand-ins of
test_scattered_host_logic (a recorder for ``hip.lib``, ``hip.ptr`` -> ``data_ptr()``, ``hip.stream`` -> None, the device check answered), and each call becomes a
plain record - the entry's name, the library's flavour argument, the scalars, struct fields by name, float triples as lists, every input pointer as (which input
storage it falls in, byte offset) or "copy" when it falls in none, the output pointers as "patches" / "image" / null with the outputs' shapes and dtypes.  A
refusal becomes (exception class name, message).  What a splitter or a byte counter returns is recorded the same way (views as storage, offset, shape, strides).

tests/golden/frontend_call_records.json holds, in the order of the sorted case keys, the first 6 hex digits of the SHA-256 of each record's canonical JSON (a
refusal: the first letter of the class name - CLASSES -, then the digest of the message): the records of 460 cases do not fit the size a golden file may have,
their digests do.  The file was written by THIS module run as a script against a checkout of commit 9e7cd56 and must never be regenerated from the code under
test.  To regenerate it (a new case, a new axis), check out the commit whose behaviour is the reference into another directory and run

    python tests/test_frontend_call_records.py --root <that checkout> [--full records.json]

``--full`` also writes the whole records; run it against both trees and diff the two files to see HOW a case that fails here differs.
"""
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "frontend_call_records.json")
U8, U16 = torch.uint8, torch.uint16
RP = dict(R=28, patch=14)

#: case key -> the refusal's new text (the class is still the golden file's).  Reason, all but the first two: at 9e7cd56 the tensor form and the list form worded
#: one condition in two sentences; one body now serves both forms and they share one sentence - the list form's, with the frame axis in the shapes it names.
#: The first two: ClipFeatureExtractor.encode_video takes its pix_fmt / layout refusal from the front-end module, whose sentence names the shape.
REWORDED = {
    "ex/chunks/pix_fmt-nchw": "pix_fmt 'bgr24' names the byte order of packed pixels [n,H,W,3]: layout 'NCHW' does not go with it",
    "ex/pix_fmt-nchw": "pix_fmt 'bgra' names the byte order of packed pixels [n,H,W,4]: layout 'NCHW' does not go with it",
    "rgb/t/dim3": "frames come as a uint8 tensor [n,3,H,W] or [n,H,W,3], got torch.uint8 (3, 6, 10)",
    "rgb/t/float": "frames come as a uint8 tensor [n,3,H,W] or [n,H,W,3], got torch.float32 (3, 3, 6, 10)",
    "y8/t/interleaved/misshapen": "yuv_to_patches: interleaved CbCr of frames 8 x 12 is [3,4,6,2], got (3, 4, 6)",
    "y8/t/planar/cb-interleaved": "yuv_to_patches: Cb and Cr of frames 8 x 12 are [3,4,6], got (3, 4, 6, 2) and (3, 4, 6)",
    "y8/t/planar/misshapen": "yuv_to_patches: Cb and Cr of frames 8 x 12 are [3,4,6], got (3, 4, 6) and (2, 4, 6)",
    "y8/t/y-dim4": "yuv_to_patches: Y planes are [n,H,W] with H a multiple of 2 and W of 2, got (3, 1, 8, 12)",
    "y8/t/y-odd-h": "yuv_to_patches: Y planes are [n,H,W] with H a multiple of 2 and W of 2, got (3, 9, 12)",
    "y8/t/y-odd-w": "yuv_to_patches: Y planes are [n,H,W] with H a multiple of 2 and W of 2, got (3, 8, 13)",
    "ys/t/422/misshapen": "yuv_surface_to_patches: Cb and Cr of frames 8 x 12 are [3,8,6], got (3, 4, 6) and (3, 4, 6)",
    "ys/t/422/odd-w": "yuv_surface_to_patches: Y planes are [n,H,W] with H a multiple of 1 and W of 2, got (2, 8, 7)",
    "ys/t/interleaved/misshapen": "yuv_surface_to_patches: interleaved CbCr of frames 8 x 12 is [3,4,6,2], got (3, 4, 6)",
    "ys/t/planar/cb-interleaved": "yuv_surface_to_patches: Cb and Cr of frames 8 x 12 are [3,4,6], got (3, 4, 6, 2) and (3, 4, 6)",
    "ys/t/planar/misshapen": "yuv_surface_to_patches: Cb and Cr of frames 8 x 12 are [3,4,6], got (3, 4, 6) and (2, 4, 6)",
    "ys/t/y-dim4": "yuv_surface_to_patches: Y planes are [n,H,W] with H a multiple of 2 and W of 2, got (3, 1, 8, 12)",
    "ys/t/y-odd-h": "yuv_surface_to_patches: Y planes are [n,H,W] with H a multiple of 2 and W of 2, got (3, 9, 12)",
    "ys/t/y-odd-w": "yuv_surface_to_patches: Y planes are [n,H,W] with H a multiple of 2 and W of 2, got (3, 8, 13)",
}


def z(*shape, dt=U8):
    return torch.zeros(*shape, dtype=dt)


# ---- the cases: key -> (function name, args, kwargs[, flags]); flags: "cpu" = is_cuda is left alone, "device" = the list forms' device check is left alone ----
def rgb_cases():
    c = {}
    f = "frames_to_patches"
    H, W = 6, 10
    nchw, nhwc = z(3, 3, H, W), z(3, H, W, 3)
    c["rgb/t/nchw"] = (f, (nchw, 28, 14), {})
    c["rgb/t/nchw/n0"] = (f, (z(0, 3, H, W), 28, 14), {})
    c["rgb/t/nchw/n1"] = (f, (z(1, 4, H + 3, W + 7)[:, 1:4, 2:2 + H, 5:5 + W], 28, 14), {})
    c["rgb/t/nchw/window"] = (f, (z(3, 3, H + 3, W + 7)[:, :, 2:2 + H, 5:5 + W], 28, 14), {})
    c["rgb/t/nchw/every-other-frame"] = (f, (z(6, 3, H, W)[::2], 28, 14), {})
    c["rgb/t/nchw/permuted"] = (f, (nhwc.permute(0, 3, 1, 2), 28, 14), {})
    c["rgb/t/nchw/h1"] = (f, (z(2, 3, 1, W), 28, 14), {})
    c["rgb/t/nhwc"] = (f, (nhwc, 28, 14), {})
    c["rgb/t/nhwc/n0"] = (f, (z(0, H, W, 3), 28, 14), {})
    c["rgb/t/nhwc/n1"] = (f, (z(1, H, W, 3), 28, 14), {})
    c["rgb/t/nhwc/window"] = (f, (z(3, H + 2, W + 4, 3)[:, 1:1 + H, 2:2 + W], 28, 14), {})
    c["rgb/t/nhwc/permuted"] = (f, (nchw.permute(0, 2, 3, 1), 28, 14), {})
    c["rgb/t/nhwc/h1"] = (f, (z(2, 1, W, 3), 28, 14), {})
    c["rgb/t/both"] = (f, (z(2, 3, 5, 3), 28, 14), {})
    c["rgb/t/both/nchw"] = (f, (z(2, 3, 5, 3), 28, 14), dict(layout="NCHW"))
    c["rgb/t/both/nhwc"] = (f, (z(2, 3, 5, 3), 28, 14, "NHWC"), {})
    c["rgb/t/neither"] = (f, (z(2, 4, 5, 6), 28, 14), {})
    c["rgb/t/misfit"] = (f, (nchw, 28, 14), dict(layout="NHWC"))
    c["rgb/t/layout-unknown"] = (f, (nchw, 28, 14), dict(layout="CHWN"))
    c["rgb/t/cpu"] = (f, (nchw, 28, 14), {}, "cpu")
    c["rgb/t/not-a-tensor"] = (f, ("frames", 28, 14), {})
    c["rgb/t/float"] = (f, (nchw.float(), 28, 14), {})
    c["rgb/t/dim3"] = (f, (z(3, H, W), 28, 14), {})
    for k, kw in (("rot90", dict(rotate=90)), ("hflip", dict(hflip=True)), ("rot180-vflip", dict(rotate=180, vflip=True)), ("image", dict(want=("image",))),
                  ("both-outputs", dict(want=("patches", "image"))), ("want-list", dict(want=["image", "patches"])), ("bf16", dict(op_dtype=torch.bfloat16)),
                  ("f16-name", dict(op_dtype="f16")), ("mean-std", dict(mean=(0.5, 0.25, 0.125), std=(1.0, 2.0, 4.0)))):
        c["rgb/t/nchw/" + k] = (f, (nchw, 28, 14), kw)
    c["rgb/t/nhwc/rot270"] = (f, (nhwc, 28, 14), dict(rotate=270))
    c["rgb/t/rotate-45"] = (f, (nchw, 28, 14), dict(rotate=45))
    c["rgb/t/rotate-true"] = (f, (nchw, 28, 14), dict(rotate=True))
    c["rgb/t/hflip-1"] = (f, (nchw, 28, 14), dict(hflip=1))
    # pix_fmt, tensor form
    bgra = z(3, H, W, 4)
    c["rgb/t/bgr24"] = (f, (nhwc, 28, 14), dict(pix_fmt="bgr24"))
    c["rgb/t/bgra"] = (f, (bgra, 28, 14), dict(pix_fmt="bgra", layout="NHWC"))
    c["rgb/t/argb/rot270"] = (f, (bgra, 28, 14), dict(pix_fmt="argb", rotate=270, want=("patches", "image")))
    c["rgb/t/bgra/n0"] = (f, (z(0, H, W, 4), 28, 14), dict(pix_fmt="bgra"))
    c["rgb/t/bgra/n1"] = (f, (z(1, H, W, 4), 28, 14), dict(pix_fmt="bgra"))
    c["rgb/t/bgra/window"] = (f, (z(3, H + 2, W + 4, 4)[:, 1:1 + H, 2:2 + W], 28, 14), dict(pix_fmt="bgra"))
    c["rgb/t/bgra/permuted"] = (f, (z(3, 4, H, W).permute(0, 2, 3, 1), 28, 14), dict(pix_fmt="bgra"))
    c["rgb/t/bgra/h1"] = (f, (z(2, 1, W, 4), 28, 14), dict(pix_fmt="bgra"))
    c["rgb/t/pix_fmt-unknown"] = (f, (bgra, 28, 14), dict(pix_fmt="rgb48le"))
    c["rgb/t/pix_fmt-nchw"] = (f, (bgra, 28, 14), dict(pix_fmt="bgra", layout="NCHW"))
    c["rgb/t/bgra/3-bytes"] = (f, (nhwc, 28, 14), dict(pix_fmt="bgra"))
    c["rgb/t/bgra/float"] = (f, (bgra.float(), 28, 14), dict(pix_fmt="bgra"))
    c["rgb/t/bgra/not-a-tensor"] = (f, (7, 28, 14), dict(pix_fmt="bgra"))
    c["rgb/t/bgra/cpu"] = (f, (bgra, 28, 14), dict(pix_fmt="bgra"), "cpu")
    # list form
    pool = [z(3, H + 3, W + 7) for _ in range(4)]
    win = [pool[i][:, 2:2 + H, 5:5 + W] for i in (2, 0, 3, 0)]                                # frame 0 of the pool is listed twice
    c["rgb/l/nchw"] = (f, ([z(3, H, W) for _ in range(3)], 28, 14), {})
    c["rgb/l/nchw/n1"] = (f, ([z(3, H, W)], 28, 14), {})
    c["rgb/l/nchw/window-twice"] = (f, (win, 28, 14), dict(want=("patches", "image")))
    c["rgb/l/nchw/tuple"] = (f, (tuple(win[:3]), 28, 14), dict(rotate=90))
    c["rgb/l/nchw/permuted"] = (f, ([z(H, W, 3).permute(2, 0, 1) for _ in range(3)], 28, 14), dict(layout="NCHW"))
    c["rgb/l/nchw/h1"] = (f, ([z(3, 1, W) for _ in range(2)], 28, 14), {})
    c["rgb/l/nhwc"] = (f, ([z(H, W, 3) for _ in range(3)], 28, 14), dict(hflip=True, op_dtype="bf16"))
    c["rgb/l/nhwc/window"] = (f, ([z(H + 2, W + 4, 3)[1:1 + H, 2:2 + W] for _ in range(3)], 28, 14), {})
    c["rgb/l/nhwc/permuted"] = (f, ([z(3, H, W).permute(1, 2, 0) for _ in range(3)], 28, 14), {})
    c["rgb/l/both"] = (f, ([z(3, 5, 3)], 28, 14), {})
    c["rgb/l/both/nchw"] = (f, ([z(3, 5, 3)], 28, 14), dict(layout="NCHW"))
    c["rgb/l/both/nhwc"] = (f, ([z(3, 5, 3)], 28, 14), dict(layout="NHWC"))
    c["rgb/l/neither"] = (f, ([z(4, 5, 6)], 28, 14), {})
    c["rgb/l/misfit"] = (f, ([z(3, H, W)], 28, 14), dict(layout="NHWC"))
    c["rgb/l/float"] = (f, ([z(3, H, W).float()], 28, 14), {})
    c["rgb/l/dim4"] = (f, ([z(1, 3, H, W)], 28, 14), {})
    c["rgb/l/bgra"] = (f, ([z(H, W + 2, 4)[:, 1:1 + W] for _ in range(3)], 28, 14), dict(pix_fmt="bgra", rotate=90))
    c["rgb/l/bgr24/permuted"] = (f, (tuple(z(3, H, W).permute(1, 2, 0) for _ in range(2)), 28, 14), dict(pix_fmt="bgr24"))
    c["rgb/l/pix_fmt-unknown"] = (f, ([z(H, W, 4)], 28, 14), dict(pix_fmt="rgb48le"))
    c["rgb/l/pix_fmt-nchw"] = (f, ([z(H, W, 4)], 28, 14), dict(pix_fmt="bgra", layout="NCHW"))
    c["rgb/l/bgra/3-bytes"] = (f, ([z(H, W, 3)], 28, 14), dict(pix_fmt="bgra"))
    c["rgb/l/empty"] = (f, ([], 28, 14), {})
    c["rgb/l/not-a-tensor"] = (f, ([z(3, H, W), "frame"], 28, 14), {})
    c["rgb/l/disagrees"] = (f, ([z(3, H, W), z(3, H, W + 2)], 28, 14), {})
    c["rgb/l/cpu"] = (f, ([z(3, H, W)], 28, 14), {}, "cpu device")
    c["rgb/l/rotate-45"] = (f, ([z(3, H, W)], 28, 14), dict(rotate=45))
    return c


def yuv_cases():
    c = {}
    H, W, h, w = 8, 12, 4, 6
    for f, tag in (("yuv_to_patches", "y8"), ("yuv_surface_to_patches", "ys")):
        planar = lambda n=3: (z(n, H, W), z(n, h, w), z(n, h, w))                              # noqa: E731
        c[tag + "/t/planar"] = (f, planar(), RP)
        c[tag + "/t/planar/n0"] = (f, planar(0), RP)
        c[tag + "/t/planar/n1"] = (f, (z(1, H + 2, W)[:, :H], z(1, h + 1, w)[:, 1:], z(1, h + 1, w)[:, 1:]), RP)
        c[tag + "/t/planar/rot90"] = (f, planar(), dict(RP, rotate=90, matrix="bt709", full_range=True, chroma_loc="centre"))
        c[tag + "/t/planar/hflip"] = (f, planar(1), dict(RP, hflip=True, want=("image",), op_dtype=torch.bfloat16))
        c[tag + "/t/planar/tags"] = (f, planar(), dict(RP, matrix="bt709", full_range=1, chroma_loc="centre", want=("patches", "image"), op_dtype="bf16"))
        c[tag + "/t/interleaved"] = (f, (z(3, H, W), z(3, h, w, 2)), RP)
        c[tag + "/t/interleaved/n0"] = (f, (z(0, H, W), z(0, h, w, 2)), RP)
        c[tag + "/t/interleaved/window"] = (f, (z(3, H + 2, W + 4)[:, 1:1 + H, 2:2 + W], z(3, h, w + 2, 2)[:, :, 1:1 + w]), RP)
        c[tag + "/t/interleaved/every-other-pair"] = (f, (z(3, H, W), z(3, h, w, 4)[..., ::2]), RP)
        c[tag + "/t/interleaved/permuted"] = (f, (z(3, H, W), z(3, 2, h, w).permute(0, 2, 3, 1)), RP)
        vu = z(3, h, w, 2)
        c[tag + "/t/nv21-views"] = (f, (z(3, H, W), vu[..., 1], vu[..., 0]), RP)
        c[tag + "/t/nv21-views/rot270"] = (f, (z(3, H, W), vu[..., 1], vu[..., 0]), dict(RP, rotate=270))
        c[tag + "/t/two-apart-not-one"] = (f, (z(3, H, W), z(3, h, w, 4)[..., 0], z(3, h, w, 4)[..., 2]), RP)
        c[tag + "/t/cb-cr-strides-differ"] = (f, (z(3, H, W), z(3, h, w), z(3, h, w + 2)[:, :, :w]), RP)
        c[tag + "/t/planar/window"] = (f, (z(3, H + 2, W + 4)[:, 1:1 + H, 2:2 + W], z(3, h, w + 2)[:, :, :w], z(3, h, w + 2)[:, :, 2:]), RP)
        c[tag + "/t/y-transposed"] = (f, (z(3, W, H).transpose(1, 2),) + planar()[1:], RP)
        c[tag + "/t/y-every-other-frame"] = (f, (z(6, H, W)[::2],) + planar()[1:], RP)
        c[tag + "/t/one-chroma-row"] = (f, (z(2, 2, W), z(2, 1, w + 2)[:, :, :w], z(2, 1, w + 2)[:, :, :w]), RP)
        c[tag + "/t/one-chroma-row/interleaved"] = (f, (z(2, 2, W), z(2, 1, w + 2, 2)[:, :, :w]), RP)
        c[tag + "/t/one-chroma-column"] = (f, (z(2, H, 2), z(2, h, 1, 2)), RP)
        c[tag + "/t/one-chroma-column/planar"] = (f, (z(2, H, 4)[:, :, :2], z(2, h, 2)[:, :, :1], z(2, h, 2)[:, :, :1]), RP)
        # refusals of the tensor form
        c[tag + "/t/cpu"] = (f, planar(), RP, "cpu")
        c[tag + "/t/not-a-tensor"] = (f, (z(3, H, W), None, z(3, h, w)), RP)
        c[tag + "/t/float"] = (f, (z(3, H, W).float(), z(3, h, w), z(3, h, w)), RP)
        c[tag + "/t/cr-int16"] = (f, (z(3, H, W), z(3, h, w), z(3, h, w, dt=torch.int16)), RP)
        c[tag + "/t/u16"] = (f, (z(3, H, W, dt=U16), z(3, h, w, dt=U16), z(3, h, w, dt=U16)), RP)
        c[tag + "/t/matrix-unknown"] = (f, planar(), dict(RP, matrix="bt470"))
        c[tag + "/t/matrix-bt2020"] = (f, planar(), dict(RP, matrix="bt2020"))
        c[tag + "/t/chroma_loc-topleft"] = (f, planar(), dict(RP, chroma_loc="topleft"))
        c[tag + "/t/chroma_loc-unknown"] = (f, planar(), dict(RP, chroma_loc="bottom"))
        c[tag + "/t/y-dim4"] = (f, (z(3, 1, H, W), z(3, h, w), z(3, h, w)), RP)
        c[tag + "/t/y-odd-h"] = (f, (z(3, H + 1, W), z(3, h, w), z(3, h, w)), RP)
        c[tag + "/t/y-odd-w"] = (f, (z(3, H, W + 1), z(3, h, w), z(3, h, w)), RP)
        c[tag + "/t/interleaved/misshapen"] = (f, (z(3, H, W), z(3, h, w)), RP)
        c[tag + "/t/planar/misshapen"] = (f, (z(3, H, W), z(3, h, w), z(2, h, w)), RP)
        c[tag + "/t/planar/cb-interleaved"] = (f, (z(3, H, W), z(3, h, w, 2), z(3, h, w)), RP)
        c[tag + "/t/rotate-45"] = (f, planar(), dict(RP, rotate=45))
        # list form
        sep = lambda n=3: ([z(H, W) for _ in range(n)], [z(h, w) for _ in range(n)], [z(h, w) for _ in range(n)])   # noqa: E731
        c[tag + "/l/planar"] = (f, sep(), dict(RP, matrix="bt709", chroma_loc="centre", rotate=180))
        c[tag + "/l/planar/n1"] = (f, sep(1), dict(RP, want=("patches", "image")))
        c[tag + "/l/planar/tuples"] = (f, tuple(tuple(p) for p in sep()), dict(RP, op_dtype="bf16", full_range=True))
        ys, cs = [z(H, W + 4)[:, :W] for _ in range(3)], [z(h + 1, w + 2)[1:, 1:1 + w] for _ in range(3)]
        c[tag + "/l/planar/window-twice"] = (f, ([ys[i] for i in (2, 0, 1, 0)], [cs[i] for i in (0, 1, 2, 1)], [cs[i] for i in (1, 2, 0, 2)]), RP)
        c[tag + "/l/interleaved"] = (f, ([z(H, W) for _ in range(3)], [z(h, w, 2) for _ in range(3)]), dict(RP, vflip=True))
        c[tag + "/l/interleaved/window"] = (f, ([z(H, W) for _ in range(2)], [z(h, w + 1, 2)[:, :w] for _ in range(2)]), RP)
        c[tag + "/l/interleaved/every-other-pair"] = (f, ([z(H, W) for _ in range(2)], [z(h, w, 4)[..., ::2] for _ in range(2)]), RP)
        vus = [z(h, w, 2) for _ in range(2)]
        c[tag + "/l/nv21-views"] = (f, ([z(H, W) for _ in range(2)], [t[..., 1] for t in vus], [t[..., 0] for t in vus]), RP)
        c[tag + "/l/cb-cr-strides-differ"] = (f, ([z(H, W) for _ in range(2)], [z(h, w) for _ in range(2)], [z(h, w + 2)[:, :w] for _ in range(2)]), RP)
        c[tag + "/l/y-transposed"] = (f, ([z(W, H).t() for _ in range(2)],) + sep(2)[1:], RP)
        c[tag + "/l/one-chroma-row"] = (f, ([z(2, W) for _ in range(2)], [z(1, w + 2)[:, :w] for _ in range(2)], [z(1, w + 2)[:, :w] for _ in range(2)]), RP)
        c[tag + "/l/one-chroma-column"] = (f, ([z(H, 2) for _ in range(2)], [z(h, 1, 2) for _ in range(2)]), RP)
        # refusals of the list form
        y2, c2 = [z(4, 8), z(4, 8)], [z(2, 4), z(2, 4)]
        c[tag + "/l/matrix-unknown"] = (f, (y2, c2, c2), dict(RP, matrix="bt470"))
        c[tag + "/l/matrix-bt2020"] = (f, (y2, c2, c2), dict(RP, matrix="bt2020"))
        c[tag + "/l/chroma_loc-topleft"] = (f, (y2, c2, c2), dict(RP, chroma_loc="topleft"))
        c[tag + "/l/u16"] = (f, ([t.to(U16) for t in y2], [t.to(U16) for t in c2], [t.to(U16) for t in c2]), RP)
        c[tag + "/l/int16"] = (f, ([t.to(torch.int16) for t in y2], [t.to(torch.int16) for t in c2], [t.to(torch.int16) for t in c2]), RP)
        c[tag + "/l/cb-a-tensor"] = (f, (y2, z(2, 2, 4), c2), RP)
        c[tag + "/l/cr-a-tensor"] = (f, (y2, c2, z(2, 2, 4)), RP)
        c[tag + "/l/empty"] = (f, ([], [], []), RP)
        c[tag + "/l/cb-empty"] = (f, (y2, [], c2), RP)
        c[tag + "/l/cr-not-a-tensor"] = (f, (y2, c2, [c2[0], None]), RP)
        c[tag + "/l/cb-disagrees"] = (f, (y2, [z(2, 4), z(2, 5)], c2), RP)
        c[tag + "/l/cb-shorter"] = (f, (y2, c2[:1], c2), RP)
        c[tag + "/l/cr-shorter"] = (f, (y2, c2, c2[:1]), RP)
        c[tag + "/l/cb-shorter/interleaved"] = (f, (y2, [z(2, 4, 2)]), RP)
        c[tag + "/l/cb-u16"] = (f, (y2, [t.to(U16) for t in c2], c2), RP)
        c[tag + "/l/cr-on-meta"] = (f, (y2, c2, [t.to("meta") for t in c2]), RP)
        c[tag + "/l/y-dim3"] = (f, ([z(2, 4, 8)], c2[:1], c2[:1]), RP)
        c[tag + "/l/y-odd-h"] = (f, ([z(5, 8)], c2[:1], c2[:1]), RP)
        c[tag + "/l/interleaved/misshapen"] = (f, (y2, c2), RP)
        c[tag + "/l/planar/misshapen"] = (f, (y2, [z(2, 4, 2), z(2, 4, 2)], c2), RP)
        c[tag + "/l/planar/cr-misshapen"] = (f, (y2, c2, [z(2, 5), z(2, 5)]), RP)
        c[tag + "/l/cpu"] = (f, sep(), RP, "cpu device")
        c[tag + "/l/hflip-none"] = (f, sep(), dict(RP, hflip=None))
    # the surface wrapper's own axes
    f = "yuv_surface_to_patches"
    p010 = lambda n=3: (z(n, H, W, dt=U16), z(n, h, w, 2, dt=U16))                             # noqa: E731
    hdr10 = dict(RP, depth=10, msb_aligned=True, matrix="bt2020", chroma_loc="topleft")
    c["ys/t/p010"] = (f, p010(), hdr10)
    c["ys/t/p010/pq"] = (f, p010(), dict(hdr10, transfer="pq", peak_nits=600.0))
    c["ys/t/p010/hlg"] = (f, p010(), dict(hdr10, transfer="hlg", sdr_white_nits=100, gamut=False, want=("patches", "image")))
    c["ys/t/p010/smpte2084/rot90"] = (f, p010(), dict(hdr10, transfer="smpte2084", rotate=90))
    c["ys/t/p010/pq/bt709-matrix"] = (f, p010(), dict(hdr10, transfer="pq", matrix="bt709"))
    c["ys/t/p010/pq/gamut-forced"] = (f, p010(), dict(hdr10, transfer="pq", matrix="bt709", gamut=1))
    c["ys/t/p010/transfer-unknown"] = (f, p010(), dict(hdr10, transfer="gamma"))
    c["ys/t/p010/window"] = (f, (z(3, H + 2, W + 4, dt=U16)[:, 1:1 + H, 2:2 + W], z(3, h, w + 2, 2, dt=U16)[:, :, 1:1 + w]), hdr10)
    vu16 = z(3, h, w, 2, dt=U16)
    c["ys/t/u16/crcb-views"] = (f, (z(3, H, W, dt=U16), vu16[..., 1], vu16[..., 0]), dict(RP, depth=16))
    c["ys/t/u16/planar/12-bit"] = (f, (z(3, H, W, dt=U16), z(3, h, w, dt=U16), z(3, h, w, dt=U16)), dict(RP, depth=12, hflip=True))
    c["ys/t/u16/y-transposed"] = (f, (z(3, W, H, dt=U16).transpose(1, 2), z(3, h, w, 4, dt=U16)[..., ::2]), dict(RP, depth=10))
    c["ys/t/cb-u16-y-u8"] = (f, (z(3, H, W), z(3, h, w, dt=U16), z(3, h, w, dt=U16)), RP)
    c["ys/t/422"] = (f, (z(3, H, W), z(3, H, w), z(3, H, w)), dict(RP, subsampling="422"))
    c["ys/t/422/interleaved/rot90"] = (f, (z(3, H, W), z(3, H, w, 2)), dict(RP, subsampling="422", rotate=90))
    c["ys/t/444"] = (f, (z(3, H, W), z(3, H, W), z(3, H, W)), dict(RP, subsampling="444"))
    c["ys/t/444/odd-sides"] = (f, (z(2, 5, 7), z(2, 5, 7, 2)), dict(RP, subsampling="444"))
    c["ys/t/444/one-row"] = (f, (z(2, 1, W + 2)[:, :, :W], z(2, 1, W, 2)), dict(RP, subsampling="444"))
    c["ys/t/422/odd-h"] = (f, (z(2, 5, W), z(2, 5, w), z(2, 5, w)), dict(RP, subsampling="422"))
    c["ys/t/422/odd-w"] = (f, (z(2, H, 7), z(2, H, 3), z(2, H, 3)), dict(RP, subsampling="422"))
    c["ys/t/422/misshapen"] = (f, (z(3, H, W), z(3, h, w), z(3, h, w)), dict(RP, subsampling="422"))
    c["ys/t/subsampling-unknown"] = (f, (z(3, H, W), z(3, h, w), z(3, h, w)), dict(RP, subsampling="411"))
    c["ys/l/subsampling-unknown"] = (f, ([z(H, W)], [z(h, w)], [z(h, w)]), dict(RP, subsampling="411"))
    c["ys/l/transfer-unknown"] = (f, ([z(H, W)], [z(h, w)], [z(h, w)]), dict(RP, transfer="gamma"))
    c["ys/l/p010/pq"] = (f, ([z(H, W, dt=U16) for _ in range(2)], [z(h, w + 1, 2, dt=U16)[:, :w] for _ in range(2)]), dict(hdr10, transfer="pq", peak_nits=600.0))
    c["ys/l/p010/hlg/rot270"] = (f, ([z(H, W, dt=U16) for _ in range(2)], [z(h, w, 2, dt=U16) for _ in range(2)]), dict(hdr10, transfer="hlg", rotate=270))
    vus16 = [z(h, w, 2, dt=U16) for _ in range(2)]
    c["ys/l/u16/crcb-views"] = (f, ([z(H, W, dt=U16) for _ in range(2)], [t[..., 1] for t in vus16], [t[..., 0] for t in vus16]), dict(RP, depth=16))
    c["ys/l/u16/y-transposed"] = (f, ([z(W, H, dt=U16).t() for _ in range(2)], [z(h, w, 4, dt=U16)[..., ::2] for _ in range(2)]), dict(RP, depth=10))
    c["ys/l/422"] = (f, ([z(H, W) for _ in range(2)], [z(H, w) for _ in range(2)], [z(H, w) for _ in range(2)]), dict(RP, subsampling="422", hflip=True))
    c["ys/l/444/one-row"] = (f, ([z(1, W + 2)[:, :W] for _ in range(2)], [z(1, W, 2) for _ in range(2)]), dict(RP, subsampling="444"))
    c["ys/l/422/odd-w"] = (f, ([z(H, 7)], [z(H, 3)], [z(H, 3)]), dict(RP, subsampling="422"))
    # a 60-frame pool, as a decoder hands it over
    c["ys/l/60-frames"] = (f, ([z(H, W) for _ in range(60)], [z(h, w, 2) for _ in range(60)]), RP)
    return c


def split_cases():
    """Every PIX_FMTS name through split_yuv into the surface wrapper (the record holds where each plane lies in the buffer), the three formats of split_yuv420 into
    the 8-bit wrapper, and the splitters' and byte counters' own returns and refusals."""
    from revisionllm_amd import ops
    c = {}
    H, W = 8, 12
    for name in sorted(ops.PIX_FMTS):
        for n in (2,) if name not in ("nv12", "yuv420p10le") else (0, 1, 2):
            c[f"split/{name}/n{n}"] = ("split_yuv+yuv_surface_to_patches", (z(n, ops.yuv_frame_bytes(H, W, name)), H, W, name), RP)
        c[f"split/{name}/views"] = ("split_yuv", (z(5, ops.yuv_frame_bytes(H, W, name) + 2)[1:4, 2:], H, W, name), {})
        c[f"bytes/{name}"] = ("yuv_frame_bytes", (H, W, name), {})
    c["split/p010le/odd-offset"] = ("split_yuv", (z(3, ops.yuv_frame_bytes(H, W, "p010le") + 1)[:, 1:], H, W, "p010le"), {})
    c["split/p010le/odd-frame-stride"] = ("split_yuv", (z(3, ops.yuv_frame_bytes(H, W, "p010le") + 1)[:, :-1], H, W, "p010le"), {})
    c["split/nv12/every-other-byte"] = ("split_yuv", (z(3, 2 * ops.yuv_frame_bytes(H, W, "nv12"))[:, ::2], H, W, "nv12"), {})
    c["split/nv12/misshapen"] = ("split_yuv", (z(3, 10), H, W, "nv12"), {})
    c["split/nv12/not-a-tensor"] = ("split_yuv", (b"bytes", H, W, "nv12"), {})
    c["split/pix_fmt-unknown"] = ("split_yuv", (z(3, 10), H, W, "yuyv422"), {})
    c["bytes/pix_fmt-unknown"] = ("yuv_frame_bytes", (H, W, "rgb24"), {})
    c["bytes/nv12/odd-h"] = ("yuv_frame_bytes", (H + 1, W, "nv12"), {})
    c["bytes/nv16/odd-h"] = ("yuv_frame_bytes", (H + 1, W, "nv16"), {})
    c["bytes/nv16/odd-w"] = ("yuv_frame_bytes", (H, W + 1, "nv16"), {})
    c["bytes/nv24/zero"] = ("yuv_frame_bytes", (0, W, "nv24"), {})
    for fmt in ("nv12", "nv21", "i420"):
        c[f"split420/{fmt}"] = ("split_yuv420+yuv_to_patches", (z(2, H * 3 // 2, W), H, W, fmt), RP)
        c[f"split420/{fmt}/rot90"] = ("split_yuv420+yuv_to_patches", (z(2, H * 3 // 2, W), H, W, fmt), dict(RP, rotate=90))
        c[f"split420/{fmt}/views"] = ("split_yuv420", (z(4, H * 3 // 2, W)[1:3], H, W, fmt), {})
    c["split420/fmt-unknown"] = ("split_yuv420", (z(2, H * 3 // 2, W), H, W, "p010le"), {})
    c["split420/odd-h"] = ("split_yuv420", (z(2, 9, 12), 6, W + 1, "nv12"), {})
    c["split420/too-small"] = ("split_yuv420", (z(2, 0, 12), 0, W, "nv12"), {})
    c["split420/misshapen"] = ("split_yuv420", (z(2, H, W), H, W, "nv12"), {})
    c["split420/not-a-tensor"] = ("split_yuv420", (None, H, W, "nv12"), {})
    c["split420/padded-pitch"] = ("split_yuv420", (z(2, H * 3 // 2, W + 4)[:, :, :W], H, W, "i420"), {})
    c["split420/every-other-byte"] = ("split_yuv420", (z(2, H * 3 // 2, 2 * W)[:, :, ::2], H, W, "i420"), {})
    for k, a in (("default", ()), ("rot90", (90,)), ("rot180-hflip", (180, True)), ("rot270-both", (270, True, True)), ("vflip", (0, False, True)), ("rotate-45", (45,)),
                 ("rotate-90.0", (90.0,)), ("vflip-0", (0, False, 0))):
        c["orientation/" + k] = ("orientation", a, {})
    for k, a in (("none", (None,)), ("pq", ("pq",)), ("hlg-bt709", ("hlg", "bt709")), ("pq-gamut-off", ("pq", "bt2020", False, 4000, 100)), ("unknown", ("linear",))):
        c["hdr_map/" + k] = ("hdr_map", a, {})
    return c


def packed_cases():
    from revisionllm_amd import ops
    c = {}
    f = "packed_to_patches"
    H, W = 4, 8
    for name in ("yuyv422", "y210le", "xv30le"):
        rb, fb = ops.packed_frame_bytes(1, W, name), ops.packed_frame_bytes(H, W, name)
        kw = dict(RP, H=H, W=W, pix_fmt=name)
        c[f"pk/{name}/t/rows"] = (f, (z(3, H, rb),), kw)
        c[f"pk/{name}/t/flat"] = (f, (z(3, fb),), dict(kw, matrix="bt709", full_range=True, chroma_loc="centre"))
        c[f"pk/{name}/t/n0"] = (f, (z(0, H, rb),), kw)
        c[f"pk/{name}/t/flat/n0"] = (f, (z(0, fb),), kw)
        c[f"pk/{name}/t/n1"] = (f, (z(1, H + 1, rb)[:, :H],), kw)
        c[f"pk/{name}/t/window"] = (f, (z(3, H + 2, rb + 24)[:, 1:1 + H, 8:8 + rb],), dict(kw, hflip=True, want=("patches", "image")))
        c[f"pk/{name}/t/flat/window"] = (f, (z(3, fb + 16)[:, 8:8 + fb],), kw)
        c[f"pk/{name}/t/transposed"] = (f, (z(3, rb, H).transpose(1, 2),), kw)
        c[f"pk/{name}/t/flat/every-other-byte"] = (f, (z(3, 2 * fb)[:, ::2],), kw)
        c[f"pk/{name}/t/every-other-frame"] = (f, (z(6, H, rb)[::2],), kw)
        c[f"pk/{name}/t/h1"] = (f, (z(2, 1, rb + 8)[:, :, :rb],), dict(kw, H=1))
        c[f"pk/{name}/t/offset-1"] = (f, (z(3, H, rb + 1)[:, :, 1:],), kw)
        c[f"pk/{name}/t/offset-2"] = (f, (z(3, H, rb + 4)[:, :, 2:2 + rb],), kw)
        c[f"pk/{name}/t/row-stride-odd"] = (f, (z(3, H, rb + 1)[:, :, :rb],), kw)
        c[f"pk/{name}/t/frame-stride-odd"] = (f, (z(3, fb + 1)[:, :fb],), kw)
        c[f"pk/{name}/t/transposed/offset-1"] = (f, (z(3, rb + 1, H).transpose(1, 2)[:, :, 1:],), kw)
        c[f"pk/{name}/t/pq/rot90"] = (f, (z(3, H, rb),), dict(kw, transfer="pq", matrix="bt2020", rotate=90, op_dtype="bf16"))
        c[f"pk/{name}/t/hlg"] = (f, (z(3, H, rb),), dict(kw, transfer="hlg", peak_nits=400.0))
        c[f"pk/{name}/l/rows"] = (f, ([z(H, rb) for _ in range(3)],), kw)
        c[f"pk/{name}/l/flat"] = (f, (tuple(z(fb) for _ in range(3)),), dict(kw, vflip=True))
        c[f"pk/{name}/l/n1"] = (f, ([z(fb)],), kw)
        big = [z(H + 2, rb + 24) for _ in range(3)]
        c[f"pk/{name}/l/window-twice"] = (f, ([big[i][1:1 + H, 8:8 + rb] for i in (2, 0, 1, 0)],), dict(kw, matrix="bt709", want=("patches", "image")))
        c[f"pk/{name}/l/flat/window"] = (f, ([z(fb + 16)[8:8 + fb] for _ in range(2)],), kw)
        c[f"pk/{name}/l/transposed"] = (f, ([z(rb, H).t() for _ in range(2)],), kw)
        c[f"pk/{name}/l/flat/every-other-byte"] = (f, ([z(2 * fb)[::2] for _ in range(2)],), kw)
        c[f"pk/{name}/l/h1"] = (f, ([z(1, rb + 8)[:, :rb] for _ in range(2)],), dict(kw, H=1))
        c[f"pk/{name}/l/offset-1"] = (f, ([z(H, rb + 1)[:, 1:] for _ in range(2)],), kw)
        c[f"pk/{name}/l/row-stride-odd"] = (f, ([z(H, rb + 1)[:, :rb] for _ in range(2)],), kw)
        c[f"pk/{name}/l/pq/rot270"] = (f, ([z(H, rb) for _ in range(2)],), dict(kw, transfer="pq", rotate=270))
    kw = dict(RP, H=H, W=W, pix_fmt="yuyv422")
    good = z(3, H, 16)
    c["pk/t/pix_fmt-planar"] = (f, (good,), dict(kw, pix_fmt="nv12"))
    c["pk/t/rotate-45"] = (f, (good,), dict(kw, rotate=45))
    c["pk/t/transfer-unknown"] = (f, (good,), dict(kw, transfer="gamma"))
    c["pk/t/matrix-unknown"] = (f, (good,), dict(kw, matrix="bt470"))
    c["pk/t/chroma_loc-unknown"] = (f, (good,), dict(kw, chroma_loc="bottom"))
    c["pk/t/odd-w"] = (f, (good,), dict(kw, W=7))
    c["pk/t/h-zero"] = (f, (good,), dict(kw, H=0))
    c["pk/t/misshapen"] = (f, (z(3, H, 20),), kw)
    c["pk/t/flat/misshapen"] = (f, (z(3, 60),), kw)
    c["pk/t/dim4"] = (f, (z(3, 1, H, 16),), kw)
    c["pk/t/int16"] = (f, (good.short(),), kw)
    c["pk/t/not-a-tensor"] = (f, (bytearray(64),), kw)
    c["pk/t/cpu"] = (f, (good,), kw, "cpu")
    c["pk/l/empty"] = (f, ([],), kw)
    c["pk/l/not-a-tensor"] = (f, ([z(H, 16), 7],), kw)
    c["pk/l/disagrees"] = (f, ([z(H, 16), z(H, 32)],), kw)
    c["pk/l/misshapen"] = (f, ([z(H, 20)],), kw)
    c["pk/l/int16"] = (f, ([z(H, 16).short()],), kw)
    c["pk/l/matrix-unknown"] = (f, ([z(H, 16)],), dict(kw, matrix="bt470"))
    c["pk/l/cpu"] = (f, ([z(H, 16)],), kw, "cpu device")
    for k, a in (("yuyv422", (H, W, "yuyv422")), ("xv30le", (H, W, "xv30le")), ("y210le/odd-w", (H, 7, "y210le")), ("y210le/h-true", (True, W, "y210le")),
                 ("pix_fmt-unknown", (H, W, "p010le"))):
        c["pk/bytes/" + k] = ("packed_frame_bytes", a, {})
    return c


class Towers:
    """Stands in for ClipTowers in the extractor cases: nothing of it is reached by a refusal."""
    device, cfg = "cpu", dict(image_res=14, patch=14, embed_dim=4)


def extractor_cases():
    f = "ClipFeatureExtractor.encode_video"
    return {"ex/pix_fmt-unknown": (f, (z(2, 4, 6, 4),), dict(pix_fmt="rgb48le")),
            "ex/pix_fmt-nchw": (f, (z(2, 4, 6, 4),), dict(pix_fmt="bgra", layout="NCHW")),
            "ex/chunks/pix_fmt-nchw": (f, ([z(2, 4, 6, 3)],), dict(pix_fmt="bgr24", layout="NCHW", scattered=True)),
            "ex/rotate-45": (f, (z(2, 4, 6, 4),), dict(pix_fmt="bgra", rotate=45))}


def all_cases():
    c = {}
    for part in (rgb_cases, yuv_cases, split_cases, packed_cases, extractor_cases):
        for k, v in part().items():
            assert k not in c, k
            c[k] = v
    return c


# ---- running a case with the stand-ins, and the record it leaves ----
class Ptr(int):
    """What the stand-in for hip.ptr returns: the address, known to be one."""


class Recorder:
    def __init__(self):
        self.calls, self.flavours = [], []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, self.flavours[-1], args))
            return 0
        return fn


@contextlib.contextmanager
def patched(pairs):
    old = [(o, n, getattr(o, n)) for o, n, _ in pairs]
    for o, n, v in pairs:
        setattr(o, n, v)
    try:
        yield
    finally:
        for o, n, v in old:
            setattr(o, n, v)


def tensors_in(x):
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, (list, tuple)):
        for e in x:
            yield from tensors_in(e)
    elif isinstance(x, dict):
        for e in x.values():
            yield from tensors_in(e)


class Resolver:
    """Addresses -> where they point: into the n-th distinct storage of the inputs, into an output, or into a copy."""

    def __init__(self, inputs):
        self.storages, self.outputs = [], {}
        for t in tensors_in(inputs):
            if t.device.type == "cpu":
                s = t.untyped_storage()
                if s.nbytes() and all(s.data_ptr() != p for p, _ in self.storages):
                    self.storages.append((s.data_ptr(), s.nbytes()))

    def __call__(self, p):
        if not p:
            return None
        for name, t in self.outputs.items():
            if t is not None and t.numel() and t.data_ptr() == p:
                return name
        for i, (base, size) in enumerate(self.storages):
            if base <= p < base + size:
                return [i, p - base]
        return "copy"

    def view(self, t):
        """A returned tensor: the view of an input that it is, or new memory."""
        where = self(t.data_ptr()) if t.device.type == "cpu" else None
        return dict(at=where, shape=list(t.shape), strides=list(t.stride()), dtype=str(t.dtype))


def plain(v, resolve):
    """One argument of an entry, or one returned value -> JSON."""
    if hasattr(v, "_obj"):                                                                   # ctypes.byref(struct)
        v = v._obj
    if isinstance(v, ctypes.Structure):
        return {n: (resolve(getattr(v, n)) if t is ctypes.c_void_p else plain(getattr(v, n), resolve)) for n, t in v._fields_}
    if isinstance(v, ctypes.Array):
        if v._type_ is ctypes.c_void_p:
            return [resolve(p) for p in v]
        return [plain(e, resolve) for e in v]
    if isinstance(v, Ptr):
        return dict(ptr=resolve(int(v)))
    if torch.is_tensor(v):
        return resolve.view(v)
    if isinstance(v, (list, tuple)):
        return [plain(e, resolve) for e in v]
    if isinstance(v, dict):
        return {str(k): plain(e, resolve) for k, e in v.items()}
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return repr(v)


def run_case(case):
    """-> the record of one case: {"calls": [...], "returns": ...} or {"refused": [class name, message]}."""
    from revisionllm_amd import hip, ops
    from revisionllm_amd.data.clip_extractor import ClipFeatureExtractor
    fn, args, kwargs = case[:3]
    flags = case[3].split() if len(case) > 3 else []
    home = sys.modules[ops.frames_to_patches.__module__]                                     # where the wrappers look the device check up
    rec = Recorder()
    pairs = [(hip, "lib", lambda f=None: (rec.flavours.append(str(f)), rec)[1]), (hip, "ptr", lambda t: None if t is None else Ptr(t.data_ptr())),
             (hip, "stream", lambda: None)]
    if "cpu" not in flags:
        pairs.append((torch.Tensor, "is_cuda", property(lambda self: True)))
    if "device" not in flags:
        pairs.append((home, "_require_device", lambda tensors, who, *a: None))
    resolve = Resolver((args, kwargs))

    def call():
        if fn.startswith("ClipFeatureExtractor."):
            return getattr(ClipFeatureExtractor(Towers()), fn.split(".")[1])(*args, **kwargs)
        if fn == "split_yuv+yuv_surface_to_patches":
            planes, kw = ops.split_yuv(*args)
            return ops.yuv_surface_to_patches(*planes, **kw, **kwargs)
        if fn == "split_yuv420+yuv_to_patches":
            return ops.yuv_to_patches(*ops.split_yuv420(*args), **kwargs)
        return getattr(ops, fn)(*args, **kwargs)

    with patched(pairs):
        try:
            out = call()
        except Exception as e:                                                               # noqa: BLE001 (whatever is raised is the record)
            assert rec.calls == [], "refused after the library was touched"
            return dict(refused=[type(e).__name__, str(e)])
    if fn.endswith("_to_patches"):
        resolve.outputs = dict(patches=out[0], image=out[1])
        out = [None if t is None else dict(shape=list(t.shape), dtype=str(t.dtype)) for t in out]
    return dict(calls=[dict(entry=name, lib=flavour, args=[plain(a, resolve) for a in a_]) for name, flavour, a_ in rec.calls], returns=plain(out, resolve))


CLASSES = {"V": "ValueError", "H": "HipLibraryError"}


def digest(x):
    return hashlib.sha256(json.dumps(x, sort_keys=True).encode()).hexdigest()[:6]


def short(record):
    """What the golden file keeps of a record."""
    if "refused" in record:
        return record["refused"][0][0] + digest(record["refused"][1])
    return digest(record)


@pytest.fixture(scope="module")
def records():
    return {k: run_case(c) for k, c in all_cases().items()}


@pytest.fixture(scope="module")
def golden_records():
    with open(GOLDEN) as f:
        g = json.load(f)
    return dict(keys=g["keys"], records=g["records"].split())


def test_the_golden_file_is_small_and_names_these_cases(records, golden_records):
    smallest_npz = min(os.path.getsize(os.path.join(HERE, "golden", n)) for n in os.listdir(os.path.join(HERE, "golden")) if n.endswith(".npz"))
    assert os.path.getsize(GOLDEN) < smallest_npz
    assert golden_records["keys"] == digest(sorted(records)), "the case list has changed: regenerate the golden file from the REFERENCE commit (module docstring)"
    assert len(golden_records["records"]) == len(records)
    assert set(REWORDED) <= set(records)


def test_every_entry_both_forms_and_every_axis_are_covered(records):
    entries = {}
    for k, r in records.items():
        for call in r.get("calls", []):
            entries.setdefault(call["entry"], []).append(k)
    assert sorted(entries) == sorted(["rv_frames_to_patches", "rv_frames_to_patches_oriented", "rv_frames_to_patches_packed", "rv_frames_to_patches_scattered",
                                      "rv_yuv_to_patches", "rv_yuv_surface_to_patches", "rv_yuv_surface_to_patches_hdr", "rv_yuv_surface_to_patches_oriented",
                                      "rv_yuv_surfaces_to_patches", "rv_packed_to_patches", "rv_packed_surfaces_to_patches"])
    for fam in ("rgb", "y8", "ys", "pk"):                                                    # the four wrappers, tensor and list form, calls and refusals of each
        for form in ("/t/", "/l/"):
            mine = [r for k, r in records.items() if k.startswith(fam) and form in k]
            assert any("calls" in r for r in mine) and any("refused" in r for r in mine), (fam, form)
    launches = [r for r in records.values() if r.get("calls")]
    assert all(len(r["calls"]) == 1 for r in launches)
    assert any("copy" in json.dumps(r["calls"]) for r in launches)
    assert {r["calls"][0]["lib"] for r in launches} == {"torch.float16", "torch.bfloat16"}
    assert {r["refused"][0] for r in records.values() if "refused" in r} == set(CLASSES.values())


def test_the_records_are_the_reference_commits(records, golden_records):
    """Every case: the same entry with the same arguments, or the same refusal - class always, text unless the key is in REWORDED (then the text given there)."""
    wrong = []
    for i, k in enumerate(sorted(records)):
        want, r = golden_records["records"][i], records[k]
        if k in REWORDED:
            assert "refused" in r and want[0] in CLASSES, k
            if r["refused"] != [CLASSES[want[0]], REWORDED[k]]:
                wrong.append((k, "reworded refusal: expected " + repr([CLASSES[want[0]], REWORDED[k]]), r))
        elif short(r) != want:
            wrong.append((k, "expected " + want, r))
    assert not wrong, "%d case(s) differ from the reference commit (the module docstring says how to see the reference's records):\n" % len(wrong) + \
        "\n".join(f"{k}: {why}, got {short(r)}: {json.dumps(r, sort_keys=True)}" for k, why, r in wrong[:20])


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="write tests/golden/frontend_call_records.json from the checkout at --root (the reference commit)")
    ap.add_argument("--root", required=True)
    ap.add_argument("--full", help="also write the whole records to this file")
    a = ap.parse_args()
    if os.path.realpath(a.root) == os.path.realpath(os.path.dirname(HERE)):
        sys.exit("--root is the tree this module sits in: the golden file comes from the REFERENCE commit, never from the code under test")
    sys.path.insert(0, os.path.abspath(a.root))
    recs = {k: run_case(c) for k, c in all_cases().items()}
    with open(GOLDEN, "w") as f:
        json.dump(dict(keys=digest(sorted(recs)), records=" ".join(short(recs[k]) for k in sorted(recs))), f, separators=(",", ":"))
        f.write("\n")
    if a.full:
        with open(a.full, "w") as f:
            json.dump(recs, f, sort_keys=True, indent=1)
    print(f"{len(recs)} cases, {sum('refused' in r for r in recs.values())} refusals -> {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
