"""CLIP front end at 1080p: the fused rv_frames_to_patches call against the torch composition a user would otherwise write on the GPU.

60 uint8 NHWC frames of 1080 x 1920 -> R = 224, patch = 14 (one encode_video batch).  Both forms run in one process, alternating, each launch between
two device events: 5 warm-up + 20 timed launches per form.  Reported: median, min .. max, and the bytes of the source region the crop uses over the
fused call's median as a fraction of the 8 TB/s HBM figure.  Writes one JSON object to --out (default profiles/frontend_1080p.json) and prints it.

    python tools/frontend_prof.py [--frames 60] [--height 1080] [--width 1920] [--out FILE] [--once]   (--once: one fused launch, for a kernel trace)"""
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


def torch_composition(nhwc, R, patch, dt):
    """permute -> float -> antialiased bicubic resize -> centre crop -> normalise -> unfold -> pad -> operand type."""
    n, H, W, _ = nhwc.shape
    x = nhwc.permute(0, 3, 1, 2).float()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--res", type=int, default=224)
    ap.add_argument("--patch", type=int, default=14)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend_1080p.json"))
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "frontend_prof needs the GPU: a CPU run says nothing about time"
    dt = hip.op_dtype()
    n, H, W, R = a.frames, a.height, a.width, a.res
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    fused = lambda: ops.frames_to_patches(frames, R, a.patch, layout="NHWC", op_dtype=dt)[0]
    if a.once:
        fused()
        torch.cuda.synchronize()
        return
    comp = lambda: torch_composition(frames, R, a.patch, dt)
    t, first = {"fused": [], "torch": []}, {}
    for i in range(a.warmup + a.iters):
        for name, fn in (("fused", fused), ("torch", comp)):
            s, out = timed(fn)
            if i >= a.warmup:
                t[name].append(s)
            if i == 0:
                first[name] = out
    # source bytes the crop uses: the centred square (the shorter side) of every frame, 3 bytes a pixel
    used = n * min(H, W) ** 2 * 3
    med = {k: statistics.median(v) for k, v in t.items()}
    dist = float((first["fused"].float() - first["torch"].float()).abs().max())
    res = dict(device=torch.cuda.get_device_name(0), operand=hip.flavour(), frames=n, height=H, width=W, res=R, patch=a.patch, warmup=a.warmup, iters=a.iters,
               fused_ms=dict(median=med["fused"] * 1e3, min=min(t["fused"]) * 1e3, max=max(t["fused"]) * 1e3),
               torch_ms=dict(median=med["torch"] * 1e3, min=min(t["torch"]) * 1e3, max=max(t["torch"]) * 1e3),
               speedup=med["torch"] / med["fused"], used_source_bytes=used, fused_bytes_per_s=used / med["fused"],
               fused_fraction_of_8TBps=used / med["fused"] / HBM_PEAK, max_abs_diff_fused_vs_torch=dist)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
