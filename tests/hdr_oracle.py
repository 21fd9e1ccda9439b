"""The float64 oracle of rv_yuv_surface_to_patches_hdr (include/revision_hip.h: an HDR surface -> resampling -> YCbCr to R'G'B' -> PQ / HLG to display light ->
BT.2390 tone mapping -> BT.2020 to BT.709 primaries -> BT.709 OETF -> normalise), the inputs the HDR tests share, and a float32 transcription of the HDR steps
that says what f32 arithmetic alone costs.  NumPy throughout; nothing here touches the GPU or the library.

``sdr_rgb64`` restates the resampling and the colour equations of tests/test_gpu_yuv_surface_frontend.py's ``oracle64`` (one dense float64 matrix per plane and
axis, the depth-aware matrix) and stops in front of the normalisation; ``hdr_steps64`` is steps 1 to 5 of the header, ``normalise`` step 6.

Inputs.  ``kind`` "noise": uniform integer words over the whole of [0, 2^depth) with a fixed seed - resampled values leave the code range and colours leave the
RGB cube, so both clamps of the definition are exercised.  ``kind`` "ramp-pq" / "ramp-hlg": one smooth frame whose luma runs in raster order from code 0 to
the studio-range code of the display peak (PQinv(1000 nits), or E' = 1 for HLG), with slowly varying chroma around the mid code."""
import functools
import os

import numpy as np

SEED = 1234
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
SDR_IMAGE_BOUND = 2e-4       # tests/test_gpu_yuv_surface_frontend.py's IMAGE_BOUND
SUB = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}
KR, KB = 0.2627, 0.0593      # BT.2020 non-constant luminance: what an HDR10 / HLG stream is tagged with
TRANSFER_CODE = {"pq": 1, "hlg": 2}

#          H    W   R  patch n  (sample bytes, depth, value in the high bits, subsampling, interleaved CbCr)
GEOMS = [(2, 2, 14, 14, 2, (2, 10, False, "420", False)),        # yuv420p10le: the 1 x 1 chroma plane
         (30, 50, 28, 14, 2, (2, 10, True, "420", True)),        # P010: interleaved, value in the high bits, an odd tile split
         (96, 64, 28, 14, 2, (2, 12, False, "444", False)),      # 12-bit 4:4:4: a downscale with several taps
         (15, 17, 28, 14, 2, (2, 10, False, "444", False))]      # 10-bit 4:4:4: an upscale, odd sizes
GEOM_IDS = ["2x2-420p10", "30x50-p010", "96x64-444p12", "15x17-444p10"]
RAMP_GEOM = GEOMS[1]
LEVELS_GEOM = GEOMS[1]
LEVELS = [(peak, white) for peak in (400.0, 1000.0, 4000.0) for white in (100.0, 203.0)]


def model_cases():
    """Everything the GPU test compares with the oracle: (geometry, kind, transfer, gamut, peak_nits, sdr_white_nits)."""
    out = [(g, "noise", t, gm, 1000.0, 203.0) for g in GEOMS for t in ("pq", "hlg") for gm in (1, 0)]
    out += [(RAMP_GEOM, "ramp-" + t, t, 1, 1000.0, 203.0) for t in ("pq", "hlg")]
    out += [(LEVELS_GEOM, "noise", t, 1, peak, white) for t in ("pq", "hlg") for peak, white in LEVELS if (peak, white) != (1000.0, 203.0)]
    return out


# ---- the constants of the definition ----
M1, M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
C1, C2, C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
HLG_A = 0.17883277
HLG_B = 1.0 - 4.0 * HLG_A
HLG_C = 0.5 - HLG_A * np.log(4.0 * HLG_A)
TO709 = np.array([[1.6605, -0.5876, -0.0728], [-0.1246, 1.1329, -0.0083], [-0.0182, -0.1006, 1.1187]])     # BT.2087


def pq_eotf(e):
    """ST 2084 code value in [0, 1] -> nits (float64)."""
    p = np.power(e, 1.0 / M2)
    return 10000.0 * np.power(np.maximum(p - C1, 0.0) / (C2 - C3 * p), 1.0 / M1)


def pq_inv(nits):
    y = np.power(np.asarray(nits, dtype=np.float64) / 10000.0, M1)
    return np.power((C1 + C2 * y) / (1.0 + C3 * y), M2)


def hlg_scene(e):
    """HLG code value in [0, 1] -> scene light in [0, 1] (the inverse OETF of BT.2100)."""
    return np.where(e <= 0.5, e * e / 3.0, (np.exp((e - HLG_C) / HLG_A) + HLG_B) / 12.0)


def hdr_display_light(e, transfer, peak):
    """Steps 1 and 2: E'c [n,3,...] unclamped -> display light in nits."""
    e = np.clip(e, 0.0, 1.0)
    if transfer == "pq":
        return np.clip(pq_eotf(e), 0.0, peak)
    s = hlg_scene(e)
    ys = 0.2627 * s[:, 0:1] + 0.6780 * s[:, 1:2] + 0.0593 * s[:, 2:3]
    gamma = 1.2 + 0.42 * np.log10(peak / 1000.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ys > 0.0, peak * np.power(ys, gamma - 1.0), 0.0) * s


def eetf(e, max_lum):
    """BT.2390's EETF with black level 0 on e = PQinv(Y) / PQinv(Lw): the identity up to the knee KS = 1.5 maxLum - 0.5, a Hermite spline to maxLum above."""
    ks = 1.5 * max_lum - 0.5
    if ks >= 1.0:
        return e
    t = (e - ks) / (1.0 - ks)
    spline = (2 * t ** 3 - 3 * t ** 2 + 1) * ks + (t ** 3 - 2 * t ** 2 + t) * (1.0 - ks) + (-2 * t ** 3 + 3 * t ** 2) * max_lum
    return np.where(e <= ks, e, spline)


def tone_map(F, peak, white):
    """Step 3: display light [n,3,...] in nits -> linear light relative to SDR white, the ratio taken on the brightest channel."""
    mx = F.max(axis=1, keepdims=True)
    pq_lw = pq_inv(peak)
    max_lum = pq_inv(white) / pq_lw
    ks = 1.5 * max_lum - 0.5
    e = pq_inv(mx) / pq_lw
    with np.errstate(divide="ignore", invalid="ignore"):
        mapped = pq_eotf(eetf(e, max_lum) * pq_lw) / mx
    ratio = np.where((ks >= 1.0) | (e <= ks) | (mx == 0.0), 1.0, mapped)
    return F * ratio / white


def oetf709(L):
    return np.where(L < 0.018, 4.5 * L, 1.099 * np.power(L, 0.45) - 0.099)


def hdr_steps64(v, transfer, gamut, peak, white):
    """Steps 1 to 5 in float64: v [n,3,R,R] on the 0 .. 255 scale (the R'G'B' of the colour equations, unclamped) -> the BT.709-coded SDR values, same scale."""
    L = tone_map(hdr_display_light(v / 255.0, transfer, peak), peak, white)
    if gamut:
        L = np.einsum("ck,nkyx->ncyx", TO709, L)
    return 255.0 * oetf709(np.clip(L, 0.0, 1.0))


def hdr_steps32(v, transfer, gamut, peak, white):
    """The same steps as the kernel does them, in float32 NumPy: powers as exp2(k * log2(x)), every operation in the kernel's order, the scalars that depend on
    peak / white computed in float64 and rounded once.  v: float32 [n,3,R,R]."""
    f = np.float32
    rm1, rm2, m1, m2, c1, c2, c3 = f(1.0 / M1), f(1.0 / M2), f(M1), f(M2), f(C1), f(C2), f(C3)
    max_lum64 = float(pq_inv(white) / pq_inv(peak))
    lw, rlt, pq_lw, max_lum, ks, gm1 = f(peak), f(1.0 / white), f(pq_inv(peak)), f(max_lum64), f(1.5 * max_lum64 - 0.5), f(0.2 + 0.42 * np.log10(peak / 1000.0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pw = lambda x, k: np.exp2(k * np.log2(x))

        def eotf(e):
            p = pw(e, rm2)
            return f(10000.0) * pw(np.maximum(p - c1, f(0)) / (c2 - c3 * p), rm1)

        def inv(nits):
            y = pw(nits / f(10000.0), m1)
            return pw((c1 + c2 * y) / (f(1) + c3 * y), m2)

        assert v.dtype == np.float32
        F = np.minimum(np.maximum(v / f(255), f(0)), f(1))
        if transfer == "pq":
            F = np.minimum(np.maximum(eotf(F), f(0)), lw)
        else:
            F = np.where(F <= f(0.5), F * F / f(3), (np.exp2((F - f(HLG_C)) * f(1.4426950408889634 / HLG_A)) + f(HLG_B)) / f(12))
            ys = f(0.2627) * F[:, 0:1] + f(0.6780) * F[:, 1:2] + f(0.0593) * F[:, 2:3]
            F = np.where(ys > f(0), lw * pw(ys, gm1), f(0)) * F
        mx = np.maximum(F[:, 0:1], np.maximum(F[:, 1:2], F[:, 2:3]))
        e = inv(mx) / pq_lw
        omk = f(1) - ks
        t = (e - ks) / omk
        t2 = t * t
        t3 = t2 * t
        e2 = (f(2) * t3 - f(3) * t2 + f(1)) * ks + (t3 - f(2) * t2 + t) * omk + (f(-2) * t3 + f(3) * t2) * max_lum
        ratio = np.where((ks < f(1)) & (mx > f(0)) & (e > ks), eotf(e2 * pq_lw) / mx, f(1))
        L = F * ratio * rlt
        g = (TO709 if gamut else np.eye(3)).astype(f)
        L = np.stack([g[c, 0] * L[:, 0] + g[c, 1] * L[:, 1] + g[c, 2] * L[:, 2] for c in range(3)], 1)
        L = np.minimum(np.maximum(L, f(0)), f(1))
        out = f(255) * np.where(L < f(0.018), f(4.5) * L, f(1.099) * pw(L, f(0.45)) - f(0.099))
    assert out.dtype == np.float32
    return out


# ---- inputs ----
def studio_code(e, depth):
    """The studio-range luma code of E' at a depth."""
    return (16.0 + 219.0 * e) * 2.0 ** (depth - 8)


@functools.lru_cache(maxsize=None)
def values(n, H, W, depth, sub, kind="noise"):
    """Sample VALUES as int64 NumPy arrays: y [n,H,W], cb and cr [n,H/sub_y,W/sub_x].  Never modified."""
    sx, sy = SUB[sub]
    shapes = ((n, H, W), (n, H // sy, W // sx), (n, H // sy, W // sx))
    if kind == "noise":
        rng = np.random.RandomState(SEED + 1000 * H + W + 7 * depth)
        out = tuple(rng.randint(0, 1 << depth, s).astype(np.int64) for s in shapes)
    else:
        top = studio_code(float(pq_inv(1000.0)) if kind == "ramp-pq" else 1.0, depth)
        y = np.rint(top * np.arange(H * W) / (H * W - 1.0)).astype(np.int64).reshape(1, H, W).repeat(n, 0)
        y[1:] = y[1:, ::-1, ::-1]                                                        # the second frame runs the other way
        h, w = shapes[1][1:]
        mid, amp = 128 << (depth - 8), 24 << (depth - 8)
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        cb = np.rint(mid + amp * np.sin(2 * np.pi * xx / max(w, 2))).astype(np.int64)[None].repeat(n, 0)
        cr = np.rint(mid + amp * np.cos(2 * np.pi * yy / max(h, 2))).astype(np.int64)[None].repeat(n, 0)
        out = (y, cb, cr)
    for a in out:
        a.setflags(write=False)
    return out


def resized_size(H, W, R):
    return (R, int(R * W / H)) if H <= W else (int(R * H / W), R)


def cubic(x):
    x = np.abs(x)
    return np.where(x < 1.0, (1.5 * x - 2.5) * x * x + 1.0, np.where(x < 2.0, ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0, 0.0))


def axis_matrix(n_in, scale, div, off, first, R):
    """float64 [R, n_in]: row o holds the normalised weights of output index first + o of an axis of n_in samples, ``div`` times coarser than the frame and
    shifted by ``off`` samples: centre = scale * (i + 0.5) / div + off, filter scale = scale / div (the header's definition; div = 1, off = 0 is luma)."""
    m = np.zeros((R, n_in))
    fs = max(scale / div, 1.0)
    support = 2.0 * fs
    for o in range(R):
        centre = scale * (first + o + 0.5) / div + off
        lo, hi = max(0, int(centre - support + 0.5)), min(n_in, int(centre + support + 0.5))
        w = cubic((np.arange(lo, hi) - centre + 0.5) / fs)
        m[o, lo:hi] = w / w.sum()
    return m


def sdr_rgb_of(planes, H, W, R, depth, sub):
    """float64 [n,3,R,R] on the 0 .. 255 scale: rv_yuv_surface_to_patches' values in front of its normalisation, for BT.2020, studio range, top-left siting, on
    the sample values ``planes`` = (y [n,H,W], cb, cr [n,H/sub_y,W/sub_x])."""
    sx, sy = SUB[sub]
    hr, wr = resized_size(H, W, R)
    top, left = int(round((hr - R) / 2.0)), int(round((wr - R) / 2.0))
    fy, fx = H / hr, W / wr
    y, cb, cr = (t.astype(np.float64) for t in planes)
    offx, offy = (0.25 if sx == 2 else 0.0), (0.25 if sy == 2 else 0.0)                  # top-left: both subsampled axes sit on the even luma sample
    my, mx = axis_matrix(H, fy, 1.0, 0.0, top, R), axis_matrix(W, fx, 1.0, 0.0, left, R)
    cy, cx = axis_matrix(H // sy, fy, float(sy), offy, top, R), axis_matrix(W // sx, fx, float(sx), offx, left, R)
    yr, cbr, crr = my @ y @ mx.T, cy @ cb @ cx.T, cy @ cr @ cx.T
    kg = 1.0 - KR - KB
    s = 2.0 ** (depth - 8)
    yl, b, r = (yr - 16.0 * s) * 255.0 / (219.0 * s), (cbr - 128.0 * s) * 255.0 / (224.0 * s), (crr - 128.0 * s) * 255.0 / (224.0 * s)
    return np.stack([yl + 2.0 * (1.0 - KR) * r, yl - (2.0 * KB * (1.0 - KB) / kg) * b - (2.0 * KR * (1.0 - KR) / kg) * r, yl + 2.0 * (1.0 - KB) * b], 1)


@functools.lru_cache(maxsize=None)
def sdr_rgb64(n, H, W, R, depth, sub, kind="noise"):
    """``sdr_rgb_of`` on ``values(n, H, W, depth, sub, kind)``; never modified."""
    out = sdr_rgb_of(values(n, H, W, depth, sub, kind), H, W, R, depth, sub)
    out.setflags(write=False)
    return out


def normalise(rgb):
    out = (rgb / 255.0 - np.array(MEAN).reshape(1, 3, 1, 1)) / (np.array(STD).reshape(1, 3, 1, 1) + 1e-8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle64(n, H, W, R, depth, sub, kind, transfer, gamut, peak=1000.0, white=203.0):
    """float64 [n,3,R,R]: the definition of rv_yuv_surface_to_patches_hdr's image on ``values(n, H, W, depth, sub, kind)``."""
    return normalise(hdr_steps64(sdr_rgb64(n, H, W, R, depth, sub, kind), transfer, gamut, peak, white))


def case_oracle(case):
    (H, W, R, _, n, fmt), kind, transfer, gamut, peak, white = case
    return oracle64(n, H, W, R, fmt[1], fmt[3], kind, transfer, gamut, peak, white)


@functools.lru_cache(maxsize=None)
def f32_model():
    """The worst normalised-image distance, over ``model_cases()``, between the float32 transcription of steps 1 to 6 (fed the float64 R'G'B' rounded once to
    float32) and the float64 oracle: what f32 arithmetic in the HDR steps costs by itself."""
    worst = 0.0
    f = np.float32
    for case in model_cases():
        (H, W, R, _, n, fmt), kind, transfer, gamut, peak, white = case
        v = hdr_steps32(sdr_rgb64(n, H, W, R, fmt[1], fmt[3], kind).astype(f), transfer, gamut, peak, white)
        img = (v / f(255) - np.array(MEAN, dtype=f).reshape(1, 3, 1, 1)) / (np.array(STD, dtype=f).reshape(1, 3, 1, 1) + f(1e-8))
        worst = max(worst, float(np.abs(img.astype(np.float64) - case_oracle(case)).max()))
    return worst


def image_bound():
    """The SDR front end's bound where f32 arithmetic in the HDR steps stays below a quarter of it; otherwise four times what that arithmetic costs (the factor
    covers the few-ulp differences between the device's exp2 / log2 and NumPy's, amplified by the PQ slope)."""
    m = f32_model()
    return SDR_IMAGE_BOUND if m < SDR_IMAGE_BOUND / 4.0 else 4.0 * m


def log_err(who, what, value):
    """RV_LOG_ERR=<file>: measured maxima are appended there (profiles/hdr_frontend_err.log is the place for one such run)."""
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            fh.write(f"{who} {what} {value:.3e}\n")
