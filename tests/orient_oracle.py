"""The float64 oracle of rv_frames_to_patches_oriented / rv_yuv_surface_to_patches_oriented (include/revision_hip.h: the front end on the picture as it is
displayed) and the inputs the orientation tests share.  NumPy throughout; nothing here touches the GPU or the library.

The definition, written out on its own: orient every plane with the three NumPy steps of the header (transpose, mirror x, mirror y), then do what the
un-oriented entry defines on that picture - one dense float64 resampling matrix per DISPLAY axis and plane, where a chroma axis carries the siting offset of
the CODED axis it came from, negated where the display axis is mirrored - then the colour equations and the normalisation.  ``rgb_oracle64`` is the RGB form.

Inputs: uniform integer noise over the whole code range with the suite's seed, as in the sibling front-end tests."""
import functools
import os

import numpy as np

SEED = 1234
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
IMAGE_BOUND = 2e-4           # the sibling front-end tests' image bound, in normalised units
SUB = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}
K_RB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
ORIENTS = tuple(range(8))
ROTATE_CODE = {0: 0, 90: 3, 180: 6, 270: 5}          # clockwise degrees -> code: what ops.orientation must give


def orient(S, code):
    """The header's three steps on the last two axes of ``S``."""
    D = S.swapaxes(-1, -2) if code & 1 else S
    D = D[..., ::-1] if code & 2 else D
    D = D[..., ::-1, :] if code & 4 else D
    return D


# ---- inputs (computed once, shared, never modified) ----
@functools.lru_cache(maxsize=None)
def rgb_values(n, H, W):
    """uint8 [n,3,H,W] noise."""
    out = np.random.RandomState(SEED + 1000 * H + W).randint(0, 256, (n, 3, H, W)).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def yuv_values(n, H, W, depth, sub):
    """Sample VALUES, uniform over [0, 2^depth): int64 y [n,H,W], cb and cr [n,H/sub_y,W/sub_x]."""
    sx, sy = SUB[sub]
    rng = np.random.RandomState(SEED + 1000 * H + W + 7 * depth)
    out = tuple(rng.randint(0, 1 << depth, s).astype(np.int64) for s in ((n, H, W), (n, H // sy, W // sx), (n, H // sy, W // sx)))
    for a in out:
        a.setflags(write=False)
    return out


# ---- the resampling of the un-oriented definition ----
def resized_size(H, W, R):
    return (R, int(R * W / H)) if H <= W else (int(R * H / W), R)


def cubic(x):
    x = np.abs(x)
    return np.where(x < 1.0, (1.5 * x - 2.5) * x * x + 1.0, np.where(x < 2.0, ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0, 0.0))


def axis_matrix(n_in, scale, div, off, first, R):
    """float64 [R, n_in]: row o holds the normalised weights of output index first + o of an axis of n_in samples, ``div`` times coarser than the frame and
    shifted by ``off`` samples (signed): centre = scale * (i + 0.5) / div + off, filter scale = scale / div."""
    m = np.zeros((R, n_in))
    fs = max(scale / div, 1.0)
    support = 2.0 * fs
    for o in range(R):
        centre = scale * (first + o + 0.5) / div + off
        lo, hi = max(0, int(centre - support + 0.5)), min(n_in, int(centre + support + 0.5))
        w = cubic((np.arange(lo, hi) - centre + 0.5) / fs)
        m[o, lo:hi] = w / w.sum()
    return m


def display_geometry(H, W, R, code):
    """(Hd, Wd, fy, fx, top, left) of the displayed picture: its size, in / out per axis, the crop offsets (round half even)."""
    Hd, Wd = (W, H) if code & 1 else (H, W)
    hr, wr = resized_size(Hd, Wd, R)
    return Hd, Wd, Hd / hr, Wd / wr, int(round((hr - R) / 2.0)), int(round((wr - R) / 2.0))


def normalise(rgb):
    out = (rgb / 255.0 - np.array(MEAN).reshape(1, 3, 1, 1)) / (np.array(STD).reshape(1, 3, 1, 1) + 1e-8)
    out.setflags(write=False)
    return out


# ---- RGB ----
@functools.lru_cache(maxsize=None)
def rgb_oracle64(n, H, W, R, code):
    """float64 [n,3,R,R]: rv_frames_to_patches' definition on the oriented channel planes of ``rgb_values(n, H, W)``."""
    D = orient(rgb_values(n, H, W).astype(np.float64), code)
    Hd, Wd, fy, fx, top, left = display_geometry(H, W, R, code)
    assert D.shape[2:] == (Hd, Wd)
    return normalise(axis_matrix(Hd, fy, 1.0, 0.0, top, R) @ D @ axis_matrix(Wd, fx, 1.0, 0.0, left, R).T)


# ---- YCbCr surfaces ----
def display_chroma(sub, loc, code, negate=True):
    """(sub_x, sub_y, off_x, off_y) of the DISPLAY axes: the subsampling pair swapped under transpose; the siting offset computed per CODED axis (0.25 where a
    subsampled axis is sited on the even luma sample: the horizontal axis for "left" and "topleft", the vertical one for "topleft"), carried to the display
    axis its axis becomes and negated where that display axis is mirrored.  ``negate=False`` is the WRONG definition the sensitivity test measures against."""
    sx, sy = SUB[sub]
    offx = 0.25 if sx == 2 and loc in ("left", "topleft") else 0.0
    offy = 0.25 if sy == 2 and loc == "topleft" else 0.0
    if code & 1:
        sx, sy, offx, offy = sy, sx, offy, offx
    if negate:
        offx, offy = (-offx if code & 2 else offx), (-offy if code & 4 else offy)
    return sx, sy, offx, offy


def yuv_rgb_of(planes, H, W, R, depth, sub, code, matrix="bt601", full_range=False, loc="left", negate=True):
    """float64 [n,3,R,R] on the 0 .. 255 scale: the values in front of the normalisation (and of the HDR steps) for the CODED sample values ``planes`` =
    (y [n,H,W], cb, cr [n,H/sub_y,W/sub_x])."""
    y, cb, cr = (orient(t.astype(np.float64), code) for t in planes)
    Hd, Wd, fy, fx, top, left = display_geometry(H, W, R, code)
    sx, sy, offx, offy = display_chroma(sub, loc, code, negate)
    assert y.shape[1:] == (Hd, Wd) and cb.shape[1:] == (Hd // sy, Wd // sx)
    my, mx = axis_matrix(Hd, fy, 1.0, 0.0, top, R), axis_matrix(Wd, fx, 1.0, 0.0, left, R)
    cy, cx = axis_matrix(Hd // sy, fy, float(sy), offy, top, R), axis_matrix(Wd // sx, fx, float(sx), offx, left, R)
    yr, cbr, crr = my @ y @ mx.T, cy @ cb @ cx.T, cy @ cr @ cx.T
    kr, kb = K_RB[matrix]
    kg = 1.0 - kr - kb
    s = 2.0 ** (depth - 8)
    if full_range:
        top_code = 2.0 ** depth - 1.0
        yl, b, r = yr * 255.0 / top_code, (cbr - 128.0 * s) * 255.0 / top_code, (crr - 128.0 * s) * 255.0 / top_code
    else:
        yl, b, r = (yr - 16.0 * s) * 255.0 / (219.0 * s), (cbr - 128.0 * s) * 255.0 / (224.0 * s), (crr - 128.0 * s) * 255.0 / (224.0 * s)
    return np.stack([yl + 2.0 * (1.0 - kr) * r, yl - (2.0 * kb * (1.0 - kb) / kg) * b - (2.0 * kr * (1.0 - kr) / kg) * r, yl + 2.0 * (1.0 - kb) * b], 1)


@functools.lru_cache(maxsize=None)
def yuv_rgb64(n, H, W, R, depth, sub, code, matrix="bt601", full_range=False, loc="left", negate=True):
    out = yuv_rgb_of(yuv_values(n, H, W, depth, sub), H, W, R, depth, sub, code, matrix, full_range, loc, negate)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def yuv_oracle64(n, H, W, R, depth, sub, code, matrix="bt601", full_range=False, loc="left", negate=True):
    """float64 [n,3,R,R]: the definition of rv_yuv_surface_to_patches_oriented's SDR image on ``yuv_values(n, H, W, depth, sub)``."""
    return normalise(yuv_rgb64(n, H, W, R, depth, sub, code, matrix, full_range, loc, negate))


@functools.lru_cache(maxsize=None)
def hdr_oracle64(n, H, W, R, depth, sub, code, transfer, gamut=1, peak=1000.0, white=203.0):
    """The HDR form: the oriented resampling and colour equations (BT.2020, studio range, top-left siting: the HDR tests' tags), then tests/hdr_oracle.py's
    steps 1 to 5 and the normalisation."""
    import hdr_oracle as ho
    return normalise(ho.hdr_steps64(yuv_rgb64(n, H, W, R, depth, sub, code, "bt2020", False, "topleft"), transfer, gamut, peak, white))


def log_err(who, what, value):
    """RV_LOG_ERR=<file>: measured maxima are appended there (profiles/frontend_orient_err.log is the place for one such run)."""
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            fh.write(f"{who} {what} {value:.3e}\n")
