"""The host side of the HDR front end (rv_yuv_surface_to_patches_hdr), without a GPU: the symbol in the header, the ctypes table and both libraries; every
refusal through ctypes (validation runs before any launch, so nothing here needs a device); the argument handling of ops.yuv_surface_to_patches / ops.hdr_map,
yuv_surface_colour_defaults and ClipFeatureExtractor.encode_video_pix_fmt; the definition itself, pinned on constant frames through the float64 oracle of
tests/hdr_oracle.py; and, last, what float32 arithmetic in the HDR steps costs against that oracle on the inputs of tests/test_gpu_hdr_frontend.py - the
figure that test's image bound is derived from (RV_LOG_ERR=<file> appends it as ``f32_model``; profiles/hdr_frontend_err.log holds one such run)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import hdr_oracle as ho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "rv_yuv_surface_to_patches_hdr"
FLAVOURS = ("f16", "bf16")


def lib_error(flavour):
    from revisionllm_amd import hip
    buf = ctypes.create_string_buffer(512)
    hip.lib(flavour).rv_last_error(buf, 512)
    return buf.value.decode()


def raw_call(flavour, surface=None, hdr=None, args=None, null_surface=False, null_map=False):
    """The entry through ctypes on a 96 x 64 yuv420p10le surface whose plane pointers are never read (every call here is refused, or has n = 0).
    ``surface`` / ``hdr`` / ``args``: fields and arguments to override."""
    from revisionllm_amd import hip
    H, W = 96, 64
    s = dict(y=0x10000, cb=0x20000, cr=0x30000, y_frame_stride=H * W * 2, y_row_stride=W * 2, c_frame_stride=H * W // 2, c_row_stride=W, sample_bytes=2,
             depth=10, msb_aligned=0, c_pix=2, sub_x=2, sub_y=2, n=2, H=H, W=W, matrix=2, full_range=0, chroma_loc=2)
    s.update(surface or {})
    m = dict(transfer=1, gamut=1, peak_nits=1000.0, sdr_white_nits=203.0)
    m.update(hdr or {})
    a = dict(R=28, patch=14, ldp=640, patches=0x40000, image=0x50000)
    a.update(args or {})
    f3 = ctypes.c_float * 3
    return hip.lib(flavour).rv_yuv_surface_to_patches_hdr(None if null_surface else ctypes.byref(hip.RvYuvSurface(**s)),
                                                          None if null_map else ctypes.byref(hip.RvHdrMap(**m)), a["R"], a["patch"], f3(*ho.MEAN), f3(*ho.STD),
                                                          a["patches"], a["ldp"], a["image"], None)


def test_header_ctypes_table_and_both_libraries_carry_the_symbol():
    from revisionllm_amd import hip
    header = open(os.path.join(ROOT, "include", "revision_hip.h")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(const rv_yuv_surface\* s, const rv_hdr_map\* m,", header)
    assert re.search(r"typedef struct rv_hdr_map \{\s*int32_t transfer;[^}]*int32_t gamut;[^}]*float peak_nits;[^}]*float sdr_white_nits;[^}]*\} rv_hdr_map;", header)
    assert "#define RV_ABI_VERSION 5" in header
    # the header no longer leaves HDR values "as coded" without saying how to convert them
    assert "reach CLIP as coded" in header and "rv_yuv_surface_to_patches_hdr (below)" in header
    assert "No dynamic metadata is read" in header and "peak_nits is the caller's number" in header
    res, args = hip.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 10 and args[1]._type_ is hip.RvHdrMap and args[0]._type_ is hip.RvYuvSurface
    assert [f for f, _ in hip.RvHdrMap._fields_] == ["transfer", "gamut", "peak_nits", "sdr_white_nits"] and ctypes.sizeof(hip.RvHdrMap) == 16
    assert "rv_*" in open(os.path.join(ROOT, "revisionllm_amd", "csrc", "exports.map")).read()
    for flavour in FLAVOURS:
        assert hasattr(hip.lib(flavour), NAME), flavour
        assert hip.lib(flavour).rv_abi_version() == 5


MAP_REFUSALS = [("transfer 0", dict(transfer=0), "transfer"),
                ("transfer 3", dict(transfer=3), "transfer"),
                ("transfer -1", dict(transfer=-1), "transfer"),
                ("gamut 2", dict(gamut=2), "gamut"),
                ("gamut -1", dict(gamut=-1), "gamut"),
                ("peak NaN", dict(peak_nits=float("nan")), "peak_nits"),
                ("peak inf", dict(peak_nits=float("inf")), "peak_nits"),
                ("peak 0.5", dict(peak_nits=0.5), "peak_nits"),
                ("peak 0", dict(peak_nits=0.0), "peak_nits"),
                ("peak -100", dict(peak_nits=-100.0), "peak_nits"),
                ("peak 10001", dict(peak_nits=10001.0), "peak_nits"),
                ("white NaN", dict(sdr_white_nits=float("nan")), "sdr_white_nits"),
                ("white -inf", dict(sdr_white_nits=float("-inf")), "sdr_white_nits"),
                ("white 0.99", dict(sdr_white_nits=0.99), "sdr_white_nits"),
                ("white 20000", dict(sdr_white_nits=20000.0), "sdr_white_nits")]


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("what,hdr,msg", MAP_REFUSALS, ids=[r[0] for r in MAP_REFUSALS])
def test_the_map_is_validated(flavour, what, hdr, msg):
    assert raw_call(flavour, hdr=hdr) < 0
    assert lib_error(flavour).startswith(NAME + ":") and msg in lib_error(flavour), lib_error(flavour)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_null_struct_null_map_and_the_edges_of_the_ranges(flavour):
    assert raw_call(flavour, null_map=True) < 0
    assert lib_error(flavour) == NAME + ": null map"
    assert raw_call(flavour, null_surface=True) < 0
    assert lib_error(flavour) == NAME + ": null surface"
    # a bad map is refused even when there is nothing to do; a good one with n = 0 returns 0 and launches nothing (1 and 10000 are inside the range)
    assert raw_call(flavour, surface=dict(n=0), hdr=dict(transfer=5)) < 0
    for hdr in (dict(), dict(transfer=2, gamut=0), dict(peak_nits=1.0, sdr_white_nits=10000.0), dict(peak_nits=10000.0, sdr_white_nits=1.0)):
        assert raw_call(flavour, surface=dict(n=0, y=None, cb=None, cr=None), hdr=hdr) == 0


#                    what                         surface fields              arguments            message
SURFACE_REFUSALS = [("null y", dict(y=None), {}, "null plane"),
                    ("null cr", dict(cr=None), {}, "null plane"),
                    ("sample_bytes 3", dict(sample_bytes=3), {}, "sample_bytes"),
                    ("depth 17", dict(depth=17), {}, "depth"),
                    ("depth 10 in bytes", dict(sample_bytes=1, c_pix=1), {}, "depth"),
                    ("msb_aligned 2", dict(msb_aligned=2), {}, "msb_aligned"),
                    ("sub 1,2", dict(sub_x=1, sub_y=2), {}, "sub_x"),
                    ("odd H at 4:2:0", dict(H=95), {}, "odd"),
                    ("W = 1 at 4:2:0", dict(W=1), {}, "frame size"),
                    ("W = 8194", dict(W=8194), {}, "frame size"),
                    ("c_pix 3", dict(c_pix=3), {}, "c_pix"),
                    ("c_pix 4 on separate planes", dict(c_pix=4), {}, "interleaved"),
                    ("odd y pointer", dict(y=0x10001), {}, "aligned"),
                    ("odd c row stride", dict(c_row_stride=65), {}, "aligned"),
                    ("matrix 3", dict(matrix=3), {}, "matrix"),
                    ("full_range 2", dict(full_range=2), {}, "full_range"),
                    ("chroma_loc 3", dict(chroma_loc=3), {}, "chroma_loc"),
                    ("n = -1", dict(n=-1), {}, "n = -1"),
                    ("R not a multiple of patch", {}, dict(R=30), "multiple"),
                    ("R above 8192", {}, dict(R=8194, patch=2), "R = 8194"),
                    ("ldp < Kp", {}, dict(ldp=639), "ldp"),
                    ("both outputs null", {}, dict(patches=None, image=None), "both outputs null"),
                    ("taps beyond the LDS budget", dict(H=8192, W=8192), dict(R=1, patch=1), "LDS"),
                    ("more workgroups than a launch", dict(n=2 ** 30), {}, "workgroups")]


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("what,surface,args,msg", SURFACE_REFUSALS, ids=[r[0] for r in SURFACE_REFUSALS])
def test_everything_the_surface_entry_refuses_is_refused_under_the_new_name(flavour, what, surface, args, msg):
    for transfer in (1, 2):
        assert raw_call(flavour, surface=surface, args=args, hdr=dict(transfer=transfer)) < 0
        assert lib_error(flavour).startswith(NAME + ":") and msg in lib_error(flavour), lib_error(flavour)


def test_ops_argument_handling():
    from revisionllm_amd import hip, ops
    assert ops.hdr_map(None) is None and ops.hdr_map(None, "bt2020", True, 5.0, 7.0) is None
    fields = lambda m: (m.transfer, m.gamut, m.peak_nits, m.sdr_white_nits)
    for names, code in ((("pq", "smpte2084"), 1), (("hlg", "arib-std-b67"), 2)):
        for name in names:
            m = ops.hdr_map(name)
            assert isinstance(m, hip.RvHdrMap) and fields(m) == (code, 1, 1000.0, 203.0)
    # gamut follows the matrix unless it is given
    assert [ops.hdr_map("pq", mx).gamut for mx in ("bt2020", "bt709", "bt601")] == [1, 0, 0]
    assert ops.hdr_map("hlg", "bt2020", gamut=False).gamut == 0 and ops.hdr_map("hlg", "bt709", gamut=True).gamut == 1
    assert fields(ops.hdr_map("pq", "bt2020", None, 4000, 100)) == (1, 1, 4000.0, 100.0)
    for bad in ("PQ", "bt2020", "linear", "smpte428", 1, ""):
        with pytest.raises(ValueError, match="transfer"):
            ops.hdr_map(bad)
    planes, kw = ops.split_yuv(torch.zeros(2, ops.yuv_frame_bytes(6, 8, "p010le"), dtype=torch.uint8), 6, 8, "p010le")
    with pytest.raises(ValueError, match="transfer"):                                   # the name is checked before anything else
        ops.yuv_surface_to_patches(*planes, R=28, patch=14, matrix="bt2020", transfer="gamma22", **kw)
    with pytest.raises(hip.HipLibraryError, match="CPU"):                               # ... and a good one goes on to the device check: there is no CPU path
        ops.yuv_surface_to_patches(*planes, R=28, patch=14, matrix="bt2020", transfer="pq", peak_nits=600.0, sdr_white_nits=100.0, gamut=False, **kw)


class _Towers:
    """Stands in for ClipTowers: records what encode_video_pix_fmt hands to encode_surfaces_yuv."""
    device, cfg = "cpu", dict(embed_dim=4)

    def __init__(self):
        self.calls = []

    def encode_surfaces_yuv(self, y, cb, cr=None, **surface):
        self.calls.append((len(y), surface))
        return torch.zeros(len(y), 4)


def test_colour_defaults_and_pass_through_of_the_extractor():
    from revisionllm_amd import ops
    from revisionllm_amd.data.clip_extractor import ClipFeatureExtractor, yuv_colour_defaults, yuv_surface_colour_defaults
    bt2020 = dict(matrix="bt2020", full_range=False, chroma_loc="topleft")
    assert yuv_surface_colour_defaults(1080) == yuv_surface_colour_defaults(1080, transfer=None) == yuv_colour_defaults(1080)
    assert yuv_surface_colour_defaults(2160, bt2020=True, transfer=None) == bt2020
    for name in ("pq", "hlg", "smpte2084", "arib-std-b67"):
        assert yuv_surface_colour_defaults(480, transfer=name) == yuv_surface_colour_defaults(2160, bt2020=True, transfer=name) == dict(bt2020, transfer=name)
    fb = ops.yuv_frame_bytes(6, 8, "p010le")
    buf = torch.zeros(3, fb, dtype=torch.uint8)
    p010 = dict(depth=10, msb_aligned=True, subsampling="420")
    tw = _Towers()
    ex = ClipFeatureExtractor(tw)
    ex.encode_video_pix_fmt(buf, 6, 8, "p010le", transfer="pq")
    ex.encode_video_pix_fmt(buf, 6, 8, "p010le", transfer="arib-std-b67", peak_nits=600.0, sdr_white_nits=100.0, gamut=False, chroma_loc="left")
    ex.encode_video_pix_fmt(buf, 6, 8, "p010le", transfer="hlg", matrix="bt709")
    ex.encode_video_pix_fmt(buf, 6, 8, "p010le", transfer=None)
    ex.encode_video_pix_fmt(buf, 6, 8, "p010le")
    sdr = dict(p010, matrix="bt601", full_range=False, chroma_loc="left")
    assert tw.calls == [(3, dict(p010, **bt2020, transfer="pq")),
                        (3, dict(p010, matrix="bt2020", full_range=False, chroma_loc="left", transfer="arib-std-b67", peak_nits=600.0, sdr_white_nits=100.0, gamut=False)),
                        (3, dict(p010, matrix="bt709", full_range=False, chroma_loc="topleft", transfer="hlg")),
                        (3, sdr), (3, sdr)]                                               # transfer=None is the call it always was
    with pytest.raises(ValueError, match="transfer"):
        ex.encode_video_pix_fmt(buf, 6, 8, "p010le", transfer="bt709")
    assert len(tw.calls) == 5


# ---- the definition, pinned on constant frames ----
def constant(code_y, depth=10, n=1, R=4):
    """The R'G'B' (0 .. 255 scale, float64 [n,3,R,R]) of a neutral constant frame whose studio-range luma code is ``code_y``: what the resampling (normalised
    weights) and the colour equations give for it."""
    return np.full((n, 3, R, R), (code_y / 2.0 ** (depth - 8) - 16.0) * 255.0 / 219.0)


def neutral(e):
    return np.full((1, 3, 2, 2), 255.0 * e)


def test_oracle_resampling_of_a_constant_frame_is_the_constant():
    """The oracle's front half on a frame of one luma code and mid chroma is that grey in every pixel: the weights are normalised, the matrix leaves grey alone."""
    for H, W, R, _, n, fmt in ho.GEOMS:
        sx, sy = ho.SUB[fmt[3]]
        s = 1 << (fmt[1] - 8)
        planes = (np.full((n, H, W), 125 * s), np.full((n, H // sy, W // sx), 128 * s), np.full((n, H // sy, W // sx), 128 * s))
        assert np.abs(ho.sdr_rgb_of(planes, H, W, R, fmt[1], fmt[3]) - constant(125 * s, depth=fmt[1], R=R, n=n)).max() < 1e-9


def test_pq_grey_at_50_nits_is_the_bt709_code_of_50_over_203():
    e = float(ho.pq_inv(50.0))
    want = float(ho.oetf709(np.array(50.0 / 203.0)))
    assert abs(want - (1.099 * (50.0 / 203.0) ** 0.45 - 0.099)) < 1e-15
    got = ho.hdr_steps64(neutral(e), "pq", 0, 1000.0, 203.0) / 255.0
    assert np.abs(got - want).max() < 1e-12
    # with the gamut matrix a neutral colour moves only by the matrix's row sums (1.0001, 1.0000, 0.9999: BT.2087 gives four decimals)
    got = ho.hdr_steps64(neutral(e), "pq", 1, 1000.0, 203.0)[0, :, 0, 0] / 255.0
    assert np.abs(got - ho.oetf709(ho.TO709.sum(1) * 50.0 / 203.0)).max() < 1e-12 and np.abs(got - want).max() < 1e-4
    # ... and through the studio-range code: 10-bit code 64 + 876 E'
    v = constant(64.0 + 876.0 * e)
    assert np.abs(ho.hdr_steps64(v, "pq", 0, 1000.0, 203.0) / 255.0 - want).max() < 1e-12


@pytest.mark.parametrize("peak,white", [(1000.0, 203.0), (400.0, 100.0), (4000.0, 203.0), (10000.0, 100.0)])
def test_the_code_of_peak_nits_gives_sdr_white(peak, white):
    for transfer, e in (("pq", float(ho.pq_inv(peak))), ("hlg", 1.0)):
        got = ho.hdr_steps64(neutral(e), transfer, 0, peak, white) / 255.0
        assert np.abs(got - 1.0).max() < 1e-9, (transfer, got)
        got = ho.hdr_steps64(neutral(min(1.0, e * 1.05)), transfer, 0, peak, white) / 255.0      # above the peak: clamped to it
        assert np.abs(got - 1.0).max() < 1e-9


def test_a_peak_at_or_below_sdr_white_maps_no_tones():
    e = np.linspace(0.0, 1.0, 1025).reshape(1, 1, 1, -1).repeat(3, 1) * np.array([1.0, 0.8, 0.6]).reshape(1, 3, 1, 1)
    for transfer in ("pq", "hlg"):
        for peak, white in ((203.0, 203.0), (100.0, 203.0), (300.0, 1000.0)):
            F = ho.hdr_display_light(e, transfer, peak)
            assert np.array_equal(ho.tone_map(F, peak, white), F / white)
            assert np.array_equal(ho.hdr_steps64(255.0 * e, transfer, 0, peak, white), 255.0 * ho.oetf709(np.clip(F / white, 0.0, 1.0)))
    F = ho.hdr_display_light(e, "pq", 1000.0)
    assert np.abs(ho.tone_map(F, 1000.0, 203.0) - F / 203.0).max() > 1.0            # ... and a peak above it does


@pytest.mark.parametrize("peak,white", [(1000.0, 203.0), (400.0, 203.0), (4000.0, 100.0), (10000.0, 100.0)])
def test_the_eetf_is_continuous_at_the_knee_and_monotone(peak, white):
    max_lum = float(ho.pq_inv(white) / ho.pq_inv(peak))
    ks = 1.5 * max_lum - 0.5
    assert 0.0 < ks < 1.0
    eps = 1e-9
    assert abs(float(ho.eetf(np.array(ks + eps), max_lum)) - ks) < 2 * eps and float(ho.eetf(np.array(ks), max_lum)) == ks
    ramp = np.linspace(0.0, 1.0, 4096)
    out = ho.eetf(ramp, max_lum)
    assert np.all(np.diff(out) >= 0.0) and np.all(np.diff(out)[:-1] > 0.0) and out[0] == 0.0 and abs(out[-1] - max_lum) < 1e-15
    assert np.all(out <= ramp + 1e-15)
    # the whole step 3 on a neutral ramp of display light: continuous at the knee, monotone, never above the input, SDR white at the peak
    F = (peak * ramp).reshape(1, 1, 1, -1).repeat(3, 1)
    L = ho.tone_map(F, peak, white)[0, 0, 0]
    assert np.all(np.diff(L) >= 0.0) and abs(L[-1] - 1.0) < 1e-12 and np.all(L <= F[0, 0, 0] / white + 1e-12)
    knee = float(ho.pq_eotf(np.array(ks * float(ho.pq_inv(peak)))))
    below, above = (ho.tone_map(np.full((1, 3, 1, 1), knee * (1.0 + s * 1e-9)), peak, white)[0, 0, 0, 0] for s in (-1.0, 1.0))
    assert abs(above - below) < 1e-8 * knee / white


def test_hlg_reference_white_is_about_203_nits_on_a_1000_nit_display():
    F = ho.hdr_display_light(np.full((1, 3, 1, 1), 0.75), "hlg", 1000.0)
    assert np.all(F == F[0, 0]) and abs(float(F[0, 0, 0, 0]) / 203.0 - 1.0) < 0.01       # BT.2408's reference white
    assert abs(float(ho.hdr_display_light(np.ones((1, 3, 1, 1)), "hlg", 1000.0)[0, 0, 0, 0]) - 1000.0) < 1e-3
    assert np.all(ho.hdr_display_light(np.zeros((1, 3, 1, 1)), "hlg", 1000.0) == 0.0)     # Ys = 0 -> 0, not NaN
    # the two branches of the inverse OETF meet at E' = 0.5 (scene light 1 / 12)
    assert abs(float(ho.hlg_scene(np.array(0.5))) - 1.0 / 12.0) < 1e-15 and abs(float(ho.hlg_scene(np.array(0.5 + 1e-12))) - 1.0 / 12.0) < 1e-11


def test_f32_error_budget():
    """What float32 arithmetic in steps 1 to 6 costs: the float32 transcription of the kernel's HDR steps (hdr_oracle.hdr_steps32: exp2 / log2 powers, the
    kernel's order of operations) against the float64 oracle, on every input the GPU test compares - its worst normalised-image distance is ``f32_model``.
    The GPU test's image bound follows from it (hdr_oracle.image_bound): the SDR front end's 2e-4 if f32_model is below a quarter of that, else 4 x f32_model.
    Measured here: 2.7e-4 (PQ near the top of the range: c2 - c3 p cancels to ~0.2 and the 1 / m1 = 6.3 power and the gamut matrix amplify what is left), so the
    bound is about 1.1e-3 - a quarter of an 8-bit code step after the normalisation's 1 / std.  Sanity limits only: the figure is a measurement of NumPy's
    float32, not of the code under test."""
    m = ho.f32_model()
    ho.log_err("test_hdr_host_logic.py", "f32_model", m)
    ho.log_err("test_hdr_host_logic.py", "image_bound", ho.image_bound())
    assert math.isfinite(m) and 1e-7 < m < 1e-3, m                                       # float32 was really used, and it did not fall apart
    assert ho.image_bound() == (ho.SDR_IMAGE_BOUND if m < ho.SDR_IMAGE_BOUND / 4 else 4 * m)
    assert len(ho.model_cases()) == 16 + 2 + 10
