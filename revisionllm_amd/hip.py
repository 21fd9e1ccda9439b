"""ctypes binding of librevision_hip.so (the C ABI declared in include/revision_hip.h).

There is NO CPU fallback: if the library is missing or fails to load, every compute entry point
raises.  torch is used only as the owner of device memory and streams; the library sees raw device
pointers and a ``hipStream_t``.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# The library exists in two operand FLAVOURS with one ABI (include/revision_hip.h "dtypes"): fp16 operands (the default: the checkpoints'
# own storage type, 11 significand bits) and bf16 operands (the reference's GPU dtype).  An Engine is built for one flavour and calls that
# library; the functional wrappers in ops.py pick the library from the dtype of the 16-bit tensors they are handed.
# REVISION_HIP_LIB / REVISION_HIP_LIB_BF16: load another build of the same ABI (A/B kernel measurements); default: the in-tree libraries.
LIB_PATHS = {"f16": os.environ.get("REVISION_HIP_LIB") or os.path.join(_HERE, "librevision_hip.so"),
             "bf16": os.environ.get("REVISION_HIP_LIB_BF16") or os.path.join(_HERE, "librevision_hip_bf16.so")}
LIB_PATH = LIB_PATHS["f16"]
OP_DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}

RV_F32, RV_BF16, RV_I32, RV_I64, RV_U8, RV_F16 = 0, 1, 2, 3, 4, 5
RV_ACT_NONE, RV_ACT_RELU, RV_ACT_SILU_MUL, RV_ACT_QUICK_GELU = 0, 1, 2, 3
RV_FEAT_CLS, RV_FEAT_ALL = 0, 2
TOPK_CAP = 64
RV_WINDOWS_SHIFTED, RV_WINDOWS_CLIPPED = 0, 1

_DT = {torch.float32: RV_F32, torch.bfloat16: RV_BF16, torch.float16: RV_F16, torch.int32: RV_I32, torch.int64: RV_I64, torch.uint8: RV_U8}


class RvConfig(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("inter", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32),
                ("vocab", C.c_int32), ("rms_eps", C.c_float), ("rope_theta", C.c_float), ("adapter_dim", C.c_int32),
                ("adapter_heads", C.c_int32), ("adapter_ff", C.c_int32), ("adapter_layers", C.c_int32),
                ("adapter_text", C.c_int32)]


class RvPrefillGroup(C.Structure):
    """``rv_prefill_group``: one group of a mixed-geometry prefill pass (rv_llm_prefill_pool_mixed)."""
    _fields_ = [("B", C.c_int32), ("P0", C.c_int32), ("S", C.c_int32), ("kv_row0", C.c_int32)]


class RvYuvSurface(C.Structure):
    """``rv_yuv_surface``: the planes, strides (bytes), sample format, subsampling and colour tags of a decoder surface (rv_yuv_surface_to_patches)."""
    _fields_ = [("y", C.c_void_p), ("cb", C.c_void_p), ("cr", C.c_void_p), ("y_frame_stride", C.c_int64), ("y_row_stride", C.c_int64),
                ("c_frame_stride", C.c_int64), ("c_row_stride", C.c_int64), ("sample_bytes", C.c_int32), ("depth", C.c_int32), ("msb_aligned", C.c_int32),
                ("c_pix", C.c_int32), ("sub_x", C.c_int32), ("sub_y", C.c_int32), ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("matrix", C.c_int32), ("full_range", C.c_int32), ("chroma_loc", C.c_int32)]


class RvHdrMap(C.Structure):
    """``rv_hdr_map``: how rv_yuv_surface_to_patches_hdr converts an HDR surface to SDR (transfer 1 = PQ, 2 = HLG; gamut 1 = BT.2020 -> BT.709 primaries)."""
    _fields_ = [("transfer", C.c_int32), ("gamut", C.c_int32), ("peak_nits", C.c_float), ("sdr_white_nits", C.c_float)]


class RvPackedSurface(C.Structure):
    """``rv_packed_surface``: base pointer, strides (bytes), unit layout, component offsets, sample format and colour tags of a packed YCbCr surface
    (rv_packed_to_patches)."""
    _fields_ = [("base", C.c_void_p), ("frame_stride", C.c_int64), ("row_stride", C.c_int64), ("unit_bytes", C.c_int32), ("pix_per_unit", C.c_int32),
                ("sample_bytes", C.c_int32), ("y_off", C.c_int32), ("cb_off", C.c_int32), ("cr_off", C.c_int32), ("depth", C.c_int32), ("msb_aligned", C.c_int32),
                ("n", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("matrix", C.c_int32), ("full_range", C.c_int32), ("chroma_loc", C.c_int32)]


#: ``RV_FRAME_TABLE_MAX``: frames of one launch of the scattered entries (longer batches are cut by the library; callers need not)
FRAME_TABLE_MAX = 64


class RvSurfacePlanes(C.Structure):
    """``rv_surface_planes``: the Y, Cb and Cr device pointers of ONE frame of a pool of separately allocated surfaces (rv_yuv_surfaces_to_patches)."""
    _fields_ = [("y", C.c_void_p), ("cb", C.c_void_p), ("cr", C.c_void_p)]


class HipLibraryError(RuntimeError):
    pass


_libs = {}
_flavour = os.environ.get("REVISION_OP_DTYPE", "f16")
if _flavour not in OP_DTYPES:
    raise ValueError(f"REVISION_OP_DTYPE={_flavour!r}: expected one of {sorted(OP_DTYPES)}")


def flavour():
    """The process-wide DEFAULT flavour ("f16" unless REVISION_OP_DTYPE / set_flavour say otherwise): what an Engine built without an
    explicit ``op_dtype`` and the wrappers without a 16-bit input tensor use."""
    return _flavour


def set_flavour(f):
    global _flavour
    f = flavour_of(f)
    prev, _flavour = _flavour, f
    return prev


def flavour_of(x):
    """"f16" / "bf16" from a flavour name, a torch dtype or a tensor (None -> the default flavour)."""
    if x is None:
        return _flavour
    if isinstance(x, str):
        if x not in OP_DTYPES:
            raise ValueError(f"unknown operand flavour {x!r}")
        return x
    dt = x.dtype if torch.is_tensor(x) else x
    for k, v in OP_DTYPES.items():
        if v == dt:
            return k
    raise HipLibraryError(f"{dt} is not an operand type of librevision_hip (fp16 or bf16)")


def op_dtype(f=None):
    """torch dtype of a flavour's 16-bit operands."""
    return OP_DTYPES[flavour_of(f)]

_p, _i32, _i64, _f, _sz, _u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t, C.c_uint64

#: every symbol include/revision_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "rv_abi_version": (C.c_int, []),
    "rv_operand_dtype": (C.c_int, []),
    "rv_last_error": (C.c_int, [C.c_char_p, _sz]),
    "rv_ctx_create": (C.c_int, [C.POINTER(RvConfig), C.POINTER(_p)]),
    "rv_ctx_destroy": (None, [_p]),
    "rv_weights_bind": (C.c_int, [_p, C.c_char_p, _p, C.c_int, _i64]),
    "rv_init_hash": (C.c_int, [_p, C.c_int, _i64, _u64, _f, _f, _p]),
    "rv_ctx_set_option": (C.c_int, [_p, C.c_char_p, _i64]),
    "rv_ctx_get_option": (C.c_int, [_p, C.c_char_p, C.POINTER(_i64)]),
    "rv_numeric_status_bind": (C.c_int, [_p]),
    "rv_gemm_ws_bytes": (_sz, []),
    "rv_gemm_rows_ws_bytes": (_sz, []),
    "rv_gemm_rows": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _p, _p, C.c_int, C.c_int, _p]),
    "rv_gemm": (C.c_int, [_p, _p, _i64, _p, _i64, C.c_int, _p, _p, _i64, _p, _i64, C.c_int, C.c_int, _i64, _i64, _i64, _p, _sz, _p]),
    "rv_rmsnorm_quant_fp8": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _f, _p]),
    "rv_quant_rows_fp8": (C.c_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _p]),
    "rv_gemm_fp8": (C.c_int, [_p, _p, _i64, _p, _p, _p, _p, _i64, _p, _i64, C.c_int, C.c_int, _i64, _i64, _i64, _p, C.c_size_t, _p]),
    "rv_gemv_fp8": (C.c_int, [_p, _i64, _p, _p, _p, _p, _i64, _p, _i64, C.c_int, C.c_int, _i64, _i64, _i64, _p]),
    "rv_layernorm": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i32, _p]),
    "rv_rmsnorm": (C.c_int, [_p, _p, _p, _i64, _i32, _f, _p]),
    "rv_sine_pos": (C.c_int, [_p, _i32, _i32, _p]),
    "rv_attention": (C.c_int, [_p, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _p, _i32, _i32,
                               _i32, _i32, _i32, _i32, _i32, _i32, _f, _p]),
    "rv_frames_to_patches": (C.c_int, [_p, C.c_int, _i64, _i64, _i32, _i32, _i32, _i32, _i32, C.POINTER(_f), C.POINTER(_f), _p, _i64, _p, _p]),
    "rv_yuv_to_patches": (C.c_int, [_p, _i64, _i64, _p, _p, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_f), C.POINTER(_f), _p,
                                    _i64, _p, _p]),
    "rv_yuv_surface_to_patches": (C.c_int, [C.POINTER(RvYuvSurface), _i32, _i32, C.POINTER(_f), C.POINTER(_f), _p, _i64, _p, _p]),
    "rv_yuv_surface_to_patches_hdr": (C.c_int, [C.POINTER(RvYuvSurface), C.POINTER(RvHdrMap), _i32, _i32, C.POINTER(_f), C.POINTER(_f), _p, _i64, _p, _p]),
    "rv_frames_to_patches_oriented": (C.c_int, [_p, C.c_int, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_f), C.POINTER(_f), _p, _i64, _p, _p]),
    "rv_yuv_surface_to_patches_oriented": (C.c_int, [C.POINTER(RvYuvSurface), C.POINTER(RvHdrMap), _i32, _i32, _i32, C.POINTER(_f), C.POINTER(_f), _p, _i64, _p,
                                                     _p]),
    "rv_packed_to_patches": (C.c_int, [C.POINTER(RvPackedSurface), C.POINTER(RvHdrMap), _i32, _i32, _i32, C.POINTER(_f), C.POINTER(_f), _p, _i64, _p, _p]),
    "rv_frames_to_patches_packed": (C.c_int, [_p, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_f), C.POINTER(_f), _p, _i64, _p,
                                              _p]),
    "rv_frames_to_patches_scattered": (C.c_int, [C.POINTER(_p), C.c_int, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_f),
                                                 C.POINTER(_f), _p, _i64, _p, _p]),
    "rv_yuv_surfaces_to_patches": (C.c_int, [C.POINTER(RvYuvSurface), C.POINTER(RvSurfacePlanes), C.POINTER(RvHdrMap), _i32, _i32, _i32, C.POINTER(_f),
                                             C.POINTER(_f), _p, _i64, _p, _p]),
    "rv_packed_surfaces_to_patches": (C.c_int, [C.POINTER(RvPackedSurface), C.POINTER(_p), C.POINTER(RvHdrMap), _i32, _i32, _i32, C.POINTER(_f), C.POINTER(_f), _p,
                                                _i64, _p, _p]),
    "rv_project_dense": (C.c_int, [_p, _p, _p, C.c_int, _i64, _p]),
    "rv_clip_encoder_ws_bytes": (_sz, [_p, _i32, _i32, _i32, _i32]),
    "rv_clip_encoder": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p, _sz, _p]),
    "rv_splice_embed": (C.c_int, [_p, _p, _p, _p, _i64, _p]),
    "rv_kv_bytes": (_sz, [_p, _i32, _i32]),
    "rv_llm_ws_bytes": (_sz, [_p, _i32, _i32]),
    "rv_llm_forward": (C.c_int, [_p, _p, _i32, _i32, _i32, _p, _i32, _p, _p, _sz, _p]),
    "rv_llm_layers": (C.c_int, [_p, _p, _i32, _i32, _i32, _p, _i32, _i32, _i32, _p, _sz, _p]),
    "rv_llm_prefill_shared_ws_bytes": (_sz, [_p, _i32, _i32, _i32]),
    "rv_llm_prefill_shared": (C.c_int, [_p, _p, _i32, _i32, _i32, _p, _i32, _p, _p, _sz, _p]),
    "rv_llm_prefill_pool": (C.c_int, [_p, _p, _i32, _i32, _i32, _p, _i32, _i32, _i32, _p, _p, _sz, _p]),
    "rv_llm_prefill_pool_groups": (C.c_int, [_p, _p, _i32, _i32, _i32, _i32, _p, _i32, _p, _i32, _p, _p, _sz, _p]),
    "rv_llm_prefill_pool_groups_ragged": (C.c_int, [_p, _p, _i32, _i32, _i32, _i32, _p, _i32, _p, _i32, _p, _p, _p, _sz, _p]),
    "rv_llm_prefill_pool_mixed": (C.c_int, [_p, _p, _i32, _p, _p, _i32, _i32, _p, _p, _p, _sz, _p]),
    "rv_llm_decode_rows": (C.c_int, [_p, _p, _i32, _p, _p, _i32, _p, _p, _sz, _p]),
    "rv_llm_decode_rows_shared": (C.c_int, [_p, _p, _i32, _p, _p, _p, _i32, _p, _p, _sz, _p]),
    "rv_sample": (C.c_int, [_p, _p, _i32, _i32, _p, _i32, _f, _i32, _f, _p, _p, _p, _p, _p, _p, _p, _p]),
    "rv_entropy_stats": (C.c_int, [_p, _i32, _i32, _i32, _p, _p]),
    "rv_topk_cosine": (C.c_int, [_p, C.c_int, _p, _i32, _i32, _i32, _i32, _p, _p]),
    "rv_topk_pool": (C.c_int, [_p, C.c_int, _p, _i32, _i32, _i32, _i32, _i32, _p, _p, _p]),
    "rv_frame_cosine": (C.c_int, [_p, C.c_int, _p, _i32, _i32, _i32, _p, _p]),
    "rv_span_scores": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _i32, _f, _p, _p, _p]),
    "rv_frame_cosine_multi": (C.c_int, [_p, C.c_int, _p, _i32, _i32, _i32, _i32, _p, _p, _p]),
    "rv_span_scores_multi": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _f, _p, _p, _p]),
    "rv_attn_pool": (C.c_int, [_p, C.c_int, _p, _i32, _i32, _i32, _i32, _f, _p, _p]),
    "rv_span_rank": (C.c_int, [_p, _p, _i32, _i32, _i32, _i32, _f, _p, _p, _i32, _p, _p, _p, _p, _p, _p]),
    "rv_span_propose": (C.c_int, [_p, _p, _i32, _i32, _i32, C.POINTER(_f), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p]),
    "rv_window_select": (C.c_int, [_p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "rv_window_gather": (C.c_int, [_p, _i32, _i64, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _i32, _p, _p]),
    "rv_window_gather_rule": (C.c_int, [_p, _i32, _i64, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _i32, _p, _i32, _p]),
    "rv_proposal_cosine": (C.c_int, [_p, C.c_int, _p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p]),
}


#: the companion library (include/revision_hip_ext.h): f32-only entries, ONE build for both operand flavours; every exported name starts with rvx_.
#: REVISION_HIP_LIB_EXT: load another build of it.
EXT_LIB_PATH = os.environ.get("REVISION_HIP_LIB_EXT") or os.path.join(_HERE, "librevision_hip_ext.so")
RVX_ABI_VERSION = 1
#: every symbol include/revision_hip_ext.h declares: name -> (restype, argtypes)
EXT_SIGNATURES = {
    "rvx_abi_version": (C.c_int, []),
    "rvx_last_error": (C.c_int, [C.c_char_p, _sz]),
    "rvx_window_select_clipped": (C.c_int, [_p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
}


def _load(path, signatures, complaint):
    """One loader for every library: existence check, CDLL, the signature table, then ``complaint(handle)`` -> what is wrong with this build, or None.
    Raises HipLibraryError when the library is missing or is not the build that was asked for (there is no fallback)."""
    if not os.path.exists(path):
        raise HipLibraryError(f"{path} not found: build it with `python -m revisionllm_amd.build` (hipcc, gfx950). "
                              "revisionllm_amd has no CPU fallback.")
    try:
        h = C.CDLL(path)
    except OSError as e:
        raise HipLibraryError(f"cannot load {path}: {e}") from e
    for name, (res, args) in signatures.items():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = res, args
    wrong = complaint(h)
    if wrong:
        raise HipLibraryError(f"{path} {wrong}")
    return h


_companions = {}


def _load_versioned(path, signatures, prefix, version):
    """The f32-only libraries: loaded once each (kept in _companions under their prefix: "rvx", "rvc"), refused unless <prefix>_abi_version() is ``version``."""
    if prefix not in _companions:
        def complaint(h):
            got = getattr(h, prefix + "_abi_version")()
            return None if got == version else f"has {prefix}_abi_version() = {got} (expected {version})"
        _companions[prefix] = _load(path, signatures, complaint)
    return _companions[prefix]


def _last_error_of(prefix):
    if prefix not in _companions:
        return ""
    buf = C.create_string_buffer(512)
    getattr(_companions[prefix], prefix + "_last_error")(buf, 512)
    return buf.value.decode()


def _check_of(prefix, rc, what):
    if rc != 0:
        raise HipLibraryError(f"{what} failed (status {rc}): {_last_error_of(prefix)}")


def ext_lib():
    """Load (once) and return the ctypes handle of the companion library; raises HipLibraryError when it is missing (there is no fallback)."""
    return _load_versioned(EXT_LIB_PATH, EXT_SIGNATURES, "rvx", RVX_ABI_VERSION)


def ext_last_error():
    """The calling thread's last error message of the companion library ("" when it is not loaded)."""
    return _last_error_of("rvx")


def ext_check(rc, what):
    _check_of("rvx", rc, what)


#: the chain library (include/revision_hip_chain.h): the grounding chain's entries added after the companion library was closed too; f32-only, ONE
#: build for both operand flavours; every exported name starts with rvc_.  This table is open: a new chain entry gets a line here.
#: REVISION_HIP_LIB_CHAIN: load another build of it.
CHAIN_LIB_PATH = os.environ.get("REVISION_HIP_LIB_CHAIN") or os.path.join(_HERE, "librevision_hip_chain.so")
RVC_ABI_VERSION = 1
RV_FRAMES_ALL, RV_FRAMES_SAMPLED = 0, 1
RVC_MAX_SAMPLED = 1024
RVC_ANCHORS_MEAN, RVC_ANCHORS_CONTRAST = 0, 1
#: every symbol include/revision_hip_chain.h declares: name -> (restype, argtypes)
CHAIN_SIGNATURES = {
    "rvc_abi_version": (C.c_int, []),
    "rvc_last_error": (C.c_int, [C.c_char_p, _sz]),
    "rvc_window_select_frames": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p,
                                           _p, _p]),
    "rvc_span_scores_masked": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _f, _i32, _p, _p, _p, _p]),
    "rvc_span_propose_masked": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, C.POINTER(_f), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p]),
    "rvc_windows_valid": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p]),
    "rvc_span_scores_masked_rows": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f, _i32, _p, _p, _p, _p]),
    "rvc_span_propose_masked_rows": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, C.POINTER(_f), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p,
                                               _p, _p, _p]),
    "rvc_span_refine": (C.c_int, [_p, _p, _i32, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p]),
    "rvc_span_anchors_workspace": (_i64, [_i32, C.POINTER(_i32), _i32, _i32]),
    "rvc_span_anchors": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _i64, _p]),
}


def chain_lib():
    """Load (once) and return the ctypes handle of the chain library; raises HipLibraryError when it is missing (there is no fallback)."""
    return _load_versioned(CHAIN_LIB_PATH, CHAIN_SIGNATURES, "rvc", RVC_ABI_VERSION)


def chain_last_error():
    """The calling thread's last error message of the chain library ("" when it is not loaded)."""
    return _last_error_of("rvc")


def chain_check(rc, what):
    _check_of("rvc", rc, what)


def lib(f=None):
    """Load (once) and return the ctypes handle of a flavour's library (f: flavour name, torch dtype, tensor or None = the default
    flavour); raises HipLibraryError when the extension is missing."""
    f = flavour_of(f)
    if f not in _libs:
        def complaint(h):
            got = h.rv_operand_dtype()
            return None if got == _DT[OP_DTYPES[f]] else f"is not the {f} build of the library (rv_operand_dtype() = {got})"
        _libs[f] = _load(LIB_PATHS[f], SIGNATURES, complaint)
    return _libs[f]


_numeric = {}


def numeric_status(f=None, device=None):
    """The numeric status buffer of a flavour's library on a device (``rv_numeric_status_bind``): int32 [4] device tensor, word 0 = the sticky count of
    f32 -> fp16 stores that saturated.  Created, zeroed and bound on first use (one per library instance and device; the library keeps the pointer, this
    module keeps the tensor alive).  Reading it is an ordinary device -> host copy: pipelines that copy results out anyway take it along."""
    f = flavour_of(f)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = (f, dev.index)
    t = _numeric.get(key)
    if t is None:
        t = torch.zeros(4, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            torch.cuda.synchronize(dev)          # the zero fill is complete before any kernel can add to the buffer
            check(lib(f).rv_numeric_status_bind(C.c_void_p(t.data_ptr())), "rv_numeric_status_bind")
        _numeric[key] = t
    return t


def last_error():
    """The calling thread's last error message (of whichever loaded library has one)."""
    buf = C.create_string_buffer(512)
    msgs = []
    for h in _libs.values():
        h.rv_last_error(buf, 512)
        if buf.value:
            msgs.append(buf.value.decode())
    return " | ".join(msgs)


def check(rc, what):
    if rc != 0:
        # the error string is per library and thread and is not cleared by later successes: with both builds loaded, prefer the message that names
        # the entry point that just failed
        msgs = last_error().split(" | ")
        name = what.split("(")[0]
        mine = [m for m in msgs if name in m]
        raise HipLibraryError(f"{what} failed (status {rc}): {' | '.join(mine or msgs)}")


OPTION_KEYS = ("gemm_tile_variant", "gemm_cus", "gemm_arows", "fp8_decode", "fp8_prefill", "sample_variant", "rows_fill", "rows_spread", "rows_persistent", "rows_single", "gemm_waves", "gemm_mhalf", "precision", "lm_head_split", "last_block_rows", "adapter_stream16", "adapter_fold_t2v", "attn_lds", "qkv_lds")


class Options:
    """Owner of an OPTIONS-ONLY ``rv_ctx`` (``rv_ctx_create(NULL, ...)``): tunables for the building-block entry points that take
    an optional context (``rv_gemm``, ``rv_gemm_fp8``, ``rv_sample``).  ``Options(gemm_tile_variant=6)``; pass it as ``ctx=``.
    A context belongs to ONE library: ``flavour`` (default: the process default) names it."""

    def __init__(self, flavour=None, **kw):
        self.flavour = flavour_of(flavour)
        self.lib = lib(self.flavour)
        self._ctx = C.c_void_p()
        check(self.lib.rv_ctx_create(None, C.byref(self._ctx)), "rv_ctx_create(options)")
        for k, v in kw.items():
            self.set(k, v)

    def set(self, key, value):
        check(self.lib.rv_ctx_set_option(self._ctx, key.encode(), int(value)), f"rv_ctx_set_option({key})")
        return self

    def get(self, key):
        v = _i64()
        check(self.lib.rv_ctx_get_option(self._ctx, key.encode(), C.byref(v)), f"rv_ctx_get_option({key})")
        return int(v.value)

    def __del__(self):
        try:
            if self._ctx and self._ctx.value:
                self.lib.rv_ctx_destroy(self._ctx)
                self._ctx = C.c_void_p()
        except Exception:
            pass


def ctx_ptr(ctx, f=None):
    """``rv_ctx*`` of an ``Options`` / ``Engine`` (or None -> NULL: the library's default tunables).  ``f``: the flavour of the library
    about to be called - a context of the other library is refused."""
    if ctx is None:
        return None
    if f is not None and ctx.flavour != flavour_of(f):
        raise HipLibraryError(f"a {ctx.flavour} context was passed to a {flavour_of(f)} call")
    return ctx._ctx


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Tensors must live on the GPU and be contiguous."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HipLibraryError("librevision_hip needs device tensors (got a CPU tensor); there is no CPU path")
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dtype_code(t):
    return _DT[t.dtype]
