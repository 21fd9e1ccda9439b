"""Functional wrappers over the C ABI building blocks (used by the engine, the scoring helpers and the tests).

Every function takes / returns torch DEVICE tensors and enqueues on torch's current stream.
"""
import math

import torch

from . import hip
from .utils import hashinit


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def init_hash_(t, name, seed, a, base=0.0, offset=0):
    """Fill ``t`` in place with the hash-seeded uniform(base-a, base+a) stream of tensor ``name``.  ``a``: one amplitude, or
    (row_end, amplitude) pieces over the leading dimension (``hashinit.amplitude_pieces``): one launch per piece, same stream."""
    assert t.is_contiguous()
    key = hashinit.tensor_key(name, seed) + offset
    flat = t.view(-1)
    for e0, cnt, amp in hashinit.amplitude_pieces(a, tuple(t.shape)):
        piece = flat[e0:e0 + cnt]
        hip.check(hip.lib(None if t.dtype == torch.float32 else t).rv_init_hash(hip.ptr(piece), hip.dtype_code(t), cnt, (key + e0) & 0xFFFFFFFFFFFFFFFF, float(hashinit.step_for(amp)),
                                         float(base), hip.stream()), "rv_init_hash")
    return t


def pack_fragments(w):
    """Row-major [N,K] 16-bit operands (fp16 / bf16; any 2-byte dtype) -> fragment-packed (same shape / numel): every 16x32 MFMA operand fragment becomes one
    contiguous 1 KiB block in lane order (lane = (n&15) + 16*((k>>3)&3), 8 bf16 per lane).  See include/revision_hip.h."""
    N, K = w.shape
    assert N % 16 == 0 and K % 32 == 0, (N, K)
    return w.view(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(N, K)


_SK_WS = {}


def stream_k_workspace(device, f=None):
    """Zero-initialised stream-K workspace for stand-alone rv_gemm calls (cached per device and library: the hand-off epochs are per library)."""
    key = (str(device), hip.flavour_of(f))
    if key not in _SK_WS:
        _SK_WS[key] = torch.zeros(hip.lib(f).rv_gemm_ws_bytes(), dtype=torch.uint8, device=device)
    return _SK_WS[key]


def gemm(a, w, bias=None, residual=None, out_dtype=None, act=hip.RV_ACT_NONE, out=None, w_packed=False, stream_k=None, ctx=None):
    """act(a @ w.T + bias) + residual.  a [M,K] fp16 / bf16 (row stride allowed), w [N,K] of the same dtype, row-major or fragment-packed;
    the library is chosen by a's dtype; ``out_dtype``: a's dtype (default) or float32.
    ``stream_k`` (default: on for packed W) hands the library a workspace so it may pick the persistent stream-K kernel.
    ``ctx``: an ``hip.Options`` / ``Engine`` whose tunables apply (None: defaults)."""
    M, K = a.shape
    N = w.shape[0]
    n_out = N // 2 if act == hip.RV_ACT_SILU_MUL else N
    if out is None:
        out = torch.empty(M, n_out, dtype=out_dtype or a.dtype, device=a.device)
    assert a.stride(1) == 1 and w.stride(1) == 1 and out.stride(1) == 1 and w.dtype == a.dtype
    ws = stream_k_workspace(a.device, a) if (w_packed if stream_k is None else stream_k) else None
    hip.check(hip.lib(a).rv_gemm(hip.ctx_ptr(ctx, a), hip.ptr(a), a.stride(0), hip.ptr(w), w.stride(0), int(w_packed), hip.ptr(bias), hip.ptr(residual),
                                residual.stride(0) if residual is not None else 0, hip.ptr(out), out.stride(0),
                                hip.dtype_code(out), act, M, N, K, hip.ptr(ws), ws.numel() if ws is not None else 0, hip.stream()),
              "rv_gemm")
    return out


def xp_blocks(rows):
    """Row blocks of the fragment-packed decode layout (csrc/kernels.h rv_xp_blocks)."""
    return 2 if rows <= 32 else 4 if rows <= 64 else 5 if rows <= 80 else 8 if rows <= 128 else 9


def pack_rows(x):
    """[M,K] bf16 (M <= 144, K % 32 == 0) -> the fragment-packed decode layout [16 * mbp * K] (csrc/kernels.h rv_xp_index): every
    16-row x 32-k operand fragment one contiguous 1 KiB block, the mbp row blocks of a k-fragment adjacent; rows past M are zero."""
    M, K = x.shape
    mbp = xp_blocks(M)
    xp = torch.zeros(mbp * 16, K, dtype=x.dtype, device=x.device)
    xp[:M] = x
    return xp.view(mbp, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous().view(-1)


_ROWS_WS = {}


def gemm_rows(x, wp, act=hip.RV_ACT_NONE, out_dtype=torch.float32, out=None, xp=None, w_scale=None, N=None):
    """One projection of a merged decode step on 33 .. 144 rows (rv_gemm_rows: the split-K kernel with LDS-shared activations).
    x [M,K] bf16 row-major (packed here; or ``xp`` already packed), wp fragment-packed [N,K] -> row-major [M, N] (N / 2 with SILU_MUL).
    ``w_scale`` f32 [N]: ``wp`` holds FP8 bytes (``pack_fragments_fp8``: uint8 [N*K]) instead of bf16 fragments."""
    M, K = x.shape
    N = (w_scale.shape[0] if w_scale is not None else wp.shape[0]) if N is None else N
    key = (str(x.device), torch.cuda.current_stream(x.device).cuda_stream, hip.flavour_of(x))
    if key not in _ROWS_WS:
        _ROWS_WS[key] = (torch.zeros(hip.lib(x).rv_gemm_rows_ws_bytes(), dtype=torch.uint8, device=x.device),
                         torch.zeros(2048, dtype=torch.int32, device=x.device))
    planes, arrive = _ROWS_WS[key]
    if xp is None:
        xp = pack_rows(x)
    n_out = N // 2 if act == hip.RV_ACT_SILU_MUL else N
    if out is None:
        out = torch.empty(M, n_out, dtype=x.dtype if act == hip.RV_ACT_SILU_MUL else out_dtype, device=x.device)
    hip.check(hip.lib(x).rv_gemm_rows(hip.ptr(xp), hip.ptr(wp), hip.ptr(w_scale), hip.ptr(out), M, N, K, hip.ptr(planes), hip.ptr(arrive), act, hip.dtype_code(out),
                                     hip.stream()), "rv_gemm_rows")
    return out


FP8_MAX = 448.0   # largest finite e4m3fn value


def quantize_rows_fp8(w):
    """Per-row symmetric FP8 (e4m3fn, OCP) quantisation of a [N,K] matrix: -> (q float8_e4m3fn [N,K], scale f32 [N]) with
    w ~ q * scale[:, None], scale = max|row| / 448 (1 for an all-zero row)."""
    w = w.double()            # float64 divisions are correctly rounded on host and device alike: the same bits everywhere
    amax = w.abs().amax(dim=1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax)).float()
    q = (w / scale.double()[:, None]).float().to(torch.float8_e4m3fn)
    return q, scale.contiguous()


def pack_fragments_fp8(w):
    """[N,K] (any float dtype; N % 16 == 0, K % 64 == 0) -> (uint8 [N*K] in the FP8 fragment-packed layout of the decode
    kernel, f32 [N] row scales).  Byte of element (n, k): (((n>>4)*(K/64) + (k>>6))*64 + (n&15) + 16*((k>>3)&3))*16 +
    ((k>>5)&1)*8 + (k&7): a lane's 16-byte load carries its MFMA operand of two consecutive 32-k blocks."""
    q, scale = quantize_rows_fp8(w)
    return pack_fp8_decode(q), scale


def pack_fp8_decode(q):
    """float8_e4m3fn [N,K] -> uint8 [N*K] in the decode kernel's FP8 fragment layout (see pack_fragments_fp8)."""
    N, K = q.shape
    assert N % 16 == 0 and K % 64 == 0
    b = q.view(torch.uint8).view(N // 16, 16, K // 64, 2, 4, 8)           # (nb, r, kc, half, kq, e)
    return b.permute(0, 2, 4, 1, 3, 5).contiguous().view(-1)              # (nb, kc, kq, r, half, e): lane = kq * 16 + r


def pack_fp8_prefill(q):
    """float8_e4m3fn [N,K] (K % 128 == 0) -> uint8 [N*K]: the byte matrix taken as [N, K/2] 16-bit words, fragment-packed like
    a bf16 weight (``pack_fragments``) - the operand layout of the FP8 prefill GEMM (rv_gemm_fp8)."""
    N, K = q.shape
    assert N % 16 == 0 and K % 128 == 0
    words = q.contiguous().view(torch.uint8).view(torch.int16)            # [N, K/2]
    return pack_fragments(words).view(torch.uint8).reshape(-1)


def gemv_fp8(a, w8, scale, bias=None, residual=None, out_dtype=None, act=hip.RV_ACT_NONE, out=None):
    """Decode projection (M <= 16) with FP8 fragment-packed weights: act(a @ (q * scale).T + bias) + residual."""
    M, K = a.shape
    N = scale.numel()
    n_out = N // 2 if act == hip.RV_ACT_SILU_MUL else N
    if out is None:
        out = torch.empty(M, n_out, dtype=out_dtype or a.dtype, device=a.device)
    hip.check(hip.lib(a).rv_gemv_fp8(hip.ptr(a), a.stride(0), hip.ptr(w8), hip.ptr(scale), hip.ptr(bias), hip.ptr(residual),
                                    residual.stride(0) if residual is not None else 0, hip.ptr(out), out.stride(0), hip.dtype_code(out),
                                    act, M, N, K, hip.stream()), "rv_gemv_fp8")
    return out


def pack_fragments_fp8_prefill(w):
    """[N,K] (any float dtype; N % 16 == 0, K % 128 == 0) -> (uint8 [N*K], f32 [N] row scales) for the FP8 prefill GEMM: the
    quantised byte matrix is taken as [N, K/2] 16-bit words and fragment-packed like a bf16 weight (``pack_fragments``)."""
    q, scale = quantize_rows_fp8(w)
    return pack_fp8_prefill(q), scale


def quant_rows_fp8(x, out=None):
    """fp16 / bf16 activations [M,K] -> (e4m3fn bytes uint8 [M,K], f32 [M] row scales) on the device (rv_quant_rows_fp8).  ``x`` and ``out`` (uint8
    [M,K], written in place and returned) may be column windows of wider tensors: rows with unit column stride, a row stride that is a multiple of 8 and
    at least K, and a 16-byte aligned start are passed with their row strides; any other ``x`` is copied first.  ``out`` is never copied: the entry point
    refuses a row stride that is no multiple of 8."""
    M, K = x.shape
    if x.stride(1) != 1 or x.stride(0) < K or x.stride(0) % 8 != 0 or x.data_ptr() % 16 != 0:
        x = x.contiguous()          # what the kernel's 16-byte loads cannot take is copied, as before
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device) if out is None else out
    assert q.dtype == torch.uint8 and tuple(q.shape) == (M, K) and q.device == x.device, "quant_rows_fp8: out must be uint8 [M,K] on x's device"
    assert q.stride(1) == 1 and (M <= 1 or q.stride(0) >= K), "quant_rows_fp8: out needs unit column stride and rows that do not overlap"
    sc = torch.empty(M, dtype=torch.float32, device=x.device)
    hip.check(hip.lib(x).rv_quant_rows_fp8(hip.ptr(x), x.stride(0), hip.ptr(q), q.stride(0), hip.ptr(sc), M, K, hip.stream()), "rv_quant_rows_fp8")
    return q, sc


def rmsnorm_quant_fp8(x, w, eps, op_dtype=None):
    """f32 [rows, 4096] -> (e4m3fn bytes, f32 row scales) of the operand-rounded LlamaRMSNorm output (rv_rmsnorm_quant_fp8; ``op_dtype``: the flavour)."""
    rows, d = x.shape
    q = torch.empty(rows, d, dtype=torch.uint8, device=x.device)
    sc = torch.empty(rows, dtype=torch.float32, device=x.device)
    hip.check(hip.lib(op_dtype).rv_rmsnorm_quant_fp8(hip.ptr(_c(x)), hip.ptr(w), hip.ptr(q), hip.ptr(sc), rows, d, eps, hip.stream()), "rv_rmsnorm_quant_fp8")
    return q, sc


def gemm_fp8(a8, a_scale, w8p, w_scale, residual=None, out_dtype=torch.float32, act=hip.RV_ACT_NONE, out=None, ctx=None, op_dtype=None):
    """FP8 x FP8 prefill GEMM: act((a8 @ w8.T) * a_scale[:, None] * w_scale[None]) + residual (rv_gemm_fp8)."""
    M, K = a8.shape
    N = w_scale.numel()
    n_out = N // 2 if act == hip.RV_ACT_SILU_MUL else N
    if out is None:
        out = torch.empty(M, n_out, dtype=out_dtype, device=a8.device)
    f = hip.flavour_of(out if out.dtype != torch.float32 else (ctx.flavour if ctx is not None else op_dtype))
    ws = stream_k_workspace(a8.device, f)
    hip.check(hip.lib(f).rv_gemm_fp8(hip.ctx_ptr(ctx, f), hip.ptr(a8), a8.stride(0), hip.ptr(a_scale), hip.ptr(w8p), hip.ptr(w_scale), hip.ptr(residual),
                                    residual.stride(0) if residual is not None else 0, hip.ptr(out), out.stride(0), hip.dtype_code(out), act,
                                    M, N, K, hip.ptr(ws), ws.numel(), hip.stream()), "rv_gemm_fp8")
    return out


def layernorm(x, w, b, pos=None, period=0, want=("f32", "op16"), op_dtype=None):
    """LayerNorm of f32 rows -> (f32 copy, 16-bit operand copy, operand copy of y + pos); ``op_dtype``: the flavour of the 16-bit outputs."""
    rows, d = x.shape
    dt = hip.op_dtype(op_dtype)
    y32 = torch.empty_like(x) if "f32" in want else None
    y16 = torch.empty(rows, d, dtype=dt, device=x.device) if ("op16" in want or "bf16" in want) else None
    yp = torch.empty(rows, d, dtype=dt, device=x.device) if pos is not None else None
    if rows == 0:          # (an empty tensor has no pointer to pass)
        return y32, y16, yp
    hip.check(hip.lib(dt).rv_layernorm(hip.ptr(_c(x)), hip.ptr(w), hip.ptr(b), hip.ptr(y32), hip.ptr(y16), hip.ptr(yp),
                                     hip.ptr(pos), period, rows, d, hip.stream()), "rv_layernorm")
    return y32, y16, yp


def rmsnorm(x, w, eps, op_dtype=None):
    rows, d = x.shape
    y = torch.empty(rows, d, dtype=hip.op_dtype(op_dtype), device=x.device)
    hip.check(hip.lib(y).rv_rmsnorm(hip.ptr(_c(x)), hip.ptr(w), hip.ptr(y), rows, d, eps, hip.stream()), "rv_rmsnorm")
    return y


def sine_pos(T, d=768, device="cuda"):
    pos = torch.empty(T, d, dtype=torch.float32, device=device)
    hip.check(hip.lib().rv_sine_pos(hip.ptr(pos), T, d, hip.stream()), "rv_sine_pos")
    return pos


def attention(q, k, v, causal=False, key_pad=None, q_pos0=0, scale=None):
    """q [B,Lq,H,dh], k/v [Bk,Lk,H,dh] fp16 / bf16 (B % Bk == 0) -> [B,Lq,H*dh] of the same dtype.  Transposes V itself
    (test / convenience entry; the engine keeps V^T resident)."""
    B, Lq, H, dh = q.shape
    Bk, Lk = k.shape[0], k.shape[1]
    Lpad = (Lk + 31) // 32 * 32
    vt = torch.zeros(Bk, H, dh, Lpad, dtype=q.dtype, device=q.device)
    vt[..., :Lk] = v.permute(0, 2, 3, 1)
    q, k = _c(q), _c(k)
    out = torch.empty(B, Lq, H * dh, dtype=q.dtype, device=q.device)
    pad = _c(key_pad.to(torch.uint8)) if key_pad is not None else None
    hip.check(hip.lib(q).rv_attention(hip.ptr(q), H * dh, Lq * H * dh, hip.ptr(k), H * dh, Lk * H * dh, dh, hip.ptr(vt),
                                     H * dh * Lpad, dh * Lpad, Lpad, hip.ptr(out), H * dh, Lq * H * dh, hip.ptr(pad), B, H, dh,
                                     Lq, Lk, int(causal), q_pos0, B // Bk, scale if scale is not None else 1.0 / math.sqrt(dh),
                                     hip.stream()), "rv_attention")
    return out


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


def _require_device(tensors, who):
    """The list forms' device check: the pointer tables hold device addresses, there is no CPU path."""
    if not all(t.is_cuda for t in tensors):
        raise hip.HipLibraryError(f"{who} needs device tensors (got a CPU tensor); there is no CPU path")


def _frame_outputs(n, R, patch, op_dtype, want, device):
    dt = hip.op_dtype(op_dtype)
    g = R // max(patch, 1)
    kp = (3 * patch * patch + 127) // 128 * 128
    patches = torch.empty(n * g * g, kp, dtype=dt, device=device) if "patches" in want else None
    image = torch.empty(n, 3, R, R, dtype=torch.float32, device=device) if "image" in want else None
    return dt, kp, patches, image


def _frames_to_patches_scattered(frames, R, patch, layout, mean, std, op_dtype, want, orient, pix_fmt):
    """``frames_to_patches`` on a list of per-frame tensors [3,H,W] / [H,W,3] (with ``pix_fmt`` [H,W,3|4]): one pointer per frame, the strides of frame 0 for
    all (rv_frames_to_patches_scattered).  Every ValueError comes before the library is touched."""
    who = "frames_to_patches"
    frames = _frame_list(frames, who)
    e = frames[0]
    if pix_fmt is not None:
        if pix_fmt not in RGB_PIX_FMTS:
            raise ValueError(f"pix_fmt {pix_fmt!r}: one of {sorted(RGB_PIX_FMTS)} (packed 8-bit RGB)")
        pix, r, g, b = RGB_PIX_FMTS[pix_fmt]
        if layout not in (None, "NHWC"):
            raise ValueError(f"pix_fmt {pix_fmt!r} names the byte order of packed pixels [H,W,{pix}]: layout {layout!r} does not go with it")
        if e.dtype != torch.uint8 or e.dim() != 3 or e.shape[2] != pix:
            raise ValueError(f"{pix_fmt} frames in a list come as uint8 tensors [H,W,{pix}], got {e.dtype} {tuple(e.shape)}")
        layout = "NHWC"
    else:
        pix, r, g, b = 3, 0, 1, 2
        if e.dtype != torch.uint8 or e.dim() != 3:
            raise ValueError(f"frames in a list come as uint8 tensors [3,H,W] or [H,W,3], got {e.dtype} {tuple(e.shape)}")
        nchw, nhwc = e.shape[0] == 3, e.shape[2] == 3
        if layout is None:
            if nchw == nhwc:
                raise ValueError(f"frames of shape {tuple(e.shape)} read as " + ("NCHW and as NHWC: pass layout=" if nchw else "neither NCHW nor NHWC"))
            layout = "NCHW" if nchw else "NHWC"
        if layout not in _LAYOUTS or not (nchw if layout == "NCHW" else nhwc):
            raise ValueError(f"layout {layout!r} does not fit frames of shape {tuple(e.shape)}")
    if layout == "NCHW":
        H, W = e.shape[1], e.shape[2]
        if not (e.stride(2) == 1 and e.stride(1) >= W and e.stride(0) > 0):
            frames = [t.contiguous() for t in frames]
        cs, rs = frames[0].stride(0), frames[0].stride(1)
    else:
        H, W = e.shape[0], e.shape[1]
        if not (e.stride(2) == 1 and e.stride(1) == pix and e.stride(0) >= pix * W):
            frames = [t.contiguous() for t in frames]
        cs, rs = 0, frames[0].stride(0)
    _require_device(frames, who)
    n = len(frames)
    dt, kp, patches, image = _frame_outputs(n, R, patch, op_dtype, want, e.device)
    table = (hip.C.c_void_p * n)(*[t.data_ptr() for t in frames])
    f3 = hip.C.c_float * 3
    hip.check(hip.lib(dt).rv_frames_to_patches_scattered(table, _LAYOUTS[layout], pix, r, g, b, cs, rs, n, H, W, orient, R, patch, f3(*mean), f3(*std),
                                                         hip.ptr(patches), kp, hip.ptr(image), hip.stream()), "rv_frames_to_patches_scattered")
    return patches, image


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
    orient = orientation(rotate, hflip, vflip)
    if isinstance(frames, (list, tuple)):
        return _frames_to_patches_scattered(frames, R, patch, layout, mean, std, op_dtype, want, orient, pix_fmt)
    if pix_fmt is not None:
        return _frames_to_patches_packed(frames, R, patch, layout, mean, std, op_dtype, want, orient, pix_fmt)
    if not torch.is_tensor(frames) or not frames.is_cuda:
        raise hip.HipLibraryError("frames_to_patches needs a device tensor (got a CPU tensor); there is no CPU path")
    if frames.dtype != torch.uint8 or frames.dim() != 4:
        raise hip.HipLibraryError(f"frames_to_patches takes uint8 frames [n,3,H,W] or [n,H,W,3], got {frames.dtype} {tuple(frames.shape)}")
    nchw, nhwc = frames.shape[1] == 3, frames.shape[3] == 3
    if layout is None:
        if nchw == nhwc:
            raise ValueError(f"frames of shape {tuple(frames.shape)} read as " + ("NCHW and as NHWC: pass layout=" if nchw else "neither NCHW nor NHWC"))
        layout = "NCHW" if nchw else "NHWC"
    if layout not in _LAYOUTS or not (nchw if layout == "NCHW" else nhwc):
        raise ValueError(f"layout {layout!r} does not fit frames of shape {tuple(frames.shape)}")
    n = frames.shape[0]
    if layout == "NCHW":
        H, W = frames.shape[2], frames.shape[3]
        ok = frames.stride(3) == 1 and frames.stride(2) >= W and frames.stride(1) > 0 and (n <= 1 or frames.stride(0) == 3 * frames.stride(1))
        frames = frames if ok else frames.contiguous()
        fs, rs = 3 * frames.stride(1), frames.stride(2)
    else:
        H, W = frames.shape[1], frames.shape[2]
        ok = frames.stride(3) == 1 and frames.stride(2) == 3 and frames.stride(1) >= 3 * W and (n <= 1 or frames.stride(0) > 0)
        frames = frames if ok else frames.contiguous()
        fs, rs = (frames.stride(0) if n > 1 else frames.stride(1) * H), frames.stride(1)
    dt = hip.op_dtype(op_dtype)
    g = R // max(patch, 1)
    kp = (3 * patch * patch + 127) // 128 * 128
    patches = torch.empty(n * g * g, kp, dtype=dt, device=frames.device) if "patches" in want else None
    image = torch.empty(n, 3, R, R, dtype=torch.float32, device=frames.device) if "image" in want else None
    f3 = hip.C.c_float * 3
    if orient:
        hip.check(hip.lib(dt).rv_frames_to_patches_oriented(hip.ptr(frames), _LAYOUTS[layout], fs, rs, n, H, W, orient, R, patch, f3(*mean), f3(*std),
                                                            hip.ptr(patches), kp, hip.ptr(image), hip.stream()), "rv_frames_to_patches_oriented")
        return patches, image
    hip.check(hip.lib(dt).rv_frames_to_patches(hip.ptr(frames), _LAYOUTS[layout], fs, rs, n, H, W, R, patch, f3(*mean), f3(*std), hip.ptr(patches), kp,
                                               hip.ptr(image), hip.stream()), "rv_frames_to_patches")
    return patches, image


def _frames_to_patches_packed(frames, R, patch, layout, mean, std, op_dtype, want, orient, pix_fmt):
    """``frames_to_patches(..., pix_fmt=...)``: every refusal comes before anything is read or launched."""
    if pix_fmt not in RGB_PIX_FMTS:
        raise ValueError(f"pix_fmt {pix_fmt!r}: one of {sorted(RGB_PIX_FMTS)} (packed 8-bit RGB)")
    pix, r, g, b = RGB_PIX_FMTS[pix_fmt]
    if layout not in (None, "NHWC"):
        raise ValueError(f"pix_fmt {pix_fmt!r} names the byte order of packed pixels [n,H,W,{pix}]: layout {layout!r} does not go with it")
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != pix:
        raise ValueError(f"{pix_fmt} frames come as a uint8 tensor [n,H,W,{pix}], got "
                         + (f"{frames.dtype} {tuple(frames.shape)}" if torch.is_tensor(frames) else type(frames).__name__))
    if not frames.is_cuda:
        raise hip.HipLibraryError("frames_to_patches needs a device tensor (got a CPU tensor); there is no CPU path")
    n, H, W = frames.shape[:3]
    ok = frames.stride(3) == 1 and frames.stride(2) == pix and frames.stride(1) >= pix * W and (n <= 1 or frames.stride(0) > 0)
    frames = frames if ok else frames.contiguous()
    fs, rs = (frames.stride(0) if n > 1 else frames.stride(1) * H), frames.stride(1)
    dt = hip.op_dtype(op_dtype)
    g_ = R // max(patch, 1)
    kp = (3 * patch * patch + 127) // 128 * 128
    patches = torch.empty(n * g_ * g_, kp, dtype=dt, device=frames.device) if "patches" in want else None
    image = torch.empty(n, 3, R, R, dtype=torch.float32, device=frames.device) if "image" in want else None
    f3 = hip.C.c_float * 3
    hip.check(hip.lib(dt).rv_frames_to_patches_packed(hip.ptr(frames), pix, r, g, b, fs, rs, n, H, W, orient, R, patch, f3(*mean), f3(*std), hip.ptr(patches), kp,
                                                      hip.ptr(image), hip.stream()), "rv_frames_to_patches_packed")
    return patches, image


_MATRICES = {"bt601": 0, "bt709": 1}
_CHROMA_LOCS = {"left": 0, "centre": 1}
_YUV_FORMATS = ("nv12", "nv21", "i420")


def _rows_of_samples(t, n, rows, cols, pix):
    """Can a plane [n,rows,cols] be passed by its strides?  Samples of a row ``pix`` bytes apart, rows and frames in ascending order (a dimension of
    extent 1 has no stride to speak of)."""
    return (cols == 1 or t.stride(2) == pix) and (rows == 1 or t.stride(1) >= pix * cols) and (n <= 1 or t.stride(0) > 0)


def _plane_strides(t, n, rows, cols, pix):
    """(frame stride, row stride) in bytes of a plane ``_rows_of_samples`` accepted."""
    rs = t.stride(1) if rows > 1 else pix * cols
    return (t.stride(0) if n > 1 else rs * rows), rs


def _yuv_surfaces_scattered(who, y, cb, cr, R, patch, depth, msb_aligned, subsampling, matrix, full_range, chroma_loc, hdr, orient, mean, std, op_dtype, want):
    """The YCbCr wrappers on lists of per-frame planes (y [H,W]; cb [h,w,2] with cr None, or cb and cr [h,w] each): one pointer triple per frame, the row
    strides of frame 0 for all (rv_yuv_surfaces_to_patches).  ``matrix`` / ``chroma_loc`` / ``subsampling`` arrive validated, as their codes.  Every
    ValueError comes before the library is touched."""
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
    sx, sy = subsampling
    if e.dim() != 2 or e.shape[0] % sy or e.shape[1] % sx:
        raise ValueError(f"{who}: Y planes in a list are [H,W] with H a multiple of {sy} and W of {sx}, got {tuple(e.shape)}")
    H, W = e.shape
    h, w, es = H // sy, W // sx, e.element_size()

    def rows(t, r, c, pix):   # can a plane [r,c] be passed by its strides?  samples of a row ``pix`` apart, rows in ascending order
        return (c == 1 or t.stride(1) == pix) and (r == 1 or t.stride(0) >= pix * c)

    if cr is None:
        if tuple(cb[0].shape) != (h, w, 2):
            raise ValueError(f"{who}: interleaved CbCr of frames {H} x {W} is [{h},{w},2] per frame, got {tuple(cb[0].shape)}")
        if not (cb[0].stride(2) == 1 and rows(cb[0], h, w, 2)):
            cb = [t.contiguous() for t in cb]
        cb, cr = [t[..., 0] for t in cb], [t[..., 1] for t in cb]
    elif tuple(cb[0].shape) != (h, w) or tuple(cr[0].shape) != (h, w):
        raise ValueError(f"{who}: Cb and Cr of frames {H} x {W} are [{h},{w}] per frame, got {tuple(cb[0].shape)} and {tuple(cr[0].shape)}")
    if not rows(e, H, W, 1):
        y = [t.contiguous() for t in y]
    if abs(cb[0].data_ptr() - cr[0].data_ptr()) == es and cb[0].stride() == cr[0].stride() and rows(cb[0], h, w, 2):
        c_pix = 2
    else:
        c_pix = 1
        if not (cb[0].stride() == cr[0].stride() and rows(cb[0], h, w, 1)):
            cb, cr = [t.contiguous() for t in cb], [t.contiguous() for t in cr]
    yrs = y[0].stride(0) if H > 1 else W
    crs = cb[0].stride(0) if h > 1 else c_pix * w
    _require_device(y + cb + cr, who)
    dt, kp, patches, image = _frame_outputs(n, R, patch, op_dtype, want, e.device)
    table = (hip.RvSurfacePlanes * n)(*[(a.data_ptr(), b.data_ptr(), c.data_ptr()) for a, b, c in zip(y, cb, cr)])
    s = hip.RvYuvSurface(None, None, None, 0, yrs * es, 0, crs * es, es, int(depth), int(bool(msb_aligned)), c_pix * es, sx, sy, n, H, W, matrix,
                         int(bool(full_range)), chroma_loc)
    f3 = hip.C.c_float * 3
    hip.check(hip.lib(dt).rv_yuv_surfaces_to_patches(hip.C.byref(s), table, None if hdr is None else hip.C.byref(hdr), orient, R, patch, f3(*mean), f3(*std),
                                                     hip.ptr(patches), kp, hip.ptr(image), hip.stream()), "rv_yuv_surfaces_to_patches")
    return patches, image


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
    orient = orientation(rotate, hflip, vflip)
    if isinstance(y, (list, tuple)):
        if matrix not in _MATRICES or chroma_loc not in _CHROMA_LOCS:
            raise ValueError(f"matrix {matrix!r} / chroma_loc {chroma_loc!r}: one of {sorted(_MATRICES)} / {sorted(_CHROMA_LOCS)}")
        if y and torch.is_tensor(y[0]) and y[0].dtype != torch.uint8:
            raise ValueError(f"yuv_to_patches takes uint8 planes, got {y[0].dtype}")
        return _yuv_surfaces_scattered("yuv_to_patches", y, cb, cr, R, patch, 8, False, (2, 2), _MATRICES[matrix], full_range, _CHROMA_LOCS[chroma_loc], None, orient,
                                       mean, std, op_dtype, want)
    for t in (y, cb) + (() if cr is None else (cr,)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise hip.HipLibraryError("yuv_to_patches needs device tensors (got a CPU tensor); there is no CPU path")
        if t.dtype != torch.uint8:
            raise hip.HipLibraryError(f"yuv_to_patches takes uint8 planes, got {t.dtype} {tuple(t.shape)}")
    if matrix not in _MATRICES or chroma_loc not in _CHROMA_LOCS:
        raise ValueError(f"matrix {matrix!r} / chroma_loc {chroma_loc!r}: one of {sorted(_MATRICES)} / {sorted(_CHROMA_LOCS)}")
    if y.dim() != 3 or y.shape[1] % 2 or y.shape[2] % 2:
        raise hip.HipLibraryError(f"yuv_to_patches takes a Y plane [n,H,W] with even H and W, got {tuple(y.shape)}")
    n, H, W = y.shape
    h2, w2 = H // 2, W // 2
    if cr is None:
        if tuple(cb.shape) != (n, h2, w2, 2):
            raise hip.HipLibraryError(f"interleaved CbCr of {n} frames {H} x {W} is [{n},{h2},{w2},2], got {tuple(cb.shape)}")
        if not (cb.stride(3) == 1 and _rows_of_samples(cb, n, h2, w2, 2)):
            cb = cb.contiguous()
        cb, cr = cb[..., 0], cb[..., 1]
    elif tuple(cb.shape) != (n, h2, w2) or tuple(cr.shape) != (n, h2, w2):
        raise hip.HipLibraryError(f"Cb and Cr of {n} frames {H} x {W} are [{n},{h2},{w2}] each, got {tuple(cb.shape)} and {tuple(cr.shape)}")
    if not _rows_of_samples(y, n, H, W, 1):
        y = y.contiguous()
    # cb, cr: [n,h2,w2] views from here on; one stride pair serves both planes
    if abs(cb.data_ptr() - cr.data_ptr()) == 1 and cb.stride() == cr.stride() and _rows_of_samples(cb, n, h2, w2, 2):
        c_pix = 2
    else:
        c_pix = 1
        if not (cb.stride() == cr.stride() and _rows_of_samples(cb, n, h2, w2, 1)):
            cb, cr = cb.contiguous(), cr.contiguous()
    yfs, yrs = _plane_strides(y, n, H, W, 1)
    cfs, crs = _plane_strides(cb, n, h2, w2, c_pix)
    dt = hip.op_dtype(op_dtype)
    g = R // max(patch, 1)
    kp = (3 * patch * patch + 127) // 128 * 128
    patches = torch.empty(n * g * g, kp, dtype=dt, device=y.device) if "patches" in want else None
    image = torch.empty(n, 3, R, R, dtype=torch.float32, device=y.device) if "image" in want else None
    f3 = hip.C.c_float * 3
    if orient:
        s = hip.RvYuvSurface(y.data_ptr(), cb.data_ptr(), cr.data_ptr(), yfs, yrs, cfs, crs, 1, 8, 0, c_pix, 2, 2, n, H, W, _MATRICES[matrix], int(bool(full_range)),
                             _CHROMA_LOCS[chroma_loc])
        hip.check(hip.lib(dt).rv_yuv_surface_to_patches_oriented(hip.C.byref(s), None, orient, R, patch, f3(*mean), f3(*std), hip.ptr(patches), kp, hip.ptr(image),
                                                                 hip.stream()), "rv_yuv_surface_to_patches_oriented")
        return patches, image
    hip.check(hip.lib(dt).rv_yuv_to_patches(hip.ptr(y), yfs, yrs, hip.ptr(cb), hip.ptr(cr), cfs, crs, c_pix, n, H, W, _MATRICES[matrix], int(bool(full_range)),
                                            _CHROMA_LOCS[chroma_loc], R, patch, f3(*mean), f3(*std), hip.ptr(patches), kp, hip.ptr(image), hip.stream()),
              "rv_yuv_to_patches")
    return patches, image


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
        raise ValueError(f"{fmt} frames of {H} x {W} come as a uint8 tensor [n,{H * 3 // 2},{W}], got "
                         + (f"{buf.dtype} {tuple(buf.shape)}" if torch.is_tensor(buf) else type(buf).__name__))
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


_SURFACE_MATRICES = {"bt601": 0, "bt709": 1, "bt2020": 2}
_SURFACE_LOCS = {"left": 0, "centre": 1, "topleft": 2}
_SUBSAMPLINGS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}
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
    orient = orientation(rotate, hflip, vflip)
    hdr = hdr_map(transfer, matrix, gamut, peak_nits, sdr_white_nits)
    if isinstance(y, (list, tuple)):
        if matrix not in _SURFACE_MATRICES or chroma_loc not in _SURFACE_LOCS or subsampling not in _SUBSAMPLINGS:
            raise ValueError(f"matrix {matrix!r} / chroma_loc {chroma_loc!r} / subsampling {subsampling!r}: one of {sorted(_SURFACE_MATRICES)} / "
                             f"{sorted(_SURFACE_LOCS)} / {sorted(_SUBSAMPLINGS)}")
        return _yuv_surfaces_scattered("yuv_surface_to_patches", y, cb, cr, R, patch, depth, msb_aligned, _SUBSAMPLINGS[subsampling], _SURFACE_MATRICES[matrix],
                                       full_range, _SURFACE_LOCS[chroma_loc], hdr, orient, mean, std, op_dtype, want)
    for t in (y, cb) + (() if cr is None else (cr,)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise hip.HipLibraryError("yuv_surface_to_patches needs device tensors (got a CPU tensor); there is no CPU path")
        if t.dtype not in (torch.uint8, torch.uint16) or t.dtype != y.dtype:
            raise hip.HipLibraryError(f"yuv_surface_to_patches takes planes of one dtype, uint8 or uint16, got {t.dtype} {tuple(t.shape)}")
    if matrix not in _SURFACE_MATRICES or chroma_loc not in _SURFACE_LOCS or subsampling not in _SUBSAMPLINGS:
        raise ValueError(f"matrix {matrix!r} / chroma_loc {chroma_loc!r} / subsampling {subsampling!r}: one of {sorted(_SURFACE_MATRICES)} / "
                         f"{sorted(_SURFACE_LOCS)} / {sorted(_SUBSAMPLINGS)}")
    sx, sy = _SUBSAMPLINGS[subsampling]
    if y.dim() != 3 or y.shape[1] % sy or y.shape[2] % sx:
        raise hip.HipLibraryError(f"yuv_surface_to_patches takes a Y plane [n,H,W] with H a multiple of {sy} and W of {sx} ({subsampling}), got {tuple(y.shape)}")
    n, H, W = y.shape
    h, w, es = H // sy, W // sx, y.element_size()
    if cr is None:
        if tuple(cb.shape) != (n, h, w, 2):
            raise hip.HipLibraryError(f"interleaved CbCr of {n} frames {H} x {W} ({subsampling}) is [{n},{h},{w},2], got {tuple(cb.shape)}")
        if not (cb.stride(3) == 1 and _rows_of_samples(cb, n, h, w, 2)):
            cb = cb.contiguous()
        cb, cr = cb[..., 0], cb[..., 1]
    elif tuple(cb.shape) != (n, h, w) or tuple(cr.shape) != (n, h, w):
        raise hip.HipLibraryError(f"Cb and Cr of {n} frames {H} x {W} ({subsampling}) are [{n},{h},{w}] each, got {tuple(cb.shape)} and {tuple(cr.shape)}")
    if not _rows_of_samples(y, n, H, W, 1):
        y = y.contiguous()
    # cb, cr: [n,h,w] views from here on; one stride pair serves both planes.  Strides are in samples up to the call.
    if abs(cb.data_ptr() - cr.data_ptr()) == es and cb.stride() == cr.stride() and _rows_of_samples(cb, n, h, w, 2):
        c_pix = 2
    else:
        c_pix = 1
        if not (cb.stride() == cr.stride() and _rows_of_samples(cb, n, h, w, 1)):
            cb, cr = cb.contiguous(), cr.contiguous()
    yfs, yrs = _plane_strides(y, n, H, W, 1)
    cfs, crs = _plane_strides(cb, n, h, w, c_pix)
    dt = hip.op_dtype(op_dtype)
    g = R // max(patch, 1)
    kp = (3 * patch * patch + 127) // 128 * 128
    patches = torch.empty(n * g * g, kp, dtype=dt, device=y.device) if "patches" in want else None
    image = torch.empty(n, 3, R, R, dtype=torch.float32, device=y.device) if "image" in want else None
    s = hip.RvYuvSurface(y.data_ptr(), cb.data_ptr(), cr.data_ptr(), yfs * es, yrs * es, cfs * es, crs * es, es, int(depth), int(bool(msb_aligned)), c_pix * es,
                         sx, sy, n, H, W, _SURFACE_MATRICES[matrix], int(bool(full_range)), _SURFACE_LOCS[chroma_loc])
    f3 = hip.C.c_float * 3
    if orient:
        hip.check(hip.lib(dt).rv_yuv_surface_to_patches_oriented(hip.C.byref(s), None if hdr is None else hip.C.byref(hdr), orient, R, patch, f3(*mean), f3(*std),
                                                                 hip.ptr(patches), kp, hip.ptr(image), hip.stream()), "rv_yuv_surface_to_patches_oriented")
        return patches, image
    if hdr is not None:
        hip.check(hip.lib(dt).rv_yuv_surface_to_patches_hdr(hip.C.byref(s), hip.C.byref(hdr), R, patch, f3(*mean), f3(*std), hip.ptr(patches), kp,
                                                            hip.ptr(image), hip.stream()), "rv_yuv_surface_to_patches_hdr")
        return patches, image
    hip.check(hip.lib(dt).rv_yuv_surface_to_patches(hip.C.byref(s), R, patch, f3(*mean), f3(*std), hip.ptr(patches), kp, hip.ptr(image), hip.stream()),
              "rv_yuv_surface_to_patches")
    return patches, image


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
        raise ValueError(f"{pix_fmt} frames of {H} x {W} come as a uint8 tensor [n,{fb}], got "
                         + (f"{buf.dtype} {tuple(buf.shape)}" if torch.is_tensor(buf) else type(buf).__name__))
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


def _packed_to_patches_scattered(bufs, H, W, pix_fmt, R, patch, matrix, full_range, chroma_loc, hdr, orient, mean, std, op_dtype, want):
    """``packed_to_patches`` on a list of per-frame tensors: one base pointer per frame, the row stride of frame 0 for all (rv_packed_surfaces_to_patches)."""
    who = "packed_to_patches"
    unit, ppu, sb, oy, ocb, ocr, depth, msb = _packed_fmt(pix_fmt)
    rb, fb = packed_frame_bytes(1, W, pix_fmt), packed_frame_bytes(H, W, pix_fmt)
    bufs = _frame_list(bufs, who)
    e = bufs[0]
    if e.dtype != torch.uint8 or not ((e.dim() == 2 and tuple(e.shape) == (H, rb)) or (e.dim() == 1 and e.shape[0] == fb)):
        raise ValueError(f"{pix_fmt} frames of {H} x {W} in a list come as uint8 tensors [{H},{rb}] or [{fb}], got {e.dtype} {tuple(e.shape)}")
    if e.dim() == 1:
        if e.stride(0) != 1:
            bufs = [t.contiguous() for t in bufs]
        bufs = [t.as_strided((H, rb), (rb, 1), t.storage_offset()) for t in bufs]
    elif not (e.stride(1) == 1 and (H == 1 or e.stride(0) >= rb)):
        bufs = [t.contiguous() for t in bufs]
    rs = bufs[0].stride(0) if H > 1 else rb
    for i, t in enumerate(bufs):
        if sb > 1 and (t.storage_offset() % sb or rs % sb or (t.is_cuda and t.data_ptr() % sb)):
            raise ValueError(f"{pix_fmt}: {8 * sb}-bit words must lie at multiples of {sb} bytes (frame {i}: offset {t.storage_offset()}, row stride {rs})")
    _require_device(bufs, who)
    n = len(bufs)
    dt, kp, patches, image = _frame_outputs(n, R, patch, op_dtype, want, e.device)
    table = (hip.C.c_void_p * n)(*[t.data_ptr() for t in bufs])
    s = hip.RvPackedSurface(None, 0, rs, unit, ppu, sb, oy, ocb, ocr, depth, int(msb), n, H, W, matrix, int(bool(full_range)), chroma_loc)
    f3 = hip.C.c_float * 3
    hip.check(hip.lib(dt).rv_packed_surfaces_to_patches(hip.C.byref(s), table, None if hdr is None else hip.C.byref(hdr), orient, R, patch, f3(*mean), f3(*std),
                                                        hip.ptr(patches), kp, hip.ptr(image), hip.stream()), "rv_packed_surfaces_to_patches")
    return patches, image


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
    unit, ppu, sb, oy, ocb, ocr, depth, msb = _packed_fmt(pix_fmt)
    orient = orientation(rotate, hflip, vflip)
    hdr = hdr_map(transfer, matrix, gamut, peak_nits, sdr_white_nits)
    if matrix not in _SURFACE_MATRICES or chroma_loc not in _SURFACE_LOCS:
        raise ValueError(f"matrix {matrix!r} / chroma_loc {chroma_loc!r}: one of {sorted(_SURFACE_MATRICES)} / {sorted(_SURFACE_LOCS)}")
    rb, fb = packed_frame_bytes(1, W, pix_fmt), packed_frame_bytes(H, W, pix_fmt)
    if isinstance(buf, (list, tuple)):
        return _packed_to_patches_scattered(buf, H, W, pix_fmt, R, patch, _SURFACE_MATRICES[matrix], full_range, _SURFACE_LOCS[chroma_loc], hdr, orient, mean, std,
                                            op_dtype, want)
    if not torch.is_tensor(buf) or buf.dtype != torch.uint8 or not ((buf.dim() == 3 and tuple(buf.shape[1:]) == (H, rb)) or (buf.dim() == 2 and buf.shape[1] == fb)):
        raise ValueError(f"{pix_fmt} frames of {H} x {W} come as a uint8 tensor [n,{H},{rb}] or [n,{fb}], got "
                         + (f"{buf.dtype} {tuple(buf.shape)}" if torch.is_tensor(buf) else type(buf).__name__))
    n = buf.shape[0]
    if buf.dim() == 2:
        if buf.stride(1) != 1:
            buf = buf.contiguous()
        buf = buf.as_strided((n, H, rb), (buf.stride(0), rb, 1), buf.storage_offset())
    elif not (buf.stride(2) == 1 and (H == 1 or buf.stride(1) >= rb) and (n <= 1 or buf.stride(0) > 0)):
        buf = buf.contiguous()
    rs = buf.stride(1) if H > 1 else rb
    fs = buf.stride(0) if n > 1 else rs * H
    if sb > 1 and (buf.storage_offset() % sb or rs % sb or fs % sb or (buf.is_cuda and buf.data_ptr() % sb)):
        raise ValueError(f"{pix_fmt}: {8 * sb}-bit words must lie at multiples of {sb} bytes (offset {buf.storage_offset()}, row stride {rs}, frame stride {fs})")
    if not buf.is_cuda:
        raise hip.HipLibraryError("packed_to_patches needs a device tensor (got a CPU tensor); there is no CPU path")
    dt = hip.op_dtype(op_dtype)
    g = R // max(patch, 1)
    kp = (3 * patch * patch + 127) // 128 * 128
    patches = torch.empty(n * g * g, kp, dtype=dt, device=buf.device) if "patches" in want else None
    image = torch.empty(n, 3, R, R, dtype=torch.float32, device=buf.device) if "image" in want else None
    s = hip.RvPackedSurface(buf.data_ptr(), fs, rs, unit, ppu, sb, oy, ocb, ocr, depth, int(msb), n, H, W, _SURFACE_MATRICES[matrix], int(bool(full_range)),
                            _SURFACE_LOCS[chroma_loc])
    f3 = hip.C.c_float * 3
    hip.check(hip.lib(dt).rv_packed_to_patches(hip.C.byref(s), None if hdr is None else hip.C.byref(hdr), orient, R, patch, f3(*mean), f3(*std), hip.ptr(patches), kp,
                                               hip.ptr(image), hip.stream()), "rv_packed_to_patches")
    return patches, image


def h2d(t, device, dtype=None):
    """Host -> device without stalling the host: a pageable ``.to(device)`` blocks until everything queued before it has
    run (the launch queue then runs dry after every upload); a pinned, non-blocking copy just joins the stream."""
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if t.device.type == "cpu" and torch.device(device).type == "cuda":
        if dtype is not None:
            t = t.to(dtype)
        return t.contiguous().pin_memory().to(device, non_blocking=True)
    return t.to(device=device, dtype=dtype) if dtype is not None else t.to(device)


def sample(logits, uniforms=None, do_sample=False, temperature=1.0, top_k=50, top_p=1.0, ctx=None):
    """-> dict(tokens i32 [B], entropy_proc, entropy_raw f32 [B], topk_idx i32 [B,64], topk_val f32 [B,64], n_keep i32 [B], threshold f32 [B]).
    ``top_k`` in [1, 64]; 0 / None = no top-k filter (HF: filter disabled) and ``top_k`` > 64 (kept by threshold: scores below the top_k-th largest go): no candidate list then - the kept set is {processed score >=
    threshold}.  (The kernel writes every output element, so the buffers are plain ``empty`` allocations.)"""
    top_k = 0 if top_k is None else top_k
    B, V = logits.shape
    dev = logits.device
    o = dict(tokens=torch.empty(B, dtype=torch.int32, device=dev), entropy_proc=torch.empty(B, dtype=torch.float32, device=dev),
             entropy_raw=torch.empty(B, dtype=torch.float32, device=dev),
             topk_idx=torch.empty((B, hip.TOPK_CAP), dtype=torch.int32, device=dev),
             topk_val=torch.empty((B, hip.TOPK_CAP), dtype=torch.float32, device=dev),
             n_keep=torch.empty(B, dtype=torch.int32, device=dev), threshold=torch.empty(B, dtype=torch.float32, device=dev))
    hip.check((ctx.lib if ctx is not None else hip.lib()).rv_sample(hip.ctx_ptr(ctx), hip.ptr(_c(logits)), B, V, hip.ptr(uniforms), int(do_sample), float(temperature), int(top_k),
                                  float(top_p if top_p is not None else 1.0), hip.ptr(o["tokens"]), hip.ptr(o["entropy_proc"]),
                                  hip.ptr(o["entropy_raw"]), hip.ptr(o["topk_idx"]), hip.ptr(o["topk_val"]), hip.ptr(o["n_keep"]), hip.ptr(o["threshold"]),
                                  hip.stream()), "rv_sample")
    return o


def entropy_stats(logits):
    """get_entropy_statistics on the device: logits f32 [B,G,V] -> [B,4] (max, min, mean, std)."""
    B, G, V = logits.shape
    out = torch.empty(B, 4, dtype=torch.float32, device=logits.device)
    hip.check(hip.lib().rv_entropy_stats(hip.ptr(_c(logits.float())), B, G, V, hip.ptr(out), hip.stream()), "rv_entropy_stats")
    return out


def topk_cosine(feat, q_cls, k=3):
    """feat [n,T,d] (bf16 or f32), q_cls [d] -> f32 [n]: column-normalise over frames, sum of the k best <f_t, q> (k<=0: mean)."""
    n, T, d = feat.shape
    out = torch.empty(n, dtype=torch.float32, device=feat.device)
    hip.check(hip.lib(None if feat.dtype == torch.float32 else feat).rv_topk_cosine(hip.ptr(_c(feat)), hip.dtype_code(feat), hip.ptr(_c(q_cls.float())), n, T, d, k, hip.ptr(out),
                                       hip.stream()), "rv_topk_cosine")
    return out


def topk_pool(text_embeds, video_embeds, k, return_index=False):
    """``_topk_pooling`` (similarity.py:71-94) on the device: text [Nt,d], video [Nv,T,d] (bf16 or f32) -> f32 [Nv,Nt,d], the SUM
    of each video's k frames most similar to each text."""
    Nv, T, d = video_embeds.shape
    Nt = text_embeds.shape[0]
    out = torch.empty(Nv, Nt, d, dtype=torch.float32, device=video_embeds.device)
    idx = torch.empty(Nv, Nt, k, dtype=torch.int32, device=video_embeds.device) if return_index else None
    hip.check(hip.lib(None if video_embeds.dtype == torch.float32 else video_embeds).rv_topk_pool(hip.ptr(_c(video_embeds)), hip.dtype_code(video_embeds), hip.ptr(_c(text_embeds.float())), Nv, T, d,
                                     Nt, int(k), hip.ptr(out), hip.ptr(idx), hip.stream()), "rv_topk_pool")
    return (out, idx) if return_index else out


def _score_lib(t):
    return hip.lib(None if t.dtype == torch.float32 else t)


def frame_cosine(text, video):
    """The per-frame cosine row of ``forward_clip_matching`` (similarity.py:36, :61-64): text f32 [B,d], video [B,L,d] (16-bit operands or f32) -> f32 [B,L],
    ``<f_l, t_b> / (|f_l| |t_b|)``; a zero frame or a zero text gives NaN as the reference's divisions do."""
    if video.dim() != 3 or text.dim() != 2 or text.shape != (video.shape[0], video.shape[2]):
        raise ValueError(f"frame_cosine: text {tuple(text.shape)} / video {tuple(video.shape)}")
    B, L, d = video.shape
    out = torch.empty(B, L, dtype=torch.float32, device=video.device)
    hip.check(_score_lib(video).rv_frame_cosine(hip.ptr(_c(video)), hip.dtype_code(video), hip.ptr(_c(text.float())), B, L, d, hip.ptr(out), hip.stream()),
              "rv_frame_cosine")
    return out


SPAN_POOLINGS = {"topk": 0, "attention": 1}


def span_scores(sims, spans, mask, k=3, pooling="topk", temperature=0.01, return_windows=False):
    """sims f32 [B,L], spans [B,N,2] as (centre, width), mask [B,L] -> scores f32 [B,N] (and the windows i32 [B,N,2] as (lo, hi) of ``range(L)[start:end]``):
    the reference's window rule (similarity.py:52-60) and, per window, the sum of its min(k, len) largest sims (``pooling="topk"``) or
    ``sum softmax(s / temperature) s`` (``"attention"``).  Nothing comes back to the host."""
    if pooling not in SPAN_POOLINGS:
        raise ValueError(f"span_scores: pooling={pooling!r} (expected one of {sorted(SPAN_POOLINGS)})")
    if sims.dim() != 2 or spans.dim() != 3 or spans.shape[0] != sims.shape[0] or spans.shape[2] != 2 or mask.shape != sims.shape:
        raise ValueError(f"span_scores: sims {tuple(sims.shape)} / spans {tuple(spans.shape)} / mask {tuple(mask.shape)}")
    if sims.dtype != torch.float32:
        raise ValueError(f"span_scores: sims must be float32 (got {sims.dtype})")
    B, L = sims.shape
    N = spans.shape[1]
    scores = torch.empty(B, N, dtype=torch.float32, device=sims.device)
    win = torch.empty(B, N, 2, dtype=torch.int32, device=sims.device) if return_windows else None
    if N > 0:
        hip.check(hip.lib().rv_span_scores(hip.ptr(_c(sims)), hip.ptr(_c(spans.float())), hip.ptr(_c(mask.float())), B, L, N, SPAN_POOLINGS[pooling], int(k),
                                           float(temperature), hip.ptr(scores), hip.ptr(win), hip.stream()), "rv_span_scores")
    return (scores, win) if return_windows else scores


def attn_pool(text_embeds, video_embeds, temperature):
    """``_attention_pooling`` (similarity.py:96-113) on the device: text [Nt,d], video [Nv,T,d] (16-bit operands or f32) -> f32 [Nv,Nt,d] =
    ``sum_t softmax_t(<f_t, text_j> / temperature) f_t``."""
    if text_embeds.dim() != 2 or video_embeds.dim() != 3 or text_embeds.shape[1] != video_embeds.shape[2]:
        raise ValueError(f"attn_pool: text {tuple(text_embeds.shape)} / video {tuple(video_embeds.shape)}")
    Nv, T, d = video_embeds.shape
    Nt = text_embeds.shape[0]
    out = torch.empty(Nv, Nt, d, dtype=torch.float32, device=video_embeds.device)
    hip.check(_score_lib(video_embeds).rv_attn_pool(hip.ptr(_c(video_embeds)), hip.dtype_code(video_embeds), hip.ptr(_c(text_embeds.float())), Nv, T, d, Nt,
                                                    float(temperature), hip.ptr(out), hip.stream()), "rv_attn_pool")
    return out
