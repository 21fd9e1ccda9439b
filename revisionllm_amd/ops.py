"""Functional wrappers over the C ABI building blocks (used by the engine, the scoring helpers and the tests).

Every function takes / returns torch DEVICE tensors and enqueues on torch's current stream.
"""
import collections
import math
import numbers
import struct

import torch

from . import hip
# the CLIP front end (frames / surfaces -> patches) lives in ``frontend``; its public names stay reachable here
from .frontend import (CLIP_MEAN, CLIP_STD, PACKED_PIX_FMTS, PIX_FMTS, RGB_PIX_FMTS, frames_to_patches, hdr_map, orientation, packed_frame_bytes,  # noqa: F401
                       packed_to_patches, split_yuv, split_yuv420, yuv_frame_bytes, yuv_surface_to_patches, yuv_to_patches)
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


def frame_cosine_multi(text, video):
    """``frame_cosine`` for Q texts per video: text f32 [B,Q,d], video [B,L,d] (16-bit operands or f32, passed as it is when contiguous) -> f32 [B,Q,L],
    ``<f_bl, t_bq> / (|f_bl| |t_bq|)`` with the features read once for all Q texts (``rv_frame_cosine_multi``: f32-input MFMA).  A query's row does not
    depend on Q, on its slot or on the other texts.  A zero text gives a NaN row, a zero frame a NaN column.  No synchronisation."""
    if video.dim() != 3 or text.dim() != 3 or text.shape[0] != video.shape[0] or text.shape[2] != video.shape[2]:
        raise ValueError(f"frame_cosine_multi: text {tuple(text.shape)} / video {tuple(video.shape)} (expected [B, Q, d] and [B, L, d])")
    B, L, d = video.shape
    Q = text.shape[1]
    text = _c(text.float())
    unit = torch.empty_like(text)                       # the kernel's workspace: text / |text|
    out = torch.empty(B, Q, L, dtype=torch.float32, device=video.device)
    hip.check(_score_lib(video).rv_frame_cosine_multi(hip.ptr(_c(video)), hip.dtype_code(video), hip.ptr(text), B, Q, L, d, hip.ptr(unit), hip.ptr(out),
                                                      hip.stream()), "rv_frame_cosine_multi")
    return out


def span_scores_multi(sims, spans, mask, k=3, pooling="topk", temperature=0.01, return_windows=False):
    """``span_scores`` for Q queries per video: sims f32 [B,Q,L], spans [B,Q,N,2] (each query's own (centre, width) proposals), mask [B,L] (one duration
    per video) -> scores f32 [B,Q,N] (and the windows i32 [B,Q,N,2]).  The kernel of ``span_scores``: each (b, q) row equals ``span_scores`` on that
    row bit for bit.  No synchronisation."""
    if pooling not in SPAN_POOLINGS:
        raise ValueError(f"span_scores_multi: pooling={pooling!r} (expected one of {sorted(SPAN_POOLINGS)})")
    if (sims.dim() != 3 or spans.dim() != 4 or spans.shape[:2] != sims.shape[:2] or spans.shape[3] != 2
            or mask.shape != (sims.shape[0], sims.shape[2])):
        raise ValueError(f"span_scores_multi: sims {tuple(sims.shape)} / spans {tuple(spans.shape)} / mask {tuple(mask.shape)}")
    if sims.dtype != torch.float32:
        raise ValueError(f"span_scores_multi: sims must be float32 (got {sims.dtype})")
    B, Q, L = sims.shape
    N = spans.shape[2]
    scores = torch.empty(B, Q, N, dtype=torch.float32, device=sims.device)
    win = torch.empty(B, Q, N, 2, dtype=torch.int32, device=sims.device) if return_windows else None
    if N > 0:
        hip.check(hip.lib().rv_span_scores_multi(hip.ptr(_c(sims)), hip.ptr(_c(spans.float())), hip.ptr(_c(mask.float())), B, Q, L, N,
                                                 SPAN_POOLINGS[pooling], int(k), float(temperature), hip.ptr(scores), hip.ptr(win), hip.stream()),
                  "rv_span_scores_multi")
    return (scores, win) if return_windows else scores


SPAN_FORMS = {"xx": 0, "cxw": 1}
SPAN_RANK_MAX = 2048
HIT_IOU = (0.1, 0.3, 0.5, 0.7, 0.9)
SpanRank = collections.namedtuple("SpanRank", "keep n_keep keep_iou first_hit order")
_hit_tables = collections.OrderedDict()
_HIT_TABLES_MAX = 16


def _hit_table(hit_iou, device):
    """The thresholds as an f32 device vector, uploaded once per (values, device, stream) and kept for the last 16 such keys: a ranking call then queues no
    copy.  The stream is part of the key because the upload is ordered on the stream that was current when it was queued: a call on another stream gets a
    table of its own, uploaded on that stream, instead of reading this one without ordering."""
    key = (hit_iou, str(device), torch.cuda.current_stream(device).cuda_stream)
    table = _hit_tables.get(key)
    if table is None:
        table = _hit_tables[key] = h2d(torch.tensor(hit_iou, dtype=torch.float32), device)
        while len(_hit_tables) > _HIT_TABLES_MAX:
            _hit_tables.popitem(last=False)        # (the allocator keeps a freed block ordered behind the work queued on its stream)
    else:
        _hit_tables.move_to_end(key)
    return table


def span_rank_keywords(who, top, nms_iou, hit_iou):
    """The keyword refusals of ``span_rank`` (raised before any device is looked for) -> (nms_iou as float, hit_iou as a tuple of floats)."""
    if top is not None and not (isinstance(top, numbers.Integral) and not isinstance(top, bool) and top >= 1):
        raise ValueError(f"{who}: top={top!r} must be a positive integer or None")
    try:
        nms_iou, hit_iou = float(nms_iou), tuple(float(h) for h in hit_iou)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: nms_iou={nms_iou!r} must be a number and hit_iou={hit_iou!r} a sequence of numbers") from None
    if not (math.isfinite(nms_iou) and nms_iou >= 0.0):
        raise ValueError(f"{who}: nms_iou={nms_iou} must be finite and >= 0")
    if len(hit_iou) > 16:
        raise ValueError(f"{who}: {len(hit_iou)} thresholds in hit_iou (at most 16)")
    return nms_iou, hit_iou


def span_rank(scores, spans, top=None, nms_iou=1.0, form="cxw", gt=None, hit_iou=HIT_IOU, return_order=False):
    """Rank scored proposals on the device (``rv_span_rank``): scores [R,N] or [B,Q,N], spans [...,N,2] as (centre, width) (``form="cxw"``) or (start, end)
    (``"xx"``), gt [...,2] as (start, end) or None -> SpanRank(keep i32 [...,top], n_keep i32 [...], keep_iou f32 [...,top], first_hit i32 [...,T], order
    i32 [...,N]); parts not asked for are None (keep_iou and first_hit need ``gt``, order ``return_order``).  Descending score, ties to the smaller index,
    NaN last; greedy NMS at ``inter > nms_iou * union`` (1.0: none); ``keep`` is padded with -1, ``keep_iou`` with 0; ``first_hit[..., t]`` is the first
    kept place whose IoU with gt exceeds ``hit_iou[t]``, or -1.  ``top=None`` means N, a larger ``top`` is N.  One launch, no synchronisation, no host copy."""
    if form not in SPAN_FORMS:
        raise ValueError(f"span_rank: form={form!r} (expected one of {sorted(SPAN_FORMS)})")
    if not torch.is_tensor(scores) or not torch.is_tensor(spans) or (gt is not None and not torch.is_tensor(gt)):
        raise ValueError("span_rank: scores, spans and gt must be tensors")
    if scores.dim() not in (2, 3) or spans.shape != scores.shape + (2,):
        raise ValueError(f"span_rank: scores {tuple(scores.shape)} / spans {tuple(spans.shape)} (expected [R, N] or [B, Q, N] and [..., N, 2])")
    if gt is not None and gt.shape != scores.shape[:-1] + (2,):
        raise ValueError(f"span_rank: gt {tuple(gt.shape)} for scores {tuple(scores.shape)} (expected [..., 2] rows of (start, end))")
    if scores.dtype != torch.float32:
        raise ValueError(f"span_rank: scores must be float32 (got {scores.dtype})")
    for name, t in (("spans", spans), ("gt", gt)):
        if t is not None and not t.dtype.is_floating_point:
            raise ValueError(f"span_rank: {name} must be a floating-point tensor (got {t.dtype})")
    lead, N = tuple(scores.shape[:-1]), scores.shape[-1]
    if N > SPAN_RANK_MAX:
        raise ValueError(f"span_rank: N={N} proposals per row (at most {SPAN_RANK_MAX})")
    nms_iou, hit_iou = span_rank_keywords("span_rank", top, nms_iou, hit_iou if gt is not None else ())
    top = N if top is None else min(int(top), N)
    T, dev = len(hit_iou), scores.device
    R = math.prod(lead)
    keep = torch.empty(lead + (top,), dtype=torch.int32, device=dev)
    n_keep = torch.empty(lead, dtype=torch.int32, device=dev)
    keep_iou = torch.empty(lead + (top,), dtype=torch.float32, device=dev) if gt is not None else None
    first_hit = torch.empty(lead + (T,), dtype=torch.int32, device=dev) if gt is not None else None
    order = torch.empty(lead + (N,), dtype=torch.int32, device=dev) if return_order else None
    if N > 0 and R > 0:
        hip.check(hip.lib().rv_span_rank(hip.ptr(_c(scores)), hip.ptr(_c(spans.float())), SPAN_FORMS[form], R, N, top, nms_iou,
                                         hip.ptr(_c(gt.float())) if gt is not None else None, hip.ptr(_hit_table(hit_iou, dev)) if T else None, T,
                                         hip.ptr(order), hip.ptr(keep), hip.ptr(n_keep), hip.ptr(keep_iou), hip.ptr(first_hit if T else None), hip.stream()),
                  "rv_span_rank")
    elif R > 0:                                          # no proposals: nothing kept, no hit (no launch)
        n_keep.zero_()
        if first_hit is not None:
            first_hit.fill_(-1)
    return SpanRank(keep, n_keep, keep_iou, first_hit, order)


SPAN_PROPOSE_MAX_LEVELS = 8
SPAN_PROPOSE_MAX_FRAMES = 1 << 20
SPAN_PROPOSE_LEVELS = (0.5, 0.6, 0.7, 0.8, 0.9)
SpanProposals = collections.namedtuple("SpanProposals", "spans n_spans n_found windows smoothed")


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _f32(v):
    """A Python float rounded to float32 (inf when it is out of range)."""
    try:
        return struct.unpack("f", struct.pack("f", v))[0]
    except OverflowError:
        return math.copysign(math.inf, v)


def span_propose_keywords(who, levels=SPAN_PROPOSE_LEVELS, relative=True, smooth=1, gap=0, min_len=1, max_len=None, max_spans=256):
    """The keyword refusals of ``span_propose`` (raised before any device is looked for) -> (levels as a tuple of floats, relative as 0 / 1, smooth, gap,
    min_len, max_len with None as 0, max_spans) as ``rv_span_propose`` takes them."""
    try:
        levels = tuple(float(v) for v in levels)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: levels={levels!r} must be a sequence of numbers") from None
    if not 1 <= len(levels) <= SPAN_PROPOSE_MAX_LEVELS:
        raise ValueError(f"{who}: {len(levels)} levels (1 to {SPAN_PROPOSE_MAX_LEVELS})")
    if not (isinstance(relative, (bool, numbers.Integral)) and relative in (0, 1)):
        raise ValueError(f"{who}: relative={relative!r} must be True or False")
    as_f32 = [_f32(v) for v in levels]                   # what the kernel compares
    for i, v in enumerate(as_f32):
        if not math.isfinite(v):
            raise ValueError(f"{who}: level {levels[i]} is not a finite float32")
        if i and not v > as_f32[i - 1]:
            raise ValueError(f"{who}: levels={levels} must be strictly ascending (as float32)")
        if relative and not 0.0 <= v < 1.0:
            raise ValueError(f"{who}: relative level {levels[i]} outside [0, 1)")
    if not (_is_int(smooth) and 1 <= smooth <= 65 and smooth % 2 == 1):
        raise ValueError(f"{who}: smooth={smooth!r} must be an odd integer in [1, 65]")
    if not (_is_int(gap) and 0 <= gap <= 63):
        raise ValueError(f"{who}: gap={gap!r} must be an integer in [0, 63]")
    if not (_is_int(min_len) and 1 <= min_len < 2 ** 31):
        raise ValueError(f"{who}: min_len={min_len!r} must be a positive integer")
    if max_len is not None and not (_is_int(max_len) and min_len <= max_len < 2 ** 31):
        raise ValueError(f"{who}: max_len={max_len!r} must be None or an integer >= min_len={min_len}")
    if not (_is_int(max_spans) and 1 <= max_spans <= SPAN_RANK_MAX):
        raise ValueError(f"{who}: max_spans={max_spans!r} must be an integer in [1, {SPAN_RANK_MAX}]")
    return tuple(as_f32), int(bool(relative)), int(smooth), int(gap), int(min_len), 0 if max_len is None else int(max_len), int(max_spans)


def span_propose_shapes(who, sims, mask):
    """The tensor refusals of ``span_propose`` -> (leading shape, R, rows per mask row, L)."""
    if not torch.is_tensor(sims) or not torch.is_tensor(mask):
        raise ValueError(f"{who}: sims and mask must be tensors")
    if sims.dim() not in (2, 3) or mask.dim() != 2 or mask.shape[-1] != sims.shape[-1]:
        raise ValueError(f"{who}: sims {tuple(sims.shape)} / mask {tuple(mask.shape)} (expected [R, L] or [B, Q, L] and [R, L] / [B, L])")
    lead, L = tuple(sims.shape[:-1]), sims.shape[-1]
    R, M = math.prod(lead), mask.shape[0]
    if min(R, L, M) < 1 or (sims.dim() == 3 and M != lead[0]) or R % M != 0:
        raise ValueError(f"{who}: sims {tuple(sims.shape)} / mask {tuple(mask.shape)} (one mask row per video: a whole number of rows of sims for each)")
    if L > SPAN_PROPOSE_MAX_FRAMES:
        raise ValueError(f"{who}: L={L} frames (at most {SPAN_PROPOSE_MAX_FRAMES})")
    if not sims.dtype.is_floating_point:
        raise ValueError(f"{who}: sims must be a floating-point tensor (got {sims.dtype})")
    if mask.dtype.is_complex:
        raise ValueError(f"{who}: mask must be bool, integer or floating point (got {mask.dtype})")
    return lead, R, R // M, L


def span_propose(sims, mask, *, levels=SPAN_PROPOSE_LEVELS, relative=True, smooth=1, gap=0, min_len=1, max_len=None, max_spans=256, return_windows=False,
                 return_smoothed=False):
    """Candidate spans from similarity rows on the device (``rv_span_propose``): sims f32 [R,L] or [B,Q,L] (``frame_cosine`` / ``frame_cosine_multi``'s
    rows), mask [R,L] / [B,L] of any bool, integer or float dtype (its row sum is the duration; with fewer rows than sims each serves a whole number of
    consecutive rows) -> SpanProposals(spans f32 [...,max_spans,2] as (centre, width) with NaN padding, n_spans i32 [...], n_found i32 [...], windows i32
    [...,max_spans,2] with (-1, -1) padding, smoothed f32 [...,L]); ``windows`` and ``smoothed`` are None unless asked for, and ``smoothed`` is written
    inside each row's duration only (NaN elsewhere).  The row is box-smoothed over ``smooth`` frames and thresholded at every level (``relative``: a
    fraction of the way from the row's smallest to its largest value); a maximal stretch above a threshold, gaps of at most ``gap`` frames closed, is a
    span if its length lies in [min_len, max_len] and the next level has no identical one.  Highest level first, then ascending start;
    ``n_found > n_spans`` shows that ``max_spans`` cut the list.  One launch (a mask that is not f32 adds a cast kernel, ``return_smoothed`` a fill), no
    synchronisation, no host copy.  The full rule stands in include/revision_hip.h."""
    who = "span_propose"
    kw = span_propose_keywords(who, levels, relative, smooth, gap, min_len, max_len, max_spans)
    lead, R, rpm, L = span_propose_shapes(who, sims, mask)
    if sims.dtype != torch.float32:
        raise ValueError(f"{who}: sims must be float32 (got {sims.dtype})")
    lv, relative, smooth, gap, min_len, max_len, N = kw
    dev = sims.device
    spans = torch.empty(lead + (N, 2), dtype=torch.float32, device=dev)
    n_spans = torch.empty(lead, dtype=torch.int32, device=dev)
    n_found = torch.empty(lead, dtype=torch.int32, device=dev)
    windows = torch.empty(lead + (N, 2), dtype=torch.int32, device=dev) if return_windows else None
    smoothed = torch.full(lead + (L,), float("nan"), dtype=torch.float32, device=dev) if return_smoothed else None
    table = (hip.C.c_float * len(lv))(*lv)
    hip.check(hip.lib().rv_span_propose(hip.ptr(_c(sims)), hip.ptr(_c(mask.float())), R, rpm, L, table, len(lv), relative, smooth, gap, min_len, max_len, N,
                                        hip.ptr(spans), hip.ptr(n_spans), hip.ptr(n_found), hip.ptr(windows), hip.ptr(smoothed), hip.stream()),
              "rv_span_propose")
    return SpanProposals(spans, n_spans, n_found, windows, smoothed)


WINDOW_SELECT_MAX = 2048
WindowSelection = collections.namedtuple("WindowSelection", "select n_select n_windows scores bounds order hit_rank")


def window_select_keywords(who, win, stride, keep, k=3, min_sep=1):
    """The keyword refusals of ``window_select`` that need no tensor (raised before any device is looked for) -> the five as ints."""
    for name, v in (("win", win), ("stride", stride), ("keep", keep), ("k", k), ("min_sep", min_sep)):
        if not (_is_int(v) and 1 <= v < 2 ** 31):
            raise ValueError(f"{who}: {name}={v!r} must be a positive integer")
    if win < stride:
        raise ValueError(f"{who}: win={win} frames with stride={stride} (stride <= win)")
    if k > 64:
        raise ValueError(f"{who}: k={k} must be in [1, 64]")
    return int(win), int(stride), int(keep), int(k), int(min_sep)


def window_select_capacity(who, L, win, stride, min_sep=1):
    """Wcap = max(1, ceil(L / (win // stride)) - 1), the most windows a row of L frames can have; refuses win > L, more than 2048 windows and
    min_sep > Wcap."""
    if win > L:
        raise ValueError(f"{who}: win={win} frames for rows of L={L}")
    hop = win // stride
    cap = max(1, -(-L // hop) - 1)
    if cap > WINDOW_SELECT_MAX:
        raise ValueError(f"{who}: L={L}, win={win}, stride={stride} give up to {cap} windows (at most {WINDOW_SELECT_MAX})")
    if min_sep > cap:
        raise ValueError(f"{who}: min_sep={min_sep} must be in [1, {cap}] (the most windows a row of L={L} can have)")
    return cap


def window_select_gt(who, gt, lead):
    if gt is None:
        return
    if not torch.is_tensor(gt) or gt.shape != lead + (2,):
        raise ValueError(f"{who}: gt {tuple(gt.shape) if torch.is_tensor(gt) else type(gt).__name__} (expected {lead + (2,)}: rows of (start, end) in frames)")
    if not gt.dtype.is_floating_point:
        raise ValueError(f"{who}: gt must be a floating-point tensor (got {gt.dtype})")


def window_select(sims, mask, *, win, stride, keep, k=3, min_sep=1, gt=None, return_scores=False, return_bounds=False, return_order=False):
    """Choose the recursion's windows from similarity rows on the device (``rv_window_select``): sims f32 [R,L] or [B,Q,L] (``frame_cosine`` /
    ``frame_cosine_multi``'s rows), mask [R,L] / [B,L] of any bool, integer or float dtype (its row sum is the duration; with fewer rows than sims each
    serves a whole number of consecutive rows), gt [...,2] rows of (start, end) in frames or None -> WindowSelection(select i32 [...,keep] ascending
    with -1 padding, n_select i32 [...], n_windows i32 [...], scores f32 [...,Wcap] with NaN padding, bounds i32 [mask rows,Wcap,2] as (lo, hi) with
    (-1, -1) padding, order i32 [...,Wcap] with -1 padding, hit_rank i32 [...]); ``scores``, ``bounds`` and ``order`` are None unless asked for,
    ``hit_rank`` unless ``gt`` is given.  The windows are ``stage2.cut_windows``' for ``clip_length = win``; a window's score is the sum of its ``k``
    largest sims; the windows are taken in rank order, a taken one removing the others within ``min_sep`` indices of it, then topped up in rank order;
    ``select`` is the first ``min(keep, n_windows)`` of that sequence sorted, ``hit_rank`` the first place of the sequence whose window overlaps gt.
    ``Wcap = max(1, ceil(L / (win // stride)) - 1)``; a ``keep`` above it is Wcap.  One launch (a mask that is not f32 adds a cast kernel), no
    synchronisation, no host copy.  The full rule stands in include/revision_hip.h."""
    who = "window_select"
    win, stride, keep, k, min_sep = window_select_keywords(who, win, stride, keep, k, min_sep)
    lead, R, rpm, L = span_propose_shapes(who, sims, mask)
    Wcap = window_select_capacity(who, L, win, stride, min_sep)
    window_select_gt(who, gt, lead)
    if sims.dtype != torch.float32:
        raise ValueError(f"{who}: sims must be float32 (got {sims.dtype})")
    keep = min(keep, Wcap)
    dev = sims.device
    select = torch.empty(lead + (keep,), dtype=torch.int32, device=dev)
    n_select = torch.empty(lead, dtype=torch.int32, device=dev)
    n_windows = torch.empty(lead, dtype=torch.int32, device=dev)
    scores = torch.empty(lead + (Wcap,), dtype=torch.float32, device=dev) if return_scores else None
    bounds = torch.empty((R // rpm, Wcap, 2), dtype=torch.int32, device=dev) if return_bounds else None
    order = torch.empty(lead + (Wcap,), dtype=torch.int32, device=dev) if return_order else None
    hit_rank = torch.empty(lead, dtype=torch.int32, device=dev) if gt is not None else None
    hip.check(hip.lib().rv_window_select(hip.ptr(_c(sims)), hip.ptr(_c(mask.float())), R, rpm, L, win, stride, k, keep, min_sep, Wcap,
                                         hip.ptr(_c(gt.float())) if gt is not None else None, hip.ptr(select), hip.ptr(n_select), hip.ptr(n_windows),
                                         hip.ptr(scores), hip.ptr(bounds), hip.ptr(order), hip.ptr(hit_rank), hip.stream()), "rv_window_select")
    return WindowSelection(select, n_select, n_windows, scores, bounds, order, hit_rank)


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
