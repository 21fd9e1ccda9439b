"""Frame / query feature extraction with the CLIP towers - mirror of ``ClipFeatureExtractor``
(revisionllm/data/feature_extraction/clip_extractor.py:13-54) on the HIP kernels.

Differences from the reference, all at the IO edge: frames are handed over as tensors (video decoding is not part of this
build) - either already at the towers' resolution [T,3,R,R] (what its ``VideoLoader`` produces from ffmpeg's scale + crop), or as
decoded uint8 frames of any size, NCHW or NHWC, in one tensor or in chunks: those are resized, centre-cropped, normalised and
unfolded on the device by one kernel (``ops.frames_to_patches``; the reference's Resize / CenterCrop / Normalize,
inference.py:108-117) - or as the YCbCr bytes a decoder really emits (8-bit 4:2:0 NV12 / NV21 / I420: ``encode_video_yuv``, ``ops.yuv_to_patches``; 10 / 12 /
16-bit words, 4:2:2 and 4:4:4 by ffmpeg's pix_fmt name: ``encode_video_pix_fmt``, ``ops.yuv_surface_to_patches``), which are
resampled plane by plane and converted per output pixel in one kernel of the same shape.  The CLIP weights come from ``ClipTowers`` (a loaded checkpoint or synthetic).  The on-disk format of the results is what ``data.feature_store`` reads back (f-2).
"""
import math

import torch

from .. import frontend, ops
from ..ops import CLIP_MEAN, CLIP_STD  # noqa: F401  (the constants' home is next to the kernel wrapper that defaults to them)
from .clip_model import ClipTowers


def preprocess(frames):
    """uint8 / float [T,3,H,W] in 0..255 -> (x / 255 - mean) / (std + 1e-8)   (Preprocessing, clip_extractor.py:76-97)."""
    x = frames.float() / 255.0
    mean = torch.tensor(CLIP_MEAN, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD, device=x.device).view(1, 3, 1, 1)
    return (x - mean) / (std + 1e-8)


def yuv_colour_defaults(H):
    """What ffmpeg (swscale) assumes for a stream that carries no colour tags: BT.601 below 720 lines, BT.709 from 720 on; studio range; chroma sited left."""
    return dict(matrix="bt601" if H < 720 else "bt709", full_range=False, chroma_loc="left")


def yuv_surface_colour_defaults(H, bt2020=False, transfer=None):
    """``yuv_colour_defaults(H)`` for a stream that carries no colour tags; for one the caller knows to be BT.2020 (HEVC Main10 / AV1 10-bit UHD): its
    non-constant-luminance matrix, studio range and the top-left chroma siting that is BT.2020's default for 4:2:0.  With ``transfer`` ("pq" | "hlg" or
    ffmpeg's "smpte2084" | "arib-std-b67"): the tags of an HDR10 / HLG stream - those BT.2020 tags and the transfer itself."""
    if transfer is not None:
        return dict(matrix="bt2020", full_range=False, chroma_loc="topleft", transfer=transfer)
    return dict(matrix="bt2020", full_range=False, chroma_loc="topleft") if bt2020 else yuv_colour_defaults(H)


def _split_each(frames, split):
    """A list of per-frame buffers -> the lists of per-frame plane views (y, cb, cr or None) that the list forms of the YCbCr front end take; ``split``: the
    batched splitter on a batch of one."""
    per = [split(f.unsqueeze(0)) for f in frames]
    return tuple(None if per[0][k] is None else [p[k][0] for p in per] for k in range(3))


class ClipFeatureExtractor:
    def __init__(self, towers: ClipTowers, tokenizer=None):
        self.clip_extractor = towers
        self.tokenizer = tokenizer            # ClipTokenizer (needs CLIP's merge table); only encode_text uses it
        self.device = towers.device

    @torch.no_grad()
    def encode_video(self, frames, bsz=60, layout=None, *, rotate=0, hflip=False, vflip=False, pix_fmt=None, scattered=False):
        """-> f32 [T, d], ``bsz`` frames at a time (clip_extractor.py:22-37).  ``frames``: a tensor [T,3,R,R] (0..255, float or uint8) at the towers'
        resolution R - normalised here and handed to ``encode_image`` -, or DECODED uint8 frames of any size, [T,3,H,W] or [T,H,W,3] (``layout``
        "NCHW" / "NHWC" where the shape leaves it open), as one tensor or as an iterable of such chunks (what a decoder hands over): those go through
        ``encode_frames``, so no float copy at the source resolution ever exists.  ``rotate`` / ``hflip`` / ``vflip`` (``ops.orientation``: mp4's ``rotate``
        tag, then flips) say how decoded uint8 frames that are CODED turned or flipped are displayed; the front-end kernel turns them.  Float frames at the
        towers' resolution are past the front end: a non-identity orientation is refused for them.  ``pix_fmt`` (``ops.RGB_PIX_FMTS``: "bgr24" from OpenCV,
        "bgra" / "rgba" / "argb" ... from screen capture): the frames are decoded uint8 [T,H,W,3|4] frames in that byte order, whatever their size, and are
        read as they lie.  ``scattered=True`` (decoded uint8 frames only): a batch that spans several chunks is handed over as a list of per-frame views
        and batched by a pointer table inside the front-end launch, in the place of the ``torch.cat`` that copies every such frame; the batches, and so the
        features, are the same bit for bit."""
        tw, R = self.clip_extractor, self.clip_extractor.cfg["image_res"]
        orient = ops.orientation(rotate, hflip, vflip)
        if pix_fmt is not None:
            pix = frontend._rgb_format(pix_fmt, layout)[0]      # an unknown name, or a layout that does not go with it, is refused before anything is read
            return self._features(tw.encode_frames(b, rotate=rotate, hflip=hflip, vflip=vflip, pix_fmt=pix_fmt)
                                  for b in self._batches((frames,) if torch.is_tensor(frames) else frames, bsz, shapes=f"[t,H,W,{pix}]", scattered=scattered))
        if torch.is_tensor(frames):
            native = frames.dim() == 4 and tuple(frames.shape[1:]) == (3, R, R) and layout in (None, "NCHW")
            if orient and frames.dtype == torch.uint8:
                native = False                                  # uint8 frames of the towers' size are decoded frames like any other: the kernel turns them
            if native or frames.dtype != torch.uint8:
                if not native:
                    raise ValueError(f"float frames must be [T,3,{R},{R}] (got {tuple(frames.shape)}): frames of another size or layout are taken as "
                                     "decoded uint8 frames")
                if orient:
                    raise ValueError(f"rotate={rotate} / hflip={hflip} / vflip={vflip}: float frames at the towers' resolution are past the front end; turn "
                                     "them before the call, or hand over the decoded uint8 frames")
                x = preprocess(frames)
                return self._features(tw.encode_image(x[i * bsz:(i + 1) * bsz]) for i in range(int(math.ceil(len(x) / bsz))))
            frames = (frames,)
        return self._features(tw.encode_frames(b, layout=layout, rotate=rotate, hflip=hflip, vflip=vflip) for b in self._batches(frames, bsz, scattered=scattered))

    @torch.no_grad()
    def encode_video_yuv(self, chunks, H, W, fmt, bsz=60, scattered=False, **colour):
        """-> f32 [T, d] from the bytes of a rawvideo pipe (``ffmpeg -f rawvideo -pix_fmt nv12 | nv21 | yuv420p``; ``fmt`` "nv12" | "nv21" | "i420"): ``chunks``
        is one packed uint8 buffer [t, H*3//2, W] (``torch.frombuffer(data, dtype=torch.uint8).view(-1, H * 3 // 2, W)``) or an iterable of them, CPU or
        device.  They are regrouped into batches of exactly ``bsz`` frames, split into plane views (``ops.split_yuv420``) and go through
        ``encode_frames_yuv``: no RGB frame exists anywhere.  ``colour`` (``matrix`` / ``full_range`` / ``chroma_loc``) overrides ``yuv_colour_defaults(H)``;
        ``rotate`` / ``hflip`` / ``vflip`` in it (``ops.orientation``) say how a ``-noautorotate`` pipe's coded frames are displayed.  H, W: the CODED size.
        ``scattered=True``: no ``torch.cat`` where a batch spans chunks - per-frame plane views and a pointer table, as in ``encode_video``."""
        tw = self.clip_extractor
        ops.orientation(colour.get("rotate", 0), colour.get("hflip", False), colour.get("vflip", False))     # refused before anything is read
        colour = {**yuv_colour_defaults(H), **colour}
        return self._features(
            tw.encode_frames_yuv(*(_split_each(b, lambda f: ops.split_yuv420(f, H, W, fmt)) if scattered else ops.split_yuv420(b, H, W, fmt)), **colour)
            for b in self._batches((chunks,) if torch.is_tensor(chunks) else chunks, bsz, ndim=3, shapes=f"[t,{H * 3 // 2},{W}]", scattered=scattered))

    @torch.no_grad()
    def encode_video_pix_fmt(self, chunks, H, W, pix_fmt, bsz=60, scattered=False, **colour):
        """-> f32 [T, d] from the bytes of a rawvideo pipe in any of ``ops.PIX_FMTS`` (``ffmpeg -f rawvideo -pix_fmt p010le | yuv420p10le | nv16 | yuv444p10le
        ...``): ``chunks`` is one uint8 buffer [t, ops.yuv_frame_bytes(H, W, pix_fmt)] or an iterable of them, CPU or device.  They are regrouped into
        batches of exactly ``bsz`` frames, split into plane views (``ops.split_yuv``) and go through ``encode_surfaces_yuv``: no conversion pass, no RGB
        frame.  ``colour`` (``matrix`` / ``full_range`` / ``chroma_loc``) overrides ``yuv_surface_colour_defaults``; ``matrix="bt2020"`` says the stream is
        BT.2020 and brings top-left siting with it.  ``transfer="pq"`` | ``"hlg"`` says it is HDR10 / HLG: the BT.2020 tags become the defaults and the
        frames are converted to SDR inside the kernel (``ops.yuv_surface_to_patches``; ``peak_nits`` / ``sdr_white_nits`` / ``gamut`` go through with it).
        ``rotate`` / ``hflip`` / ``vflip`` (``ops.orientation``) say how the coded frames of a ``-noautorotate`` pipe are displayed; H, W: the CODED size.
        The packed names of ``ops.PACKED_PIX_FMTS`` (yuyv422 / uyvy422 / y210le / ayuv / xv30le ...) are taken too: [t, ops.packed_frame_bytes(H, W, pix_fmt)]
        buffers go, with the same colour defaults and the same batching, through ``encode_surfaces_packed`` (``ops.packed_to_patches``) as they lie.
        ``scattered=True``: no ``torch.cat`` where a batch spans chunks - per-frame views and a pointer table, as in ``encode_video``; the same features."""
        tw = self.clip_extractor
        packed = pix_fmt in ops.PACKED_PIX_FMTS                 # decided before anything else is computed
        if not packed and pix_fmt not in ops.PIX_FMTS:
            raise ValueError(f"pix_fmt {pix_fmt!r}: one of {sorted(ops.PIX_FMTS)} (planar / semi-planar) or of {sorted(ops.PACKED_PIX_FMTS)} (packed)")
        ops.orientation(colour.get("rotate", 0), colour.get("hflip", False), colour.get("vflip", False))     # refused before anything is read
        fb = ops.packed_frame_bytes(H, W, pix_fmt) if packed else ops.yuv_frame_bytes(H, W, pix_fmt)
        ops.hdr_map(colour.get("transfer"))                     # an unknown transfer is refused before anything is read
        colour = {**yuv_surface_colour_defaults(H, bt2020=colour.get("matrix") == "bt2020", transfer=colour.get("transfer")), **colour}
        if colour.get("transfer") is None:
            colour.pop("transfer", None)                        # transfer=None is the SDR call as it always was
        out = []
        for b in self._batches((chunks,) if torch.is_tensor(chunks) else chunks, bsz, ndim=2, shapes=f"[t,{fb}]", scattered=scattered):
            if packed:
                out.append(tw.encode_surfaces_packed(b, H=H, W=W, pix_fmt=pix_fmt, **colour))
                continue
            if scattered:
                kw = ops.split_yuv(b[0].unsqueeze(0), H, W, pix_fmt)[1]
                planes = _split_each(b, lambda f: ops.split_yuv(f, H, W, pix_fmt)[0])
            else:
                planes, kw = ops.split_yuv(b, H, W, pix_fmt)
            out.append(tw.encode_surfaces_yuv(*planes, **kw, **colour))
        return self._features(out)

    def _features(self, batches):
        """The features of the batches, joined: f32 [T, d] (T = 0 for a video without frames)."""
        out = list(batches)
        return torch.cat(out, 0) if out else torch.empty(0, self.clip_extractor.cfg["embed_dim"], device=self.device)

    def _batches(self, chunks, bsz, ndim=4, shapes="[t,3,H,W] or [t,H,W,3]", scattered=False):
        """Decoded uint8 chunks of any lengths -> device batches of exactly ``bsz`` frames (the last one shorter): the batching does not depend on
        how the decoder cut the video.  ``scattered``: every batch is a LIST of per-frame views of the chunks, in the same order and with the same batch
        boundaries, and nothing is copied (no ``torch.cat``): the list forms of the front end take the frames where they lie."""
        join = (lambda held: held) if scattered else (lambda held: held[0] if len(held) == 1 else torch.cat(held, 0))
        held, n = [], 0
        for c in chunks:
            if not torch.is_tensor(c) or c.dtype != torch.uint8 or c.dim() != ndim:
                raise ValueError(f"decoded frames come as uint8 tensors {shapes}")
            c = ops.h2d(c, self.device)
            while len(c):
                take = c[:bsz - n]
                if scattered:
                    held.extend(take)                           # per-frame views
                else:
                    held.append(take)
                n, c = n + len(take), c[len(take):]
                if n == bsz:
                    yield join(held)
                    held, n = [], 0
        if n:
            yield join(held)

    @torch.no_grad()
    def encode_text(self, text_list, bsz=60, tokens=None):
        """-> (list of [L_j, d] token features = last_hidden_state[1 : len-1], list of [d] EOT features = pooler_output)
        (clip_extractor.py:39-54).  ``tokens`` [n,77] may be given instead of text (pre-tokenised queries)."""
        if tokens is None:
            if self.tokenizer is None:
                raise ValueError("encode_text needs a ClipTokenizer (CLIP's merge table) or pre-tokenised `tokens`")
            tokens = self.tokenizer.tokenize(text_list, context_length=self.clip_extractor.cfg["ctx"])
        feats, eots = [], []
        for i in range(int(math.ceil(len(tokens) / bsz))):
            t = tokens[i * bsz:(i + 1) * bsz]
            out = self.clip_extractor.encode_text(t)
            valid = (t != 0).sum(1).tolist()
            for j, n in enumerate(valid):
                eots.append(out["pooler_output"][j])
                feats.append(out["last_hidden_state"][j, 1:n - 1])
        return feats, eots
