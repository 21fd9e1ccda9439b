"""The host side of the 4:2:0 front end, without a GPU: ops.split_yuv420's zero-copy views of a rawvideo buffer (pointer arithmetic and strides per format,
refusals), ops.yuv_to_patches' refusal of CPU tensors, and the colour defaults of ClipFeatureExtractor.encode_video_yuv (BT.601 below 720 lines, BT.709 from
there on; studio range; left siting - ffmpeg's conventions for untagged streams)."""
import pytest
import torch

H, W, N = 6, 8, 3            # h2 = 3: the I420 chroma planes (3 x 4 bytes) end inside a row of the [n, H*3//2, W] buffer


def buffer():
    return torch.arange(N * (H * 3 // 2) * W, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(N, H * 3 // 2, W)


def flat_index(view, buf):
    """The index into buf's storage of every element of a view of it, from data_ptr and strides alone."""
    idx = torch.full(view.shape, view.data_ptr() - buf.data_ptr(), dtype=torch.int64)
    for d, (s, st) in enumerate(zip(view.shape, view.stride())):
        shape = [1] * view.dim()
        shape[d] = s
        idx = idx + (torch.arange(s) * st).reshape(shape)
    return idx


def test_split_views_share_the_buffer_and_sit_where_the_format_says():
    from revisionllm_amd import ops
    buf = buffer()
    fs, h2, w2 = H * 3 // 2 * W, H // 2, W // 2
    f = torch.arange(N).reshape(N, 1, 1) * fs
    r, c = torch.arange(h2).reshape(1, h2, 1), torch.arange(w2).reshape(1, 1, w2)
    luma = f + torch.arange(H).reshape(1, H, 1) * W + torch.arange(W).reshape(1, 1, W)
    want = {"i420": (f + H * W + r * w2 + c, f + H * W + h2 * w2 + r * w2 + c),
            "nv12": (f + H * W + r * W + 2 * c, f + H * W + r * W + 2 * c + 1),
            "nv21": (f + H * W + r * W + 2 * c + 1, f + H * W + r * W + 2 * c)}
    for fmt, (cb_at, cr_at) in want.items():
        y, cb, cr = ops.split_yuv420(buf, H, W, fmt)
        if fmt == "nv12":
            assert cr is None and tuple(cb.shape) == (N, h2, w2, 2) and cb.stride() == (fs, W, 2, 1)
            cb, cr = cb[..., 0], cb[..., 1]
        assert tuple(y.shape) == (N, H, W) and y.stride() == (fs, W, 1) and y.data_ptr() == buf.data_ptr()
        assert tuple(cb.shape) == tuple(cr.shape) == (N, h2, w2)
        assert cb.stride() == cr.stride() == ((fs, w2, 1) if fmt == "i420" else (fs, W, 2))
        assert torch.equal(flat_index(y, buf), luma)
        assert torch.equal(flat_index(cb, buf), cb_at) and torch.equal(flat_index(cr, buf), cr_at)
        flat = buf.reshape(-1)
        assert torch.equal(cb, flat[cb_at]) and torch.equal(cr, flat[cr_at])
        before = cb[1, 2, 3].item()
        buf[1, H + (2 * w2 + 3) // W if fmt == "i420" else H + 2].add_(1)          # writing the buffer shows through the view: no copy was made
        assert cb[1, 2, 3].item() == (before + 1) % 256
    # a batch cut out of a longer buffer keeps its frame stride and offset
    y, cb, cr = ops.split_yuv420(buf[1:], H, W, "i420")
    assert cb.data_ptr() == buf.data_ptr() + fs + H * W and cr.data_ptr() == cb.data_ptr() + h2 * w2 and len(y) == N - 1


def test_split_refuses_other_shapes_odd_sizes_and_unknown_formats():
    from revisionllm_amd import ops
    buf = buffer()
    for bad in (buf[:, :-1], buf.reshape(N, W, H * 3 // 2), buf.reshape(N, -1), buf.float()):
        with pytest.raises(ValueError):
            ops.split_yuv420(bad, H, W, "nv12")
    with pytest.raises(ValueError, match="adjacent"):
        ops.split_yuv420(torch.zeros(N, H * 3 // 2, W + 4, dtype=torch.uint8)[:, :, :W], H, W, "i420")      # a padded pitch: rows not adjacent
    for h, w in ((5, 8), (6, 7), (0, 8)):
        with pytest.raises(ValueError, match="even"):
            ops.split_yuv420(torch.zeros(N, h * 3 // 2, w, dtype=torch.uint8), h, w, "nv12")
    with pytest.raises(ValueError, match="fmt"):
        ops.split_yuv420(buf, H, W, "yuyv")


def test_yuv_to_patches_refuses_cpu_tensors():
    from revisionllm_amd import hip, ops
    for fmt in ("nv12", "i420"):
        with pytest.raises(hip.HipLibraryError, match="CPU"):
            ops.yuv_to_patches(*ops.split_yuv420(buffer(), H, W, fmt), R=28, patch=14)


class _Towers:
    """Stands in for ClipTowers: records what encode_video_yuv hands to encode_frames_yuv."""
    device, cfg = "cpu", dict(embed_dim=4)

    def __init__(self):
        self.calls = []

    def encode_frames_yuv(self, y, cb, cr=None, **colour):
        self.calls.append((len(y), colour))
        return torch.zeros(len(y), 4)


def test_encode_video_yuv_colour_defaults_flip_at_720_lines():
    from revisionllm_amd.data.clip_extractor import ClipFeatureExtractor, yuv_colour_defaults
    assert yuv_colour_defaults(718) == dict(matrix="bt601", full_range=False, chroma_loc="left")
    assert yuv_colour_defaults(720) == dict(matrix="bt709", full_range=False, chroma_loc="left")
    for h, matrix in ((718, "bt601"), (720, "bt709")):
        tw = _Towers()
        out = ClipFeatureExtractor(tw).encode_video_yuv(iter([torch.zeros(2, h * 3 // 2, 4, dtype=torch.uint8), torch.zeros(3, h * 3 // 2, 4, dtype=torch.uint8)]),
                                                        h, 4, "nv12", bsz=4)
        assert tuple(out.shape) == (5, 4)
        assert tw.calls == [(4, dict(matrix=matrix, full_range=False, chroma_loc="left")), (1, dict(matrix=matrix, full_range=False, chroma_loc="left"))]
    tw = _Towers()
    ClipFeatureExtractor(tw).encode_video_yuv(torch.zeros(1, 1080, 4, dtype=torch.uint8), 720, 4, "i420", matrix="bt601", full_range=True)
    assert tw.calls == [(1, dict(matrix="bt601", full_range=True, chroma_loc="left"))]
