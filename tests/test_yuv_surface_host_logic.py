"""The host side of the surface front end, without a GPU: ops.yuv_frame_bytes and ops.split_yuv for every pix_fmt of ops.PIX_FMTS (frame sizes, zero-copy
views with the shapes, dtypes and strides the format says, the keyword arguments that go with them), their refusals, ops.yuv_surface_to_patches' refusal of
CPU tensors, and the colour defaults of ClipFeatureExtractor.encode_video_pix_fmt (those of encode_video_yuv, except BT.2020 + top-left siting for a stream
the caller says is BT.2020)."""
import pytest
import torch

H, W, N = 6, 8, 3

#         name            bytes  depth  msb   sub    (sub_x, sub_y)  chroma layout
TABLE = [("nv12",          1,    8, False, "420", (2, 2), "cbcr"),
         ("nv21",          1,    8, False, "420", (2, 2), "crcb"),
         ("nv16",          1,    8, False, "422", (2, 1), "cbcr"),
         ("nv24",          1,    8, False, "444", (1, 1), "cbcr"),
         ("yuv420p",       1,    8, False, "420", (2, 2), "planar"),
         ("yuv422p",       1,    8, False, "422", (2, 1), "planar"),
         ("yuv444p",       1,    8, False, "444", (1, 1), "planar"),
         ("yuv420p10le",   2,   10, False, "420", (2, 2), "planar"),
         ("yuv422p10le",   2,   10, False, "422", (2, 1), "planar"),
         ("yuv444p10le",   2,   10, False, "444", (1, 1), "planar"),
         ("yuv420p12le",   2,   12, False, "420", (2, 2), "planar"),
         ("yuv444p12le",   2,   12, False, "444", (1, 1), "planar"),
         ("yuv420p16le",   2,   16, False, "420", (2, 2), "planar"),
         ("p010le",        2,   10, True,  "420", (2, 2), "cbcr"),
         ("p016le",        2,   16, True,  "420", (2, 2), "cbcr"),
         ("p210le",        2,   10, True,  "422", (2, 1), "cbcr"),
         ("p410le",        2,   10, True,  "444", (1, 1), "cbcr")]


def test_the_table_is_the_one_the_issue_lists():
    from revisionllm_amd import ops
    assert sorted(ops.PIX_FMTS) == sorted(t[0] for t in TABLE)


def byte_index(view, buf):
    """The byte offset into buf of every element of a view of it, from data_ptr and strides alone."""
    idx = torch.full(view.shape, view.data_ptr() - buf.data_ptr(), dtype=torch.int64)
    for d, (s, st) in enumerate(zip(view.shape, view.stride())):
        shape = [1] * view.dim()
        shape[d] = s
        idx = idx + (torch.arange(s) * st * view.element_size()).reshape(shape)
    return idx


@pytest.mark.parametrize("name,sb,depth,msb,sub,subxy,layout", TABLE, ids=[t[0] for t in TABLE])
def test_frame_bytes_and_split_views(name, sb, depth, msb, sub, subxy, layout):
    from revisionllm_amd import ops
    sx, sy = subxy
    h, w = H // sy, W // sx
    fb = (H * W + 2 * h * w) * sb
    assert ops.yuv_frame_bytes(H, W, name) == fb
    buf = torch.arange(N * fb, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(N, fb)
    (y, cb, cr), kw = ops.split_yuv(buf, H, W, name)
    assert kw == dict(depth=depth, msb_aligned=msb, subsampling=sub)
    dt = torch.uint8 if sb == 1 else torch.uint16
    fs = fb // sb                                                                       # strides are in samples
    f = torch.arange(N).reshape(N, 1, 1) * fb
    r, c = torch.arange(h).reshape(1, h, 1), torch.arange(w).reshape(1, 1, w)
    assert y.dtype == dt and tuple(y.shape) == (N, H, W) and y.stride() == (fs, W, 1) and y.data_ptr() == buf.data_ptr()
    assert torch.equal(byte_index(y, buf), f + (torch.arange(H).reshape(1, H, 1) * W + torch.arange(W).reshape(1, 1, W)) * sb)
    if layout == "cbcr":
        assert cr is None and cb.dtype == dt and tuple(cb.shape) == (N, h, w, 2) and cb.stride() == (fs, 2 * w, 2, 1)
        cb, cr = cb[..., 0], cb[..., 1]
    assert cb.dtype == cr.dtype == dt and tuple(cb.shape) == tuple(cr.shape) == (N, h, w)
    if layout == "planar":
        assert cb.stride() == cr.stride() == (fs, w, 1)
        cb_at, cr_at = f + (H * W + r * w + c) * sb, f + (H * W + h * w + r * w + c) * sb
    else:
        assert cb.stride() == cr.stride() == (fs, 2 * w, 2)
        first, second = f + (H * W + r * 2 * w + 2 * c) * sb, f + (H * W + r * 2 * w + 2 * c + 1) * sb
        cb_at, cr_at = (first, second) if layout == "cbcr" else (second, first)
    assert torch.equal(byte_index(cb, buf), cb_at) and torch.equal(byte_index(cr, buf), cr_at)
    # the values are the buffer's bytes, little-endian, and a write to the buffer shows through every view: no copy was made
    flat = buf.reshape(-1).to(torch.int64)
    value = lambda at: flat[at] if sb == 1 else flat[at] + 256 * flat[at + 1]
    for v, at in ((y, byte_index(y, buf)), (cb, cb_at), (cr, cr_at)):
        assert torch.equal(v.to(torch.int64), value(at))
    for v, at in ((y, byte_index(y, buf)), (cb, cb_at), (cr, cr_at)):
        i = (1, v.shape[1] - 1, v.shape[2] - 1)
        before = int(v[i])
        low = buf.reshape(-1)[int(at[i])]
        low.copy_((low.to(torch.int64) + 1) % 256)
        assert int(v[i]) == (before & ~0xFF) | ((before + 1) & 0xFF)                    # the low byte of the sample moved, nothing else
    # a batch cut out of a longer buffer keeps its frame stride and offset
    (y1, cb1, _), _ = ops.split_yuv(buf[1:], H, W, name)
    assert y1.data_ptr() == buf.data_ptr() + fb and len(y1) == N - 1 and cb1.data_ptr() - y1.data_ptr() == cb.data_ptr() - y.data_ptr()


def test_odd_sizes_are_legal_only_along_an_axis_that_is_not_subsampled():
    from revisionllm_amd import ops
    assert ops.yuv_frame_bytes(5, 7, "yuv444p10le") == 5 * 7 * 3 * 2
    assert ops.yuv_frame_bytes(5, 8, "yuv422p") == 5 * 8 * 2
    (y, cb, cr), _ = ops.split_yuv(torch.zeros(2, 5 * 8 * 2, dtype=torch.uint8), 5, 8, "nv16")
    assert tuple(y.shape) == (2, 5, 8) and tuple(cb.shape) == (2, 5, 4, 2) and cr is None
    for h, w, fmt in ((5, 8, "nv12"), (6, 7, "yuv420p10le"), (6, 7, "yuv422p"), (6, 7, "p210le"), (0, 8, "yuv444p"), (1, 8, "p010le")):
        with pytest.raises(ValueError, match="odd"):
            ops.yuv_frame_bytes(h, w, fmt)
        with pytest.raises(ValueError, match="odd"):
            ops.split_yuv(torch.zeros(1, 64, dtype=torch.uint8), h, w, fmt)


def test_split_refuses_unknown_names_other_shapes_and_bytes_that_are_not_adjacent():
    from revisionllm_amd import ops
    fb = ops.yuv_frame_bytes(H, W, "p010le")
    buf = torch.zeros(N, fb, dtype=torch.uint8)
    for fn in (lambda: ops.split_yuv(buf, H, W, "yuyv422"), lambda: ops.yuv_frame_bytes(H, W, "yuv420p10be")):
        with pytest.raises(ValueError) as e:
            fn()
        assert all(name in str(e.value) for name, *_ in TABLE)                          # the message lists the table
    for bad in (buf[:, :-2], buf.reshape(N, fb // W, W), buf.reshape(-1), buf.to(torch.int16), buf.numpy()):
        with pytest.raises(ValueError, match="uint8 tensor"):
            ops.split_yuv(bad, H, W, "p010le")
    with pytest.raises(ValueError, match="adjacent"):
        ops.split_yuv(torch.zeros(N, fb, 2, dtype=torch.uint8)[:, :, 0], H, W, "p010le")       # every second byte
    with pytest.raises(ValueError, match="adjacent"):
        ops.split_yuv(torch.zeros(N, 2 * H * W, 2, dtype=torch.uint8)[:, :, 0], H, W, "nv16")
    with pytest.raises(ValueError, match="even offset"):
        ops.split_yuv(torch.zeros(N * fb + 1, dtype=torch.uint8)[1:].reshape(N, fb), H, W, "p010le")   # words that start at an odd byte
    with pytest.raises(ValueError, match="even offset"):
        ops.split_yuv(torch.zeros(N, fb + 1, dtype=torch.uint8)[:, :fb], H, W, "yuv420p10le")         # an odd frame stride


def test_yuv_surface_to_patches_refuses_cpu_tensors_and_unknown_names():
    from revisionllm_amd import hip, ops
    for fmt in ("nv12", "p010le", "yuv444p10le", "nv21"):
        planes, kw = ops.split_yuv(torch.zeros(N, ops.yuv_frame_bytes(H, W, fmt), dtype=torch.uint8), H, W, fmt)
        with pytest.raises(hip.HipLibraryError, match="CPU"):
            ops.yuv_surface_to_patches(*planes, R=28, patch=14, **kw)


class _Towers:
    """Stands in for ClipTowers: records what encode_video_pix_fmt hands to encode_surfaces_yuv."""
    device, cfg = "cpu", dict(embed_dim=4)

    def __init__(self):
        self.calls = []

    def encode_surfaces_yuv(self, y, cb, cr=None, **surface):
        self.calls.append((len(y), y.dtype, tuple(cb.shape[1:]), surface))
        return torch.zeros(len(y), 4)


def test_encode_video_pix_fmt_regroups_chunks_and_picks_the_colour_defaults():
    from revisionllm_amd import ops
    from revisionllm_amd.data.clip_extractor import ClipFeatureExtractor, yuv_colour_defaults, yuv_surface_colour_defaults
    assert yuv_surface_colour_defaults(718) == yuv_colour_defaults(718) == dict(matrix="bt601", full_range=False, chroma_loc="left")
    assert yuv_surface_colour_defaults(720) == yuv_colour_defaults(720)
    assert yuv_surface_colour_defaults(2160, bt2020=True) == dict(matrix="bt2020", full_range=False, chroma_loc="topleft")
    p010 = dict(depth=10, msb_aligned=True, subsampling="420")
    for h, matrix in ((718, "bt601"), (720, "bt709")):
        fb = ops.yuv_frame_bytes(h, 4, "p010le")
        tw = _Towers()
        out = ClipFeatureExtractor(tw).encode_video_pix_fmt(iter([torch.zeros(2, fb, dtype=torch.uint8), torch.zeros(3, fb, dtype=torch.uint8)]), h, 4,
                                                            "p010le", bsz=4)
        assert tuple(out.shape) == (5, 4)
        want = dict(p010, matrix=matrix, full_range=False, chroma_loc="left")
        assert tw.calls == [(4, torch.uint16, (h // 2, 2, 2), want), (1, torch.uint16, (h // 2, 2, 2), want)]
    fb = ops.yuv_frame_bytes(720, 4, "yuv444p10le")
    tw = _Towers()
    ex = ClipFeatureExtractor(tw)
    ex.encode_video_pix_fmt(torch.zeros(1, fb, dtype=torch.uint8), 720, 4, "yuv444p10le", matrix="bt2020")
    ex.encode_video_pix_fmt(torch.zeros(1, fb, dtype=torch.uint8), 720, 4, "yuv444p10le", matrix="bt2020", chroma_loc="left", full_range=True)
    ex.encode_video_pix_fmt(torch.zeros(1, fb, dtype=torch.uint8), 720, 4, "yuv444p10le", matrix="bt601")
    s444 = dict(depth=10, msb_aligned=False, subsampling="444")
    assert tw.calls == [(1, torch.uint16, (720, 4), dict(s444, matrix="bt2020", full_range=False, chroma_loc="topleft")),
                        (1, torch.uint16, (720, 4), dict(s444, matrix="bt2020", full_range=True, chroma_loc="left")),
                        (1, torch.uint16, (720, 4), dict(s444, matrix="bt601", full_range=False, chroma_loc="left"))]
    with pytest.raises(ValueError, match="uint8"):
        ex.encode_video_pix_fmt(torch.zeros(1, fb), 720, 4, "yuv444p10le")
    with pytest.raises(ValueError, match="pix_fmt"):
        ex.encode_video_pix_fmt(torch.zeros(1, fb, dtype=torch.uint8), 720, 4, "rgb24")
