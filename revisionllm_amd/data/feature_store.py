"""Reader for the pre-extracted CLIP features the drivers consume.

On-disk formats follow the reference's writers / readers: per-movie ``<movie>.npy`` arrays [ctx_l, 768]
(eval_nlq_retrieval_e2e2.py:246-247), or an LMDB whose values are ``np.savez_compressed`` blobs with key ``features``
(or ``memory_global``) for videos and ``token_features`` / ``cls_features`` for queries (e2e2.py:187-192,238-255;
writers data/feature_extraction/mad_clip_text_extractor.py:101-107).  The ``lmdb`` package is optional (not installed in this image):
without it ``data/mdb_reader.py`` reads the environment's ``data.mdb`` itself; a directory of ``<key>.npz`` files with the same keys is accepted too.

``stage_windows`` is the step right before the hot path: gather the window frames on the host into a PINNED staging
buffer and copy them to the GPU asynchronously on a side stream, so the H2D transfer of query i+1 overlaps the
recursion of query i (PCIe Gen5 x16 ~ 63 GB/s: a 290-window MAD movie is 290*250*768*2 B = 111 MB ~ 2 ms).

``ResidentFeatures`` + ``WindowStager.stage_resident`` are the route without the host gather: a movie's features are uploaded once and stay on the
device across its queries, and the window tensor is cut there by one kernel (``rv_window_gather``), with the same bits.
``stage_resident_clipped`` is the same for the stage-1 driver's half-overlapping windows (``rv_window_gather_rule``).
"""
import collections
import io
import os

import numpy as np
import torch


def _npz_bytes(blob):
    """Decode one ``np.savez[_compressed]`` blob.  ``allow_pickle=False``: feature files hold plain float arrays (the reference's
    writers add an ``allow_pickle`` boolean array, also plain), and a data directory must not be able to run code."""
    if blob is None:
        raise KeyError("key not found in the feature store")
    with io.BytesIO(bytes(blob)) as reader:
        d = np.load(reader, allow_pickle=False)
        return {k: d[k] for k in d.files}


class FeatureStore:
    def __init__(self, feat_folder, q_feat_dir=None, vis_feat_storage="npy"):
        self.feat_folder, self.q_feat_dir, self.kind = feat_folder, q_feat_dir, vis_feat_storage
        self._venv = self._qenv = None
        if vis_feat_storage == "lmdb":
            self._venv = self._open_lmdb(feat_folder)
        if q_feat_dir is not None and os.path.isfile(os.path.join(q_feat_dir, "data.mdb")):
            self._qenv = self._open_lmdb(q_feat_dir)

    @staticmethod
    def _open_lmdb(path):
        try:
            import lmdb
        except ImportError:      # the package is optional: the build's own reader of the data.mdb format does point lookups (data/mdb_reader.py)
            from . import mdb_reader as lmdb
        env = lmdb.open(path, readonly=True, create=False, max_readers=4096 * 8, readahead=False)
        return env.begin(buffers=True)

    def video(self, movie):
        """-> float array [ctx_l, 768]."""
        if self._venv is not None:
            d = _npz_bytes(self._venv.get(movie.encode()))
            return d["features"] if "features" in d else d["memory_global"]
        p = os.path.join(self.feat_folder, movie + ".npy")
        if os.path.exists(p):
            return np.load(p)
        d = dict(np.load(os.path.join(self.feat_folder, movie + ".npz"), allow_pickle=False))
        return d["features"] if "features" in d else d["memory_global"]

    def query(self, query_id):
        """-> (token_features [Lq, 768], cls_features [768])."""
        if self.q_feat_dir is None:
            return None, None
        if self._qenv is not None:
            d = _npz_bytes(self._qenv.get(query_id.encode()))
        else:
            d = dict(np.load(os.path.join(self.q_feat_dir, query_id + ".npz"), allow_pickle=False))
        return d["token_features"], d["cls_features"]


class StagedWindows:
    """One staged window tensor: ``tensor`` bf16 [W, num_frames, 768] on the device, valid once ``event`` has completed.
    ``wait(stream)`` orders a consumer stream after the copy and tells the caching allocator that the block is in use on that
    stream (the tensor was allocated on the staging stream)."""

    def __init__(self, tensor, event):
        self.tensor, self.event = tensor, event

    def wait(self, stream=None):
        if self.event is None:       # produced on the consumer's own stream (the driver's --device_features --clip_prefilter branch): already in order
            return self.tensor
        stream = stream or torch.cuda.current_stream(self.tensor.device)
        stream.wait_event(self.event)
        self.tensor.record_stream(stream)
        return self.tensor

    def __iter__(self):          # ``dev, ev = stager.stage_windows(...)``
        return iter((self.tensor, self.event))


class WindowStager:
    """Pinned host staging + asynchronous H2D of the window tensor [W, num_frames, 768] (bf16 on the device, as the
    reference casts it: e2e2.py:303-306).  ``depth`` pinned buffers are used round-robin, each with the event of its last
    copy: a buffer is overwritten only after that copy has completed, so the video of query i+1 (or i+depth-1) can be staged
    while query i's copy is still in flight."""

    def __init__(self, device="cuda:0", depth=2, op_dtype=None):
        from .. import hip
        self.op_dtype = hip.op_dtype(op_dtype)     # the engine's operand type (fp16 by default; the reference casts to its model dtype)
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(self.device)
        self._slots = [{"buf": None, "event": None} for _ in range(max(1, depth))]
        self._next = 0

    def stage_windows(self, features, frame_idx):
        """features [ctx_l, 768] numpy (any float dtype), frame_idx int32 [W, num_frames] -> ``StagedWindows`` (unpacks as
        ``(device bf16 tensor, event)``).  Consumers on another stream call ``.wait(stream)`` (or wait for the event and
        ``tensor.record_stream(stream)`` themselves)."""
        W, F = frame_idx.shape
        n = W * F * features.shape[1]
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        if slot["event"] is not None:
            slot["event"].synchronize()          # the previous copy out of this buffer has finished reading it
        if slot["buf"] is None or slot["buf"].numel() < n:
            slot["buf"] = torch.empty(n, dtype=self.op_dtype).pin_memory()     # (its predecessor is idle: waited above)
        host = slot["buf"][:n].view(W, F, features.shape[1])
        src = torch.from_numpy(np.ascontiguousarray(features))
        host.copy_(src[torch.from_numpy(frame_idx.astype(np.int64))])
        with torch.cuda.stream(self.stream):
            dev = host.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        slot["event"] = ev
        return StagedWindows(dev, ev)

    def stage_resident(self, features_dev, windows, **geometry):
        """``stage_windows`` for features that are already on the device (``ResidentFeatures.get``): features_dev [ctx_l, d], windows a Python list of
        window indices (or a device i32 row), geometry = ``debug_window``, ``feature_fps``, ``stride``, ``num_frames`` as ``stage2.cut_windows`` takes
        them -> ``StagedWindows`` with the same tensor ``stage_windows(features, cut_windows(...)[1][windows])`` hands over, bit for bit, made by one
        kernel on the staging stream (``stage2.gather_windows``): no host gather, no upload of the frames, no synchronisation."""
        from ..eval import stage2
        self.stream.wait_stream(torch.cuda.current_stream(self.device))      # whatever made features_dev on the caller's stream comes first
        with torch.cuda.stream(self.stream):
            dev = stage2.gather_windows(features_dev, windows, dtype=self.op_dtype, **geometry)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        features_dev.record_stream(self.stream)
        return StagedWindows(dev, ev)

    def stage_resident_clipped(self, features_dev, **geometry):
        """``stage_resident`` for the stage-1 driver: every window of ``stage1.cut_windows`` (half-overlapping, the last ones clipped), geometry =
        ``debug_window``, ``feature_fps``, ``num_frames`` as that function takes them -> ``StagedWindows`` with the tensor
        ``stage_windows(features, stage1.cut_windows(ctx_l, ...))`` hands over, bit for bit, made by one kernel on the staging stream
        (``stage1.gather_windows``): no host gather, no upload, no synchronisation."""
        from ..eval import stage1
        self.stream.wait_stream(torch.cuda.current_stream(self.device))      # whatever made features_dev on the caller's stream comes first
        with torch.cuda.stream(self.stream):
            dev = stage1.gather_windows(features_dev, dtype=self.op_dtype, **geometry)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        features_dev.record_stream(self.stream)
        return StagedWindows(dev, ev)

    def stage_resident_selected(self, features_dev, *, windows=None, query_cls=None, keep=None, **geometry):
        """``stage_resident_clipped`` for a selection of the stage-1 windows, on the staging stream: either ``windows``, a list of window indices the
        host has (``stage1.windows_from_retrieval`` -> ``stage1.gather_selected``), or ``query_cls`` and ``keep`` (the CLIP pre-filter:
        ``stage1.clip_stage_windows``, which waits for its one ``select`` row) -> (the sorted list of windows, ``StagedWindows`` with row j =
        ``stage_resident_clipped(...)``'s row ``list[j]``)."""
        from ..eval import stage1
        if (windows is None) == (query_cls is None):
            raise ValueError("stage_resident_selected: pass either windows= or query_cls= with keep=")
        self.stream.wait_stream(torch.cuda.current_stream(self.device))      # whatever made features_dev on the caller's stream comes first
        with torch.cuda.stream(self.stream):
            if windows is not None:
                windows = sorted(windows)
                dev = stage1.gather_selected(features_dev, windows, dtype=self.op_dtype, **geometry)
            else:
                windows, dev = stage1.clip_stage_windows(features_dev, query_cls, keep=keep, dtype=self.op_dtype, **geometry)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        features_dev.record_stream(self.stream)
        return windows, StagedWindows(dev, ev)


    def stage_resident_selected_frames(self, features_dev, *, query_cls, keep, score_frames="sampled", valid=None, **geometry):
        """``stage_resident_selected(query_cls=, keep=)`` with the pre-filter's windows scored on a chosen frame set (``stage1.clip_stage_windows_frames``:
        ``score_frames="sampled"`` ranks a window by the ``num_frames`` frames that are staged of it; ``valid`` [ctx_l] hides frames from the scores) ->
        (the sorted list of windows, ``StagedWindows`` with row j = ``stage_resident_clipped(...)``'s row ``list[j]``)."""
        from ..eval import stage1
        self.stream.wait_stream(torch.cuda.current_stream(self.device))      # whatever made features_dev on the caller's stream comes first
        with torch.cuda.stream(self.stream):
            windows, dev = stage1.clip_stage_windows_frames(features_dev, query_cls, keep=keep, dtype=self.op_dtype, score_frames=score_frames, valid=valid,
                                                            **geometry)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        features_dev.record_stream(self.stream)
        return windows, StagedWindows(dev, ev)


class ResidentFeatures:
    """Movies' feature arrays kept on the device across the queries of a movie: an LRU cache by bytes, keyed by movie.  ``get(movie, array)`` -> the
    device tensor [ctx_l, d], uploaded on the first use (through a pinned buffer, asynchronously, on ``stream`` - the stager's) and handed back from the
    cache afterwards; each entry keeps the event of its upload and ``get`` orders the caller's current stream behind it.  f32 arrays stay f32; a
    16-bit array stays as stored when that is the engine's operand type (``op_dtype``) and becomes f32 otherwise (exact), so what the kernels read
    has the values of the array; anything else becomes f32.  An array larger than the whole budget is uploaded and handed back without being kept.
    ``device="cpu"`` keeps host tensors (no stream, no event): the policy runs without a GPU."""

    def __init__(self, device, budget_bytes, op_dtype=None, stream=None):
        from .. import hip
        self.device = torch.device(device)
        self.budget = int(budget_bytes)
        self.op_dtype = hip.op_dtype(op_dtype)
        self.stream = stream
        if self.device.type == "cuda" and stream is None:
            self.stream = torch.cuda.Stream(self.device)
        self._entries = collections.OrderedDict()       # movie -> (tensor, event, bytes), least recently used first
        self._pinned, self._pinned_event = None, None
        self.bytes = self.hits = self.misses = self.evictions = 0

    def __len__(self):
        return len(self._entries)

    def __contains__(self, movie):
        return movie in self._entries

    def movies(self):
        """The cached movies, least recently used first."""
        return list(self._entries)

    def kept_dtype(self, dtype):
        """The dtype an array of torch ``dtype`` is kept in."""
        return dtype if dtype in (torch.float32, self.op_dtype) else torch.float32

    def _upload(self, array):
        src = array if torch.is_tensor(array) else torch.from_numpy(np.ascontiguousarray(array))
        if src.dim() != 2 or not src.dtype.is_floating_point:
            raise ValueError(f"ResidentFeatures: features {tuple(src.shape)} {src.dtype} (expected a floating-point array [ctx_l, d])")
        dtype = self.kept_dtype(src.dtype)
        if self.device.type != "cuda":
            return src.to(self.device, dtype).contiguous(), None
        if src.is_cuda:
            return src.to(self.device, dtype).contiguous(), None
        if self._pinned_event is not None:
            self._pinned_event.synchronize()             # the previous upload has finished reading the buffer
        nbytes = src.numel() * torch.empty((), dtype=dtype).element_size()
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        host = self._pinned[:nbytes].view(dtype).view(src.shape)
        host.copy_(src)
        with torch.cuda.stream(self.stream):
            dev = host.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._pinned_event = ev
        return dev, ev

    def get(self, movie, array):
        entry = self._entries.get(movie)
        if entry is not None:
            self.hits += 1
            self._entries.move_to_end(movie)
        else:
            self.misses += 1
            tensor, event = self._upload(array)
            nbytes = tensor.numel() * tensor.element_size()
            entry = (tensor, event, nbytes)
            if nbytes <= self.budget:
                while self._entries and self.bytes + nbytes > self.budget:
                    _, (_, _, freed) = self._entries.popitem(last=False)     # (a block freed while kernels still read it stays ordered behind them: record_stream below)
                    self.bytes -= freed
                    self.evictions += 1
                self._entries[movie] = entry
                self.bytes += nbytes
        tensor, event, _ = entry
        if event is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(event)
            tensor.record_stream(cur)
        return tensor
