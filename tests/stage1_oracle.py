"""The rules of ``rv_window_gather_rule``'s clipped windows and of ``rv_proposal_cosine`` (include/revision_hip.h) a second time with Python loops: the
windows are ``stage1.cut_windows``' expressions in integers, the sampled frames are tests/gather_oracle.py's ``linspace_index``, the proposal score is
float64 numpy, and the slice is the header's min rule.  tests/test_gpu_stage1_device.py compares the kernels with these; tests/test_stage1_device_host_logic.py
holds the windows to ``stage1.cut_windows`` and the slice rule to Python's.  Nothing here is used by the package."""
import functools

import numpy as np
import torch

import gather_oracle as GO
import window_oracle as WO


def window_count(D, win):
    """max(0, ceil(D / (win // 2)) - 1)"""
    half = win // 2
    return max(0, -(-D // half) - 1)


def windows(D, win):
    """[(s, e)] of every window of a row of D frames, frames [s, e + 1); s > e is a void window."""
    return [((i * win) // 2, min((i * win) // 2 + win, D - 1)) for i in range(window_count(D, win))]


def void(s, e):
    return s > e


@functools.lru_cache(maxsize=None)
def frame_indices(D, win, F):
    """[W_r, F] int32: the sampled frames of every window, -1 for a void one."""
    wins = windows(D, win)
    rows = [[-1] * F if void(s, e) else GO.linspace_index(s, e, F) for s, e in wins]
    return np.array(rows, dtype=np.int32).reshape(len(wins), F)


def gather(video, mask, select, win, F, out_dtype, saturate=False, keep=None):
    """video torch [M, L, d] (CPU), mask numpy [M, L] of 0 / 1 or None, select int [R, keep] or None (entry n is window n; ``keep`` entries for each of
    the M rows) -> (out torch [R, keep, F, d] in out_dtype, frame_idx int32 [R, keep, F], D per row)."""
    M, L, d = video.shape
    if select is None:
        select = np.tile(np.arange(keep), (M, 1))
    select = np.asarray(select, dtype=np.int64)
    R, keep = select.shape
    rpm = R // M
    out = torch.zeros(R, keep, F, d, dtype=out_dtype)
    idx = np.full((R, keep, F), -1, dtype=np.int32)
    Ds = []
    for r in range(R):
        D = L if mask is None else WO.duration(mask[r // rpm])
        Ds.append(D)
        table = frame_indices(D, win, F)
        for n in range(keep):
            i = int(select[r, n])
            if 0 <= i < table.shape[0] and table[i, 0] >= 0:
                idx[r, n] = table[i]
                assert 0 <= table[i].min() and table[i].max() < D
                out[r, n] = GO.convert(video[r // rpm, torch.from_numpy(table[i].astype(np.int64))], out_dtype, saturate)
    return out, idx, Ds


def slice_bounds(a, b, T):
    """(lo, hi) of the frames of ``feat[window][a : b + 1]`` for a >= 0: lo = min(a, T), hi = min(b + 1, T); hi <= lo is empty."""
    return min(a, T), min(b + 1, T)


def is_void(w, a, b, W, T):
    lo, hi = slice_bounds(a, b, T)
    return not 0 <= w < W or a < 0 or hi <= lo


def topk_order(sims):
    """Frame indices in ``torch.topk``'s order: NaN first, then the larger value, then the smaller index."""
    return sorted(range(len(sims)), key=lambda t: (0, 0.0, t) if np.isnan(sims[t]) else (1, -sims[t], t))


def proposal_score(feat, q, w, a, b, k):
    """feat torch [W, T, d] (CPU, any float type), q torch [d] -> the score in float64 (NaN for a void proposal)."""
    W, T, _ = feat.shape
    if is_void(w, a, b, W, T):
        return float("nan")
    lo, hi = slice_bounds(a, b, T)
    f = feat[w, lo:hi].double().numpy()
    with np.errstate(all="ignore"):
        norm = np.sqrt((f * f).sum(0))
        sims = f @ (q.double().numpy() / norm)
    if k <= 0:
        return float(sims.sum() / len(sims))
    order = topk_order(sims)[:min(k, len(sims))]
    return float(sum(sims[t] for t in order))


def proposal_scores(feat, q, props, k):
    return np.array([proposal_score(feat, q, int(w), int(a), int(b), k) for w, a, b in props], dtype=np.float64)
