"""The rule of ``rv_window_gather`` (include/revision_hip.h) a second time with Python loops: the duration and the window rule are
tests/window_oracle.py's, the sampled frames are ``np.linspace``'s operations written out in Python floats (IEEE float64, one rounding per operation),
and the conversion to the output type goes through torch on the CPU.  ``gather`` is what tests/test_gpu_window_gather.py compares the kernel with;
tests/test_gather_host_logic.py holds ``linspace_index`` to ``np.linspace`` and ``frame_indices`` to ``stage2.cut_windows``.  Nothing here is used by
the package."""
import functools
import math

import numpy as np
import torch

import window_oracle as WO


@functools.lru_cache(maxsize=None)
def linspace_index(s, e, F):
    """``np.linspace(s, e, F, dtype=np.int32)`` as a tuple: step = (e - s) / (F - 1); y = j * step, or (j * (e - s)) / (F - 1) when the step is 0;
    y = y + s; the last one is e; floor."""
    if F == 1:
        return (int(s),)
    delta, div = float(e - s), float(F - 1)
    step = delta / div
    out = []
    for j in range(F):
        y = (float(j) * delta) / div if step == 0.0 else float(j) * step
        y = y + float(s)
        if j == F - 1:
            y = float(e)
        out.append(int(math.floor(y)))
    return tuple(out)


def integer_shortcut(s, e, F):
    """What the rule is NOT: s + j (e - s) / (F - 1) in integers."""
    return [int(s)] if F == 1 else [s + j * (e - s) // (F - 1) for j in range(F)]


@functools.lru_cache(maxsize=None)
def frame_indices(D, win, stride, F):
    """[W_r, F] int32: the sampled frames of every window of a row of D frames (the start clamped at 0)."""
    wins = WO.windows(D, win, stride)
    return np.array([linspace_index(lo, e, F) for _, e, lo, _ in wins], dtype=np.int32).reshape(len(wins), F)


def convert(rows, out_dtype, saturate=False):
    """A torch CPU tensor of rows in the output type (the same type: the same bits).  ``saturate``: the fp16 build's store conversion, which keeps
    what torch turns into an infinity (an overflow, or an infinity itself) at +-65504."""
    if rows.dtype == out_dtype:
        return rows
    out = rows.to(out_dtype)
    if saturate and out_dtype == torch.float16:
        out = torch.where(torch.isinf(out), torch.copysign(torch.full_like(out, 65504.0), out), out)
    return out


def gather(video, mask, select, win, stride, F, out_dtype, saturate=False):
    """video torch [M, L, d] (CPU; f32 or a 16-bit type), mask numpy [M, L] of 0 / 1 or None, select int [R, keep] -> (out torch [R, keep, F, d] in
    out_dtype, frame_idx int32 [R, keep, F], D per row)."""
    select = np.asarray(select, dtype=np.int64)
    R, keep = select.shape
    M, L, d = video.shape
    rpm = R // M
    out = torch.zeros(R, keep, F, d, dtype=out_dtype)
    idx = np.full((R, keep, F), -1, dtype=np.int32)
    Ds = []
    for r in range(R):
        D = L if mask is None else WO.duration(mask[r // rpm])
        Ds.append(D)
        table = frame_indices(D, win, stride, F)
        for n in range(keep):
            i = int(select[r, n])
            if 0 <= i < table.shape[0]:
                idx[r, n] = table[i]
                assert table[i].max() < D
                out[r, n] = convert(video[r // rpm, torch.from_numpy(table[i].astype(np.int64))], out_dtype, saturate)
    return out, idx, Ds
