"""The rule of ``rvc_windows_valid`` (include/revision_hip_chain.h) a second time in numpy with Python loops: the duration from the mask row, the
windows of either rule and a window's frame set (tests/frames_select_oracle.py: what ``rvc_window_select_frames`` is held to), the entries of
``select`` that name a window, and the 0 / 1 row under ``valid_in``.  ``windows_valid`` is what tests/test_gpu_windows_valid.py compares the kernel
with; ``brute_covered`` is a set-union statement of "covered" that tests/test_windows_valid_host_logic.py holds it to.  Nothing here is used by the
package."""
import numpy as np

import frames_select_oracle as FO
import window_oracle as WO

F32 = np.float32
SHIFTED, CLIPPED = FO.SHIFTED, FO.CLIPPED
ALL, SAMPLED = FO.ALL, FO.SAMPLED


def windows_valid(select, mask, rule, win, stride, frames, num_frames, valid_in=None):
    """select [R, keep] (any integers), mask [R / rpm, L], valid_in [R / rpm, L] or None -> dict of valid f32 [R, L], n_valid i32 [R], D (a list) and
    W (a list: the row's windows)."""
    select = np.asarray(select)
    mask = np.asarray(mask, dtype=F32)
    valid_in = None if valid_in is None else np.asarray(valid_in, dtype=F32)
    R, keep = select.shape
    M, L = mask.shape
    rpm = R // M
    out = dict(valid=np.zeros((R, L), F32), n_valid=np.zeros(R, np.int32), D=[], W=[])
    for r in range(R):
        D = WO.duration(mask[r // rpm])
        wins = FO.windows(D, rule, win, stride)
        out["D"].append(D)
        out["W"].append(len(wins))
        for e in range(keep):
            i = int(select[r, e])
            if i < 0 or i >= len(wins):
                continue                                                # names nothing: the padding, a void window, anything else
            lo, hi = wins[i]
            for t in FO.frame_set(lo, hi, frames, num_frames):
                if t < D and (valid_in is None or not valid_in[r // rpm, t] == 0):          # (a NaN in valid_in is not 0; -0 is)
                    out["valid"][r, t] = 1.0
        out["n_valid"][r] = int((out["valid"][r] != 0).sum())
    return out


def brute_covered(select_row, D, rule, win, stride, frames, num_frames):
    """The frames the named windows of one row cover, as a set union over their frame lists - written without ``windows_valid``'s loop: the windows
    straight from the two rules' definitions (stage2.cut_windows' shifted windows, stage1.cut_windows' clipped ones)."""
    hop = win // stride
    count = max(0, -(-D // hop) - 1)
    lists = {}
    for i in range(count):
        s = i * win // stride
        e = min(s + win, D - 1)
        if rule == SHIFTED:
            if e - s < win:
                s = e - win
            s = max(s, 0)
        elif s > e:
            continue                                                    # a void window is no window
        lists[i] = set(int(t) for t in np.linspace(s, e, num_frames, dtype=np.int32)) if frames == SAMPLED else set(range(s, e + 1))
    covered = set()
    for i in select_row:
        covered |= lists.get(int(i), set())
    return covered
