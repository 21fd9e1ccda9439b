"""The rule of ``rv_sample`` (include/revision_hip.h) a second time, one row at a time in float64: the HF warper chain temperature -> top-k -> top-p,
the inverse-CDF draw over the kept tokens in (score descending, index ascending) order, and the two entropies.  ``Row`` is what
tests/test_gpu_sample_edges.py compares the kernel with; tests/test_sample_reference_logic.py holds it to oracle/sampling.py and to rows worked out by
hand.  Nothing here is used by the package.

Only the first step is float32, because it decides WHICH numbers are compared: the processed score is ``x * (float32(1) / float32(T))`` as the kernel
forms it (model/revision_llama.py explains why that is not ``x / T``).  Everything after it - order, probabilities, cumulative sums, entropies - is
float64, added sequentially in the stated order.

``mid_step_uniform`` / ``mid_step_top_p`` place a uniform / a ``top_p`` in the MIDDLE of a step of the float64 sums and report the half-width of that
step, so a test can ask for exact tokens and exact ``n_keep`` wherever the half-width exceeds the float32 sums' error (MARGIN)."""
import math

import numpy as np

LIST_CAP = 64          # the kernel's candidate list (hip.TOPK_CAP): 1 <= top_k <= 64 keeps exactly min(top_k, V) entries
MARGIN = 1e-4          # smallest half-width of a step a test may rely on (the kernel's f32 sums err by about 64 * 3 * 2^-24 = 1.2e-5)


def processed_f32(x, temperature):
    """x [V] (anything float32-valued) -> float32 [V]: the kernel's v * (1.0f / temperature), both operations in float32."""
    x = np.asarray(x, dtype=np.float32)
    inv_t = np.float32(1.0) / np.float32(temperature)
    with np.errstate(all="ignore"):
        return np.multiply(x, inv_t, dtype=np.float32)


def _entropy(p):
    h = 0.0
    for v in p:
        h -= v * math.log(v + 1e-10)
    return h


def _softmax(s):
    """float64 probabilities of the scores s (a list); -inf gives exactly 0."""
    mx = max(s)
    e = [math.exp(v - mx) if v != -math.inf else 0.0 for v in s]
    z = 0.0
    for v in e:
        z += v
    return [v / z for v in e]


_BASE = {}


def _base(x, temperature):
    """What depends on the row and the temperature alone, kept per (row, T): the processed scores, the order of every index and the raw entropy."""
    key = (x.tobytes(), float(np.float32(temperature)))
    if key not in _BASE:
        s32 = processed_f32(x, temperature)
        s = s32.astype(np.float64)
        # (score descending, index ascending): the last key of lexsort is the first criterion; -0.0 and +0.0 compare equal, so the index decides
        order = [int(i) for i in np.lexsort((np.arange(x.size), -s))]
        _BASE[key] = (s32, order, _entropy(_softmax([float(v) for v in x])))
    return _BASE[key]


class Row:
    """One row through the warper chain.  ``top_k`` 0 / None = no top-k filter; 1 .. 64 = list mode (exactly min(top_k, V) entries: inside a tie
    at the k-th place the lowest indices); > 64 = wide mode (a tie at the k-th place stays whole).  At least one score must be finite, none NaN.

    order      every index, (score descending, index ascending); -0.0 equals +0.0
    kept       the kept indices in that order;  n_keep = len(kept)
    probs      their probabilities (softmax over the kept scores), cdf = the inclusive descending cumulative sums
    threshold  the smallest kept processed score (float32 value)
    scores     float32 [V]: the processed scores, -inf where a filter removed the token
    entropy_proc / entropy_raw   -sum p * log(p + 1e-10) over the kept / over softmax(x)"""

    def __init__(self, x, temperature=1.0, top_k=0, top_p=1.0):
        x = np.asarray(x, dtype=np.float32)
        assert x.ndim == 1 and x.size >= 1 and not np.isnan(x).any() and np.isfinite(x).any()
        self.V = V = x.size
        self.top_k = top_k = int(top_k or 0)
        self.top_p = float(np.float32(top_p))                    # what the kernel receives
        self.list_mode = 1 <= top_k <= LIST_CAP
        self.s32, self.order, self.entropy_raw = _base(x, temperature)
        s = self.s32.astype(np.float64)
        # top-k
        kept = list(self.order)
        if top_k > 0:
            k = min(top_k, V)
            kth = s[self.order[k - 1]]
            kept = self.order[:k] if self.list_mode else [i for i in self.order if s[i] >= kth]
        self.after_top_k = list(kept)
        # top-p: ascending order = the descending order backwards; the prefix whose inclusive cumulative probability is <= 1 - top_p goes
        if self.top_p < 1.0:
            p = _softmax([s[i] for i in kept])
            cum, removed = 0.0, 0
            for j in range(len(kept) - 1, 0, -1):                 # (position 0, the largest, always stays)
                cum += p[j]
                if cum <= 1.0 - self.top_p:
                    removed += 1
                else:
                    break
            kept = kept[:len(kept) - removed]
        self.kept = kept
        self.n_keep = len(kept)
        self.probs = _softmax([s[i] for i in kept])
        self.cdf = []
        c = 0.0
        for v in self.probs:
            c += v
            self.cdf.append(c)
        self.threshold = self.s32[kept[-1]]
        self.scores = np.full(V, -np.inf, dtype=np.float32)
        for i in kept:
            self.scores[i] = self.s32[i]
        self.entropy_proc = _entropy(self.probs)
        self.last_positive = max(j for j, v in enumerate(self.probs) if v > 0.0)

    def draw_pos(self, u):
        """The first position whose inclusive cumulative probability exceeds u, clamped to the last position with p > 0."""
        for j, c in enumerate(self.cdf):
            if c > u:
                return min(j, self.last_positive)
        return self.last_positive

    def draw(self, u):
        return self.kept[self.draw_pos(u)]


def mid_step_uniform(row, rank):
    """-> (u, half-width): the middle of the CDF interval that draws position ``rank`` of row.kept."""
    lo = row.cdf[rank - 1] if rank > 0 else 0.0
    hi = row.cdf[rank]
    return (lo + hi) / 2, (hi - lo) / 2


def mid_step_top_p(row, n_keep):
    """-> (top_p, half-width) for a ``row`` built with top_p = 1: ``1 - top_p`` in the middle of the step of the ascending cumulative sum over
    row.kept that leaves exactly ``n_keep`` tokens (the m - n_keep smallest go; the step's upper end for n_keep = 1 is the whole mass, as the
    largest token always stays)."""
    m = row.n_keep
    assert row.top_p >= 1.0 and 1 <= n_keep <= m
    asc = [0.0]                                   # asc[j] = the sum of the j smallest probabilities, added smallest first
    for v in reversed(row.probs):
        asc.append(asc[-1] + v)
    lo, hi = asc[m - n_keep], (asc[m - n_keep + 1] if n_keep > 1 else 1.0)
    return 1.0 - (lo + hi) / 2, (hi - lo) / 2
