"""The case tables of tests/test_gpu_sample_edges.py, built on the CPU from seeded rows and the float64 reference (tests/sample_oracle.py).  A table is a
list of ``Launch``: the rows of one ``ops.sample`` call, a uniform per row and the reference ``Row`` of each.  tests/test_sample_reference_logic.py walks
the same tables and asserts that every step a test relies on has a half-width of at least ``sample_oracle.MARGIN`` - so the GPU module excuses no draw
and no ``n_keep``.

The rows are short and only mildly peaked ON PURPOSE: a mid-step uniform at the LAST kept rank needs that rank's probability to be >= 2 * MARGIN, which
a row whose processed scores span more than about 7 cannot give at 64 candidates.  The list-path rows are therefore ``uniform(+-sqrt 3) * 1.25 * T``: the
processed scores span +-2.2 at every temperature, while T = 0.7 and T = 0.05 still exercise the kernel's float32 ``x * (1 / T)``."""
import functools

import numpy as np

from helpers import feats
from sample_oracle import Row, mid_step_top_p, mid_step_uniform

ONE_BELOW = float(np.nextafter(np.float32(1), np.float32(0)))      # the largest float32 uniform


class Launch:
    """x f32 [R, V], u f32 [R], one (T, top_k, top_p) and the reference Row of every row.  ``want`` [R] = ref.draw(u); ``hw`` [R] = the half-width
    of the CDF step the uniform sits in (None where the uniform is 0, ONE_BELOW or 1: the ends of the range need no margin, the answer there is the
    first / the last token with mass whatever the rounding); ``p_hw`` = the half-width of the top-p step (None at top_p = 1)."""

    def __init__(self, label, T, top_k, top_p, p_hw=None):
        self.label, self.T, self.top_k, self.top_p, self.p_hw = label, T, top_k, top_p, p_hw
        self.rows, self.refs, self.ranks, self.us, self.hw = [], [], [], [], []

    def add_rank(self, x, ref, rank):
        u, hw = mid_step_uniform(ref, rank)
        self._add(x, ref, rank, u, hw)

    def add_uniform(self, x, ref, u):
        self._add(x, ref, ref.draw_pos(u), u, None)

    def _add(self, x, ref, rank, u, hw):
        self.rows.append(np.asarray(x, dtype=np.float32))
        self.refs.append(ref)
        self.ranks.append(rank)
        self.us.append(float(np.float32(u)))
        self.hw.append(hw)

    @property
    def x(self):
        return np.stack(self.rows)

    @property
    def u(self):
        return np.asarray(self.us, dtype=np.float32)

    @property
    def want(self):
        return [ref.draw(u) for ref, u in zip(self.refs, self.us)]


def spread_ranks(n):
    """{0, 1, middle, last} of n kept tokens."""
    return sorted({0, min(1, n - 1), n // 2, n - 1})


# ---- the list path at short vocabularies -----------------------------------------------------------------------------------------------------------
LIST_V = (1, 2, 40, 63, 64, 65, 100, 1000, 1023, 1024, 1025, 4099, 32768)
LIST_K = (1, 7, 50, 64)
LIST_SETTINGS = ((1.0, 1.0), (0.7, "mid-step, 3 kept"), (0.05, 1.0))
LIST_SCALE = 1.25


def list_rows(V, T):
    return feats(f"smpe.list.v{V}", (3, V)).numpy() * np.float32(LIST_SCALE * T)


@functools.lru_cache(maxsize=None)
def list_launches(V):
    out = []
    for T, p in LIST_SETTINGS:
        x = list_rows(V, T)
        for k in LIST_K:
            if p == 1.0:
                L = Launch(f"list V{V} k{k} T{T}", T, k, 1.0)
                for b in range(3):
                    ref = Row(x[b], T, k, 1.0)
                    for r in spread_ranks(ref.n_keep):
                        L.add_rank(x[b], ref, r)
                out.append(L)
                continue
            for b in range(3):                         # a top_p of its own per row: one launch each
                base = Row(x[b], T, k, 1.0)
                n = min(3, base.n_keep)
                tp, p_hw = mid_step_top_p(base, n)
                L = Launch(f"list V{V} k{k} T{T} row{b} top-p leaving {n}", T, k, tp, p_hw)
                L.n_wanted = n
                ref = Row(x[b], T, k, tp)
                for r in spread_ranks(ref.n_keep):
                    L.add_rank(x[b], ref, r)
                out.append(L)
    return out


# ---- exact n_keep under top-p: the rows of a batch are permutations of one vector of distinct scores ---------------------------------------------------
NKEEP_V, NKEEP_B = 300, 4
# (top_k, the n_keep asked for).  top_k = 100 cannot keep 150 or 299: its last two are the last step (99) and the whole filtered set (100).
NKEEP_CASES = ((64, (1, 2, 17, 63, 64)), (0, (1, 2, 17, 150, 299)), (100, (1, 2, 17, 99, 100)))


def nkeep_rows():
    v = feats("smpe.nkeep.values", (NKEEP_V,)).numpy() * np.float32(0.8)
    rs = np.random.RandomState(20)
    return np.stack([v] + [v[rs.permutation(NKEEP_V)] for _ in range(NKEEP_B - 1)])


@functools.lru_cache(maxsize=None)
def nkeep_launches():
    x = nkeep_rows()
    out = []
    for k, wanted in NKEEP_CASES:
        base = Row(x[0], 1.0, k, 1.0)
        for n in wanted:
            tp, p_hw = mid_step_top_p(base, n)
            L = Launch(f"n_keep V{NKEEP_V} k{k} wanted {n}", 1.0, k, tp, p_hw)
            L.n_wanted = n
            for b in range(NKEEP_B):
                ref = Row(x[b], 1.0, k, tp)
                for r in sorted({0, ref.n_keep // 2, ref.n_keep - 1}):
                    L.add_rank(x[b], ref, r)
            out.append(L)
    return out


# ---- wide-path draws -----------------------------------------------------------------------------------------------------------------------------------
WIDE_V = (65, 1000, 1025, 4099)
WIDE_T = 0.8


def wide_top_ks(V):
    """{0, 65, V - 1, V, V + 7} as far as they take the wide path (V - 1 = 64 at V = 65 is the list path's: list_launches(65) has it)."""
    return sorted({k for k in (0, 65, V - 1, V, V + 7) if k == 0 or k > 64})


@functools.lru_cache(maxsize=None)
def wide_launches(V):
    x = feats(f"smpe.wide.v{V}", (3, V)).numpy() * np.float32(2.0)
    out = []
    for k in wide_top_ks(V):
        L = Launch(f"wide V{V} k{k}", WIDE_T, k, 1.0)
        for b in range(3):
            ref = Row(x[b], WIDE_T, k, 1.0)
            last = max(j for j, p in enumerate(ref.probs) if p >= 2e-4)
            for r in sorted({0, 1, 10, last}):
                L.add_rank(x[b], ref, r)
        out.append(L)
    return out


# ---- ties and signed zeros -----------------------------------------------------------------------------------------------------------------------------
TIE_V = 100


def tie_quantised_row():
    """(x * 2).round() / 2 of a seeded row; the zeros alternate -0.0, +0.0, .. by index, so the lowest-indexed zero is a -0.0 and a +0.0 follows it.
    -> (row, number of scores above zero, indices of the zeros)."""
    g = feats("smpe.tie.q", (TIE_V,)).numpy() * np.float32(2.0)
    q = (np.round(g * 2) / 2).astype(np.float32)
    zeros = [int(i) for i in np.flatnonzero(q == 0)]
    for n, i in enumerate(zeros):
        q[i] = np.float32(-0.0 if n % 2 == 0 else 0.0)
    return q, int((q > 0).sum()), zeros


def tie_flat_row(V=TIE_V):
    return np.full(V, 1.25, dtype=np.float32)


def tie_two_maxima_row():
    x = np.full(TIE_V, -30.0, dtype=np.float32)
    x[17] = x[71] = 2.0
    x[9] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def tie_launches():
    q, above, zeros = tie_quantised_row()
    out = []
    # both zeros inside the top top_k (the whole zero group is); the pair straddling the K-th place (only the first zero, a -0.0, is inside); the wide path
    for T in (1.0, 1.25):                             # (T < 1 peaks the row: the zero group's steps fall under the margin)
        for k in (above + len(zeros), above + 1, above + 2, 0, 65, TIE_V):
            L = Launch(f"ties quantised k{k} T{T}", T, k, 1.0)
            ref = Row(q, T, k, 1.0)
            in_group = [r for r in range(above, above + len(zeros)) if r < ref.n_keep]
            for r in sorted({0, above - 1, *in_group, min(above + len(zeros), ref.n_keep - 1)}):
                L.add_rank(q, ref, r)
            out.append(L)
    flat = tie_flat_row()
    for k in (7, 50, 64, 0, 65, TIE_V):
        L = Launch(f"ties flat k{k}", 1.0, k, 1.0)
        ref = Row(flat, 1.0, k, 1.0)
        for r in spread_ranks(ref.n_keep) + [ref.n_keep // 3]:
            L.add_rank(flat, ref, r)
        out.append(L)
    two = tie_two_maxima_row()
    for k in (2, 50, 0, 99):
        L = Launch(f"ties two maxima k{k}", 1.0, k, 1.0)
        ref = Row(two, 1.0, k, 1.0)
        for r in range(min(3, ref.n_keep)):
            L.add_rank(two, ref, r)
        out.append(L)
    return out


# ---- masked rows ---------------------------------------------------------------------------------------------------------------------------------------
MASK_V, MASK_FINITE, MASK_ROWS, MASK_T = 200, 10, 64, 0.8
MASK_TOP_KS = (50, 0, 100)
MASK_RANKS = (1, 5, MASK_FINITE - 1)


def masked_rows():
    vals = feats("smpe.masked", (MASK_ROWS, MASK_FINITE)).numpy()
    rs = np.random.RandomState(21)
    x = np.full((MASK_ROWS, MASK_V), -np.inf, dtype=np.float32)
    for b in range(MASK_ROWS):
        x[b, rs.permutation(MASK_V)[:MASK_FINITE]] = vals[b]
    return x


@functools.lru_cache(maxsize=None)
def masked_launches():
    x = masked_rows()
    out = []
    for k in MASK_TOP_KS:
        refs = [Row(x[b], MASK_T, k, 1.0) for b in range(MASK_ROWS)]
        # (u = 1.0 is outside [0, 1) - no generator hands it out - but it is the one uniform that reaches the clamp for certain: no sum exceeds it)
        for what in (0.0, ONE_BELOW, 1.0) + MASK_RANKS:
            L = Launch(f"masked k{k} " + (f"u={what}" if isinstance(what, float) else f"rank {what}"), MASK_T, k, 1.0)
            for b in range(MASK_ROWS):
                if isinstance(what, float):
                    L.add_uniform(x[b], refs[b], what)
                else:
                    L.add_rank(x[b], refs[b], what)
            out.append(L)
    return out


# ---- many rows: row indexing ---------------------------------------------------------------------------------------------------------------------------
MANY_B, MANY_V = 257, 64


@functools.lru_cache(maxsize=None)
def many_rows_launches():
    x = feats("smpe.many", (MANY_B, MANY_V)).numpy() * np.float32(LIST_SCALE)
    out = []
    for k in (50, 0):
        L = Launch(f"many rows B{MANY_B} V{MANY_V} k{k}", 1.0, k, 1.0)
        for b in range(MANY_B):
            ref = Row(x[b], 1.0, k, 1.0)
            L.add_rank(x[b], ref, b % ref.n_keep)
        out.append(L)
    return out


def all_launches():
    for V in LIST_V:
        yield from list_launches(V)
    yield from nkeep_launches()
    for V in WIDE_V:
        yield from wide_launches(V)
    yield from tie_launches()
    yield from masked_launches()
    yield from many_rows_launches()
