"""rv_span_propose (the kernel behind ``ops.span_propose`` / ``eval.similarity.propose_spans`` / ``ground_queries``: candidate spans from a similarity
row in one launch) against tests/propose_oracle.py, the rule restated in numpy float32 operation by operation.  The oracle IS the f32 rule, so ``windows``,
``n_spans`` and ``n_found`` must be equal and ``spans`` and ``smoothed`` must have the oracle's bits; no case is left out and there is no tolerance.  (One
thing is compared as a class, not as bits: where s' is NaN the oracle must have a NaN too - which NaN an addition returns is the adder's choice, and no
rule here looks at it.)  tests/test_propose_host_logic.py holds the oracle itself to a brute-force statement of the rule.

Every direct call writes into buffers with 64 sentinel elements on either side of each output, and ``smoothed`` must still hold the sentinel from each
row's D on; the surroundings are compared bitwise.  In every case the frames of ``sims`` from D on are NaN: a read past the duration would show in a result.
A tile is 256 frames and a wave 64, so the shapes sit around 64, 256 and 512; the kernel is f32 only, and the module runs in both builds because each
library carries its own copy of it."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import propose_oracle as P
from helpers import fl

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")
PAD = 64
NAN, INF = float("nan"), float("inf")
LEVELS = (0.5, 0.6, 0.7, 0.8, 0.9)


@pytest.fixture(scope="module", params=[None] if _FORCED else ["f16", "bf16"])
def flav(request, op_flavour):
    from revisionllm_amd import hip
    f = request.param or op_flavour or hip.flavour()
    prev = hip.set_flavour(f)
    yield f
    hip.set_flavour(prev)


@pytest.fixture(scope="module")
def dev(flav):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import hip
    hip.lib()
    return torch.device("cuda:0")


# ------------------------------------------------------------------ running the entry ------------------------------------------------------------------
class _Guarded:
    """An output of ``n`` elements inside a sentinel-filled buffer."""

    def __init__(self, n, dtype, dev):
        self.n = n
        self.sentinel = -12345 if dtype == torch.int32 else -777.25
        self.buf = torch.full((n + 2 * PAD,), self.sentinel, dtype=dtype, device=dev)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + PAD * self.buf.element_size())

    def take(self, shape):
        b = self.buf.cpu()
        assert bool((b[:PAD] == self.sentinel).all()) and bool((b[PAD + self.n:] == self.sentinel).all()), "a write outside the output"
        return b[PAD:PAD + self.n].reshape(shape).numpy()


def durations(L, Ds):
    return (np.arange(L)[None, :] < np.asarray(Ds)[:, None]).astype(np.float32)


def fenced(sims, mask):
    """The rows with NaN from each row's duration on (mask [R / rpm, L] of 0 / 1 prefixes)."""
    sims = np.array(sims, dtype=np.float32)
    rpm = sims.shape[0] // mask.shape[0]
    sims[np.repeat(mask, rpm, axis=0) == 0] = NAN
    return sims


def run(dev, sims, mask, levels=LEVELS, relative=1, smooth=1, gap=0, min_len=1, max_len=0, N=64, windows=True, smoothed=True, n_found=True):
    """The C entry on numpy inputs -> dict like the oracle's (parts not asked for: None), after the sentinel checks."""
    from revisionllm_amd import hip
    R, L = sims.shape
    rpm = R // mask.shape[0]
    s = torch.from_numpy(np.ascontiguousarray(sims, dtype=np.float32)).to(dev)
    m = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float32)).to(dev)
    o = dict(spans=_Guarded(R * N * 2, torch.float32, dev), n_spans=_Guarded(R, torch.int32, dev), n_found=_Guarded(R, torch.int32, dev) if n_found else None,
             windows=_Guarded(R * N * 2, torch.int32, dev) if windows else None, smoothed=_Guarded(R * L, torch.float32, dev) if smoothed else None)
    ptr = lambda x: x.ptr if x is not None else None                                            # noqa: E731
    table = (ctypes.c_float * len(levels))(*levels)
    rc = hip.lib().rv_span_propose(hip.ptr(s), hip.ptr(m), R, rpm, L, table, len(levels), relative, smooth, gap, min_len, max_len, N, ptr(o["spans"]),
                                   ptr(o["n_spans"]), ptr(o["n_found"]), ptr(o["windows"]), ptr(o["smoothed"]), hip.stream())
    hip.check(rc, "rv_span_propose")
    torch.cuda.synchronize()
    shapes = dict(spans=(R, N, 2), n_spans=(R,), n_found=(R,), windows=(R, N, 2), smoothed=(R, L))
    out = {k: (v.take(shapes[k]) if v is not None else None) for k, v in o.items()}
    out["sentinel"] = -777.25
    return out


def same(got, ref, what=""):
    for k in ("windows", "n_spans", "n_found"):
        if got[k] is not None:
            assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:4].tolist())
    a, b = got["spans"].view(np.uint32), np.ascontiguousarray(ref["spans"]).view(np.uint32)
    assert np.array_equal(a, b), (what, "spans", np.argwhere(a != b)[:4].tolist())
    if got["smoothed"] is not None:
        for r, (sp, D) in enumerate(zip(ref["smoothed"], ref["D"])):
            g = got["smoothed"][r]
            assert (g[D:] == got["sentinel"]).all(), (what, "smoothed written past the duration", r)
            nan = np.isnan(sp)
            assert np.array_equal(np.isnan(g[:D]), nan), (what, "smoothed NaN places", r)
            assert np.array_equal(g[:D][~nan].view(np.uint32), sp[~nan].view(np.uint32)), (what, "smoothed", r, np.argwhere(g[:D] != sp)[:4].tolist())


def check(dev, sims, mask, what="", **kw):
    """Fence, run, compare with the oracle -> (got, ref)."""
    sims = fenced(sims, mask)
    got = run(dev, sims, mask, **kw)
    ok = {k: v for k, v in kw.items() if k in ("levels", "relative", "smooth", "gap", "min_len", "max_len", "N")}
    ref = _oracle(sims.tobytes(), sims.shape, mask.tobytes(), mask.shape, tuple(sorted(ok.items())))
    same(got, ref, what)
    return got, ref


@functools.lru_cache(maxsize=None)
def _oracle(sims_b, sims_shape, mask_b, mask_shape, kw):
    """The oracle once per distinct case: both builds' runs share it."""
    sims = np.frombuffer(sims_b, dtype=np.float32).reshape(sims_shape)
    mask = np.frombuffer(mask_b, dtype=np.float32).reshape(mask_shape)
    kw = dict(kw)
    kw.setdefault("levels", LEVELS)
    kw.setdefault("N", 64)
    return P.propose(sims, mask, **kw)


def bumpy(R, L, seed):
    """Rows as a cosine row looks: a few raised stretches of several heights on noise."""
    rng = np.random.default_rng(seed)
    s = rng.normal(0.0, 0.05, (R, L)).astype(np.float32)
    for r in range(R):
        for _ in range(int(rng.integers(1, 6))):
            a = int(rng.integers(0, L))
            s[r, a:a + int(rng.integers(1, max(2, L // 4)))] += np.float32(rng.choice([0.3, 0.5, 0.8, 1.0]))
    return s


# ------------------------------------------------------------------ sizes and layouts ------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 127, 129, 255, 256, 257, 511, 513, 1000])
def test_sizes(dev, L):
    """D = L, L - 1, 1 and 0 (two rows each), smoothing and gap closing on."""
    Ds = [L, L, max(L - 1, 0), max(L - 1, 0), 1, 1, 0, 0]
    _, ref = check(dev, bumpy(8, L, L), durations(L, Ds), f"L={L}", smooth=3, gap=1)
    assert ref["D"] == Ds
    check(dev, bumpy(8, L, L + 1), durations(L, Ds), f"L={L} plain")
    if L >= 63:
        assert ref["n_found"][:2].min() > 0


@pytest.mark.parametrize("R", [1, 3, 5, 260])
def test_row_counts(dev, R):
    L = 150
    rng = np.random.default_rng(R)
    check(dev, bumpy(R, L, 40 + R), durations(L, rng.integers(0, L + 1, R)), f"R={R}", smooth=5, gap=2, N=16)


def test_three_rows_per_mask_row(dev):
    """rpm = 3: a video's mask row is shared by three rows with different sims."""
    L = 300
    Ds = [300, 257, 64, 0]
    sims = bumpy(12, L, 3)
    got, ref = check(dev, sims, durations(L, Ds), "rpm=3", smooth=3, gap=1)
    assert ref["D"] == [300] * 3 + [257] * 3 + [64] * 3 + [0] * 3
    assert len({got["windows"][r].tobytes() for r in range(3)}) == 3


def test_the_bql_form_and_the_optional_parts(dev):
    from revisionllm_amd import ops
    B, Q, L = 3, 4, 200
    mask = durations(L, [200, 131, 77])
    sims = fenced(bumpy(B * Q, L, 17), mask)
    ref = P.propose(sims, mask, LEVELS, smooth=3, gap=1, min_len=2, max_len=90, N=32)
    s, m = torch.from_numpy(sims).view(B, Q, L).to(dev), torch.from_numpy(mask).to(dev)
    for mk in (m, m.bool(), m.to(torch.int32), m.to(torch.uint8), m.half(), m.double()):
        out = ops.span_propose(s, mk, smooth=3, gap=1, min_len=2, max_len=90, max_spans=32, return_windows=True, return_smoothed=True)
        assert out.spans.shape == (B, Q, 32, 2) and out.n_spans.shape == (B, Q) and out.windows.shape == (B, Q, 32, 2) and out.smoothed.shape == (B, Q, L)
        got = dict(spans=out.spans.cpu().numpy().reshape(B * Q, 32, 2), n_spans=out.n_spans.cpu().numpy().reshape(-1),
                   n_found=out.n_found.cpu().numpy().reshape(-1), windows=out.windows.cpu().numpy().reshape(B * Q, 32, 2), smoothed=None)
        same(got, ref, str(mk.dtype))
        sm = out.smoothed.cpu().numpy().reshape(B * Q, L)
        for r, D in enumerate(ref["D"]):
            assert np.isnan(sm[r, D:]).all() and np.array_equal(sm[r, :D].view(np.uint32), ref["smoothed"][r].view(np.uint32))
    bare = ops.span_propose(s, m, smooth=3, gap=1, min_len=2, max_len=90, max_spans=32)
    assert bare.windows is None and bare.smoothed is None and torch.equal(bare.spans.view(torch.int32), out.spans.view(torch.int32))
    flat = ops.span_propose(s.view(B * Q, L), m, smooth=3, gap=1, min_len=2, max_len=90, max_spans=32)          # [R, L] with fewer mask rows: rpm = R / rows
    assert torch.equal(flat.spans.view(torch.int32), out.spans.view(torch.int32).view(B * Q, 32, 2))
    assert ref["n_found"].max() > 3


# ------------------------------------------------------------------ wave and tile edges ------------------------------------------------------------------
def _steps(L, runs, low=0.0, high=1.0):
    s = np.full(L, low, dtype=np.float32)
    for a, b in runs:
        s[a:b] = high
    return s


def test_runs_that_straddle_wave_and_tile_edges(dev):
    L = 1000
    cases = [[(60, 70)], [(250, 262)], [(0, L)], [(200, 800)], [(60, 70), (250, 262), (500, 530), (767, 769)], [(63, 64)], [(64, 65)], [(255, 256)],
             [(256, 257)], [(0, 1)], [(L - 1, L)], [(0, 256)], [(256, 512)], [(255, 513)], [(0, 64), (128, 192)], [(1, 999)]]
    sims = np.stack([_steps(L, c) for c in cases])
    for gap, smooth in ((0, 1), (3, 1), (63, 1), (0, 3)):
        got, ref = check(dev, sims, durations(L, [L] * len(cases)), f"gap={gap}", levels=(0.5,), relative=0, gap=gap, smooth=smooth)
        if smooth == 1 and gap == 0:
            for r, c in enumerate(cases):
                assert got["windows"][r, :len(c)].tolist() == [list(x) for x in c] and got["n_found"][r] == len(c)
    short = durations(L, [900] * len(cases))                                  # the run to the row's end now ends at D
    got, _ = check(dev, sims, short, "D=900", levels=(0.5,), relative=0)
    assert got["windows"][2, 0].tolist() == [0, 900] and got["windows"][10, 0].tolist() == [-1, -1]
    # three levels, the nested runs of a pyramid across both edges of the tile 256 .. 511
    pyr = np.zeros((1, L), dtype=np.float32)
    pyr[0, 200:600], pyr[0, 250:520], pyr[0, 300:400] = 1.0, 2.0, 3.0
    got, _ = check(dev, pyr, durations(L, [L]), "pyramid", levels=(0.1, 0.5, 0.9))
    assert got["windows"][0, :4].tolist() == [[300, 400], [250, 520], [200, 600], [-1, -1]]


@pytest.mark.parametrize("gap", [0, 1, 2, 63])
def test_gaps_astride_frames_63_64_and_255_256(dev, gap):
    """Below-threshold stretches of exactly ``gap`` (closed) and ``gap + 1`` (open) frames lying across the wave edge and the tile edge, at several
    offsets, between two 5-frame stretches above."""
    L = 700
    rows, want = [], []
    for edge in (64, 256, 512):
        for g in (gap, gap + 1):
            for shift in sorted({0, 1, g // 2, g - 1, g} - {-1}):
                if g == 0 or shift > g:
                    continue
                p = edge - shift                                              # the stretch [p, p + g) has `shift` frames before the edge
                a = max(p - 5, 0)
                if a == p:
                    continue
                rows.append(_steps(L, [(a, p), (p + g, p + g + 5)]))
                want.append([[a, p + g + 5]] if g <= gap else [[a, p], [p + g, p + g + 5]])
    assert len(rows) >= 6
    got, _ = check(dev, np.stack(rows), durations(L, [L] * len(rows)), f"gap={gap}", levels=(0.5,), gap=gap)
    for r, w in enumerate(want):
        assert got["windows"][r, :len(w)].tolist() == w and got["n_found"][r] == len(w), (r, w)


@pytest.mark.parametrize("smooth", [1, 3, 65])
def test_smoothing(dev, smooth):
    """The halo crosses tile edges and both row ends; D below the window; an arithmetic row whose sums round (order matters)."""
    L = 600
    Ds = [600, 599, 513, 512, 300, 257, 256, 255, 70, 33, 32, 10, 2, 1, 0]
    rng = np.random.default_rng(smooth)
    sims = (rng.normal(0.3, 0.2, (len(Ds), L)) * rng.choice([1.0, 1e-3, 1e3], (len(Ds), 1))).astype(np.float32)
    check(dev, sims, durations(L, Ds), f"smooth={smooth}", smooth=smooth, gap=1)
    check(dev, bumpy(len(Ds), L, 60 + smooth), durations(L, Ds), f"smooth={smooth} bumpy", smooth=smooth, levels=(0.2, 0.5, 0.8))


# ------------------------------------------------------------------ levels ------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 5, 8])
def test_level_counts(dev, T):
    levels = tuple(np.linspace(0.1, 0.9, T).tolist()) if T > 1 else (0.5,)
    L = 520
    for relative in (1, 0):
        got, ref = check(dev, bumpy(6, L, 70 + T), durations(L, [520, 519, 400, 256, 100, 7]), f"T={T}", levels=levels, relative=relative, smooth=3, gap=2, N=128)
    assert ref["n_found"].max() >= T


def test_duplicates_across_two_and_three_levels(dev):
    """Staircases: a run shared by 2 and by 3 consecutive levels is kept once, at the highest; the same steps astride the edges."""
    L = 600
    rows = np.zeros((4, L), dtype=np.float32)
    rows[0, 10:50], rows[0, 20:40], rows[0, 100:130] = 1.0, 4.0, 4.0                       # (100, 130) at all four levels
    rows[1, 60:70], rows[1, 250:262], rows[1, 255:258] = 2.0, 3.0, 4.0                      # (60, 70) at two levels, (250, 262) at three
    rows[2, 0:600], rows[2, 200:300] = 1.0, 2.0
    rows[2, 0] = 0.0                                                                        # (1, 600) at one level, (200, 300) at one
    rows[3, 500:520], rows[3, 505:515] = 3.0, 4.0
    levels = (0.1, 0.3, 0.6, 0.9)                                                           # thresholds 0.4, 1.2, 2.4, 3.6 on rows with mn 0, mx 4
    rows[2, 599] = 4.0
    got, _ = check(dev, rows, durations(L, [L] * 4), "stairs", levels=levels)
    assert got["windows"][0, :4].tolist() == [[20, 40], [100, 130], [10, 50], [-1, -1]]
    assert got["windows"][1, :4].tolist() == [[255, 258], [250, 262], [60, 70], [-1, -1]]
    assert got["windows"][3, :3].tolist() == [[505, 515], [500, 520], [-1, -1]]
    assert got["windows"][2, :4].tolist() == [[599, 600], [200, 300], [1, 600], [-1, -1]]
    assert got["n_found"].tolist() == [3, 3, 3, 2]


def test_levels_that_round_to_one_threshold_and_thresholds_that_are_attained(dev):
    L = 300
    one = np.float32(1.0)
    tiny = np.full((2, L), one, dtype=np.float32)
    tiny[:, 100:260] = np.nextafter(one, np.float32(2))                                     # mx - mn = one ulp: every level in (0, 0.5) gives theta = mn
    tiny[1, 150] = one
    got, ref = check(dev, tiny, durations(L, [L, L]), "equal thresholds", levels=(0.1, 0.2, 0.3, 0.7))
    assert got["windows"][0, :2].tolist() == [[100, 260], [-1, -1]] and got["n_found"].tolist() == [1, 2]
    s = np.tile(np.array([0.25, 0.5, 0.75, 0.5], dtype=np.float32), L // 4)[None]
    got, _ = check(dev, s, durations(L, [L]), "attained", levels=(0.25, 0.5, 0.75), relative=0, N=256)
    assert got["n_found"].tolist() == [75 + 75] and got["windows"][0, 0].tolist() == [2, 3] and got["windows"][0, 75].tolist() == [1, 4]
    got, _ = check(dev, s, durations(L, [L]), "attained, relative", levels=(0.0, 0.5), relative=1, N=256)   # theta = 0.25 and 0.5: 0.5 > 0.5 is false
    assert got["windows"][0, 0].tolist() == [2, 3] and got["windows"][0, 75].tolist() == [1, 4]


# ------------------------------------------------------------------ capacity ------------------------------------------------------------------
def test_capacity(dev):
    L = 1000
    comb = np.zeros((2, L), dtype=np.float32)
    comb[0, 1::2] = 1.0                                                                     # 500 runs of one frame at each level: kept at the highest
    comb[1, 1::2] = 1.0
    comb[1, 1::4] = 2.0                                                                     # 250 at the upper level, 500 at the lower, 250 shared
    mask = durations(L, [L, L])
    for N in (499, 500, 501, 1, 2048, 249, 250, 251):
        got, ref = check(dev, comb, mask, f"N={N}", levels=(0.2, 0.7), N=N)
        assert got["n_found"].tolist() == [500, 500] and got["n_spans"].tolist() == [min(N, 500)] * 2
    got, _ = check(dev, comb, mask, "N=300", levels=(0.2, 0.7), N=300)
    assert got["windows"][1, 249].tolist() == [997, 998] and got["windows"][1, 250].tolist() == [3, 4]       # the lower level fills what is left
    for N in (3, 4, 5):
        got, ref = check(dev, bumpy(3, 400, 9), durations(400, [400, 300, 5]), f"small N={N}", smooth=3, N=N)
    assert ref["n_found"].max() > 5


# ------------------------------------------------------------------ non-finite values ------------------------------------------------------------------
def test_non_finite_values(dev):
    L = 400
    base = _steps(L, [(20, 60), (100, 140), (250, 262), (300, 330)], 0.1, 0.9)
    rows = []
    for at in ([30], [20], [59], [80], [0], [255, 256], [61, 62], [19], list(range(140, 250))):
        x = base.copy()
        x[at] = NAN
        rows.append(x)
    for v, at in ((INF, 120), (-INF, 120), (INF, 200), (-INF, 200)):
        x = base.copy()
        x[at] = v
        rows.append(x)
    both = base.copy()
    both[5], both[350] = INF, -INF
    rows += [both, np.full(L, NAN, dtype=np.float32), np.full(L, 0.5, dtype=np.float32)]
    sims = np.stack(rows)
    mask = durations(L, [L] * len(rows))
    for kw in (dict(), dict(gap=1), dict(smooth=3), dict(smooth=3, gap=2), dict(relative=0), dict(relative=0, smooth=5, gap=1)):
        got, ref = check(dev, sims, mask, str(kw), **kw)
        assert got["n_found"][-2:].tolist() == [0, 0]                                       # all NaN, flat
    got, _ = check(dev, sims, mask, "plain, absolute", relative=0, levels=(0.5,))
    assert got["windows"][0, :2].tolist() == [[20, 30], [31, 60]] and got["windows"][9, 1].tolist() == [100, 140]   # a NaN splits a run; +inf is above
    fence = np.full((3, L), NAN, dtype=np.float32)                                          # NaN rows around a short row, NaN behind its duration
    fence[1, :100] = base[:100]
    got, _ = check(dev, fence, durations(L, [0, 100, 0]), "fences", relative=0, levels=(0.5,), smooth=3)
    assert got["n_found"].tolist() == [0, 1, 0]


# ------------------------------------------------------------------ independence, round trip ------------------------------------------------------------------
def test_a_row_does_not_depend_on_the_batch_or_its_place(dev):
    L, R = 300, 260
    sims = bumpy(R, L, 23)
    Ds = np.random.default_rng(4).integers(1, L + 1, R)
    row, D = bumpy(1, L, 99), 277
    for at in (0, 130, 259):
        sims[at], Ds[at] = row[0], D
    kw = dict(smooth=5, gap=2, N=32)
    got, _ = check(dev, sims, durations(L, Ds), "R=260", **kw)
    alone, _ = check(dev, row, durations(L, [D]), "R=1", **kw)
    assert alone["n_found"][0] > 2
    for at in (0, 130, 259):
        for k in ("spans", "windows", "n_spans", "n_found"):
            assert got[k][at].tobytes() == alone[k][0].tobytes(), (at, k)
        assert got["smoothed"][at, :D].tobytes() == alone["smoothed"][0, :D].tobytes()


def test_the_spans_give_back_their_windows_through_span_scores(dev):
    """``ops.span_scores(..., return_windows=True)`` on the generated spans equals ``windows``, padding included."""
    from revisionllm_amd import ops
    for L, Ds in ((1000, [1000, 999, 513, 1]), (257, [257, 256, 100, 0])):
        mask = durations(L, Ds)
        sims = fenced(bumpy(len(Ds), L, L), mask)
        s, m = torch.from_numpy(sims).to(dev), torch.from_numpy(mask).to(dev)
        out = ops.span_propose(s, m, levels=(0.2, 0.4, 0.6, 0.8), smooth=3, gap=1, max_spans=48, return_windows=True)
        scores, win = ops.span_scores(torch.nan_to_num(s), out.spans, m, return_windows=True)
        assert torch.equal(win, out.windows)
        n = out.n_spans.cpu()
        assert int(n.max()) > 4 and bool((out.windows.cpu()[0, :int(n[0]), 1] > out.windows.cpu()[0, :int(n[0]), 0]).all())
        assert bool(torch.isnan(scores.cpu()[3, int(n[3]):]).all())
    B, Q = 2, 3
    mask = durations(300, [300, 150])
    s = torch.from_numpy(fenced(bumpy(B * Q, 300, 5), mask)).view(B, Q, 300).to(dev)
    out = ops.span_propose(s, torch.from_numpy(mask).to(dev), gap=2, max_spans=16, return_windows=True)
    assert torch.equal(ops.span_scores_multi(torch.nan_to_num(s), out.spans, torch.from_numpy(mask).to(dev), return_windows=True)[1], out.windows)


# ------------------------------------------------------------------ the grounder ------------------------------------------------------------------
def _features(B, L, d, Q, seed, op16):
    g = torch.Generator().manual_seed(seed)
    video = torch.randn(B, L, d, generator=g)
    text = torch.randn(B, Q, d, generator=g)
    for b in range(B):
        for q in range(Q):
            a = 20 + 37 * q + 11 * b
            video[b, a:a + 25 + 9 * q] += 1.5 * text[b, q]                                  # each query has a stretch of its own
    return text, video.to(op16) if op16 is not None else video


def _chained(text, video, mask, top, nms_iou, gt, **pk):
    """The four public calls one by one, and the gather on the host."""
    from revisionllm_amd import ops
    multi = text.dim() == 3
    sims = (ops.frame_cosine_multi if multi else ops.frame_cosine)(text.float(), video)
    prop = ops.span_propose(sims, mask, **pk)
    scores = (ops.span_scores_multi if multi else ops.span_scores)(sims, prop.spans, mask.float())
    rank = ops.span_rank(scores, prop.spans, top=top, nms_iou=nms_iou, gt=gt)
    keep, n = rank.keep.cpu(), prop.n_spans.cpu()
    sp, sc = prop.spans.cpu(), scores.cpu()
    spans = torch.full(keep.shape + (2,), NAN)
    kept = torch.full(keep.shape, NAN)
    count = torch.zeros(keep.shape[:-1], dtype=torch.int32)
    for idx in np.ndindex(*keep.shape):
        i = int(keep[idx])
        if 0 <= i < int(n[idx[:-1]]):
            spans[idx], kept[idx] = sp[idx[:-1] + (i,)], sc[idx[:-1] + (i,)]
            count[idx[:-1]] += 1
    return spans, kept, count, prop, rank


def _bits(t):
    return t.cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.cpu()


def test_ground_queries_is_the_four_calls_chained(dev):
    from revisionllm_amd.eval.similarity import ground_queries
    op16 = {"f16": torch.float16, "bf16": torch.bfloat16}[fl()]
    B, L, d, Q = 3, 300, 64, 4
    mask = torch.from_numpy(durations(L, [300, 257, 140])).to(dev)
    pk = dict(levels=(0.3, 0.5, 0.7, 0.9), smooth=5, gap=2, min_len=3, max_spans=24, return_windows=True)
    for dt in (None, op16):
        text, video = _features(B, L, d, Q, 31, dt)
        gt = torch.tensor([[[0.05, 0.2]] * Q] * B)
        for t, g in ((text.to(dev), gt.to(dev)), (text[:, 0].contiguous().to(dev), gt[:, 0].contiguous().to(dev))):
            out = ground_queries(t, video.to(dev), mask, top=6, nms_iou=0.4, gt=g, **pk)
            spans, kept, count, prop, rank = _chained(t, video.to(dev), mask, 6, 0.4, g, **pk)
            assert out.spans.shape == t.shape[:-1] + (6, 2) and out.scores.shape == t.shape[:-1] + (6,) and out.spans.device == dev
            assert torch.equal(_bits(out.spans), _bits(spans)) and torch.equal(_bits(out.scores), _bits(kept)) and torch.equal(out.n_keep.cpu(), count)
            for a, b in list(zip(out.proposals, prop)) + list(zip(out.rank, rank)):
                assert (a is None and b is None) or torch.equal(_bits(a), _bits(b))
            assert int(out.n_keep.min()) >= 1 and out.rank.first_hit is not None
    host = ground_queries(text, video, mask.cpu().bool(), top=6, nms_iou=0.4, **pk)              # host tensors: staged, results back on the host
    assert not host.spans.is_cuda and not host.proposals.windows.is_cuda and not host.rank.keep.is_cuda
    again = ground_queries(text.to(dev), video.to(dev), mask, top=6, nms_iou=0.4, **pk)
    assert torch.equal(_bits(host.spans), _bits(again.spans)) and torch.equal(host.rank.keep, again.rank.keep.cpu())


@pytest.mark.parametrize("ab", [(40, 90), (250, 262), (255, 256), (0, 299), (1, 300), (256, 300), (1, 257), (63, 65), (100, 256)])
def test_ground_queries_finds_a_planted_stretch(dev, ab):
    """Frames [a, b) equal to the text direction, the rest orthogonal to it: the best proposal's window is exactly (a, b)."""
    from revisionllm_amd.eval.similarity import ground_queries
    a, b = ab
    L, d = 300, 16
    video = torch.zeros(2, L, d)
    video[:, :, 1] = 1.0
    video[0, a:b] = 0.0
    video[0, a:b, 0] = 2.0
    video[1] = video[0]
    text = torch.zeros(2, 3, d)
    text[:, :, 0] = 0.5
    text[1, 1, 0], text[1, 1, 1] = 0.0, 1.0                                                 # this query matches the other frames
    op16 = {"f16": torch.float16, "bf16": torch.bfloat16}[fl()]
    for v in (video, video.to(op16)):
        out = ground_queries(text.to(dev), v.to(dev), torch.ones(2, L).to(dev), return_windows=True)
        win, keep = out.proposals.windows.cpu(), out.rank.keep.cpu()
        for bq in ((0, 0), (0, 2), (1, 0)):
            assert win[bq][int(keep[bq][0])].tolist() == [a, b] and int(out.n_keep[bq]) == 1
        got = {tuple(w) for w in win[1, 1][: int(out.proposals.n_spans[1, 1])].tolist()}
        assert got == {w for w in ((0, a), (b, L)) if w[1] > w[0]}
        single = ground_queries(text[:, 0].contiguous().to(dev), v.to(dev), torch.ones(2, L).to(dev), return_windows=True)
        assert single.proposals.windows.cpu()[0][int(single.rank.keep[0, 0])].tolist() == [a, b]
        assert float(single.spans[0, 0, 0]) == pytest.approx((a + b) / 2 / L, abs=1e-6) and float(single.spans[0, 0, 1]) == pytest.approx((b - a - 0.5) / L, abs=1e-6)


def test_the_calls_do_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the calls: with the stream kept busy by work queued before them, an event recorded just before a
    call has not completed when the call returns (a call that waited for its own kernel would have waited for that work first)."""
    from revisionllm_amd.eval.similarity import ground_queries, propose_spans
    text, video = _features(4, 300, 64, 3, 77, torch.float16 if fl() == "f16" else torch.bfloat16)
    text, video, mask = text.to(dev), video.to(dev), torch.ones(4, 300, device=dev)
    sims = torch.from_numpy(bumpy(12, 300, 1)).view(4, 3, 300).to(dev)
    gt = torch.tensor([0.25, 0.5]).repeat(4, 3, 1).to(dev)
    one, flags = text[:, 0].contiguous(), mask.bool()
    calls = (lambda: propose_spans(sims, mask, smooth=5, gap=2, return_windows=True, return_smoothed=True),
             lambda: ground_queries(text, video, mask, smooth=5, gap=2, gt=gt),
             lambda: ground_queries(one, video, flags))
    for which, call in enumerate(calls):
        want = call()                                                                          # (warm: library loaded, tables uploaded, allocator blocks cached)
        a = torch.ones(8192, 8192, device=dev)
        c = torch.empty_like(a)
        torch.mm(a, a, out=c)
        torch.cuda.synchronize()
        for _ in range(12):                                                                    # ~1.1 TFLOP of f32 each: tens of milliseconds of queued work
            torch.mm(a, a, out=c)
        ev = torch.cuda.Event()
        ev.record()
        got = call()
        still_busy = not ev.query()
        torch.cuda.synchronize()
        assert still_busy, f"call {which} returned only after the work queued before it had finished: it synchronised"
        flat = lambda o: [t for x in o for t in (x if isinstance(x, tuple) else (x,)) if t is not None]      # noqa: E731
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(flat(got), flat(want)))
