"""rv_span_rank (the kernel behind ``ops.span_rank`` / ``eval.similarity.rank_proposals``: sort, greedy temporal NMS, top-M and hits against a ground
truth in one launch) against tests/rank_oracle.py, the rule restated in numpy float32 operation by operation.  The oracle IS the f32 rule, so ``order``,
``keep``, ``n_keep`` and ``first_hit`` must be equal and ``keep_iou`` must have the oracle's bits (one correctly rounded division); no case is left out and
there is no tolerance.  tests/test_rank_host_logic.py holds the oracle itself to a float64 statement and to hand-made cases.

Every direct call writes into buffers with 64 sentinel elements on either side of each output; the surroundings are compared bitwise.
Shapes: the wave form holds N <= 64 proposals in one wave, four rows per block (R = 4 / 5: the last block full / one row); the block form sorts N padded to
a power of two from 128 on (N = 65, 127, 128, 129, 1000, 2048).  The kernel is f32 only; the module runs in both builds because each library carries its
own copy of it."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import rank_oracle as K
from helpers import fl

pytestmark = pytest.mark.gpu

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")
HITS = (0.1, 0.3, 0.5, 0.7, 0.9)
PAD = 64
NAN, INF = float("nan"), float("inf")


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


@pytest.fixture(scope="module")
def g17(golden):
    return {k: torch.from_numpy(v) for k, v in golden.npz("g17_similarity").items()}


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


def run(dev, scores, spans, form, top, nms, gt=None, hit=(), order=True, keep_iou=True, first_hit=True):
    """The C entry on numpy inputs -> dict like the oracle's (parts not asked for: None), after the sentinel check."""
    from revisionllm_amd import hip
    R, N = scores.shape
    T = len(hit)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)          # noqa: E731
    s, p = up(scores), up(spans)
    g = up(gt) if gt is not None else None
    h = up(np.array(hit, dtype=np.float32)) if T else None
    o = dict(order=_Guarded(R * N, torch.int32, dev) if order else None, keep=_Guarded(R * top, torch.int32, dev), n_keep=_Guarded(R, torch.int32, dev),
             keep_iou=_Guarded(R * top, torch.float32, dev) if gt is not None and keep_iou else None,
             first_hit=_Guarded(R * T, torch.int32, dev) if gt is not None and first_hit and T else None)
    ptr = lambda x: x.ptr if x is not None else None                                            # noqa: E731
    rc = hip.lib().rv_span_rank(hip.ptr(s), hip.ptr(p), form, R, N, top, float(nms), hip.ptr(g), hip.ptr(h), T, ptr(o["order"]), ptr(o["keep"]),
                                ptr(o["n_keep"]), ptr(o["keep_iou"]), ptr(o["first_hit"]), hip.stream())
    hip.check(rc, "rv_span_rank")
    torch.cuda.synchronize()
    shapes = dict(order=(R, N), keep=(R, top), n_keep=(R,), keep_iou=(R, top), first_hit=(R, T))
    return {k: (v.take(shapes[k]) if v is not None else None) for k, v in o.items()}


def same(got, ref, what=""):
    """Integer outputs equal, keep_iou bit for bit (its zeros included: +0)."""
    for k in ("order", "keep", "n_keep", "first_hit"):
        if got[k] is not None:
            assert ref[k] is not None and np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:4].tolist())
    if got["keep_iou"] is not None:
        a, b = got["keep_iou"].view(np.uint32), np.ascontiguousarray(ref["keep_iou"]).view(np.uint32)
        assert np.array_equal(a, b), (what, "keep_iou", np.argwhere(a != b)[:4].tolist())


# ------------------------------------------------------------------ inputs ------------------------------------------------------------------
def random_rows(R, N, seed, ties=False):
    """Clustered proposals as a proposal head makes them ((centre, width); neighbours overlap heavily), scores random (``ties``: on a grid of 8 values), a
    ground truth per row."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.05, 0.95, (R, N))
    w = rng.choice([0.03, 0.06, 0.12, 0.25, 0.5], (R, N)) * rng.uniform(0.9, 1.1, (R, N))
    spans = np.stack([c, w], -1).astype(np.float32)
    scores = (rng.integers(0, 8, (R, N)) / 8 if ties else rng.normal(size=(R, N))).astype(np.float32)
    gt = np.sort(rng.uniform(0, 1, (R, 2)), -1).astype(np.float32)
    return scores, spans, gt


@functools.lru_cache(maxsize=None)
def sized(R, N, top, nms, seed=0):
    scores, spans, gt = random_rows(R, N, 1000 * N + R + seed)
    return scores, spans, gt, K.rank(scores, spans, 1, top, nms, gt, HITS)


def score_patterns(N):
    """One row per pattern."""
    rng = np.random.default_rng(N)
    base = rng.normal(size=N).astype(np.float32)
    rows = [base, np.full(N, 0.25, dtype=np.float32), (rng.integers(0, 3, N) / 2).astype(np.float32),
            np.where(rng.integers(0, 2, N) == 1, -0.0, 0.0).astype(np.float32)]
    for at in (0, N // 2, N - 1):
        x = base.copy()
        x[at] = NAN
        rows.append(x)
    x = base.copy()
    x[[0, N // 2, N - 1]] = NAN                       # several NaNs: among them the smaller index first
    rows.append(x)
    x = base.copy()
    x[0], x[N // 3], x[N - 1], x[N // 2] = -INF, INF, INF, NAN
    rows.append(x)
    rows.append(np.full(N, NAN, dtype=np.float32))
    x = np.where(np.arange(N) % 2 == 0, 0.0, -0.0).astype(np.float32)
    x[N // 2] = 1e-45                                 # a denormal above both zeros
    rows.append(x)
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def pattern_case(N, top, nms):
    scores = score_patterns(N)
    _, spans, gt = random_rows(scores.shape[0], N, 77 + N)
    return scores, spans, gt, K.rank(scores, spans, 1, top, nms, gt, HITS)


def span_patterns(N):
    """(start, end) rows: all duplicates, disjoint, the greedy chain repeated, void spans of every kind among solid ones."""
    i = np.arange(N, dtype=np.float32)
    dup = np.tile(np.array([0.25, 0.75], dtype=np.float32), (N, 1))
    disjoint = np.stack([i, i + 0.5], -1)
    chain = np.stack([0.5 * i, 0.5 * i + 1.0], -1)                    # neighbours at IoU 1/3, next-but-one disjoint
    void = np.stack([0.125 * (i % 5), 0.125 * (i % 5) + 0.5], -1)     # five distinct solid spans, heavily overlapping ...
    for at, bad in zip(range(0, N, 2), [(1.0, 0.5), (0.5, 0.5), (0.25, NAN), (NAN, 0.75), (0.25, INF), (-INF, 0.75), (-INF, INF), (NAN, NAN)] * N):
        void[at] = bad                                                # ... every other one void
    return np.stack([dup, disjoint, chain, void]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def span_case(N, top, nms):
    spans = span_patterns(N)
    rng = np.random.default_rng(5 + N)
    scores = rng.permutation(4 * N).reshape(4, N).astype(np.float32)
    scores[2] = -np.arange(N)                                          # the chain in its own order: A, B, C, ...
    gt = np.array([[0.25, 0.75], [1.0, 2.5], [0.0, 1.0], [0.0, 0.5]], dtype=np.float32)
    return scores, spans, gt, K.rank(scores, spans, 0, top, nms, gt, HITS)


def tops(N):
    return sorted({1, min(5, N), N})


# ------------------------------------------------------------------ sizes ------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 2048])
def test_sizes_of_both_forms(dev, N):
    """The wave form up to 64, the block form from 65 (padded and unpadded sorts), top = 1, 5 and N, with a ground truth; R = 5 (3 at the large sizes)."""
    R = 5 if N <= 129 else 3
    for top in tops(N):
        scores, spans, gt, ref = sized(R, N, top, 0.5)
        same(run(dev, scores, spans, 1, top, 0.5, gt, HITS), ref, (N, top))
        assert (ref["n_keep"] >= 1).all() and (N < 63 or top < N or (ref["n_keep"] < N).all())       # NMS did remove something where it could


@pytest.mark.parametrize("R", [1, 4, 5, 4099])
def test_row_counts(dev, R):
    """One row, a full block of four, one more, and many: the wave form (N = 7) and the block form (N = 65)."""
    for N, top in ((7, 3), (65, 2)):
        scores, spans, gt, ref = sized(R, N, top, 0.5)
        same(run(dev, scores, spans, 1, top, 0.5, gt, HITS), ref, (R, N))


# ------------------------------------------------------------------ scores ------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 130])
@pytest.mark.parametrize("nms", [0.0, 0.5, 1.0])
def test_score_patterns(dev, N, nms):
    """Random, all equal, ties at the top-th place, +-0, NaN at the first / middle / last index, several NaNs, +-inf, all NaN, a denormal."""
    for top in (5, N):
        scores, spans, gt, ref = pattern_case(N, top, nms)
        got = run(dev, scores, spans, 1, top, nms, gt, HITS)
        same(got, ref, (N, top, nms))
        assert got["order"][1].tolist() == list(range(N)) and got["order"][9].tolist() == list(range(N))        # all equal, all NaN: the identity
        assert got["order"][3].tolist() == list(range(N))                                                       # -0 and +0 tie
        for row, at in ((4, 0), (5, N // 2), (6, N - 1)):
            assert got["order"][row][-1] == at                                                                   # a NaN score ranks last
        assert got["order"][7][-3:].tolist() == [0, N // 2, N - 1]
        assert got["order"][8][:2].tolist() == [N // 3, N - 1] and got["order"][8][-2:].tolist() == [0, N // 2]   # inf, inf, ..., -inf, NaN
        assert got["order"][10][0] == N // 2
        if nms == 1.0:
            assert (got["n_keep"] == top).all() and np.array_equal(got["keep"], got["order"][:, :top])


# ------------------------------------------------------------------ spans ------------------------------------------------------------------
@pytest.mark.parametrize("N", [9, 64, 100])
@pytest.mark.parametrize("nms", [0.0, 0.25, 0.5, 1.0])
def test_span_patterns(dev, N, nms):
    for top in tops(N):
        scores, spans, gt, ref = span_case(N, top, nms)
        got = run(dev, scores, spans, 0, top, nms, gt, HITS)
        same(got, ref, (N, top, nms))
        if nms < 1.0:
            assert got["n_keep"][0] == 1 and got["keep"][0].tolist() == [int(np.argmax(scores[0]))] + [-1] * (top - 1)       # duplicates: one kept
            assert (got["keep_iou"][0][1:] == 0).all()
        assert got["n_keep"][1] == top                                                                                      # disjoint: nothing suppressed
        if nms == 0.25:                                                                                                     # the chain: A kills B, C stays
            assert got["keep"][2].tolist() == (list(range(0, N, 2)) + [-1] * N)[:top]
        if nms == 0.5:
            assert got["keep"][2].tolist() == list(range(top))
        if top == N:                                                                                                        # every void span is kept
            assert set(range(0, N, 2)) <= set(got["keep"][3].tolist())
            if nms < 0.5:
                assert got["n_keep"][3] < N                                                                                 # ... while solid ones died


def test_both_forms_of_the_same_proposals_agree(dev):
    """Bounds on a grid of 2^-6: (centre, width) -> (start, end) is exact, so the two readings give the same result."""
    rng = np.random.default_rng(3)
    for N in (40, 200):
        a = np.sort(rng.integers(0, 129, (4, N, 2)), -1)
        a[..., 1] += 1
        xx = (a / 64).astype(np.float32)
        cxw = np.stack([(xx[..., 0] + xx[..., 1]) / 2, xx[..., 1] - xx[..., 0]], -1).astype(np.float32)
        scores, gt = rng.normal(size=(4, N)).astype(np.float32), xx[:, 0]
        ref = K.rank(scores, xx, 0, N, 0.5, gt, HITS)
        one, two = run(dev, scores, xx, 0, N, 0.5, gt, HITS), run(dev, scores, cxw, 1, N, 0.5, gt, HITS)
        same(one, ref, N)
        same(two, ref, N)


# ------------------------------------------------------------------ ground truth ------------------------------------------------------------------
@pytest.mark.parametrize("N", [33, 150])
def test_ground_truth_cases(dev, N):
    """gt inside, outside and identical to a proposal, void gts; T = 1, 5, 16; a threshold equal to an attained IoU; each optional output alone."""
    scores, spans, _ = random_rows(6, N, 900 + N)
    s0, e0 = K.bounds(spans[2][int(np.argmax(scores[2]))], 1)
    gt = np.array([[0.4, 0.45], [5.0, 6.0], [s0, e0], [0.7, 0.2], [NAN, 0.5], [0.1, INF]], dtype=np.float32)
    first = K.rank(scores, spans, 1, N, 0.5, gt, ())
    attained = sorted({float(x) for x in first["keep_iou"][0][:8] if x > 0})[:3]
    assert attained and first["keep_iou"][2][0] == 1.0 and (first["keep_iou"][1] == 0).all() and (first["keep_iou"][3:] == 0).all()
    for hit in ((0.5,), HITS, tuple(attained) + tuple(np.linspace(0.02, 0.98, 16 - len(attained)))):
        ref = K.rank(scores, spans, 1, N, 0.5, gt, hit)
        got = run(dev, scores, spans, 1, N, 0.5, gt, hit)
        same(got, ref, (N, len(hit)))
        assert (got["first_hit"][1] == -1).all() and (got["first_hit"][3:] == -1).all()
    for t, a in enumerate(attained):                                  # strict >: the place that attains the threshold exactly is no hit
        row, p = got["keep_iou"][0], int(got["first_hit"][0][t])
        assert (row == np.float32(a)).any() and p != int(np.argmax(row == np.float32(a)))
        assert (row[:p] <= np.float32(a)).all() and row[p] > np.float32(a) if p >= 0 else (row <= np.float32(a)).all()
    ref = K.rank(scores, spans, 1, 5, 0.5, gt, HITS)
    only_iou = run(dev, scores, spans, 1, 5, 0.5, gt, HITS, first_hit=False)
    only_hit = run(dev, scores, spans, 1, 5, 0.5, gt, HITS, keep_iou=False, order=False)
    none = run(dev, scores, spans, 1, 5, 0.5, order=False)
    t0 = run(dev, scores, spans, 1, 5, 0.5, gt, ())
    assert only_iou["first_hit"] is None and only_hit["keep_iou"] is None and only_hit["order"] is None and t0["first_hit"] is None
    for got in (only_iou, only_hit, none, t0):
        same(got, ref)


# ------------------------------------------------------------------ independence ------------------------------------------------------------------
def test_a_row_alone_is_the_row_in_a_batch_and_two_runs_agree(dev):
    for N, R in ((50, 9), (300, 6)):
        scores, spans, gt = random_rows(R, N, 40 + N, ties=True)
        batch, again = run(dev, scores, spans, 1, 20, 0.5, gt, HITS), run(dev, scores, spans, 1, 20, 0.5, gt, HITS)
        for k in batch:
            assert batch[k].tobytes() == again[k].tobytes(), k
        for r in (0, R // 2, R - 1):
            alone = run(dev, scores[r:r + 1], spans[r:r + 1], 1, 20, 0.5, gt[r:r + 1], HITS)
            for k in batch:
                assert alone[k][0].tobytes() == batch[k][r].tobytes(), (N, r, k)
        same(batch, K.rank(scores, spans, 1, 20, 0.5, gt, HITS))


def test_the_wave_form_equals_the_block_form_on_the_same_proposals(dev):
    """64 proposals through the wave form; the same 64 plus one worst-scored proposal far away through the block form: the first 64 entries of the order
    agree, and so does everything else but for the far proposal, which is kept behind the others where there is room."""
    scores, spans, gt = random_rows(5, 64, 64, ties=True)
    far = np.concatenate([spans, np.tile(np.array([[[50.0, 0.5]]], dtype=np.float32), (5, 1, 1))], 1)
    worse = np.concatenate([scores, np.full((5, 1), -9.0, dtype=np.float32)], 1)
    for top in (5, 64):
        w, b = run(dev, scores, spans, 1, top, 0.5, gt, HITS), run(dev, worse, far, 1, top, 0.5, gt, HITS)
        assert np.array_equal(b["order"][:, :64], w["order"]) and (b["order"][:, 64] == 64).all()
        for k in ("keep_iou", "first_hit"):                                 # (the far proposal overlaps nothing: IoU 0, no hit)
            assert w[k].tobytes() == b[k].tobytes(), (top, k)
        for r in range(5):                                                  # the far proposal is kept last where the list has room for it
            n = int(w["n_keep"][r])
            want = w["keep"][r].copy()
            if n < top:
                want[n] = 64
            assert b["n_keep"][r] == min(n + 1, top) and np.array_equal(b["keep"][r], want), (top, r)


# ------------------------------------------------------------------ the Python surface ------------------------------------------------------------------
def _as_np(out):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out._asdict().items()}


def test_ops_span_rank_shapes_defaults_and_refusals(dev):
    from revisionllm_amd import ops
    scores, spans, gt = random_rows(6, 30, 1)
    ref = K.rank(scores, spans, 1, 30, 1.0, gt, HITS)
    s, p, g = (torch.from_numpy(x).to(dev) for x in (scores, spans, gt))
    out = ops.span_rank(s, p, gt=g, return_order=True)                                      # defaults: top = N, no NMS, (centre, width), five thresholds
    assert all(t.device == dev for t in out) and out.keep.shape == (6, 30) and out.first_hit.shape == (6, 5) and out.keep.dtype == torch.int32
    same(_as_np(out), ref)
    out = ops.span_rank(s.reshape(2, 3, 30), p.reshape(2, 3, 30, 2), top=99, nms_iou=0.5, gt=g.reshape(2, 3, 2))       # [B, Q, N]; top clamped to N
    assert out.keep.shape == (2, 3, 30) and out.n_keep.shape == (2, 3) and out.keep_iou.shape == (2, 3, 30) and out.first_hit.shape == (2, 3, 5) and out.order is None
    same({k: (None if v is None else v.reshape((6,) + v.shape[2:])) for k, v in _as_np(out).items()}, K.rank(scores, spans, 1, 30, 0.5, gt, HITS))
    out = ops.span_rank(s, p, top=4)
    assert out.keep_iou is None and out.first_hit is None and out.order is None
    same(_as_np(out), K.rank(scores, spans, 1, 4, 1.0))
    xx = torch.stack([p[..., 0] - 0.5 * p[..., 1], p[..., 0] + 0.5 * p[..., 1]], -1)
    same(_as_np(ops.span_rank(s, xx, top=7, nms_iou=0.3, form="xx", gt=g, hit_iou=(0.5,))), K.rank(scores, xx.cpu().numpy(), 0, 7, 0.3, gt, (0.5,)))
    same(_as_np(ops.span_rank(s, p.half(), top=7, nms_iou=0.3)), K.rank(scores, p.half().float().cpu().numpy(), 1, 7, 0.3))      # 16-bit spans: read as f32
    empty = ops.span_rank(s[:, :0], p[:, :0], gt=g)                                        # no proposals: empty outputs, no launch
    assert empty.keep.shape == (6, 0) and empty.keep_iou.shape == (6, 0) and empty.n_keep.tolist() == [0] * 6 and (empty.first_hit == -1).all()
    for bad in (lambda: ops.span_rank(s, p[:, :5]), lambda: ops.span_rank(s.double(), p), lambda: ops.span_rank(s, p, gt=g[:3]), lambda: ops.span_rank(s, p, top=0),
                lambda: ops.span_rank(s, p, nms_iou=-1.0), lambda: ops.span_rank(s, p, form="xyxy"), lambda: ops.span_rank(s, p, gt=g, hit_iou=(0.5,) * 17),
                lambda: ops.span_rank(torch.zeros(1, 2049, device=dev), torch.zeros(1, 2049, 2, device=dev))):
        with pytest.raises(ValueError, match="span_rank"):
            bad()


def _host_metrics(scores, proposal, gt):
    """The route the device ranking replaces: logs from the scores copied back and the oracle's IoUs, through grounding_metrics_stream."""
    from revisionllm_amd.eval.metrics import grounding_metrics_stream
    R, N = scores.shape
    full = K.rank(scores, proposal, 1, N, 1.0, gt, HITS)
    logs = []
    for r in range(R):
        iou = np.zeros(N)
        iou[full["keep"][r]] = full["keep_iou"][r]
        logs.append({"info": {"scores": scores[r].tolist(), "iou": iou.tolist()}})
    return grounding_metrics_stream(logs), full


def test_matching_to_metrics_end_to_end_on_g17(dev, g17):
    """forward_clip_matching_multi -> rank_proposals -> grounding_metrics_ranked on the device against the host route on the same scores.  The ground truth
    is made here: per (video, query) one of its proposals, shifted and stretched."""
    from revisionllm_amd.eval.metrics import grounding_metrics_ranked
    from revisionllm_amd.eval.similarity import forward_clip_matching_multi, rank_proposals, span_cxw_to_xx
    text = g17["text"][None].repeat(3, 1, 1).contiguous()
    spans = torch.stack([g17["spans"], g17["spans"].flip(1), g17["spans"]], dim=1).contiguous()                # [3, 3, 11, 2]
    pick = torch.tensor([[0, 4, 9], [2, 2, 7], [10, 5, 1]])
    gt = span_cxw_to_xx(spans[torch.arange(3)[:, None], torch.arange(3)[None], pick] * torch.tensor([1.03, 0.8])).contiguous()
    op16 = {"f16": torch.float16, "bf16": torch.bfloat16}[fl()]
    for video in (g17["video"], g17["video"].to(op16)):
        y = forward_clip_matching_multi(text.to(dev), video.to(dev), g17["mask"].to(dev), spans.to(dev))
        assert y.dtype == video.dtype and y.shape == (3, 3, 11)
        out = rank_proposals(y, spans.to(dev), gt=gt.to(dev), return_order=True)
        assert all(t.device == dev for t in out) and out.keep.shape == (3, 3, 11) and out.first_hit.shape == (3, 3, 5)
        got = grounding_metrics_ranked(out.keep_iou, out.first_hit)
        want, full = _host_metrics(y.float().cpu().numpy().reshape(9, 11), spans.numpy().reshape(9, 11, 2), gt.numpy().reshape(9, 2))
        same({k: (None if v is None else v.reshape((9,) + v.shape[2:])) for k, v in _as_np(out).items()}, full)
        assert set(got) == set(want)
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=9 * 2.0 ** -52, abs=0), k                  # (float64 sums of 9 terms in another order)
        assert want["mIoU"] > 0
        nms = rank_proposals(y, spans.to(dev), top=5, nms_iou=0.3, gt=gt.to(dev))
        same({k: (None if v is None else v.reshape((9,) + v.shape[2:])) for k, v in _as_np(nms).items()},
             K.rank(y.float().cpu().numpy().reshape(9, 11), spans.numpy().reshape(9, 11, 2), 1, 5, 0.3, gt.numpy().reshape(9, 2), HITS))
    host = rank_proposals(y.cpu(), spans, gt=gt, return_order=True)                                   # host tensors: staged, results back on the host
    assert not any(t.is_cuda for t in host) and all(torch.equal(a, b.cpu()) for a, b in zip(host, out))


def test_rank_proposals_does_not_wait_for_the_device(dev):
    """No device -> host copy and no synchronise inside the call: with the stream kept busy by work queued before it, an event recorded just before the call
    has not completed when the call returns (a call that waited for its own kernel would have waited for that work first)."""
    from revisionllm_amd.eval.similarity import rank_proposals
    for N in (64, 300):
        scores, spans, gt = random_rows(24, N, 8)
        s, p, g = (torch.from_numpy(x).to(dev) for x in (scores, spans, gt))
        want = rank_proposals(s, p, top=50, nms_iou=0.5, gt=g, return_order=True)             # (warm: library loaded, thresholds uploaded, allocator blocks cached)
        a = torch.ones(8192, 8192, device=dev)
        c = torch.empty_like(a)
        torch.mm(a, a, out=c)
        torch.cuda.synchronize()
        for _ in range(12):                                                                    # ~1.1 TFLOP of f32 each: tens of milliseconds of queued work
            torch.mm(a, a, out=c)
        ev = torch.cuda.Event()
        ev.record()
        got = rank_proposals(s, p, top=50, nms_iou=0.5, gt=g, return_order=True)
        still_busy = not ev.query()
        torch.cuda.synchronize()
        assert still_busy, "rank_proposals returned only after the work queued before it had finished: it synchronised"
        assert all(torch.equal(x, y) for x, y in zip(got, want))
        same(_as_np(got), K.rank(scores, spans, 1, 50, 0.5, gt, HITS))
