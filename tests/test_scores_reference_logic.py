"""CPU checks of the float64 references that tests/test_gpu_rowops_scores_edges.py holds the row-op and score kernels to: they agree with the project's
fp32 oracle (oracle/scores.py, oracle/sampling.py) at fp32 resolution, they rank NaN as ``torch.topk`` does on this torch build, every top-k pooling
seed of the GPU file keeps its neighbouring similarities apart, and the fp32 oracle's own distance from float64 at T = 7937 - the measurement the
bound of the cosine score rests on - stays under the limit at which that bound would have had to follow it."""
import math

import pytest
import torch

import test_gpu_rowops_scores_edges as E
from helpers import feats, rel_err
from oracle import sampling, scores

KINDS = ("f16", "bf16", "f32")


def test_entropy_reference_agrees_with_the_oracle():
    logits = feats("srl.ent", (3, 7, 1000)) * 1.3
    ref, orc = E.entropy_stats_ref64(logits), scores.entropy_statistics(logits)
    assert torch.allclose(ref[:, :3].float(), orc[:, :3], rtol=1e-5) and float((ref[:, 3].float() - orc[:, 3]).abs().max()) < 2e-6 * float(orc[:, 0].max())
    # filtered (-inf) entries, as the warper chain leaves them: p = 0, no NaN
    sc = sampling.process_logits(logits[:, 0], 0.7, 20, 0.9)
    assert int(torch.isinf(sc).sum()) > 0
    assert torch.allclose(E.entropy_stats_ref64(sc[:, None])[:, :3].float(), scores.entropy_statistics(sc[:, None])[:, :3], rtol=1e-5)
    # one step: the reference's std is NaN (the device's too); the oracle's slice rule only differs where V <= G, which no driver reaches
    assert bool(torch.isnan(E.entropy_stats_ref64(logits[:, :1])[:, 3]).all()) and bool(torch.isnan(scores.entropy_statistics(logits[:, :1])[:, 3]).all())
    flat = E.entropy_stats_ref64(torch.full((1, 2, 1025), 1.25))
    assert torch.allclose(flat[0, :3], torch.full((3,), math.log(1025), dtype=torch.float64), rtol=1e-6)


@pytest.mark.parametrize("kind", KINDS)
def test_cosine_reference_agrees_with_the_oracle(kind):
    f, q = E.cosine_inputs(4, 250, 768, kind)
    orc = torch.stack([scores.stage2_cosine(f[i:i + 1], q)[0] for i in range(4)])
    assert rel_err(orc, E.topk_cosine_ref64(f, q, 3)) < 1e-5
    seg = f[0, 5:19]
    assert rel_err(scores.stage1_cosine(seg, q), E.topk_cosine_ref64(seg[None], q, 3)) < 1e-5
    assert rel_err(scores.stage1_cosine(seg, q, topk_pool=False), E.topk_cosine_ref64(seg[None], q, 0)[0]) < 1e-5
    assert rel_err(scores.stage1_cosine(seg[:2], q), E.topk_cosine_ref64(seg[None, :2], q, 3)) < 1e-5          # min(k, T) values
    assert rel_err(E.topk_cosine_ref64(seg[None, :2], q, 7), E.topk_cosine_ref64(seg[None, :2], q, 2)) == 0.0


@pytest.mark.parametrize("case", E.POOL_CASES, ids=lambda c: "Nv%d-T%d-d%d-Nt%d-k%d" % c)
def test_pool_reference_agrees_with_the_oracle_and_the_seeds_keep_the_rank_gap(case):
    k = case[4]
    for kind in KINDS:
        video, text = E.pool_inputs(case, kind)
        ref, idx, sims = E.topk_pool_ref64(text, video, k)
        assert E.rank_gap(sims, k) >= E.GAP, (case, kind, E.rank_gap(sims, k))
        assert rel_err(scores.topk_pooling(text, video, k), ref) < 1e-6
        top = torch.topk(video @ text.t(), k, dim=1)[1].permute(0, 2, 1)
        assert torch.equal(torch.sort(top, -1).values, torch.sort(idx, -1).values)                         # the same frames (torch.topk's order within is unspecified)


@pytest.mark.parametrize("T,k", [(3, 3), (17, 3)])
def test_nan_pool_inputs_keep_the_rank_gap_and_match_the_oracle(T, k):
    for kind in KINDS:
        for nan_frames in E.pool_nan_cases(T):
            video, text = E.pool_nan_inputs(T, kind, nan_frames)
            ref, idx, sims = E.topk_pool_ref64(text, video, k)
            assert E.pool_nan_gap(sims, k, nan_frames) >= E.GAP
            orc = scores.topk_pooling(text, video, k)
            assert torch.equal(torch.isnan(orc), torch.isnan(ref)) and torch.allclose(orc.double(), ref, rtol=1e-6, atol=1e-6, equal_nan=True)
            assert all(set(nan_frames) <= set(idx[1, j].tolist()) for j in range(2))


def test_nan_ranks_first_as_torch_topk_ranks_it():
    """Pinned on three frames: torch.topk on this build takes a NaN before every number, and so do the references (and the fixed score kernels)."""
    s = torch.tensor([1.0, float("nan"), 2.0], dtype=torch.float64)
    assert torch.topk(s, 2).indices.tolist() == [1, 2] and torch.topk(s.float(), 1).indices.tolist() == [1]
    assert E.rank_order(s, 0).tolist() == [1, 2, 0]
    assert E.rank_order(torch.tensor([float("nan"), 3.0, float("nan"), 3.0]), 0).tolist() == [0, 2, 1, 3]        # equals: the smaller index first
    video = torch.tensor([[[1.0, 0.0], [float("nan"), 1.0], [2.0, 0.5]]])
    text = torch.tensor([[1.0, 0.0]])
    ref, idx, _ = E.topk_pool_ref64(text, video, 2)
    assert idx.tolist() == [[[1, 2]]]
    orc = scores.topk_pooling(text, video, 2)
    assert torch.isnan(orc[0, 0, 0]) and torch.isnan(ref[0, 0, 0]) and float(orc[0, 0, 1]) == float(ref[0, 0, 1]) == 1.5
    # the cosine score: one NaN element, or a column of zeros, makes every similarity of the segment NaN - for k = 3 as for the mean
    f, q = E.cosine_inputs(2, 5, 8, "f32")
    f[0, 2, 3] = float("nan")
    f[1, :, 0] = 0
    for i in range(2):
        assert torch.isnan(scores.stage2_cosine(f[i:i + 1], q)).all() and torch.isnan(scores.stage1_cosine(f[i], q, topk_pool=False))
    assert torch.isnan(E.topk_cosine_ref64(f, q, 3)).all() and torch.isnan(E.topk_cosine_ref64(f, q, 0)).all()
    # one +inf element: ONE NaN similarity among numbers - NaN first makes the score NaN for k < T too, in the oracle as in the reference
    f, q = E.cosine_inputs(1, 5, 8, "f32")
    f[0, 2, 3] = float("inf")
    assert torch.isnan(E.cosine_sims64(f) @ q.double()).tolist() == [[False, False, True, False, False]]
    assert torch.isnan(scores.stage2_cosine(f, q)).all() and torch.isnan(scores.stage1_cosine(f[0], q, topk_pool=False))
    for k in (1, 3, 0):
        assert torch.isnan(E.topk_cosine_ref64(f, q, k)).all()


def test_fp32_oracle_against_float64_at_T7937():
    """The project's 1e-4 for rv_topk_cosine had only been measured at T = 250.  At the first length the generic kernel takes over (d = 768, 16-bit
    features) the fp32 oracle is this far from float64: 1.6e-6 on the fp16-valued data, 5.3e-6 on the bf16-valued data - under 2.5e-5, so the GPU
    file asserts the project's 1e-4 unchanged."""
    T = E.last_T(768, 2, "fast") + 1
    assert T == 7937 and E.last_T(768, 2, "generic") == 12544
    for kind in ("f16", "bf16"):
        f, q = E.cosine_inputs(1, T, 768, kind)
        e = rel_err(scores.stage2_cosine(f, q), E.topk_cosine_ref64(f, q, 3))
        print(f"fp32 oracle vs float64 at T = {T}, {kind}-valued features: {e:.3e}")
        assert e <= E.COSINE_ORACLE_LIMIT, e
    assert E.COSINE_BOUND == 1e-4


def test_host_mirror_of_the_cosine_kernel_choice():
    assert E.cosine_plan(768, 250, 2) == "fast" and E.cosine_plan(772, 250, 2) == "generic" and E.cosine_plan(772, 250, 4) == "fast"
    assert E.cosine_plan(6, 250, 4) == "generic" and E.cosine_plan(4096, 4097, 2) == "refuse" and E.cosine_plan(4096, 4097, 4) == "fast"
    assert E.last_T(12, 2, "generic") == 16324 and E.last_T(6, 4, "generic") == 16354
