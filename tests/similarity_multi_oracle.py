"""Float64 restatements for several texts per video (``forward_clip_matching_multi``, rv_frame_cosine_multi, rv_span_scores_multi): the single-text
oracle of tests/similarity_oracle.py looped over the queries, so each ``[b, q]`` IS the single-text oracle's result.  Nothing here is used by the package."""
import torch

import similarity_oracle as O


def frame_cosine_multi64(text, video):
    """text [B,Q,d], video [B,L,d] -> float64 [B,Q,L]."""
    return torch.stack([O.frame_cosine64(text[:, q], video) for q in range(text.shape[1])], dim=1)


def windows_multi(spans, mask):
    """spans [B,Q,N,2], mask [B,L] -> int64 [B,Q,N,2]: every query's windows by its video's duration."""
    return torch.stack([O.windows(spans[:, q], mask) for q in range(spans.shape[1])], dim=1)


def span_scores_multi64(sims, win, pooling="topk", k=3, temperature=0.01):
    """sims [B,Q,L], win [B,Q,N,2] -> float64 [B,Q,N]."""
    return torch.stack([O.span_scores64(sims[:, q], win[:, q], pooling, k, temperature) for q in range(sims.shape[1])], dim=1)


def forward_clip_matching_multi64(text, video, mask, spans, pooling="topk", k=3, temperature=0.01):
    """text [B,Q,d], video [B,L,d], mask [B,L], spans [B,Q,N,2] -> (float64 [B,Q,N], int64 [B,Q,N,2])."""
    per_q = [O.forward_clip_matching64(text[:, q], video, mask, spans[:, q], pooling, k, temperature) for q in range(text.shape[1])]
    return torch.stack([s for s, _ in per_q], dim=1), torch.stack([w for _, w in per_q], dim=1)
