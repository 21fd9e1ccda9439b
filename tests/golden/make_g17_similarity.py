"""Fixture G17: the reference's ``eval/similarity.py`` on a small seeded case, f32 on the CPU.

Run where the reference is mounted:  ``python tests/golden/make_g17_similarity.py``.  The reference module is imported through ``ref_import`` from where it
lies (nothing of it is copied); ``g17_similarity.npz`` holds the seeded inputs and the OUTPUTS of its ``span_cxw_to_xx``, ``forward_clip_matching`` (twice:
as seeded, and with frame 3 of video 0 zeroed - that frame's 0 / 0 norm turns every window that holds it NaN) and ``_attention_pooling`` at temperature 0.01
and 1.  ``windows`` are the (lo, hi) of tests/similarity_oracle.py's window rule, accepted only if every slice the reference pooled has that many frames and its
scores follow from those windows."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import ref_import  # noqa: E402
import similarity_oracle as O  # noqa: E402
from revisionllm_amd.utils import synth  # noqa: E402

torch.set_grad_enabled(False)
SEED = 1234
B, L, D = 3, 40, 32
DURATIONS = (40, 25, 7)
SPANS = [(0.5, 1.0), (0.3, 0.2), (0.5, 0.0), (0.95, 0.3), (0.05, 0.3), (0.52, 0.01), (1.5, 0.2), (0.25, 0.5), (-0.2, 0.1), (0.0, 0.05), (0.1, -0.3)]


def inputs():
    video = torch.from_numpy(synth.features("g17.video", (B, L, D), SEED))
    text = torch.from_numpy(synth.features("g17.text", (B, D), SEED))
    mask = torch.zeros(B, L)
    for b, n in enumerate(DURATIONS):
        mask[b, :n] = 1
    spans = torch.tensor(SPANS, dtype=torch.float32)[None].repeat(B, 1, 1)
    return text, video, mask, spans


def main():
    S = ref_import.install()["similarity"]
    text, video, mask, spans = inputs()
    xx = S.span_cxw_to_xx(spans)
    pooled_frames, pool = [], S._topk_pooling

    def recording_pool(text_embeds, video_embeds, k):
        pooled_frames.append(int(video_embeds.shape[1]))
        return pool(text_embeds, video_embeds, k)
    S._topk_pooling = recording_pool
    scores = S.forward_clip_matching(text, video, mask, spans)
    video_z = video.clone()
    video_z[0, 3] = 0
    scores_z = S.forward_clip_matching(text, video_z, mask, spans)
    S._topk_pooling = pool
    # the slices the reference took: the window rule of tests/similarity_oracle.py, held to the reference run itself - the frame count of every slice it
    # pooled (recorded through its _topk_pooling) and, below, its scores recomputed over those windows
    win = O.windows(spans, mask).numpy().astype(np.int32)
    assert [max(int(hi) - int(lo), 0) for lo, hi in win.reshape(-1, 2)] == pooled_frames[:B * len(SPANS)], "the oracle's windows are not the reference's slices"
    again = O.span_scores64(O.frame_cosine64(text, video), torch.from_numpy(win).long())
    assert float((again - scores.double()).abs().max()) < 2e-5 and torch.equal(again == 0, scores == 0)
    out = dict(text=text, video=video, mask=mask, spans=spans, xx=xx, scores=scores, scores_zero_frame=scores_z, windows=win,
               attn_pool_t001=S._attention_pooling(text, video, 0.01), attn_pool_t1=S._attention_pooling(text, video, 1.0))
    path = os.path.join(HERE, "g17_similarity.npz")
    np.savez_compressed(path, **{k: (v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()})
    print("wrote", path, os.path.getsize(path), "bytes")
    print("scores\n", scores, "\nzero frame\n", scores_z, "\nwindows\n", win.tolist())


if __name__ == "__main__":
    main()
