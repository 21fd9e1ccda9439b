"""rv_clip_encoder at every dispatch edge of engine.hip and in all four option forms, against oracle.adapter.clip_encoder evaluated in float64 on
the same rounded weights and inputs.  The encoder picks another kernel chain at small integer thresholds (rows per query, text length, N and T of the
CLS-only last layer, key count of the self-attention, row count of every GEMM): each case below sits on one side of one of them.

The synthetic text features need no scaling (constant 1) for the asserted bound to notice a dropped key, an ignored mask or a wrong text row:
test_oracle_sensitivity_to_text_faults checks exactly that, on the CPU."""
import functools
import os

import pytest
import torch

from helpers import SEED, clip_weights, feats, fl, rel_err, tol

pytestmark = pytest.mark.gpu

D = 768
BOUND = 1e-2                 # the project's number for this operation (test_gpu_kernels.test_clip_encoder): rel_err < tol(1e-2)
DEFAULTS = {"adapter_fold_t2v": 1, "adapter_stream16": 1}

_FORCED = os.environ.get("REVISION_TEST_FLAVOURS")


@pytest.fixture(scope="module", params=[None] if _FORCED else ["f16", "bf16"])
def flav(request, op_flavour):
    """Both operand flavours (the module list of conftest.py is fixed, so the module brings its own parameter; REVISION_TEST_FLAVOURS still narrows it)."""
    from revisionllm_amd import hip
    f = request.param or op_flavour or hip.flavour()
    prev = hip.set_flavour(f)
    yield f
    hip.set_flavour(prev)


@pytest.fixture(scope="module")
def engines(flav):
    """One engine per (flavour, text on / off) for the whole module, set up as test_clip_encoder does."""
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from revisionllm_amd import engine
    from revisionllm_amd.utils import synth
    made = {}

    def get(text):
        if text not in made:
            eng = engine.Engine(synth.LlamaShape(layers=0), adapter_text=text, device="cuda:0")
            eng.init_synthetic(seed=SEED, llm=False, clip=True, clip_prefix="mm_projector.")
            made[text] = eng
        return made[text]
    return get


# ---- inputs and the float64 reference (computed once per case and flavour, shared by every test that needs it) ----
@functools.lru_cache(maxsize=None)
def _weights64(flavour, text):
    """Oracle weights: matrices rounded to the flavour, vectors fp32 (what the device holds), all as float64."""
    w, w32 = clip_weights(text=text, bf16=flavour), clip_weights(text=text, bf16=False)
    return {k: (w32[k] if w[k].dim() == 1 else w[k]).double() for k in w}


def ragged_mask(Nq, Lq):
    """Query 0: every token valid; query 1: only token 0; query 2: Lq // 2 + 1 tokens; then again."""
    m = torch.zeros(Nq, Lq)
    for q in range(Nq):
        m[q, :(Lq, 1, Lq // 2 + 1)[q % 3]] = 1
    return m


def _x(flavour, N, T):
    return feats(f"cee.x.{N}.{T}", (N, T, D), bf16=flavour)


def _txt(flavour, Nq, Lq):
    return feats(f"cee.txt.{Nq}.{Lq}", (Nq, Lq, D), bf16=flavour)


def _oracle(flavour, x, txt=None, mask=None, rows=None):
    """oracle "all" output [N, T + 1, 4096] in float64; ``rows``: text row of every sequence (default n // (N / Nq))."""
    from oracle import adapter
    text = txt is not None
    w = _weights64(flavour, text)
    if not text:
        return adapter.clip_encoder(x.double(), w, None, None, False, "all", False)
    N, Nq = x.shape[0], txt.shape[0]
    if rows is None:
        qf, qm = txt.repeat_interleave(N // Nq, 0), mask.repeat_interleave(N // Nq, 0)
    else:
        qf, qm = txt[rows], mask[rows]
    return adapter.clip_encoder(x.double(), w, qf.double(), qm, True, "all", False)


@functools.lru_cache(maxsize=None)
def _ref(flavour, N, Nq, T, Lq, first_valid=None):
    """(reference "all", reference "cls") of a case; Nq = 0: no text layers.  ``first_valid``: the valid-token count of query 0 (default: all)."""
    if not Nq:
        ref = _oracle(flavour, _x(flavour, N, T))
    else:
        ref = _oracle(flavour, _x(flavour, N, T), _txt(flavour, Nq, Lq), _mask(Nq, Lq, first_valid))
    return ref, ref[:, 0]          # (the oracle's "cls" selection is row 0 of the same hidden state through the same projector)


def _mask(Nq, Lq, first_valid=None):
    m = ragged_mask(Nq, Lq)
    if first_valid is not None:
        m[0] = 0
        m[0, :first_valid] = 1
    return m


def _err(y, ref, label):
    """helpers.rel_err, plus a line that names the case in the RV_LOG_ERR file."""
    e = rel_err(y.cpu(), ref)
    log = os.environ.get("RV_LOG_ERR")
    if log:
        with open(log, "a") as fh:
            fh.write(f"  edges {fl()} {label} {e:.3e}\n")
    return e


def _run(eng, flavour, N, Nq, T, Lq, feature, first_valid=None, txt=None, mask=None):
    x = _x(flavour, N, T)
    if not Nq:
        return eng.clip_encoder(x, None, None, feature)
    return eng.clip_encoder(x, _txt(flavour, Nq, Lq) if txt is None else txt, _mask(Nq, Lq, first_valid) if mask is None else mask, feature)


def _check(eng, flavour, N, Nq, T, Lq, label, first_valid=None):
    refall, refcls = _ref(flavour, N, Nq, T, Lq, first_valid)
    ycls = _run(eng, flavour, N, Nq, T, Lq, "cls", first_valid)
    yall = _run(eng, flavour, N, Nq, T, Lq, "all", first_valid)
    assert ycls.shape == refcls.shape and yall.shape == refall.shape
    assert torch.isfinite(ycls).all() and torch.isfinite(yall).all()
    ec, ea = _err(ycls, refcls, label + " cls"), _err(yall, refall, label + " all")
    print(f"{fl()} {label}: cls {ec:.3e} all {ea:.3e}")
    assert ec < tol(BOUND), (label, ec)
    assert ea < tol(BOUND), (label, ea)
    return ycls, yall


# ---- 1. branch edges ----
TEXT_CASES = [
    # fold off / on by rows per query ((N / Nq) * T = 32 | 33), grouped and single GEMMs
    (2, 2, 32, 7), (2, 2, 33, 7), (1, 1, 33, 7), (1, 1, 32, 7),
    # hierarchy mapping with three distinct texts: sequence n uses text n // 2 (all three mask patterns)
    (6, 3, 40, 7), (6, 3, 40, 20), (6, 3, 40, 33),
    # key slots: LK = 16 full, LK = 32 sparse, LK = 32 with its last slot empty / full (mask bit 31), first unfolded length
    (4, 2, 40, 16), (4, 2, 40, 17), (4, 2, 40, 31), (4, 2, 40, 32), (4, 2, 40, 33), (3, 3, 40, 32), (1, 1, 40, 32),
    # the longest CLIP text: unfolded, three key blocks
    (4, 2, 40, 77), (3, 1, 40, 77),
    # 16-bit residual stream switch (N * T = 32 | 33)
    (2, 1, 16, 7), (3, 1, 11, 7),
    # few-row GEMM families (N * T = 1, 16, 17, 32)
    (1, 1, 1, 7), (1, 1, 16, 7), (1, 1, 17, 7), (2, 2, 16, 7),
    # CLS-only last layer (feature CLS, N = 16 | 17, T = 2 | 3), its N-row GEMMs at 32 | 33 rows
    (16, 2, 3, 7), (17, 1, 3, 7), (17, 1, 2, 7), (18, 3, 40, 20), (32, 2, 16, 7), (33, 1, 16, 7), (36, 3, 40, 20),
    # self-attention key counts T + 1 = 2, 95, 96, 97, 128, 129
    (2, 1, 1, 7), (2, 1, 94, 7), (2, 1, 95, 7), (2, 1, 96, 7), (2, 1, 127, 7), (2, 1, 128, 7),
    # largest: CLS-only layer with the LDS-staged self-attention
    (17, 1, 128, 7),
]
# single-text cases once more with a partly masked query 0 (a lone query is otherwise never ragged): (N, Nq, T, Lq, valid tokens of query 0)
PARTIAL_CASES = [(1, 1, 33, 7, 1), (1, 1, 32, 7, 4), (1, 1, 40, 32, 17), (3, 1, 40, 77, 33), (17, 1, 3, 7, 4)]
NOTEXT_CASES = [(1, 1), (2, 16), (17, 3), (17, 2), (2, 95), (2, 128)]


@pytest.mark.parametrize("N,Nq,T,Lq", TEXT_CASES)
def test_branch_edges_with_text(engines, flav, N, Nq, T, Lq):
    """"cls" and "all" outputs against the float64 oracle, ragged mask, at the thresholds of the fold, the key-slot template, the 16-bit stream, the
    CLS-only last layer, the self-attention forms and the GEMM families.  Bound: rel_err < tol(1e-2) (bf16 1e-2, fp16 1.67e-3).
    measured (every case of this file: profiles/adapter_edges_err_{f16,bf16}.log): worst fp16 8.6e-4 at (32,2,16,7) "all", worst bf16 4.2e-3 at (3,1,11,7) "all"."""
    _check(engines(True), flav, N, Nq, T, Lq, f"text N{N} Nq{Nq} T{T} Lq{Lq}")


@pytest.mark.parametrize("N,Nq,T,Lq,valid", PARTIAL_CASES)
def test_branch_edges_single_text_partly_masked(engines, flav, N, Nq, T, Lq, valid):
    """The single-query forms (rv_gemm_impl fold GEMMs, kv_batch_div = N) with a mask that hides the tail of the only query."""
    _check(engines(True), flav, N, Nq, T, Lq, f"text N{N} Nq{Nq} T{T} Lq{Lq} valid{valid}", first_valid=valid)


@pytest.mark.parametrize("N,T", NOTEXT_CASES)
def test_branch_edges_without_text(engines, flav, N, T):
    """adapter_text = False: k_build_x feeds the self-attention layers directly."""
    _check(engines(False), flav, N, 0, T, 0, f"notext N{N} T{T}")


SENS_BOUND = 3 * BOUND / 6          # 3 x the asserted fp16 bound


@pytest.mark.parametrize("N,Nq,T,Lq", [(4, 2, 40, 17), (4, 2, 40, 33), (6, 3, 40, 7)])
def test_oracle_sensitivity_to_text_faults(N, Nq, T, Lq):
    """The bound bites (CPU only, the oracle against deliberately wrong oracles on the fp16-rounded inputs): dropping the last valid token of query 0,
    ignoring the mask, and assigning texts as n % Nq each move the "all" output by at least 3 x the asserted fp16 bound (5e-3, max-norm relative).
    Text scale: 1 (the unscaled features suffice).  measured (token dropped / mask ignored / n % Nq): (4,2,40,17) 7.1e-2 / 7.8e-1 / 8.0e-1;
    (4,2,40,33) 4.2e-2 / 7.7e-1 / 8.4e-1; (6,3,40,7) 1.8e-1 / 7.6e-1 / 9.6e-1."""
    f = "f16"
    x, txt, mask = _x(f, N, T), _txt(f, Nq, Lq), ragged_mask(Nq, Lq)
    ref = _ref(f, N, Nq, T, Lq)[0]
    dropped = mask.clone()
    dropped[0, int(mask[0].sum()) - 1] = 0
    wrong = {"token dropped": _oracle(f, x, txt, dropped), "mask ignored": _oracle(f, x, txt, torch.ones_like(mask)),
             "n % Nq": _oracle(f, x, txt, mask, rows=torch.arange(N) % Nq)}
    dist = {k: float((v - ref).abs().max() / ref.abs().max()) for k, v in wrong.items()}
    print(f"sensitivity N{N} Nq{Nq} T{T} Lq{Lq}: " + ", ".join(f"{k} {v:.3e}" for k, v in dist.items()))
    for k, v in dist.items():
        assert v >= SENS_BOUND, (k, v)


# ---- 2. the four option forms ----
def _with_options(eng, fold, s16, fn):
    try:
        eng.set_option("adapter_fold_t2v", fold).set_option("adapter_stream16", s16)
        return fn()
    finally:
        for k, v in DEFAULTS.items():
            eng.set_option(k, v)


@pytest.mark.parametrize("N,Nq,T,Lq", [(4, 2, 40, 7), (4, 2, 40, 20), (1, 1, 33, 16), (17, 1, 40, 7), (4, 2, 40, 40)])
def test_option_forms_agree_with_the_oracle(engines, flav, N, Nq, T, Lq):
    """adapter_fold_t2v x adapter_stream16: every setting is within the bound of the oracle (the plain forms, fold 0 / stream 0, are "the same function" as the
    defaults); the bf16 build ignores adapter_stream16 (equal bits); where the fold cannot apply (Lq = 40) adapter_fold_t2v changes nothing (equal bits)."""
    eng = engines(True)
    out = {}
    for fold in (0, 1):
        for s16 in (0, 1):
            out[fold, s16] = _with_options(eng, fold, s16, lambda: _check(eng, flav, N, Nq, T, Lq, f"options fold{fold} s16{s16} N{N} Nq{Nq} T{T} Lq{Lq}"))
    assert eng.get_option("adapter_fold_t2v") == 1 and eng.get_option("adapter_stream16") == 1
    for i in range(2):                       # "cls", "all"
        if flav == "bf16":
            for fold in (0, 1):
                assert torch.equal(out[fold, 0][i], out[fold, 1][i]), ("adapter_stream16 is ignored by the bf16 build", fold, i)
        if Lq > 32:
            for s16 in (0, 1):
                assert torch.equal(out[0, s16][i], out[1, s16][i]), ("no fold beyond 32 text tokens", s16, i)


# ---- 3. properties that need no tolerance ----
@pytest.mark.parametrize("Lq", [20, 40])
def test_masked_text_tokens_are_inert(engines, flav, Lq):
    """The CONTENTS of masked text tokens cannot reach the output: rows the mask hides overwritten with other finite values 50 x as large leave every
    output bit unchanged, folded (A1 / A2 are built from every row j < Lq; t2v_softmax_kernel alone zeroes them) and unfolded."""
    eng = engines(True)
    N, Nq, T = 4, 2, 40
    txt, mask = _txt(flav, Nq, Lq), ragged_mask(Nq, Lq)
    other = feats(f"cee.junk.{Lq}", (Nq, Lq, D), bf16=flav) * 50
    dirty = torch.where(mask[:, :, None] != 0, txt, other)
    assert not torch.equal(dirty, txt) and torch.isfinite(dirty).all() and torch.equal(dirty[0], txt[0])
    for fold in (1, 0):
        for feature in ("cls", "all"):
            a = _with_options(eng, fold, 1, lambda: _run(eng, flav, N, Nq, T, Lq, feature, txt=txt, mask=mask))
            b = _with_options(eng, fold, 1, lambda: _run(eng, flav, N, Nq, T, Lq, feature, txt=dirty, mask=mask))
            assert torch.isfinite(a).all() and torch.equal(a, b), (fold, feature)


@pytest.mark.parametrize("N,Nq,T,Lq", [(17, 1, 3, 7), (18, 3, 40, 20), (32, 1, 128, 7), (33, 1, 16, 7), (36, 3, 40, 20)])
def test_cls_only_last_layer_matches_row_0_of_the_full_layer(engines, flav, N, Nq, T, Lq):
    """Where the CLS-only last layer runs (feature CLS, N > 16, T >= 3) its rows equal row 0 of the "all" output, which takes the full-length layer: to
    1e-6, and bit for bit at these shapes (measured on the GPU in both flavours, so asserted).  With 17 .. 32 sequences the layer's N-row GEMMs used to take the weight-streaming kernel (other sums than the full-length launches): measured
    2.7e-4 / 1.8e-6 (fp16) and 9.0e-4 / 1.8e-6 (bf16) on the first two shapes before they were kept on the kernels of more than 32 rows."""
    eng = engines(True)
    ycls = _run(eng, flav, N, Nq, T, Lq, "cls")
    yall = _run(eng, flav, N, Nq, T, Lq, "all")
    e = rel_err(yall[:, 0].cpu(), ycls.cpu())
    print(f"{fl()} cls-only N{N} T{T}: rel_err {e:.3e} equal {torch.equal(yall[:, 0], ycls)}")
    assert e < 1e-6
    assert torch.equal(yall[:, 0], ycls)


@pytest.mark.parametrize("Lq", [20, 40])
def test_two_calls_are_bit_identical(engines, flav, Lq):
    """Determinism, one folded and one unfolded shape."""
    eng = engines(True)
    for feature in ("cls", "all"):
        a = _run(eng, flav, 4, 2, 40, Lq, feature).clone()
        assert torch.equal(a, _run(eng, flav, 4, 2, 40, Lq, feature))


def test_sequences_not_a_multiple_of_texts_are_refused(engines, flav):
    """With text, N % Nq != 0 is RV_ERR_ARG (status -1); the engine takes the next call as if nothing had happened."""
    from revisionllm_amd import hip
    eng = engines(True)
    before = _run(eng, flav, 4, 2, 40, 7, "cls").clone()
    with pytest.raises(hip.HipLibraryError, match=r"rv_clip_encoder failed \(status -1\).*multiple of Nq"):
        eng.clip_encoder(_x(flav, 5, 40), _txt(flav, 2, 7), ragged_mask(2, 7), "cls")
    assert torch.equal(before, _run(eng, flav, 4, 2, 40, 7, "cls"))


# ---- 4. a query with no valid token ----
@pytest.mark.parametrize("N,Nq,T,Lq", [(4, 2, 40, 7), (4, 2, 16, 7), (4, 2, 40, 77)])
def test_query_without_a_valid_token(engines, flav, N, Nq, T, Lq):
    """A query whose every token is padded has no key: its attention output is zero in both forms of the text layers (the reference's
    nn.MultiheadAttention yields NaN there), so its sequences stay finite and the other queries' sequences do not notice.  T = 40, Lq = 7: the fold against the
    unfolded attention; T = 16: the unfolded attention's key-split form (<= 16 query rows; no fold at 32 rows per query); Lq = 77: three key blocks, all padded."""
    eng = engines(True)
    normal, empty = ragged_mask(Nq, Lq), ragged_mask(Nq, Lq)
    empty[1] = 0
    got = {}
    for fold in (1, 0):
        a = _with_options(eng, fold, 1, lambda: _run(eng, flav, N, Nq, T, Lq, "all", mask=normal))
        b = _with_options(eng, fold, 1, lambda: _run(eng, flav, N, Nq, T, Lq, "all", mask=empty))
        assert torch.equal(a[:N // Nq], b[:N // Nq]), fold                 # query 0's sequences
        got[fold] = b[N // Nq:]
        print(f"{fl()} empty query T{T} Lq{Lq}, fold {fold}: finite {bool(torch.isfinite(got[fold]).all())}")
    assert torch.equal(torch.isfinite(got[0]), torch.isfinite(got[1]))
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()


def test_attention_row_with_every_key_padded_is_zero(flav):
    """rv_attention with a key-padding mask: a batch whose keys are all padded yields zero rows (not NaN), in the key-split form (<= 16 queries) and the
    per-wave form, over one and over three key blocks; the other batch is untouched by it."""
    from revisionllm_amd import ops
    B, H, dh = 2, 8, 96
    for Lq, Lk in ((9, 7), (40, 7), (9, 77), (40, 77)):
        q = feats(f"cee.at.q.{Lq}", (B, Lq, H, dh), bf16=flav).to(_op16()).cuda()
        k = feats(f"cee.at.k.{Lk}", (B, Lk, H, dh), bf16=flav).to(_op16()).cuda()
        v = feats(f"cee.at.v.{Lk}", (B, Lk, H, dh), bf16=flav).to(_op16()).cuda()
        pad = torch.zeros(B, Lk, dtype=torch.uint8)
        live = ops.attention(q, k, v, causal=False, key_pad=pad.cuda())
        pad[1] = 1
        y = ops.attention(q, k, v, causal=False, key_pad=pad.cuda())
        assert torch.equal(y[0], live[0]) and torch.isfinite(live).all(), (Lq, Lk)
        assert (y[1] == 0).all(), (Lq, Lk)


def _op16():
    from revisionllm_amd import hip
    return hip.op_dtype()
