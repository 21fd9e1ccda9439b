/*
 * revision_hip.h - C ABI of librevision_hip.so: the MI355X (gfx950) implementation of ReVisionLLM's
 * recursive temporal-grounding inference path.
 *
 * The reference has no FFI layer: its boundary for this path is the Python API
 *   revisionllm/model/builder.py:21-67   load_pretrained_model
 *   revisionllm/inference.py:28-75       inference  (-> model.generate, inference.py:45-59)
 *   revisionllm/mm_utils.py:22-75        tokenizer_image_token
 * which revisionllm_amd/ keeps verbatim.  This header is the build-defined boundary directly beneath
 * that API: what a maintainer binds (ctypes) in place of the torch modules the
 * reference calls.  Each entry point cites the reference code it replaces.
 *
 * Conventions
 *   - plain C, no torch types; every pointer is a caller-owned DEVICE pointer unless marked host;
 *   - all work is enqueued on the caller's hipStream_t (passed as void*); nothing synchronises;
 *   - the library allocates nothing on the device: workspaces are caller-provided, sizes come from
 *     the *_ws_bytes queries; rv_ctx only stores pointers + configuration + its tunables.  A workspace must be ZERO when it is
 *     handed over for the first time (its first 16 KiB hold the hand-off flags of the persistent GEMMs and the arrival counters
 *     of the split-K decode kernel; both only ever count up, so it never needs cleaning afterwards) and must not be used by two
 *     streams at once;
 *   - no process-wide mutable state: tunables live in the context (rv_ctx_set_option), contexts are independent and
 *     re-entrant across threads; the only shared things are a monotonic launch counter (atomic; the hand-off flags of the
 *     persistent GEMMs carry it, so a workspace never needs cleaning) and the thread-local error string.  At most ONE launch
 *     that waits in-kernel for its sibling workgroups (the persistent stream-K GEMMs of a prefill with > 16 rows) may be in
 *     flight per device at a time: callers that use several streams order those launches (Engine does, with an event);
 *   - return 0 on success, negative rv_status on error; rv_last_error() gives the message of the
 *     last failure on the calling thread;
 *   - dtypes: 16-bit OPERANDS (activations / weights / KV caches), RV_F32 residual streams, statistics and logits.  The library is
 *     built in two flavours with this same ABI (same entry points, same layouts - both operand types are 2 bytes wide):
 *         librevision_hip.so       fp16 operands (RV_F16; v_mfma_f32_16x16x32_f16).  The default: Vicuna checkpoints ARE fp16
 *                                  (builder.py:22 loads them with torch_dtype=float16, e2e2.py:185 widens them to fp32 on the CPU), so the weights
 *                                  are held exactly, and activations keep 11 significand bits - the reference's fp32 scores to 1e-3;
 *         librevision_hip_bf16.so  bf16 operands (RV_BF16; v_mfma_f32_16x16x32_bf16): the reference's own GPU dtype (e2e2.py:181-185), 8 bits.
 *     rv_operand_dtype() says which one a loaded library is; wherever this header says "bf16" for a buffer it means "the library's operand
 *     type".  A library REFUSES the other flavour's dtype code (rv_weights_bind, rv_init_hash, rv_gemm out_dtype, ...): a bf16 tensor can
 *     never be read as fp16 bits silently.  f32 -> fp16 conversions saturate at +-65504 (no inf is ever produced by a conversion), a NaN
 *     stays a NaN, and every saturation is COUNTED in the status buffer bound with rv_numeric_status_bind (option "saturated").
 */
#ifndef REVISION_HIP_H
#define REVISION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RV_ABI_VERSION 5

typedef enum { RV_OK = 0, RV_ERR_ARG = -1, RV_ERR_UNBOUND = -2, RV_ERR_HIP = -3, RV_ERR_WORKSPACE = -4 } rv_status;
typedef enum { RV_F32 = 0, RV_BF16 = 1, RV_I32 = 2, RV_I64 = 3, RV_U8 = 4, RV_F16 = 5 } rv_dtype;
typedef enum { RV_ACT_NONE = 0, RV_ACT_RELU = 1, RV_ACT_SILU_MUL = 2, RV_ACT_QUICK_GELU = 3 } rv_act;
typedef enum { RV_W_ROWMAJOR = 0, RV_W_PACKED = 1 } rv_wlayout;
/* ClipEncoder output selection, revisionllm/model/adapter/transformer.py:134-145 */
typedef enum { RV_FEAT_CLS = 0, RV_FEAT_ALL = 2 } rv_feature;

typedef struct rv_ctx rv_ctx;

typedef struct rv_config {
    /* LLM (HF LlamaConfig of Vicuna-7B-v1.5: 4096/11008/32/32/32000, eps 1e-5, theta 1e4) */
    int32_t hidden, inter, layers, heads, vocab;
    float rms_eps, rope_theta;
    /* adapter (revisionllm/model/adapter/transformer.py:61-62: 768, 8 heads, 2+2 layers, ff 2048).  adapter_dim == hidden == 4096 selects the
     * `cross_attn` ClipEncoder of transformer.py:65-67 (d_model = hidden_size, 8 heads of 512): its inputs are hidden-wide and, with "adp.proj_w"
     * left unbound, it has no output projector (nn.Identity, transformer.py:86) */
    int32_t adapter_dim, adapter_heads, adapter_ff, adapter_layers;
    int32_t adapter_text; /* clip_adapter_text: run the two text->video layers */
} rv_config;

/* Everything below is exported; nothing else is (the library is built with -fvisibility=hidden). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int rv_abi_version(void);
/* RV_F16 or RV_BF16: the 16-bit operand type this build of the library computes in (see "dtypes" above). */
int rv_operand_dtype(void);
int rv_last_error(char* buf, size_t n);

/* ---- context + weights ------------------------------------------------------------------- */
/* cfg == NULL creates an OPTIONS-ONLY context: no model, nothing can be bound; it carries tunables for the building-block
 * entry points that take an optional context (rv_gemm, rv_gemm_fp8, rv_sample). */
int rv_ctx_create(const rv_config* cfg, rv_ctx** out);
void rv_ctx_destroy(rv_ctx* ctx);
/* Per-context tunables (measurement / tuning; every default is the production setting).  Keys:
 *   "gemm_tile_variant"  packed-W GEMM family: 2 (default) = 128x128x32 3-stage LDS ring kernel + the 256x256x64 ping-pong kernel
 *                        where it pays (stream-K for few-row deep-K problems when a workspace is given, output-tiled for long-K
 *                        problems whose tile count fills the CUs); 6 = ring kernel only; 1 = 4-stage ring; 0 = 128x128x64 double
 *                        buffer; 3 = register-double-buffered ring; 4 / 5 = ping-pong output-tiled / stream-K wherever supported
 *   "gemm_cus"           CUs (multiple of 8; 0 = all) the persistent prefill GEMMs occupy: their 128 KiB-LDS workgroups own a CU
 *                        each, so a smaller grid leaves whole CUs to the launches of another stream
 *   "gemm_arows"         1 (default): short-K many-row GEMMs (the K = 768 adapter / projector family) take the A-resident kernel
 *   "fp8_decode"         1 (default): KV-cached decode steps stream the FP8 weight copies when all of them are bound ("<name>.f8" /
 *                        "<name>.s8" next to every LLM projection and lm_head); 0: always decode on the bf16 weights
 *   "fp8_prefill"        1 (default): prefill passes run their QKV / o / gate-up / down GEMMs as FP8 x FP8 when the "<name>.f8p"
 *                        copies of every layer are bound and the shape has a persistent plan; 0: always the bf16 weights
 *   "gemm_waves"         8 (default) / 4: waves of a persistent prefill GEMM workgroup (bf16 operands, 256-column panels): 8 = two waves per SIMD
 *                        in ping-pong (128 x 64 outputs each); 4 = one wave per SIMD owning 128 x 128 outputs (accumulators in the AGPR half of
 *                        the register file; 128 instead of 192 KiB of LDS fragment reads per k-tile).  Bit-identical results; measured level
 *                        with 8 up to ~4000 rows (0 .. -2.5 %) and ahead for more rows (8192^3: +30 %).  FP8 x FP8 and 192-column forms: always 8.
 *   "gemm_mhalf"         2 (default since round 6: from 32 row tiles on - 8 prefills to a pass - a QUARTER of the row tiles x four times the panels), 1: a persistent prefill GEMM over >= 10 row tiles of 256 (batched prefills) lets one XCD's team of workgroups cover HALF the
 *                        row tiles of twice as many weight panels (16 row tiles: 8 x 4 instead of 16 x 2 tiles per team) - fewer activation bytes
 *                        re-fetched per tile.  0: the round-3 teams.  The stream-K split points move with the team shape, so results may differ in the
 *                        last bit between the two settings (each is deterministic).
 *   "rows_single"        1 (default): an 81 .. 144-row decode projection whose 64-column groups alone fill >= 3/4 of the CUs (the fused QKV projection:
 *                        192 groups) runs WITHOUT a K split - one workgroup walks all 8 virtual k-waves and finishes its own columns: no partial
 *                        planes, no hand-over (140 rows: 84 -> 64 us per launch, step 10.06 -> 9.47 ms).  Same bits either way.  0: always split.
 *   "rows_persistent"    1 (default): a 33 .. 144-row decode projection with more (column group, split) items than workgroups fit the chip at once
 *                        runs as a persistent grid whose workgroups stream several items back to back and hand their partial sums over once, at
 *                        the end; 0: one workgroup per item (the round-2 launch).  Same results.
 *   "rows_spread"        the 33 .. 144-row decode projections: a launch with at most this many workgroups asks for a CU per workgroup
 *                        (more LDS than two can share) instead of being packed two to a CU (0 = never)
 *   "rows_fill"          (default 240) the 33 .. 144-row decode projections split K (2 / 4 / 8 ways) until a launch has at least this many
 *                        workgroups; measurement knob (same results whatever the split: the summation tree is fixed)
 *   "sample_variant"     1 (default) = top-k selection through the compacted-candidate fast path when the row qualifies (V >= 1024,
 *                        no tie across the k-th place); 0 = always the general 16-round selection.  Identical outputs.
 *   "lm_head_split"      1 (default) = the lm_head input is the split pair [hi | lo] (bf16(x), bf16(x - hi)) over the K-duplicated lm_head whenever
 *                        "llm.lm_head.p2" is bound (its bf16 rounding alone owns two thirds of the bf16 path's distance from the fp32 reference on the
 *                        entropy scores, profiles/r4_error_budget.json); 0 = bf16 lm_head input.  Not used with the FP8 decode weights.
 *   "last_block_rows"    1 (default) = a prefill that returns logits runs the LAST block's o / MLP projections (and the head) on the last row of every
 *                        sequence only - nothing reads that block's other output rows (its K / V are cached before); they go through the few-row
 *                        weight-streaming kernels, <= 32 of them at a time (sequences of >= 32 positions; whatever number of prefills shares the pass).  0 = every row through every block (rounds 1 - 4).  Logits
 *                        differ in the last bits between the two settings (other summation order in that block's projections).
 *   "adapter_fold_t2v"   1 (default) = rv_clip_encoder, text -> video layers (transformer.py:271-305) whose queries have <= 32 text tokens: Q projection + cross-attention +
 *                        output projection run as x.A1^T -> softmax -> P.A2^T with A1 / A2 folded from the text K / V rows per (layer, query) - the same function, other
 *                        rounding points (q and the attention output are never rounded to 16 bits; A1 / A2 are).  0 = the three separate steps.
 *   "attn_lds"           1 (default) = rv_attention / the ClipEncoder's and CLIP towers' self-attention with >= 96 keys and no mask (head width 64 / 96, not causal): a
 *                        workgroup of 128 query rows stages every 32-key block of K / V^T in LDS once (LDS-DMA, double-buffered) instead of each wave fetching its own
 *                        copy from L2 (transformer.py:193,210-223 at T = 256 / 1024); the LLM prefill's causal attention (rv_llm_prefill_* with > 16 rows per sequence) likewise
 *                        shares one staged copy among the four waves of a 64-row workgroup.  0 = the per-wave form.  Rows are bit-identical either way.
 *   "qkv_lds"            1 (default) = the LLM prefill's fused QKV projection (rv_llm_prefill_* / rv_llm_forward with S > 1, persistent 256-column form): a whole panel's RoPE-rotated
 *                        Q, K-cache rows and transposed V-cache pieces are staged in LDS and stored as whole 128-byte row slabs / 16-byte pieces of 8 positions; 0 = every lane
 *                        stores the 4 columns it holds (2-byte stores for V^T).  The same bytes land in the same places (vtimellm_llama.py:79-90 with past_key_values).
 *   "adapter_stream16"   1 (default) = rv_clip_encoder / the 768-d ClipEncoder with an output projector, fp16 build only: the encoder's residual stream is kept in HBM
 *                        as fp16 (the copies its GEMMs consume anyway) instead of f32 + fp16 copies: the residual operands of the out-projection / FFN-2 epilogues and the
 *                        LayerNorm inputs are read as fp16, accumulation and statistics stay f32 (transformer.py:210-223,271-305 keep fp32 activations; the measured
 *                        distance to the fp32 reference is in DESIGN section 4).  0 = the f32 stream.  Ignored by the bf16 build (always f32).
 *   "precision"          0 (default) = bf16 GEMM operands; 1 = PARITY precision of the LLM forward (every rv_llm_* entry point): every GEMM
 *                        operand (the outputs of the two RMSNorms, the attention output, silu(gate) * up, the lm_head input) is the split pair
 *                        [hi | lo] = (bf16(x), bf16(x - hi)) - 16 mantissa bits - multiplied with K-duplicated weight copies on the unchanged
 *                        GEMM kernels; no norm fusion, no FP8.  Needs "llm.L{i}.{wqkv,wo,wgu,wdown}.p2" and "llm.lm_head.p2" bound
 *                        (RV_ERR_UNBOUND otherwise).  What it is for: the reference's fp32 segment scores to the north star's 1e-3
 *                        (vtimellm_llama.py:38-90 executed in fp32 on the CPU; funs_get_feature_X.py:120-146); ~2 x the prefill GEMM time.
 *   "saturated"          (read; write 0 to reset) the sticky count of f32 -> fp16 stores that met a value outside +-65504 since the last reset - any kernel,
 *                        any context of this library instance on the current device (rv_numeric_status_bind: one buffer per instance and device).  The
 *                        reference's bf16 path cannot overflow (e2e2.py:182); this build's default operand type can, and then costs accuracy in that element
 *                        instead of producing inf: this is how a caller learns that a checkpoint's activations left the fp16 range.  Reading or resetting
 *                        waits for the device.  Always 0 in the bf16 flavour and when no buffer is bound.
 * Unknown keys / out-of-range values return RV_ERR_ARG. */
int rv_ctx_set_option(rv_ctx* ctx, const char* key, int64_t value);
int rv_ctx_get_option(const rv_ctx* ctx, const char* key, int64_t* value);
/* Numeric status buffer (ABI v5): 4 x uint32 of caller-owned device memory, 16-byte aligned, zeroed by the caller.  Word 0 = saturated fp16 stores (see
 * option "saturated"; one count per converted pair / quad that held an out-of-range element), words 1 - 3 reserved.  Every kernel of the library instance
 * adds into it from then on (NULL unbinds: nothing is counted); callers that copy results to the host anyway read it with them instead of through the
 * option (no extra wait).  The binding is per library instance and device, not per context: it is the one piece of device-side shared state
 * (device code of different translation units cannot share a symbol without relocatable device code, so each keeps a copy of this pointer).
 * No counterpart in the reference: torch raises / propagates inf on its own. */
int rv_numeric_status_bind(uint32_t* status_dev);
/* Bind a device tensor under a build-defined packed name (see DESIGN.md "weight layout").  Every bf16 MATRIX
 * except llm.embed is fragment-packed (rv_gemm w_layout 1); vectors are plain f32:
 *   llm.embed [V,D] bf16; llm.L{i}.wqkv [3D,D] bf16 (q;k;v rows; inside every head the q and k rows are
 *   pair-interleaved: row 2j = dim j, row 2j+1 = dim j+64, so RoPE partners meet in one lane); llm.L{i}.wo [D,D];
 *   llm.L{i}.wgu [2F,D] bf16, gate/up interleaved in 16-row blocks; llm.L{i}.wdown [D,F];
 *   llm.L{i}.norm1 / norm2 [D] f32; llm.norm [D] f32; llm.lm_head [V,D] bf16;
 *   optional, all or none: "<matrix>.p2" = the fragment packing of [W | W] ([N, 2K]: W duplicated along K) for every llm.L{i} matrix and
 *   llm.lm_head - the weight side of the parity precision (option "precision");
 *   adp.cls_token / adp.cls_pos [768] f32; adp.{t2v,enc}.{l}.{w_in[2304,768],w_out,w1,w2} bf16,
 *   adp.{..}.{b_in,b_out,b1,b2,ln1_w,ln1_b,ln2_w,ln2_b} f32; adp.proj_w [D,768] bf16; adp.proj_b [D] f32;
 *   proj.w [D,768] bf16; proj.b [D] f32   (dense nn.Linear projector, vtimellm_arch.py:42)
 * Replaces model.load_state_dict (builder.py:16,35). */
int rv_weights_bind(rv_ctx* ctx, const char* name, const void* dptr, int dtype, int64_t numel);

/* ---- synthetic weights: w[i] = base + float(int(splitmix64(i + key) >> 40) - 2^23) * step ---- */
int rv_init_hash(void* dst, int dtype, int64_t n, uint64_t key, float step, float base, void* stream);

/* ---- building blocks (exported for the unit parity tests; the engine calls the same kernels) -- */
/* C[M,N] = act(A[M,K] . W[N,K]^T + bias[N]) + residual[M,N]     (nn.Linear semantics)
 * A bf16 row-major (lda in elements).  W bf16: w_layout 0 = row-major [N,K] (ldw), w_layout 1 = fragment-packed
 * (RV_W_PACKED, what rv_weights_bind expects for every matrix):
 *     Wp[(((n>>4)*(K/32) + (k>>5))*64 + (n&15) + 16*((k>>3)&3))*8 + (k&7)]      (N % 16 == 0)
 * bias f32 or NULL, residual f32 (ldr) or NULL (may alias C), out dtype RV_BF16 or RV_F32 (ldc).
 * RV_ACT_SILU_MUL: W rows are 16-row gate/up interleaved and the output has N/2 columns.  K % 64 == 0.
 * M <= 32 takes the weight-streaming (decode) kernel (17 .. 32 rows: two MFMA column blocks per weight fragment).  ws / ws_bytes: optional workspace of rv_gemm_ws_bytes() bytes
 * enabling the persistent stream-K form of the 256x256 ping-pong kernel (packed W, N % 256 == 0, M <= 1024); its first
 * 8 KiB (hand-off flags) must be zero before the first use.  NULL -> output-tiled kernels only.  With stream-K the
 * k-summation is split across workgroups in a fixed order: results are deterministic but differ in the last bits from
 * the output-tiled kernels. */
size_t rv_gemm_ws_bytes(void);
/* Decode projection (M <= 16 rows) with FP8 weights: W8 = e4m3fn (OCP) bytes in the fp8 fragment-packed layout
 * (revisionllm_amd.ops.pack_fragments_fp8), w_scale f32 [N] per-output-row dequantisation scales; everything else as rv_gemm
 * (act: NONE or SILU_MUL).  Opt-in "fp8 LLM path" (BASELINE.json configs[4]): not what the parity / headline numbers use. */
int rv_gemv_fp8(const void* A, int64_t lda, const void* W8, const float* w_scale, const float* bias, const float* residual,
                int64_t ldr, void* C, int64_t ldc, int out_dtype, int act, int64_t M, int64_t N, int64_t K, void* stream);
/* Opt-in FP8 x FP8 prefill GEMM (the "fp8 MFMA LLM path" BASELINE.json configs[4] names; the reference has no counterpart, it
 * runs bf16 / fp16 - never the parity target or the headline).  rv_quant_rows_fp8: bf16 activations x16 [rows, K] -> e4m3fn bytes
 * q8 [rows, K] (row stride ldq bytes) + per-row scales max|row| / 448; q = RNE_e4m3(x * (1 / scale)), IEEE f32.  rv_gemm_fp8: C = act((A8 . W8^T) * a_scale[m] * w_scale[n]) (+ residual); W8p = the [N, K] e4m3fn byte matrix
 * taken as [N, K/2] 16-bit words in the bf16 fragment packing (ops.pack_fragments_fp8_prefill); v_mfma_scale_f32_16x16x128_f8f6f4
 * on the persistent 256x256 ping-pong kernel; few-row deep-K shapes only (those with a stream-K plan), act NONE or SILU_MUL. */
/* LlamaRMSNorm + rv_quant_rows_fp8 in one pass (d = 4096): quantises the bf16-rounded normalised row, i.e. the bytes and
 * scales of rv_quant_rows_fp8(rv_rmsnorm(x)). */
int rv_rmsnorm_quant_fp8(const float* x, const float* w, void* q8, float* scale, int64_t rows, int32_t d, float eps, void* stream);
int rv_quant_rows_fp8(const void* x16, int64_t ldx, void* q8, int64_t ldq, float* scale, int64_t rows, int64_t K, void* stream);
int rv_gemm_fp8(const rv_ctx* ctx /* optional: tunables */, const void* A8, int64_t lda, const float* a_scale, const void* W8p, const float* w_scale, const float* residual,
                int64_t ldr, void* C, int64_t ldc, int out_dtype, int act, int64_t M, int64_t N, int64_t K, void* ws, size_t ws_bytes,
                void* stream);
int rv_gemm(const rv_ctx* ctx /* optional: tunables */, const void* A, int64_t lda, const void* W, int64_t ldw, int w_layout, const float* bias, const float* residual,
            int64_t ldr, void* C, int64_t ldc, int out_dtype, int act, int64_t M, int64_t N, int64_t K, void* ws,
            size_t ws_bytes, void* stream);
/* One projection of a MERGED decode step (33 .. 144 rows; what rv_llm_decode_rows launches four times per block):
 * C[M,N] = act(X . Wp^T), X = M bf16 rows in the fragment-packed decode layout - element (r, k) at
 *     ((((k >> 5) * mbp + (r >> 4)) * 64 + (r & 15) + 16 * ((k >> 3) & 3)) * 8) + (k & 7),   mbp = 4 (M <= 64), 5 (<= 80), 8 (<= 128), 9 (<= 144)
 * row blocks (16 * mbp rows allocated) -, Wp fragment-packed as for rv_gemm (w_scale == NULL) or, with w_scale f32 [N], the FP8
 * (e4m3fn) bytes of rv_gemv_fp8's layout (opt-in fp8 LLM path: half the weight bytes, widened to bf16 in registers), C row-major
 * (ldc = N, or N / 2 with RV_ACT_SILU_MUL, which writes bf16).  planes: workspace of rv_gemm_rows_ws_bytes() bytes; arrive: 2048 int32 arrival counters, ZERO before the first launch
 * and private to one stream (the split-K workgroups of a column group count up in them; they are never reset, so the caller never
 * cleans them either).  N % 64 == 0, K % 128 == 0, K >= 1024, N <= 32768. */
size_t rv_gemm_rows_ws_bytes(void);
int rv_gemm_rows(const void* Xp, const void* Wp, const float* w_scale, void* C, int32_t M, int32_t N, int32_t K, void* planes,
                 int32_t* arrive, int act, int out_dtype, void* stream);
/* y = LayerNorm(x) * w + b, eps 1e-5, biased variance (nn.LayerNorm, transformer.py:202-203).
 * x f32 [rows,d]; any of y_f32 / y_bf16 / y_pos_bf16 may be NULL; y_pos = bf16(y + pos[row % period]). */
int rv_layernorm(const float* x, const float* w, const float* b, float* y_f32, void* y_bf16, void* y_pos_bf16,
                 const float* pos, int64_t period, int64_t rows, int32_t d, void* stream);
/* y = w * x * rsqrt(mean(x^2) + eps) (HF LlamaRMSNorm); x f32 [rows,d] -> y bf16 */
int rv_rmsnorm(const float* x, const float* w, void* y_bf16, int64_t rows, int32_t d, float eps, void* stream);
/* pos[t, j], t = 0..T-1 (frame t+1): transformer.py:35-57 with normalize=True, scale 2*pi */
int rv_sine_pos(float* pos, int32_t T, int32_t d, void* stream);
/* softmax(Q K^T * scale + mask) V for head dims 96 / 128.
 * q [B,Lq,H,dh] bf16 (q_row_stride, q_batch_stride in elements; heads contiguous dh chunks);
 * k [.. Lk ..] bf16 (k_row_stride, k_batch_stride, k_head_stride); vt = V^T [dh, Lk] per (b,h)
 * (vt_batch_stride, vt_head_stride, vt_d_stride); out [B,Lq,H*dh] bf16 (o_row_stride, o_batch_stride).
 * causal: query i (absolute position q_pos0 + i) sees keys <= its position; q_pos0 >= 0 (a negative one - query 0 in front of
 * key 0, a row without any key - is refused with RV_ERR_ARG).
 * key_pad: u8 [B/kv_batch_div,Lk] (1 = ignore) or NULL (nn.MultiheadAttention key_padding_mask,
 * transformer.py:293-294).  Query batch b reads K/V batch b / kv_batch_div (one text for v segments): B must be a multiple of
 * kv_batch_div (a remainder would read a key batch that does not exist: refused with RV_ERR_ARG).
 * A key batch whose keys are ALL padded has no key: its query rows come out as zeros (nn.MultiheadAttention yields NaN there).
 * V^T rows (vt_d_stride) must be padded with finite values to a multiple of 32 keys. */
int rv_attention(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride,
                 int64_t k_batch_stride, int64_t k_head_stride, const void* vt, int64_t vt_batch_stride,
                 int64_t vt_head_stride, int64_t vt_d_stride, void* out, int64_t o_row_stride, int64_t o_batch_stride,
                 const uint8_t* key_pad, int32_t B, int32_t H, int32_t dh, int32_t Lq, int32_t Lk, int32_t causal,
                 int32_t q_pos0, int32_t kv_batch_div, float scale, void* stream);

/* ---- CLIP front end: decoded frames -> patch matrix ------------------------------------------ */
/* Resize(R, BICUBIC) / CenterCrop(R) / Normalize on decoded uint8 frames (inference.py:108-117; Preprocessing, clip_extractor.py:76-97) and the conv1
 * unfold of VisualTransformer.forward (clip/model.py:223-226) in one pass over the source bytes of the cropped region.
 * frames: u8, layout 0 = NCHW [n,3,H,W] (channel planes frame_stride / 3 elements apart) or 1 = NHWC [n,H,W,3] (the 3 bytes of a pixel adjacent);
 * frame_stride / row_stride in elements, so a window of a larger decode buffer is passed as it lies.  mean / std: HOST pointers, read at launch.
 * Values (f32 throughout, no clamp, no u8 intermediate):
 *   resize   shorter side -> R, longer side -> int(R * long / short); antialiased bicubic, a = -0.5, align_corners = False: per axis scale = in / out,
 *            support = 2 * max(scale, 1), centre = scale * (i + 0.5), taps [max(0, int(centre - support + 0.5)), min(in, int(centre + support + 0.5))),
 *            weight cubic((j - centre + 0.5) / max(scale, 1)) / (sum over the taps); separable (torch's interpolate(mode="bicubic", antialias=True))
 *   crop     R x R at top = round_half_even((h' - R) / 2), left likewise
 *   norm     (v / 255 - mean[c]) / (std[c] + 1e-8)
 * Outputs (either may be NULL, not both): image f32 [n,3,R,R]; patches [n*g*g, Kp] of the library's operand type with row stride ldp >= Kp, g = R / patch,
 * Kp = ceil(3 * patch^2 / 128) * 128: patches[(f*g + gy)*g + gx, (c*patch + py)*patch + px] = the image value rounded once, columns 3 * patch^2 .. Kp - 1 zero
 * (columns from Kp on are not touched) - the A matrix of the conv1 GEMM.
 * Refused (RV_ERR_ARG, nothing launched): R % patch != 0, H or W outside 1 .. 8192, null frames, both outputs null, ldp < Kp, a layout other than 0 / 1,
 * and a downscale whose filter taps do not fit a workgroup's LDS (beyond 8192 -> 224 territory).  n = 0 returns 0 and launches nothing. */
int rv_frames_to_patches(const uint8_t* frames, int layout, int64_t frame_stride, int64_t row_stride, int32_t n, int32_t H, int32_t W, int32_t R,
                         int32_t patch, const float mean[3], const float std[3], void* patches, int64_t ldp, float* image, void* stream);

/* The same front end on the bytes a video decoder hands over: 8-bit 4:2:0 YCbCr (NV12 / NV21 / I420 surfaces).  No RGB frame exists anywhere: the kernel
 * resamples Y at full and Cb / Cr at half resolution and applies the colour matrix once per output pixel (resampling is linear, the conversion affine).
 * y: u8 [n,H,W]; cb, cr: u8 planes of H/2 x W/2 samples, neighbouring samples of one plane c_pix bytes apart: c_pix = 1 planar (I420: two planes), c_pix = 2
 * interleaved (NV12: cr == cb + 1; NV21: cb == cr + 1).  All strides in BYTES (cb and cr share theirs), so a window of a larger decode surface with a padded
 * pitch is passed as it lies (INTEGRATION.md has the pointer arithmetic).  matrix: 0 = BT.601 (Kr 0.299, Kb 0.114), 1 = BT.709 (Kr 0.2126, Kb 0.0722);
 * full_range: 0 = studio, 1 = full; chroma_loc: 0 = left (MPEG-2 / H.264 default), 1 = centre (JPEG / MPEG-1).  mean / std / patches / ldp / image / R /
 * patch: as in rv_frames_to_patches.
 * Values (f32 throughout, no clamp, no u8 or RGB intermediate); i = an output index of the RESIZED image, scale = in / out per axis, the resized size and the
 * crop offsets are rv_frames_to_patches' own:
 *   luma     Y' = rv_frames_to_patches' resampling of the Y plane (the same taps, the same normalised f32 weights computed in f64)
 *   chroma   Cb', Cr' = the same filter in chroma-plane coordinates: in_c = in / 2, scale_c = scale / 2, centre_c = scale * (i + 0.5) / 2 + off, off = 0.25 on
 *            the horizontal axis when chroma_loc = 0, else 0 (both sitings are vertically centred); support_c = 2 * max(scale_c, 1), taps
 *            [max(0, int(centre_c - support_c + 0.5)), min(in_c, int(centre_c + support_c + 0.5))), weight cubic((j - centre_c + 0.5) / max(scale_c, 1)) /
 *            (sum over the taps).  A source below 2R per axis has scale_c < 1: chroma is then interpolated.
 *   colour   studio range: yl = (Y' - 16) * 255/219, c = (C' - 128) * 255/224; full range: yl = Y', c = C' - 128;  Kg = 1 - Kr - Kb;
 *            Rv = yl + 2(1-Kr) cr,  Bv = yl + 2(1-Kb) cb,  Gv = yl - (2Kb(1-Kb)/Kg) cb - (2Kr(1-Kr)/Kg) cr;  coefficients computed in f64, rounded once to f32
 *   norm     (v / 255 - mean[c]) / (std[c] + 1e-8); image and patches laid out, rounded once and zero-padded exactly as by rv_frames_to_patches
 * This is the library's OWN definition - the chroma planes are resampled directly, which is linear and exact.  It is NOT swscale's integer conversion to rgb24
 * followed by a resize; no parity with ffmpeg's RGB bytes is claimed.
 * Refused (RV_ERR_ARG, nothing launched): odd H or W, H or W outside 2 .. 8192, c_pix outside {1, 2} (or c_pix = 2 with planes that are not one byte apart),
 * matrix / full_range / chroma_loc outside {0, 1}, a null plane, R % patch != 0, both outputs null, ldp < Kp, a geometry whose tap tables and staging do not
 * fit a workgroup's LDS, more workgroups than one launch holds.  n = 0 returns 0 and launches nothing. */
int rv_yuv_to_patches(const uint8_t* y, int64_t y_frame_stride, int64_t y_row_stride, const uint8_t* cb, const uint8_t* cr, int64_t c_frame_stride,
                      int64_t c_row_stride, int32_t c_pix, int32_t n, int32_t H, int32_t W, int32_t matrix, int32_t full_range, int32_t chroma_loc,
                      int32_t R, int32_t patch, const float mean[3], const float std[3], void* patches, int64_t ldp, float* image, void* stream);

/* The same front end on every planar or semi-planar surface a decoder produces: 8-bit or 16-bit samples, 4:2:0 / 4:2:2 / 4:4:4, interleaved or separate chroma
 * planes (NV12 / NV21 / I420, P010 / P012 / P016, yuv420p10le / yuv420p12le, nv16 / yuv422p / p210, nv24 / yuv444p / p410 ...), described by one struct.
 * rv_yuv_to_patches is this entry on {sample_bytes 1, depth 8, sub 2,2} and gives the same bits.  All strides in BYTES, so a window of a larger decode surface
 * with a padded pitch is passed as it lies (INTEGRATION.md has the pointer arithmetic for P010).  mean / std / patches / ldp / image / R / patch: as in
 * rv_frames_to_patches.
 * Values (f32 throughout, no clamp, no integer or RGB intermediate; f32 holds every 16-bit sample exactly):
 *   sample   the byte, or the little-endian 16-bit word: word >> (16 - depth) when msb_aligned (the low bits are discarded: whatever a decoder leaves there
 *            cannot matter), else the word as it lies (a word >= 2^depth is taken at face value)
 *   luma     Y' = rv_frames_to_patches' resampling of the Y plane (the same taps, the same normalised f32 weights computed in f64)
 *   chroma   per axis, with sub = sub_x or sub_y: in_c = in / sub, scale_c = scale / sub, centre_c = scale * (i + 0.5) / sub + off; off = 0.25 when the axis is
 *            subsampled (sub = 2) AND the chroma sample is sited on the even luma sample of that axis - the horizontal axis for chroma_loc 0 and 2, the vertical
 *            axis for chroma_loc 2 only - else 0; support_c = 2 * max(scale_c, 1), taps [max(0, int(centre_c - support_c + 0.5)),
 *            min(in_c, int(centre_c + support_c + 0.5))), weight cubic((j - centre_c + 0.5) / max(scale_c, 1)) / (sum over the taps).  An axis with sub = 1
 *            is the luma axis unchanged.
 *   colour   s = 2^(depth - 8); studio range: yl = (Y' - 16 s) * 255 / (219 s), c = (C' - 128 s) * 255 / (224 s); full range: yl = Y' * 255 / (2^depth - 1),
 *            c = (C' - 128 s) * 255 / (2^depth - 1); then rv_yuv_to_patches' Rv / Gv / Bv equations with the matrix's Kr, Kb (matrix 2: BT.2020
 *            non-constant luminance, Kr 0.2627, Kb 0.0593); the five coefficients are computed in f64 and rounded once to f32
 *   norm     (v / 255 - mean[c]) / (std[c] + 1e-8); crop, image and patches laid out, rounded once and zero-padded exactly as by rv_frames_to_patches
 * matrix 2 applies the BT.2020 MATRIX only: this entry converts no transfer function and maps no tones, so PQ / HLG-coded values would reach CLIP as coded -
 * HDR surfaces go through rv_yuv_surface_to_patches_hdr (below), which converts them to SDR inside the same kernel.
 * Packed surfaces (YUY2 / UYVY / Y210, AYUV / VUYA / Y410 / XV36 ...) go through rv_packed_to_patches, packed RGB in any byte order (BGR, BGRA, ARGB ...) through
 * rv_frames_to_patches_packed (both below).
 * Not taken: v210, 4:1:1, big-endian words, RGB deeper than 8 bits (rgb48le, x2rgb10le), Bayer, alpha (an alpha plane, byte or field is ignored, never blended),
 * dynamic HDR metadata.
 * Refused (RV_ERR_ARG, nothing launched): a null struct or plane; sample_bytes outside {1, 2}; a depth that does not go with it; msb_aligned outside {0, 1}, or 1
 * with sample_bytes 1; (sub_x, sub_y) outside the three pairs; H or W odd along a subsampled axis (odd sizes are legal along an axis with sub = 1), below sub or
 * above 8192; c_pix outside {sample_bytes, 2 * sample_bytes}; interleaved planes that are not sample_bytes apart; with sample_bytes 2 an odd plane pointer or
 * stride; matrix outside 0 .. 2; full_range outside {0, 1}; chroma_loc outside 0 .. 2; R % patch != 0; both outputs null; ldp < Kp; a geometry whose tap tables
 * and staging (16-bit rows take twice the bytes) do not fit a workgroup's LDS; more workgroups than one launch holds.  n = 0 returns 0 and launches nothing. */
typedef struct rv_yuv_surface {
    const void *y, *cb, *cr;          /* device pointers */
    int64_t y_frame_stride, y_row_stride, c_frame_stride, c_row_stride;   /* BYTES; cb and cr share theirs */
    int32_t sample_bytes;             /* 1, or 2 = little-endian 16-bit words */
    int32_t depth;                    /* 8 with sample_bytes 1; 9 .. 16 with sample_bytes 2 */
    int32_t msb_aligned;              /* 16-bit words only: 0 = value in the low bits (yuv420p10le), 1 = in the high bits (P010 / P012 / P016) */
    int32_t c_pix;                    /* bytes between neighbouring samples of ONE chroma plane: sample_bytes (planar) or 2 * sample_bytes (interleaved) */
    int32_t sub_x, sub_y;             /* 2,2 = 4:2:0   2,1 = 4:2:2   1,1 = 4:4:4 */
    int32_t n, H, W;
    int32_t matrix;                   /* 0 BT.601, 1 BT.709, 2 BT.2020 non-constant luminance (Kr 0.2627, Kb 0.0593) */
    int32_t full_range;               /* 0 studio, 1 full */
    int32_t chroma_loc;               /* 0 left, 1 centre, 2 top-left */
} rv_yuv_surface;
int rv_yuv_surface_to_patches(const rv_yuv_surface* s, int32_t R, int32_t patch, const float mean[3], const float std[3], void* patches, int64_t ldp,
                              float* image, void* stream);

/* rv_yuv_surface_to_patches on an HDR surface (BT.2100 PQ or HLG, typically P010 / yuv420p10le with matrix 2): the same kernel, the same resampling and
 * YCbCr -> R'G'B' equations, then per OUTPUT pixel a conversion to BT.709-coded SDR values in front of the normalisation.  No pass over the source is added.
 * Values (f32 throughout); E'c = v[c] / 255 of the colour step above, with no clamp up to here:
 *   1 clamp    E' = clamp(E'c, 0, 1) per channel
 *   2 transfer to display light F in nits, Lw = peak_nits
 *              PQ (SMPTE ST 2084)  m1 = 2610/16384, m2 = 2523/4096*128, c1 = 3424/4096, c2 = 2413/4096*32, c3 = 2392/4096*32; p = E'^(1/m2);
 *                                  F = 10000 * (max(p - c1, 0) / (c2 - c3 p))^(1/m1), clamped to [0, Lw]
 *              HLG (ARIB STD-B67 / BT.2100)  a = 0.17883277, b = 1 - 4a, c = 0.5 - a ln(4a); scene light E = E'^2 / 3 for E' <= 0.5, else
 *                                  (exp((E' - c) / a) + b) / 12; Ys = 0.2627 Er + 0.6780 Eg + 0.0593 Eb; gamma = 1.2 + 0.42 log10(Lw / 1000);
 *                                  F = Lw * Ys^(gamma - 1) * E, and 0 where Ys = 0
 *   3 tone map the BT.2390 EETF on the brightest channel (hue-preserving), black level 0, Lt = sdr_white_nits;
 *              PQinv(Y) = ((c1 + c2 y) / (1 + c3 y))^m2 with y = (Y / 10000)^m1; mx = max(Fr, Fg, Fb); e = PQinv(mx) / PQinv(Lw);
 *              maxLum = PQinv(Lt) / PQinv(Lw); KS = 1.5 maxLum - 0.5; if KS >= 1, e <= KS or mx = 0 the ratio is 1 (so peak_nits <= sdr_white_nits maps no
 *              tones); otherwise t = (e - KS) / (1 - KS), e2 = (2t^3 - 3t^2 + 1) KS + (t^3 - 2t^2 + t)(1 - KS) + (-2t^3 + 3t^2) maxLum,
 *              ratio = PQ_EOTF(e2 * PQinv(Lw)) / mx; L = F * ratio / Lt per channel
 *   4 gamut    gamut = 1: BT.2020 -> BT.709 primaries with BT.2087's matrix (rows 1.6605 -0.5876 -0.0728 / -0.1246 1.1329 -0.0083 / -0.0182 -0.1006 1.1187);
 *              gamut = 0: none; then clamp to [0, 1]
 *   5 OETF     BT.709's, not a pure power: V = 4.5 L for L < 0.018, else 1.099 L^0.45 - 0.099; v[c] = 255 V.  The linear toe keeps the slope finite at black,
 *              and it is how SDR video, which the other entries pass as coded, was encoded.
 *   6 norm     crop, normalisation, rounding, image and patch layout and zero padding exactly as by rv_yuv_surface_to_patches
 * Constants that are quotients, and the scalars that depend on peak_nits / sdr_white_nits (1 / Lt, PQinv(Lw), maxLum, KS, gamma - 1), are computed in f64 and
 * rounded once to f32; powers are exp2(k * log2(x)) in f32.  This is the library's OWN definition, as the SDR one is; no parity with another tool is claimed.
 * No dynamic metadata is read: no MaxCLL / mastering-display parsing, no Dolby Vision, no inverse tone mapping.  peak_nits is the caller's number (1000 is the
 * usual HDR10 grade and HLG's nominal peak; 203 is BT.2408's reference white).
 * Refused (RV_ERR_ARG, nothing launched): a null map; transfer outside {1, 2}; gamut outside {0, 1}; peak_nits or sdr_white_nits not finite or outside
 * 1 .. 10000; and everything rv_yuv_surface_to_patches refuses.  n = 0 returns 0 and launches nothing. */
typedef struct rv_hdr_map {
    int32_t transfer;                 /* 1 PQ (SMPTE ST 2084), 2 HLG (ARIB STD-B67) */
    int32_t gamut;                    /* 0 none, 1 BT.2020 -> BT.709 primaries */
    float peak_nits;                  /* Lw: the display peak the content was graded for */
    float sdr_white_nits;             /* Lt: the luminance that becomes SDR white (1.0) */
} rv_hdr_map;
int rv_yuv_surface_to_patches_hdr(const rv_yuv_surface* s, const rv_hdr_map* m, int32_t R, int32_t patch, const float mean[3], const float std[3],
                                  void* patches, int64_t ldp, float* image, void* stream);

/* The front end on the picture AS DISPLAYED.  Phone and action-camera streams are coded sideways or upside down and carry a display matrix (mp4's rotate tag);
 * a hardware decoder or a -noautorotate pipe hands over the coded surface.  These two entries turn and flip inside the same kernels: the load side stays in
 * coded orientation, each coded axis is resampled with the scale, crop offset and direction of the display axis it becomes, and only the store is permuted.
 * No pass over the source is added.
 * orient, 0 .. 7, the eight orientations of a rectangle: bit 0 transpose, bit 1 mirror display x, bit 2 mirror display y, applied in that order.  On a plane
 * S[rows, cols]:   D = transpose(S) if orient & 1 else S;   D = D[:, ::-1] if orient & 2;   D = D[::-1, :] if orient & 4.
 * So a turn by 90 degrees clockwise is 3, by 180 degrees 6, by 270 degrees clockwise 5; a horizontal flip is 2, a vertical flip 4; 1 and 7 are the two
 * diagonal flips.  H, W, the strides and the surface struct describe the CODED frames (windows of larger surfaces and padded pitches as before); everything
 * else is as in the un-oriented entry.
 * Values: what the un-oriented entry defines on the oriented picture.
 *   RGB      rv_frames_to_patches' definition on D of every channel plane.  The display size is (Hd, Wd) = (W, H) under transpose; the resized size, the crop
 *            offsets (round half even, in display coordinates) and the tap windows are derived from it, in display coordinates.
 *   YCbCr    every plane is oriented as above.  The display subsampling is (sub_x, sub_y) swapped under transpose: 4:2:2 turned by 90 degrees is a 1,2
 *            surface on the display, which this entry handles (the coded surface is the legal 2,1) although the un-oriented entry refuses that pair.
 *   siting   the chroma offset is computed per CODED axis as in rv_yuv_surface_to_patches (0.25 where a subsampled axis is sited on the even luma sample),
 *            follows its axis to the display axis that axis becomes, and is NEGATED where that display axis is mirrored - a left-sited sample is
 *            right-sited after a flip: centre_c = scale * (i + 0.5) / sub - 0.25.
 *   the rest colour equations, the HDR steps of rv_yuv_surface_to_patches_hdr (m != NULL), normalisation, rounding, patch layout and zero padding: unchanged.
 * The library's OWN definition, as the others are: no parity with swscale's or a transpose filter's bytes is claimed.  orient = 0 gives the bits of the
 * un-oriented entries.
 * Refused (RV_ERR_ARG, nothing launched): orient outside 0 .. 7; everything the un-oriented entry refuses (the parity of H / W is checked along the CODED
 * subsampled axes; m, when given, as by rv_yuv_surface_to_patches_hdr); a geometry whose tap tables and staging do not fit a workgroup's LDS in the oriented
 * plan.  n = 0 returns 0 and launches nothing. */
int rv_frames_to_patches_oriented(const uint8_t* frames, int layout, int64_t frame_stride, int64_t row_stride, int32_t n, int32_t H, int32_t W,
                                  int32_t orient, int32_t R, int32_t patch, const float mean[3], const float std[3], void* patches, int64_t ldp,
                                  float* image, void* stream);
int rv_yuv_surface_to_patches_oriented(const rv_yuv_surface* s, const rv_hdr_map* m /* NULL = SDR */, int32_t orient, int32_t R, int32_t patch,
                                       const float mean[3], const float std[3], void* patches, int64_t ldp, float* image, void* stream);

/* The front end on PACKED surfaces: what capture cards, webcams and V4L2 emit (YUY2 / UYVY), and the 4:2:2 / 4:4:4 surfaces of VAAPI / D3D11 / QSV decoders
 * (Y210, AYUV / VUYA, Y410, XV36), read as they lie - no de-interleave pass, every source row read once for all three components.
 * A packed surface has ONE base pointer; a row is a run of UNITS of unit_bytes bytes that cover pix_per_unit pixels each (all strides in BYTES: a window of a
 * larger surface that starts on a unit boundary, with a padded pitch, is passed as it lies; INTEGRATION.md has the pointer arithmetic for Y210):
 *   sample_bytes 1 or 2 (little-endian 16-bit words): a unit is 4 samples.  pix_per_unit 2 (4:2:2): Y0 at y_off, Y1 half a unit behind it, Cb at cb_off, Cr at
 *                  cr_off (byte offsets in the unit), one chroma pair per two pixels.  pix_per_unit 1 (4:4:4): Y, Cb, Cr at their offsets, the fourth sample (A / X)
 *                  is never read as a value.
 *   sample_bytes 4 the unit is one little-endian 32-bit word of three 10-bit fields and covers one pixel; y_off / cb_off / cr_off are BIT shifts out of 0, 10, 20:
 *                  sample = (word >> off) & 1023.  The top 2 bits are never part of a value.
 *   by ffmpeg's pix_fmt name (memory order)           unit ppu sample  y cb cr   depth msb
 *     yuyv422 (YUY2)   Y0 Cb Y1 Cr                       4   2    1     0  1  3     8    0
 *     uyvy422          Cb Y0 Cr Y1                       4   2    1     1  0  2     8    0
 *     yvyu422          Y0 Cr Y1 Cb                       4   2    1     0  3  1     8    0
 *     y210le / y212le  words Y0 Cb Y1 Cr                 8   2    2     0  2  6   10/12  1
 *     ayuv             A Y Cb Cr                         4   1    1     1  2  3     8    0
 *     vuya / vuyx      Cr Cb Y A                         4   1    1     2  1  0     8    0
 *     uyva             Cb Y Cr A                         4   1    1     1  0  2     8    0
 *     ayuv64le         words A Y Cb Cr                   8   1    2     2  4  6    16    0
 *     xv36le           words Cb Y Cr X                   8   1    2     2  0  4    12    1
 *     xv48le           words Cb Y Cr X                   8   1    2     2  0  4    16    0
 *     xv30le (Y410)    Cb bits 0-9, Y 10-19, Cr 20-29    4   1    4    10  0 20    10    0
 * Values: EXACTLY what rv_yuv_surface_to_patches defines for the planar surface that holds the same samples - sub_x = pix_per_unit, sub_y = 1, the same
 * sample_bytes (2 for the bit-field word), depth and msb_aligned: the sample rule (word >> (16 - depth) when msb_aligned: the low bits cannot matter), taps and
 * f32 weights computed in f64, the siting offset (0.25 on the horizontal axis of a 4:2:2 surface for chroma_loc 0 and 2), the colour equations, with m != NULL the
 * HDR steps of rv_yuv_surface_to_patches_hdr, with orient != 0 the orientation of rv_yuv_surface_to_patches_oriented (the struct describes the CODED surface),
 * normalisation, rounding, image and patch layout and zero padding.  The sums run in the same order: the outputs are the bits of the planar entries.
 * mean / std / patches / ldp / image / R / patch: as in rv_frames_to_patches.
 * Refused (RV_ERR_ARG, nothing launched): a null struct or base pointer; sample_bytes outside {1, 2, 4}; unit_bytes other than 4 * sample_bytes (4 for the
 * bit-field word); pix_per_unit outside {1, 2}, or 2 with the bit-field word; offsets that are negative, outside the unit, off a sample boundary, equal to one
 * another or to the second Y sample's (bit-field word: not three distinct shifts out of 0, 10, 20); a depth that does not go with sample_bytes (8 with 1;
 * 9 .. 16 with 2; 10 with 4); msb_aligned outside {0, 1}, or 1 with anything but 16-bit words; W odd with 2 pixels per unit (odd H is legal), H outside
 * 1 .. 8192, W outside pix_per_unit .. 8192; with 16 / 32-bit words a base pointer or a stride that is not a multiple of the word size; matrix outside 0 .. 2;
 * full_range outside {0, 1}; chroma_loc outside 0 .. 2; orient outside 0 .. 7; a map that rv_yuv_surface_to_patches_hdr refuses; R % patch != 0; both outputs
 * null; null mean / std; ldp < Kp; a geometry whose tap tables and staged row segments (up to 8 bytes per pixel) do not fit a workgroup's LDS - every format above
 * fits at 1080 x 1920 -> 224, the 4:2:2 formats and xv30le at 2160 x 3840 -> 224 -; more workgroups than one launch holds.  n = 0 returns 0 and launches
 * nothing. */
typedef struct rv_packed_surface {
    const void* base;                 /* device pointer: the first unit of the first row of the first frame */
    int64_t frame_stride, row_stride; /* BYTES */
    int32_t unit_bytes;               /* 4 or 8 */
    int32_t pix_per_unit;             /* 2 = 4:2:2, 1 = 4:4:4 */
    int32_t sample_bytes;             /* 1, 2 = little-endian 16-bit words, 4 = one 32-bit word of three 10-bit fields */
    int32_t y_off, cb_off, cr_off;    /* byte offsets inside the unit (y_off: the first Y sample); BIT shifts with sample_bytes 4 */
    int32_t depth;                    /* 8 with sample_bytes 1; 9 .. 16 with 2; 10 with 4 */
    int32_t msb_aligned;              /* 16-bit words only: 1 = value in the high bits (y210le, xv36le) */
    int32_t n, H, W;
    int32_t matrix;                   /* as rv_yuv_surface */
    int32_t full_range;
    int32_t chroma_loc;               /* matters for pix_per_unit 2 only */
} rv_packed_surface;
int rv_packed_to_patches(const rv_packed_surface* s, const rv_hdr_map* m /* NULL = SDR */, int32_t orient, int32_t R, int32_t patch, const float mean[3],
                         const float std[3], void* patches, int64_t ldp, float* image, void* stream);

/* rv_frames_to_patches_oriented on packed 8-bit RGB in ANY byte order, with or without a fourth byte: what cv2.VideoCapture (bgr24), screen capture, compositors
 * and hardware colour converters (bgra, rgba, argb ...) hand over - no channel-swap or repacking pass.  frames: u8 [n,H,W,pix_bytes]; a pixel is pix_bytes (3 or 4)
 * adjacent bytes with R, G, B at byte offsets r_off, g_off, b_off inside it; frame_stride / row_stride in BYTES.
 *   rgb24 3: 0 1 2   bgr24 3: 2 1 0   rgba / rgb0 4: 0 1 2   bgra / bgr0 4: 2 1 0   argb / 0rgb 4: 1 2 3   abgr / 0bgr 4: 3 2 1
 * Values: the bits of rv_frames_to_patches (layout 1; with orient != 0 of rv_frames_to_patches_oriented) on a contiguous RGB copy of the frames.  A fourth byte is
 * never read as a value (alpha is ignored, not blended).
 * Refused (RV_ERR_ARG, nothing launched): pix_bytes outside {3, 4}; an offset outside 0 .. pix_bytes - 1 or two equal offsets; orient outside 0 .. 7; everything
 * rv_frames_to_patches refuses.  n = 0 returns 0 and launches nothing. */
int rv_frames_to_patches_packed(const uint8_t* frames, int32_t pix_bytes, int32_t r_off, int32_t g_off, int32_t b_off, int64_t frame_stride, int64_t row_stride,
                                int32_t n, int32_t H, int32_t W, int32_t orient, int32_t R, int32_t patch, const float mean[3], const float std[3], void* patches,
                                int64_t ldp, float* image, void* stream);

/* The three front-end families on SEPARATELY ALLOCATED frames: a hardware decoder's surface pool hands out one device pointer per frame, in whatever order the
 * pool recycles them; a capture ring buffer and the frames of several cameras of one resolution are scattered likewise.  Every entry above addresses frame f as
 * base + f * frame_stride, which costs such a caller a device-to-device copy of every source frame into a staging batch.  These entries take the frames of a
 * batch from a table of per-frame pointers in ONE launch per RV_FRAME_TABLE_MAX frames; everything else - size, pitches, sample format, colour tags, HDR map,
 * orientation - is shared by the batch.  Each pointer is free: windows of larger surfaces keep working, frames need no slack around them (the kernels read
 * exactly the row segments of the crop), and a frame may be listed twice.  No pass over the source is added, no device workspace is used.
 * The pointer arrays (frames, planes, bases) are HOST arrays of n DEVICE pointers; they are read at the call (the table travels in the kernel arguments) and need
 * not outlive it.  A batch longer than RV_FRAME_TABLE_MAX frames is cut into launches of at most that many by the entry; n = 60 is one launch.
 *   rv_frames_to_patches_scattered   layout 0: frames[f] is an NCHW frame whose channel planes lie channel_stride bytes apart (pix_bytes 3 and offsets 0, 1, 2
 *                                    are required); layout 1: packed pixels as rv_frames_to_patches_packed takes them (pix_bytes, r_off, g_off, b_off; rgb24 is
 *                                    3 and 0, 1, 2).  row_stride in bytes.
 *   rv_yuv_surfaces_to_patches       s gives n, the geometry, the row strides, the sample format and the tags; s->y / cb / cr and the two frame strides are NOT
 *                                    read.  planes[f] holds the Y, Cb and Cr pointers of frame f; interleaved chroma (c_pix = 2 * sample_bytes) has cr = cb +-
 *                                    sample_bytes, the same way round in every frame; planar chroma may lie anywhere, frame by frame.  m: NULL = SDR.
 *   rv_packed_surfaces_to_patches    s as above (s->base and frame_stride are NOT read); bases[f] is the first unit of the first row of frame f.
 * Values: EXACTLY what the contiguous entry of the family (rv_frames_to_patches_oriented / rv_frames_to_patches_packed, rv_yuv_surface_to_patches_oriented,
 * rv_packed_to_patches) defines for frame f located at the f-th pointer(s): the same taps, weights and sums in the same order, so the outputs are the bits of that
 * entry on a stacked copy of the frames.  Output rows of frame f are where they always were.
 * Refused (RV_ERR_ARG, nothing launched - the whole table is validated before the first launch): everything the contiguous entry refuses; a null array with
 * n > 0; a null pointer in any entry; a 16 / 32-bit surface with a pointer in any entry that is not a multiple of the word size; interleaved chroma where some
 * frame's cr - cb is not that of frame 0; each of these messages names the frame.  n = 0 returns 0 and launches nothing. */
#define RV_FRAME_TABLE_MAX 64
typedef struct rv_surface_planes { const void *y, *cb, *cr; } rv_surface_planes;
int rv_frames_to_patches_scattered(const uint8_t* const* frames, int layout, int32_t pix_bytes, int32_t r_off, int32_t g_off, int32_t b_off,
                                   int64_t channel_stride, int64_t row_stride, int32_t n, int32_t H, int32_t W, int32_t orient, int32_t R, int32_t patch,
                                   const float mean[3], const float std[3], void* patches, int64_t ldp, float* image, void* stream);
int rv_yuv_surfaces_to_patches(const rv_yuv_surface* s, const rv_surface_planes* planes, const rv_hdr_map* m /* NULL = SDR */, int32_t orient, int32_t R,
                               int32_t patch, const float mean[3], const float std[3], void* patches, int64_t ldp, float* image, void* stream);
int rv_packed_surfaces_to_patches(const rv_packed_surface* s, const void* const* bases, const rv_hdr_map* m /* NULL = SDR */, int32_t orient, int32_t R,
                                  int32_t patch, const float mean[3], const float std[3], void* patches, int64_t ldp, float* image, void* stream);

/* ---- adapter ---------------------------------------------------------------------------- */
/* nn.Linear(768, D) projector on [rows,768] bf16 -> [rows,D] (vtimellm_arch.py:42,125). out f32 or bf16. */
int rv_project_dense(rv_ctx* ctx, const void* x_bf16, void* y, int out_dtype, int64_t rows, void* stream);
/* ClipEncoder.forward (transformer.py:94-145) on N independent sequences.
 * x [N,T,d] bf16; txt [Nq,Lq,d] bf16 (d = adapter_dim: 768, or 4096 for the hidden-wide cross_attn encoder, whose callers project frames and
 * text first - mm_projector / text_mm_projector, vtimellm_arch.py:125, transformer.py:105-106) and txt_mask u8 [Nq,Lq] (1 = valid) with sequence n using text
 * row n / (N/Nq) (hierarchy: '(b v) t d', vtimellm_arch.py:115-121); ignored when adapter_text == 0.
 * A query whose every token is masked has no key: its text -> video attention output is zero in every option form, so its sequences stay finite.
 * out f32: RV_FEAT_CLS [N,D]; RV_FEAT_ALL [N,T+1,D] (row 0 = CLS; the 'temporal' feature is rows 1..T,
 * sliced by the caller). */
size_t rv_clip_encoder_ws_bytes(const rv_ctx* ctx, int32_t N, int32_t T, int32_t Nq, int32_t Lq);
int rv_clip_encoder(rv_ctx* ctx, const void* x, const void* txt, const uint8_t* txt_mask, int32_t N, int32_t T,
                    int32_t Nq, int32_t Lq, int32_t feature, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- LLM -------------------------------------------------------------------------------- */
/* Embedding gather + video-row splice (vtimellm_arch.py:149-238). map i32 [rows]: v >= 0 -> token id
 * (row of llm.embed), v < 0 -> video row -(v+1) of video_rows f32 [*,D].  h f32 [rows,D]. */
int rv_splice_embed(rv_ctx* ctx, const int32_t* map, const float* video_rows, float* h, int64_t rows, void* stream);
/* KV cache for B rows, Smax positions (a multiple of 32): K [L,B,H,Smax,dh] and V^T [L,B,H,Smax/8,dh,8], bf16 - V transposed in blocks of 8
 * positions: element (d, pos) of one (row, head) at ((pos >> 3) * dh + d) * 8 + (pos & 7).  Opaque to callers that only hand it back. */
size_t rv_kv_bytes(const rv_ctx* ctx, int32_t B, int32_t Smax);
size_t rv_llm_ws_bytes(const rv_ctx* ctx, int32_t B, int32_t S);
/* 32x Llama block over h f32 [B,S,D] (clobbered), positions pos0..pos0+S-1, causal, appends to the cache;
 * logits f32 [B,V] of the LAST position only (LlamaForCausalLM.forward via vtimellm_llama.py:79-90).
 * S > 1: prefill (pos0 = 0); S == 1: one KV-cached decode step at position pos0 (vtimellm_arch.py:88-100). */
int rv_llm_forward(rv_ctx* ctx, float* h, int32_t B, int32_t S, int32_t pos0, void* kv, int32_t Smax, float* logits,
                   void* ws, size_t ws_bytes, void* stream);

/* Blocks [layer_begin, layer_end) of the decoder stack over h f32 [B,S,D], in place: the residual stream behind block
 * layer_end - 1, no final norm, no lm_head (rv_llm_forward = rv_llm_layers(0, L) + model.norm + lm_head on the last position).
 * Same kernels, cache layout and workspace as rv_llm_forward: S > 1 prefill rows at positions 0..S-1 (pos0 = 0), S == 1 one
 * KV-cached decode step at pos0 (B <= 144; above 32 rows the split-K decode kernel); only the cache planes of those blocks are
 * touched.  This is what the per-layer parity tests drive: block l is fed the REFERENCE's input of block l
 * (transformers LlamaDecoderLayer.forward as called from vtimellm_llama.py:79-90) and compared with the reference's output. */
int rv_llm_layers(rv_ctx* ctx, float* h, int32_t B, int32_t S, int32_t pos0, void* kv, int32_t Smax, int32_t layer_begin,
                  int32_t layer_end, void* ws, size_t ws_bytes, void* stream);

/* Prefill of B sequences that start with the same P0 tokens (inference() repeats one prompt, inference.py:36): under
 * causal attention the prefix rows are identical for every sequence, so they are computed once.
 * h f32 [P0 + B*S, D]: the P0 shared rows (positions 0..P0-1) followed by S rows per sequence (positions P0..P0+S-1).
 * The prefix K/V are written into all B caches; logits f32 [B,V] of each sequence's last position.  Results are
 * bit-identical to rv_llm_forward on the B full sequences. */
size_t rv_llm_prefill_shared_ws_bytes(const rv_ctx* ctx, int32_t B, int32_t P0, int32_t S);
int rv_llm_prefill_shared(rv_ctx* ctx, float* h, int32_t B, int32_t P0, int32_t S, void* kv, int32_t Smax, float* logits,
                          void* ws, size_t ws_bytes, void* stream);

/* Several generates sharing ONE KV pool of kv_rows cache rows ([L, kv_rows, H, Smax, dh] and its V^T twin), so that their decode
 * steps can be merged into one pass over the weights (a decode step streams all 13 GB whatever the number of rows).
 * rv_llm_prefill_pool: rv_llm_prefill_shared (P0 > 0) / rv_llm_forward prefill (P0 = 0) of B sequences whose cache rows are
 *   kv_row0 .. kv_row0 + B - 1 of the pool; results bit-identical to the same prefill into a cache of its own.
 * rv_llm_decode_rows: ONE KV-cached decode step of the pool's R = kv_rows rows (R <= 144: up to 32 rows take the weight-streaming kernel,
 * 33 .. 144 the split-K kernel with LDS-shared activations; both stream the FP8 weight copies when bound and enabled), row r at its OWN position row_pos[r]
 *   (device int32 [R]); row_pos[r] < 0 = inactive row: nothing is appended to its cache, its logits are unspecified; a row with
 *   row_pos[r] >= Smax (past the pool's capacity) is treated like an inactive one on the device - nothing is stored, no other row's
 *   cache is touched, its logits are unspecified (the positions live on the device: no error can be returned).  h f32 [R, D]
 *   (clobbered), logits f32 [R, V].  A row's result equals what rv_llm_forward(S = 1, pos0 = row_pos[r]) gives for it in any batch.
 *   Workspace: rv_llm_ws_bytes(ctx, R, 1). */
int rv_llm_prefill_pool(rv_ctx* ctx, float* h, int32_t B, int32_t P0, int32_t S, void* kv, int32_t kv_rows, int32_t kv_row0, int32_t Smax,
                        float* logits, void* ws, size_t ws_bytes, void* stream);
 /* rv_llm_prefill_pool_groups: G (<= 8) prefills of IDENTICAL geometry (B, P0, S) in one pass - the prefills of several generates in
 *   flight batched so that the GEMMs see G * (P0 + B * S) rows.  h f32 [G * (P0 + B * S), D]: block g = [P0 shared-prefix rows ; B x S
 *   rows] of group g, whose cache rows are kv_row0[g] .. kv_row0[g] + B - 1 (HOST array of G ints); logits f32 [G * B, V].
 *   Workspace: rv_llm_ws_bytes(ctx, G * (P0 + B * S), 1).  Per-row results equal the separate prefills up to the summation order of the
 *   GEMMs (the stream-K split points depend on the row count). */
int rv_llm_prefill_pool_groups(rv_ctx* ctx, float* h, int32_t G, int32_t B, int32_t P0, int32_t S, void* kv, int32_t kv_rows,
                               const int32_t* kv_row0, int32_t Smax, float* logits, void* ws, size_t ws_bytes, void* stream);
/* rv_llm_prefill_pool_groups_ragged (round 4): rv_llm_prefill_pool_groups for sequences of DIFFERENT lengths, right-padded to S rows each (the 9 calls
 *   of a 33-window stage-2 recursion present 32 x 8 and 33 x 1 video tokens: one generate instead of two).  Under causal attention a valid row never sees
 *   a later (pad) row, so the only thing that changes is WHICH row of a sequence feeds the lm_head: last_rows (DEVICE int32 [G * B]) holds, per
 *   sequence, the index into h of its last valid row; logits row i comes from it.  The pad rows' K / V land at cache positions the first decode steps
 *   overwrite before they are read (rv_llm_decode_rows appends at row_pos[r] = the sequence's own length, then attends to 0 .. row_pos[r]).
 *   G = 1 is the single ragged prefill.  Everything else as rv_llm_prefill_pool_groups. */
int rv_llm_prefill_pool_groups_ragged(rv_ctx* ctx, float* h, int32_t G, int32_t B, int32_t P0, int32_t S, void* kv, int32_t kv_rows,
                                      const int32_t* kv_row0, int32_t Smax, const int32_t* last_rows, float* logits, void* ws, size_t ws_bytes,
                                      void* stream);
/* rv_llm_prefill_pool_mixed: G (<= 8) prefills of DIFFERENT geometry in one pass (vtimellm_llama.py:38-90 run once per generate): group g has its own
 *   (B, P0, S) and cache rows kv_row0 .. kv_row0 + B - 1 of the pool (groups: HOST array of G entries).  h f32 [sum_g (P0_g + B_g * S_g), D]: block g =
 *   [P0_g shared-prefix rows ; B_g x S_g rows], the blocks back to back with no pad rows; logits f32 [sum_g B_g, V] in group order, then sequence order.
 *   last_rows (DEVICE int32 [sum_g B_g], or NULL): as in the ragged entry, per sequence the index into h of the row that feeds the lm_head; NULL = the last
 *   row of every sequence.  Limits (anything else returns RV_ERR_ARG, nothing falls back): non-empty groups inside the pool whose cache-row ranges do not
 *   overlap; Smax % 32 == 0 and P0_g + S_g <= Smax; S_g > 16 and (P0_g == 0 or P0_g > 16); sequences shorter than 32 positions (P0_g + S_g) only among
 *   themselves (their last block takes another form, and a sequence's logits must not depend on what shares its pass); the plain 16-bit path only (RV_ERR_ARG with precision = 1 or
 *   with the FP8 prefill weights in use).  Workspace: rv_llm_ws_bytes(ctx, total rows, 1).  Per-row results equal the separate prefills up to the
 *   summation order of the GEMMs; G groups of ONE geometry give the bytes of rv_llm_prefill_pool_groups. */
typedef struct rv_prefill_group { int32_t B, P0, S, kv_row0; } rv_prefill_group;
int rv_llm_prefill_pool_mixed(rv_ctx* ctx, float* h, int32_t G, const rv_prefill_group* groups, void* kv, int32_t kv_rows, int32_t Smax,
                              const int32_t* last_rows, float* logits, void* ws, size_t ws_bytes, void* stream);
int rv_llm_decode_rows(rv_ctx* ctx, float* h, int32_t R, const int32_t* row_pos, void* kv, int32_t Smax, float* logits, void* ws,
                       size_t ws_bytes, void* stream);
/* rv_llm_decode_rows_shared: rv_llm_decode_rows + a hint about cache contents (round 4): row_share (device int32 [R], or NULL) holds, per
 *   row r, sibling | len << 16: the first `len` cache positions of row r are BIT-IDENTICAL to those of row `sibling` (<= 143) - what the
 *   shared-prefix prefill (rv_llm_prefill_pool with P0 > 0) leaves in the rows of one generate, whose prompts start with the same P0 tokens
 *   (inference.py:36 repeats one prompt per batch row; the 7 calls of a stage-2 recursion share "system prompt + USER: <video>").  The decode
 *   attention then reads the key blocks inside that prefix from the sibling's cache rows: the rows of one (generate, head) run on one XCD and hit
 *   its L2 instead of fetching identical copies from HBM (15 % of the K / V bytes of a 140-row step).  The hint cannot change a result - the
 *   bytes read are the same - only a wrong hint can; 0 (= row 0, length 0) means "nothing shared".  Contract of a word: sibling < R, 0 <= len < 32768
 *   (the word is an int32) and len <= row_pos[r] + 1; a word that violates it is IGNORED by the kernel (the row reads its own cache), never followed out
 *   of bounds.  Smax <= 65535. */
int rv_llm_decode_rows_shared(rv_ctx* ctx, float* h, int32_t R, const int32_t* row_pos, const int32_t* row_share, void* kv, int32_t Smax,
                              float* logits, void* ws, size_t ws_bytes, void* stream);

/* ---- token selection + scores ----------------------------------------------------------- */
/* HF warper chain temperature -> top-k -> top-p, inverse-CDF draw with caller uniforms (or argmax when
 * do_sample == 0), plus the entropy of the processed and of the raw distribution
 * (vtimellm_llama.py:312-338; funs_get_feature_X.py:131-132).  logits f32 [B,V].
 * out_topk_idx i32 / out_topk_val f32 [B,top_k_cap]: kept candidates in descending order (processed
 * scores), n_keep i32 [B].  top_k in [1, 64]: the list holds the min(top_k, V) largest scores (HF's min(top_k, V): a vocabulary shorter than top_k
 * is kept whole), -1 / -inf beyond them; -0.0 and +0.0 are equal scores (ties: the smaller index first); the draw never lands on a candidate without
 * mass (a -inf score inside the list).  Or 0 = NO top-k filter (HF: `top_k` None / 0 - TopKLogitsWarper is not instantiated; what a
 * checkpoint's generation_config.json may ask for: inference.py:45-59 passes no top_k, so the config's value rules): every token is a candidate,
 * only top-p trims; no candidate list is produced then (out_topk_* = -1 / -inf, n_keep = the number kept) and the kept set is
 * {processed score >= out_threshold[b]}.  top_k > 64 (wider than the list; >= V removes nothing) runs the same way: TopKLogitsWarper's rule - every score
 * below the top_k-th largest one goes, a tie at that place stays whole - then top-p over what is left.  out_threshold f32 [B] (optional, may be NULL): the smallest processed score the filters keep. */
int rv_sample(const rv_ctx* ctx /* optional: tunables */, const float* logits, int32_t B, int32_t V, const float* uniforms, int32_t do_sample, float temperature,
              int32_t top_k, float top_p, int32_t* out_tokens, float* out_entropy_proc, float* out_entropy_raw,
              int32_t* out_topk_idx, float* out_topk_val, int32_t* out_nkeep, float* out_threshold, void* stream);
/* get_entropy_statistics (funs_get_feature_X.py:120-146): logits f32 [B,G,V] -> [B,4] = max,min,mean,std. */
int rv_entropy_stats(const float* logits, int32_t B, int32_t G, int32_t V, float* out, void* stream);
/* Stage-2 cosine score (eval_nlq_retrieval_e2e2.py:380-386): feat bf16/f32 [n,T,768]; per segment:
 * column-normalise over frames, top-k frames by <f,q>, sum, dot q.  out f32 [n]; k <= 0: the mean over the frames.
 * Non-finite input: the frames are ranked in torch.topk's order (a NaN similarity before every number, ties: smaller frame index), so out[i] is
 * NaN whenever a similarity of segment i is NaN, for every k, as the reference's is - a NaN feature, or a column that is zero in every frame
 * (0 / 0 in its norm), makes every similarity of the segment NaN.  The other segments of the launch are unaffected. */
int rv_topk_cosine(const void* feat, int feat_dtype, const float* q_cls, int32_t n, int32_t T, int32_t d, int32_t k,
                   float* out, void* stream);

/* _topk_pooling (revisionllm/eval/similarity.py:71-94): video bf16/f32 [Nv,T,d], text f32 [Nt,d] -> out f32 [Nv,Nt,d] = SUM of
 * the k frames of video v with the largest <f_t, text_j> (ties: smaller frame index), added in descending-similarity order;
 * out_idx i32 [Nv,Nt,k] (the selected frames, optional).  1 <= k <= min(64, T).
 * Non-finite input: torch.topk's order - a frame whose similarity is NaN ranks before every number (among NaN frames the smaller index first), is
 * selected, and its columns come out NaN where the frame holds NaN, as the reference's do; out_idx always holds k distinct indices in [0, T). */
int rv_topk_pool(const void* video, int dtype, const float* text, int32_t Nv, int32_t T, int32_t d, int32_t Nt, int32_t k,
                 float* out, int32_t* out_idx, void* stream);

/* ---- proposal-query matching (revisionllm/eval/similarity.py:24-69) and attention pooling (:96-113) ----
 * The reference scores a proposal by slicing its window out of the video, normalising each frame of the slice, _topk_pooling the k = min(3, len)
 * frames most similar to the normalised text CLS and taking the pooled row's dot product with the text: the SUM of the window's top-k cosines.
 * Two launches do it for all proposals: the features are read ONCE into a per-frame cosine row, then every span works on that row.  Durations and
 * windows stay on the device (the reference converts both to int32 on the host).
 * Arithmetic: 16-bit features are read as stored and every operation is f32, as in the other score kernels; the reference run in bf16 does bf16
 * arithmetic instead (its f32 run is what the tests compare to).  Not taken: per-frame masking (the mask only gives the duration, as in the
 * reference).  Several texts per video: the two _multi entries below. */

/* video f32 / 16-bit operands [B,L,d] contiguous, text f32 [B,d] -> out f32 [B,L]: out[b,l] = <f_l, t_b> / (|f_l| |t_b|)  (similarity.py:36, :61-64 for
 * every frame).  One pass over the features; 16-byte loads when d is a multiple of 16 B / element size and the base is 16-byte aligned.  A zero frame
 * or a zero text gives NaN (0 / 0, as the reference's divisions do).  d <= 8192 (the text row staged in LDS); no limit on L. */
int rv_frame_cosine(const void* video, int dtype, const float* text, int32_t B, int32_t L, int32_t d, float* out, void* stream);

/* sims f32 [B,L] (rv_frame_cosine's row), spans f32 [B,N,2] as (centre, width), mask f32 [B,L] -> scores f32 [B,N], windows i32 [B,N,2] (optional, may
 * be NULL).  The window rule is similarity.py:52-60 in f32, each operation rounded on its own: duration = sum of the mask row, x1 = c - 0.5 w,
 * x2 = c + 0.5 w, p = x * duration, start = max(0, int32(floor(p1))), end = int32(ceil(p2)); the window is Python's range(L)[start:end] over the
 * ARRAY length L: lo = min(start, L), hi = end < 0 ? max(end + L, 0) : min(end, L), empty when hi <= lo.  windows holds (lo, hi).
 * mode 0: the sum of the min(k, hi - lo) largest sims of the window in torch.topk's order (NaN first, larger value, smaller index); 1 <= k <= 64.
 * mode 1: sum_t softmax_t(s / temperature) s_t over the window (the alternative at similarity.py:63); temperature finite and not 0.
 * An empty window scores 0 (the reference sums zero frames); a NaN similarity inside the window gives NaN in both modes.
 * Build-defined (the reference's int conversion is undefined there): a non-finite p1 or p2 gives score NaN and window (-1, -1); finite values
 * outside int32 saturate.  No read of sims lies outside [b L + lo, b L + hi). */
int rv_span_scores(const float* sims, const float* spans, const float* mask, int32_t B, int32_t L, int32_t N, int32_t mode, int32_t k,
                   float temperature, float* scores, int32_t* windows, void* stream);

/* Q texts per video (similarity.py:24-69 for every query of a video in one pass over its features).
 * video f32 / 16-bit operands [B,L,d] contiguous, text f32 [B,Q,d], text_unit f32 [B,Q,d] (workspace: receives text / |text|) -> out f32 [B,Q,L]:
 * out[b,q,l] = <f_bl, t_bq> / (|f_bl| |t_bq|), each query's row contiguous for rv_span_scores_multi.  Order of operations: the texts are normalised
 * (a small launch of its own), then the dot products on the f32-input MFMA (16-bit features converted in registers, which is exact; per element a
 * k-ordered fmaf chain, no wider accumulation), then the division by |f|, whose square comes from the same loads.  The features are read from global
 * memory once per call for up to 128 queries (once per 128 beyond).  16-byte loads when d is a multiple of 16 B / element size and video and text_unit
 * are 16-byte aligned, an element-wise path otherwise.  A query's row does not depend on Q, on its slot or on the other texts, bit for bit.
 * A zero text gives a NaN row for that query only; a zero frame NaN in column l of every query; a NaN feature of frame l NaN in column l only.
 * B * Q <= 65535; no limit on L or d. */
int rv_frame_cosine_multi(const void* video, int dtype, const float* text, int32_t B, int32_t Q, int32_t L, int32_t d, float* text_unit, float* out,
                          void* stream);

/* rv_span_scores for Q queries per video: sims f32 [B,Q,L] (rv_frame_cosine_multi's rows), spans f32 [B,Q,N,2] (each query's own proposals),
 * mask f32 [B,L] (one row, hence one duration, per video) -> scores f32 [B,Q,N], windows i32 [B,Q,N,2] (optional, may be NULL).  The same kernel
 * body as rv_span_scores, so every rule above holds per (b, q) row and a row's result equals rv_span_scores' on that row bit for bit.
 * B * Q <= 65535. */
int rv_span_scores_multi(const float* sims, const float* spans, const float* mask, int32_t B, int32_t Q, int32_t L, int32_t N, int32_t mode, int32_t k,
                         float temperature, float* scores, int32_t* windows, void* stream);

/* _attention_pooling (similarity.py:96-113): video f32 / 16-bit operands [Nv,T,d], text f32 [Nt,d] -> out f32 [Nv,Nt,d] =
 * sum_t softmax_t(<f_t, text_j> / temperature) f_t.  temperature finite and not 0 (negative values are taken as given); (d + T) * 4 + 256 bytes of LDS
 * <= 64 KB.  A NaN similarity makes that (video, text) row NaN in every column, as torch.softmax does; other videos are unaffected. */
int rv_attn_pool(const void* video, int dtype, const float* text, int32_t Nv, int32_t T, int32_t d, int32_t Nt, float temperature,
                 float* out, void* stream);

/* ---- ranking scored proposals: sort, greedy temporal NMS, top-M, hits against a ground-truth span (no counterpart kernel in the reference: its
 * eval/metrics.py grounding_metrics_stream ranks on the host from JSON logs, one Python sort per query) ----
 * scores f32 [R,N] (a row = one video, or one (video, query): rv_span_scores[_multi]'s rows with R = B or B Q), spans f32 [R,N,2], gt f32 [R,2] as
 * (start, end) or NULL, hit_iou f32 [T] thresholds in DEVICE memory (NULL exactly when T = 0) ->
 *   order     i32 [R,N]    (optional) the rank order, a permutation of 0 .. N-1
 *   keep      i32 [R,top]  the indices that survive NMS, in rank order, at most `top` of them, then -1
 *   n_keep    i32 [R]      how many
 *   keep_iou  f32 [R,top]  (optional, needs gt) IoU of each kept proposal with gt[r]; 0 in the padding
 *   first_hit i32 [R,T]    (optional, needs gt) the smallest p with keep_iou[r,p] > hit_iou[t], or -1
 * Every f32 operation is rounded on its own (no contraction, no fast-math), so the result is a function of the row alone: it does not depend on R, on
 * the row's place or on which of the two kernel forms ran.
 * Bounds: form 0 reads (start, end); form 1 reads (centre, width): s = c - 0.5 w, e = c + 0.5 w (span_cxw_to_xx's rule).  A span is VOID when a bound
 * is not finite or e <= s.
 * Overlap: inter(a,b) = max(0, min(ea,eb) - max(sa,sb)), union = ((ea - sa) + (eb - sb)) - inter.  With a void span inter = 0 and the IoU is 0: a void
 * span neither suppresses nor is suppressed (it is still ranked and kept in its turn).
 * Order: descending score; ties - -0 against +0 included - go to the smaller index; a NaN score ranks AFTER every number, -inf included, and among NaNs the
 * smaller index comes first.  This differs ON PURPOSE from the torch.topk order of the score kernels above (NaN first): rv_span_scores gives NaN to a
 * proposal with non-finite bounds, and a ranked list must not open with it.
 * Greedy NMS: walk the order; a proposal still alive is kept, and every LATER proposal j with inter(i,j) > nms_iou * union(i,j) dies (one multiplication,
 * one comparison, no division; a proposal that has died suppresses nothing).  Stop after `top` kept.  nms_iou >= 1 suppresses nothing (inter <= union).
 * With gt: keep_iou = union > 0 ? inter / union : 0 (one correctly rounded division) against gt[r]; a void gt gives 0 everywhere and no hit.  The hit
 * test is a strict > in f32.
 * Refused with RV_ERR_ARG, outputs untouched: a null scores / spans / keep / n_keep; R < 1; N < 1 or N > 2048; top outside [1, N]; form not 0 or 1;
 * nms_iou negative or not finite; T outside [0, 16]; hit_iou, T > 0, keep_iou or first_hit without gt; T > 0 without hit_iou; gt with T = 0 and no keep_iou.
 * N <= 64: one wave per row (registers and cross-lane operations only); N <= 2048: one workgroup per row (bitonic sort in 38 KB of LDS).  Rows ride on
 * the grid's x dimension: no limit of 65535 on R. */
int rv_span_rank(const float* scores, const float* spans, int32_t form, int32_t R, int32_t N, int32_t top, float nms_iou, const float* gt,
                 const float* hit_iou, int32_t T, int32_t* order, int32_t* keep, int32_t* n_keep, float* keep_iou, int32_t* first_hit, void* stream);

/* ---- span proposals from a similarity row: temporal grouping of the thresholded row at several levels, in the manner of TAG / watershed proposals
 * (this project's own definition; the reference takes its proposals from the LLM and has no counterpart) ----
 * sims f32 [R,L] (a row = one video, or one (video, query): rv_frame_cosine[_multi]'s rows), mask f32 [R / rpm, L] (rpm = "rows per mask", as in
 * rv_span_scores_multi; R a multiple of rpm), levels: T floats in HOST memory (copied into the kernel arguments), 1 <= T <= 8 ->
 *   spans    f32 [R,N,2]  (centre, width) as fractions of the duration, the form rv_span_scores and rv_span_rank read; NaN (0x7fc00000) in the padding
 *   n_spans  i32 [R]      min(found, N)
 *   n_found  i32 [R]      (optional) found, the number of surviving runs: n_found > n_spans shows an overflow
 *   windows  i32 [R,N,2]  (optional) (lo, hi) of each span, (-1, -1) in the padding
 *   smoothed f32 [R,L]    (optional) s' in [0, D); the rest of it is untouched
 * Every f32 operation is rounded on its own (no contraction), so a row's result is a function of that row alone: it does not depend on R, on the
 * row's place or on the tiling.
 * Duration: dur = the f32 sum of the row's mask row, D = min(L, max(0, int(floor(dur)))), D = 0 for a non-finite dur.  Only frames [0, D) exist for the
 * row; the mask gives the duration only, as everywhere in this library, and no frame of sims at or past D is read.  The result is defined for masks
 * whose sum is exact in any order (0 / 1 masks); for other masks it is build-defined (the order of the sum is the kernel's).
 * Smoothing (smooth odd, h = smooth / 2): for t in [0, D), a = max(0, t - h), b = min(D - 1, t + h),
 * s'[t] = (((s[a] + s[a+1]) + ...) + s[b]) / float(b - a + 1): the adds in ascending order, then one division (no sliding sum: its roundings differ).
 * A NaN inside the window gives a NaN s'[t].
 * Thresholds: mx / mn = the largest / smallest non-NaN s' of the row.  relative = 1: theta_l = mn + level_l * (mx - mn) (three operations in that
 * order); relative = 0: theta_l = level_l.
 * Runs: frame t is ABOVE at level l when s'[t] > theta_l (strict; a NaN is never above).  A run [lo, hi) of level l begins and ends on an above frame,
 * holds no more than `gap` consecutive frames that are not above, and is preceded and followed by more than `gap` such frames or by the row's ends.
 * A flat row, an all-NaN row and D = 0 give no run.
 * Filter: a run goes when hi - lo < min_len, or when max_len > 0 and hi - lo > max_len (max_len = 0: no limit).  Duplicates: a run of level l < T - 1
 * goes when level l + 1 has a run with the same (lo, hi).  (That covers every higher level: thresholds ascend, so the above sets are nested, closing
 * gaps is monotone, so the runs are nested, and a run shared with level l + 2 is level l + 1's as well.)
 * Order: levels T - 1 down to 0, ascending lo inside a level - the sharpest peaks first, and a full list drops the loosest threshold's spans.
 * Encoding: c = ((float(lo) + float(hi)) * 0.5f) / dur, w = ((float(hi) - float(lo)) - 0.5f) / dur.  rv_span_scores' window rule then computes
 * p1 / p2 near lo + 0.25 / hi - 0.25 and its floor / ceil give back exactly (lo, hi) - for every L up to the limit below.  A padding span (NaN) gets
 * the score NaN and the window (-1, -1) from rv_span_scores, ranks last in rv_span_rank and is void there.
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: a null sims / mask / levels / spans / n_spans; R < 1; rpm < 1; R not a multiple of
 * rpm; L < 1 or L > 1048576; T outside [1, 8]; relative not 0 / 1; a level that is not finite, not strictly ascending, or outside [0, 1) with
 * relative = 1; smooth even or outside [1, 65]; gap outside [0, 63]; min_len < 1; max_len < 0; 0 < max_len < min_len; N outside [1, 2048] (2048 is
 * rv_span_rank's limit, so the output feeds it as it is).
 * One 256-thread workgroup per row, rows on the grid's x dimension with 64-bit offsets (no limit of 65535 on R); 2.6 KB of LDS whatever L. */
int rv_span_propose(const float* sims, const float* mask, int32_t R, int32_t rpm, int32_t L, const float* levels, int32_t T, int32_t relative,
                    int32_t smooth, int32_t gap, int32_t min_len, int32_t max_len, int32_t N, float* spans, int32_t* n_spans, int32_t* n_found,
                    int32_t* windows, float* smoothed, void* stream);

/* ---- coarse window selection for the stage-2 recursion: which windows of stage2.cut_windows' geometry a query should see, chosen from its per-frame
 * cosine row (the stage the reference evaluates in eval/evaluate_pre_filtered_window.py and feeds from a stage-1 LLM log, e2e2.py:278-294; scoring
 * the windows by their top-k cosines is this project's own definition) ----
 * sims f32 [R,L] (a row = one video, or one (video, query): rv_frame_cosine[_multi]'s rows), mask f32 [R / rpm, L] (rpm = "rows per mask", as in
 * rv_span_propose; R a multiple of rpm), gt f32 [R,2] (start, end) in frames, or NULL ->
 *   select     i32 [R,keep]          the chosen windows' indices ASCENDING (the form of run_query's grounding_windows: a sorted list that also
 *                                    indexes cut_windows' frame_idx), then -1
 *   n_select   i32 [R]               min(keep, W_r)
 *   n_windows  i32 [R]               W_r
 *   win_scores f32 [R,Wcap]          (optional) the score of every window, NaN (0x7fc00000) in the padding
 *   bounds     i32 [R / rpm,Wcap,2]  (optional) (lo, hi) of every window, (-1, -1) in the padding; written by the first row of each mask row
 *   order      i32 [R,Wcap]          (optional) the selection sequence seq, -1 in the padding
 *   hit_rank   i32 [R]               (optional, needs gt) the smallest place p with window seq[p] covering the ground truth, or -1
 * Duration (rv_span_propose's rule): dur = the f32 sum of the row's mask row, D = min(L, max(0, int(floor(dur)))), D = 0 for a non-finite dur.  Only
 * frames [0, D) exist for the row; no frame of sims at or past D is read.  The result is defined for masks whose sum is exact in any order (0 / 1
 * masks); for other masks it is build-defined (the order of the sum is the kernel's).
 * Windows (stage2.cut_windows' rule in integers, 64-bit intermediate products): hop = win / stride (integer division), W_r = max(0, ceil(D / hop) - 1);
 * for i in [0, W_r): s = (i * win) / stride, e = min(s + win, D - 1), and if e - s < win then s = e - win; the window is frames
 * [lo, hi) = [max(s, 0), e + 1).  (s, e) are cut_windows' `times` for clip_length = win; every window is non-empty and inside [0, D).  The clamp
 * at 0 is this library's own (cut_windows lets a negative start wrap; the driver skips such videos).
 * Score of a window: the sum of its min(k, hi - lo) largest sims in rv_span_scores' mode-0 order - NaN first, then the larger value, then the
 * smaller index - accumulated from 0 in that order, each add rounded: a NaN frame gives a NaN window, and the score equals rv_span_scores' on a span
 * whose window is [lo, hi) bit for bit.
 * Rank order (rv_span_rank's): descending score, ties (-0 against +0 included) to the smaller index, NaN after every number, NaNs among themselves
 * by index.
 * Selection sequence seq, a permutation of the W_r windows.  Pass 1 walks the rank order: a window still alive is taken, and every window j with
 * |i - j| < min_sep dies; a dead window is skipped and kills nothing; min_sep = 1 kills nothing.  Pass 2 appends the windows not yet taken in rank
 * order (the "top up to batch" of the reference's pre-filter).  n_select = min(keep, W_r); select = the first n_select entries of seq sorted
 * ascending.  (The first entries of pass 1 do not depend on how far the walk goes, so select needs no more of seq than n_select entries.)
 * Ground truth: a window covers it when float(lo) < ge && float(hi) > gs (both strict); a gt that is not finite or has ge <= gs is void and gives
 * hit_rank = -1.  Rank@K of the reference's windows_selection is 0 <= hit_rank < K; with min_sep = 1 the place is the score rank.
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: a null sims / mask / select / n_select / n_windows; R < 1; rpm < 1; R not a
 * multiple of rpm; L < 1 or L > 1048576; stride < 1; win < stride; win > L; k outside [1, 64]; Wcap != max(1, ceil(L / hop) - 1) or Wcap > 2048;
 * keep outside [1, Wcap]; min_sep outside [1, Wcap]; hit_rank without gt.
 * One 1024-thread workgroup per row, rows on the grid's x dimension with 64-bit offsets (no limit of 65535 on R); 24 KB of LDS whatever L. */
int rv_window_select(const float* sims, const float* mask, int32_t R, int32_t rpm, int32_t L, int32_t win, int32_t stride, int32_t k, int32_t keep,
                     int32_t min_sep, int32_t Wcap, const float* gt, int32_t* select, int32_t* n_select, int32_t* n_windows, float* win_scores,
                     int32_t* bounds, int32_t* order, int32_t* hit_rank, void* stream);

/* ---- the recursion's window tensor from features that stay on the device (what the driver builds on the host per query: stage2.cut_windows'
 * np.linspace frame indices, a fancy-index of the movie's feature array, a cast and an upload - data/feature_store.py WindowStager.stage_windows;
 * e2e2.py:262-277, :303-306) ----
 * video [M,L,d] with M = R / rpm, f32 or this library's 16-bit operand type (video_dtype, as rv_frame_cosine takes it; the other 16-bit type is
 * refused), frame stride ldv >= d elements, video stride L * ldv; mask f32 [M,L] or NULL (NULL: D = L); select i32 [R,keep]: rv_window_select's
 * `select` as it lies, -1 padding included - or any other list of window indices, unsorted or with repeats ->
 *   out        [R,keep,F,d] contiguous, out_dtype = f32 or the library's 16-bit operand type
 *   frame_idx  i32 [R,keep,F]  (optional) the source frame of every output row, -1 for an invalid entry
 * Duration (rv_window_select's rule, the same code): dur = the f32 sum of the video's mask row, D = min(L, max(0, int(floor(dur)))), D = 0 for a
 * non-finite dur; defined for 0 / 1 masks.  No frame at or past D is read.
 * Windows (rv_window_select's integer rule, the same code): hop = win / stride, W_r = max(0, ceil(D / hop) - 1); for entry i in [0, W_r):
 * s = (i * win) / stride, e = min(s + win, D - 1), if e - s < win then s = e - win, s = max(s, 0); the window is frames [s, e + 1).  Index i means
 * what it means in `select` and in cut_windows' `times`.
 * Sampled frames: np.linspace(s, e, F, dtype=int32), operation by operation in float64, each operation rounded on its own (round to nearest even):
 * step = (e - s) / (F - 1); y_j = j * step, or (j * (e - s)) / (F - 1) when step == 0; y_j = y_j + s; y_{F-1} = e; idx_j = floor(y_j); F = 1 gives
 * s.  The multiply and the add are NOT fused.  (The integer shortcut s + j * (e - s) / (F - 1) is another function: it differs at
 * (s, e, F) = (0, 130, 31), j = 27: 117 against linspace's 116.)  s <= idx_j <= e for every j.
 * Output: out[r, n, j, :] = video[r / rpm, idx_j, :] converted to out_dtype.  The same type on both sides is a copy of the bits.  f32 -> 16 bits
 * is the library's store conversion: round to nearest even, a NaN stays a NaN; the fp16 build saturates at +-65504 (an infinity included) and counts
 * it in the numeric status (rv_numeric_status_bind), the bf16 build stores infinities and large values as they round.  For a finite input that rounds
 * inside the 16-bit range that is torch.Tensor.to(dtype) bit for bit.  16 bits -> f32 is exact (a signalling NaN comes back quiet).
 * Invalid entries: a select entry outside [0, W_r) - the -1 padding, an index past a short row's windows, any other int32 - gives an all-zero
 * out[r, n] and frame_idx[r, n, :] = -1; nothing is read for it.  No value of select makes the kernel read or write outside its buffers.
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: a null video / select / out; R < 1; rpm < 1; R not a multiple of rpm; L < 1 or
 * L > 1048576; d < 1; ldv < d; stride < 1; win < stride; win > L; keep < 1; F < 1 or F > 65536; a video_dtype / out_dtype that is not f32 or this
 * library's 16-bit type; R * keep > 16777215.
 * 256-thread workgroups of 16 output rows, (R * keep) x ceil(F / 16) of them with 64-bit offsets; 16-byte loads and stores when d is a multiple of
 * 8 (4 for f32 -> f32), ldv * sizeof(element) a multiple of 16 and both base addresses 16-byte aligned, one element per lane otherwise - the same
 * bits either way.  With a mask every workgroup sums its video's mask row again (L floats per 16 output rows); callers whose rows are full pass NULL. */
int rv_window_gather(const void* video, int32_t video_dtype, int64_t ldv, const float* mask, const int32_t* select, int32_t R, int32_t rpm, int32_t L,
                     int32_t d, int32_t win, int32_t stride, int32_t keep, int32_t F, void* out, int32_t out_dtype, int32_t* frame_idx, void* stream);

/* ---- the stage-1 driver on the device: its window tensor and the cosine score of every proposal (what eval/eval_nlq_negative.py does on the host
 * per query: stage1.cut_windows' linspace indices, a fancy-index of the movie, a cast and an upload; then one rv_topk_cosine launch and one host
 * synchronisation per proposal - negative.py:224-235, :299-337) ----
 * rv_window_gather_rule is rv_window_gather with the window rule as an argument and an optional select.  Everything not named here is
 * rv_window_gather's definition word for word (the kernel is the same template): video, ldv, the duration from the mask or D = L, the sampled frames
 * np.linspace(s, e, F, dtype=int32) in un-fused float64 with the last index set to e, the copy or the store conversion with its saturation count, an
 * all-zero out[r, n] and frame_idx = -1 for an invalid entry, 64-bit offsets, the 16-byte and the one-element form, the clamp in front of the loads.
 * rule = RV_WINDOWS_SHIFTED (0): rv_window_gather's windows (stage2.cut_windows), stride as there.
 * rule = RV_WINDOWS_CLIPPED (1): stage1.cut_windows' windows for clip_length = win - half-overlapping, the last ones clipped and NOT shifted back.
 *   stride must be 2 and is otherwise unused.  half = win / 2, W_r = max(0, ceil(D / half) - 1) (rv_window_gather's count at stride 2); for i in
 *   [0, W_r): s = (i * win) / 2 in 64-bit integers - for an odd win NOT i * half: win = 625 starts at 0, 312, 625, 937 - and e = min(s + win, D - 1);
 *   the window is frames [s, e + 1), up to win + 1 of them and fewer at the end of the row.  s == e is a window of one frame.  s > e is a VOID window:
 *   it exists for an odd win only (first at D = 15 for win = 5 and at D = 195625 for win = 625; never for an even win), the host's linspace leaves the
 *   array there, and here it is an invalid entry: zeros and -1, nothing read.
 * select i32 [R,keep] as rv_window_gather reads it, -1 padding included, or NULL: entry n of a row is then window n (keep = the number of windows
 *   gives them all with nothing uploaded; an n at or past W_r is an invalid entry like any other).
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: everything rv_window_gather refuses except a null select; a rule that is neither
 * 0 nor 1; rule 1 with stride != 2. */
#define RV_WINDOWS_SHIFTED 0
#define RV_WINDOWS_CLIPPED 1
int rv_window_gather_rule(const void* video, int32_t video_dtype, int64_t ldv, const float* mask, const int32_t* select, int32_t R, int32_t rpm,
                          int32_t L, int32_t d, int32_t win, int32_t stride, int32_t keep, int32_t F, void* out, int32_t out_dtype, int32_t* frame_idx,
                          int32_t rule, void* stream);
/* The cosine score of P ragged proposals in one launch: feat [W,T,d] contiguous, f32 or this library's 16-bit operand type (16-byte aligned when d
 * is a whole number of 16-byte chunks, as rv_topk_cosine's), q_cls f32 [d], props i32 [P,3] in DEVICE memory as (window, a, b) -> out f32 [P].
 * The slice is Python's feat[window][a : b + 1]: lo = min(a, T), hi = min(b + 1, T), frames [lo, hi).  A proposal is VOID when window lies outside
 * [0, W), when a < 0 or when hi <= lo (b < a, or a >= T): out[p] = NaN (0x7fc00000) and nothing of feat is read - no value of props makes the kernel
 * read or write outside its buffers.  Otherwise out[p] is rv_topk_cosine's score of the slice: the column norms over the slice's hi - lo frames
 * only, sims[t] = <f_t, q / norm>, the sum of the min(k, hi - lo) largest in torch.topk's order (a NaN first, then the larger value, then the smaller
 * index); k <= 0: the mean.  A NaN feature or an all-zero column inside a slice gives NaN for that proposal and no other.
 * One launch, one 1024-thread workgroup per proposal on the grid's x dimension.  The two kernel bodies are rv_topk_cosine's own device functions,
 * taking a base pointer and a frame count, so out[p] equals rv_topk_cosine(feat + (window * T + lo) * d, n = 1, T = hi - lo, d, k) BIT FOR BIT whenever
 * that call takes the kernel form this entry takes.  The form and the LDS size are chosen as rv_topk_cosine chooses them for the full window
 * length T: the 16-byte form when d is a multiple of vec (8 for 16-bit features, 4 for f32), d / vec <= 1024 and ((1024 / (d / vec) + 1) * d + T)
 * floats fit 64 KB, else the generic form with 5 * d + T floats.  A slice's own call chooses by hi - lo <= T, so the forms coincide for EVERY slice
 * exactly when T itself takes the 16-byte form or d rules that form out at any length (d not a multiple of vec, or d / vec > 1024); at d = 768
 * that is every T <= 7936 for both element types (16-bit: 11 * 768 + T <= 16384).  Past that, a long window runs the generic form while a short
 * slice's own call would run the 16-byte one: the same definition, sums in another order.
 * Refused with RV_ERR_ARG, outputs untouched, before any launch: a null feat / q_cls / props / out; P < 1; W < 1; T < 1; d < 1; a dtype that is not
 * f32 or this library's 16-bit type; 5 * d + T floats above 64 KB when the 16-byte form is not taken (rv_topk_cosine's bound at T). */
int rv_proposal_cosine(const void* feat, int feat_dtype, const float* q_cls, const int32_t* props, int32_t P, int32_t W, int32_t T, int32_t d,
                       int32_t k, float* out, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* REVISION_HIP_H */
