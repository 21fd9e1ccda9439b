// softmax(Q K^T * scale + mask) V with MFMA 16x16x32, head dims 96 (adapter, nn.MultiheadAttention), 128 (Llama)
// and 64 (CLIP towers).  One wave = 16 query rows of one (batch, head); keys are walked 32 at a time with an
// online softmax.  Both products use swapped operands so that every per-query quantity is lane-local:
//   S^T[key][q] = K . Q^T     row i of score tile t (t = 0, 1) is key (i >> 2) * 8 + t * 4 + (i & 3) of the 32-key block, so
//                             lane (q = lane & 15, g = lane >> 4), which owns rows 4g + r of both tiles, holds the 8
//                             CONSECUTIVE keys 8g .. 8g + 7
//   O^T[d][q]   = V^T . P^T   the same 8 scores ARE the lane's B fragment (the sum over keys is permutation
//                             invariant), and its V^T A fragment is ONE 16-byte load (8 consecutive keys of row d) - a
//                             vector-memory instruction costs the address unit the same 16 cycles whatever it moves
// so there is no LDS traffic and no cross-lane movement besides two shuffles for the row max.  V is
// kept transposed in memory ([dh][keys]: the KV cache is written that way, the adapter transposes once).
// K / V^T tiles come straight from L2 (a head's K/V is <= 64 KB at the path's sequence lengths).
//
// Two bodies walk the keys - attn_body (every wave fetches its own fragments from L2) and attn_body_lds (a workgroup stages them in LDS once) - and both
// hand every (query tile, key block) to ONE step, ATTN_BLOCK_STEP: a row's arithmetic is the same text whichever kernel computes it, which is what the
// bit-identity tests of the staged forms against the per-wave forms rest on.
#include "kernels.h"

namespace {

// What a lane addresses.  Lane (fr = lane & 15, g = lane >> 4) owns query / output row fr of a 16-row tile and keys 8g .. 8g + 7 of a 32-key block.
// Its query row of the tile that starts at row0 (a row past the problem repeats the last one: loaded, never stored):
template <int DH>
__device__ __forceinline__ const op16_t* attn_q_ptr(const AttnArgs& a, int h, int b, int row0, int fr, int g) {
    return (const op16_t*)a.q + (int64_t)b * a.q_bs + (int64_t)min(row0 + fr, a.Lq - 1) * a.q_rs + h * DH + g * 8;
}
// kbase / vbase: its addresses in key 0 / V^T row fr of the (key batch, head); krow: the key of score-tile row fr within a block (+ 4 for tile 1)
struct AttnKV {
    const op16_t *kbase, *vbase;
    int krow;
};
__device__ __forceinline__ AttnKV attn_kv_ptrs(const AttnArgs& a, int h, int kb, int fr, int g) {
    return AttnKV{(const op16_t*)a.k + (int64_t)kb * a.k_bs + (int64_t)h * a.k_hs + g * 8,
                  (const op16_t*)a.vt + (int64_t)kb * a.vt_bs + (int64_t)h * a.vt_hs + (int64_t)fr * a.vt_ds + g * a.vt_ks, (fr >> 2) * 8 + (fr & 3)};
}

// the NC 16-byte k-chunks of one operand row (a query row, a key row)
template <int NC>
__device__ __forceinline__ void attn_load_row(const op16_t* p, op16x8 (&f)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) f[c] = *(const op16x8*)(p + c * 32);
}

// THE step of the online softmax: the 32 keys from k0 (fragments kf, vf) against one 16-row query tile (qf; ql = the low halves of the query row under split
// queries, scores = K.(Qhi + Qlo)); g = lane >> 4 (the lane's keys are k0 + 8g ..), qbase = the position of the tile's row 0, qpos = of the lane's row.
// PAD: a key-padding mask is present (the text cross-attention of the adapter); without it the per-key byte loads and their branches are compiled out.
//   - an INTERIOR block (wave-uniform: every key exists and is visible to all 16 rows) takes no per-element masking;
//   - O is rescaled only when the running maximum moved for some row of this wave (the ballot).
// The order of the operations below is what "bit-identical" means in this file.  A macro, not a function: every function form compiled cost the kernels with a
// run-time `causal` their fourth wave per SIMD (profiles/attention_refactor_isa.txt).  Its locals end in _ so that no argument expression can name one.
#define ATTN_BLOCK_STEP(DH, PAD, QS, a, g, kf, vf, qf, ql, k0, Lk, causal, qbase, qpos, pad, m_run, l_run, o)                 \
    do {                                                                                                                      \
        f32x4 s_[2];                                                                                                          \
        _Pragma("unroll") for (int t_ = 0; t_ < 2; ++t_) {                                                                    \
            s_[t_] = f32x4{0.f, 0.f, 0.f, 0.f};                                                                               \
            _Pragma("unroll") for (int c_ = 0; c_ < (DH) / 32; ++c_) s_[t_] = rv_mfma16((kf)[t_][c_], (qf)[c_], s_[t_]);      \
            if constexpr (QS) {                                                                                               \
                _Pragma("unroll") for (int c_ = 0; c_ < (DH) / 32; ++c_) s_[t_] = rv_mfma16((kf)[t_][c_], (ql)[c_], s_[t_]);  \
            }                                                                                                                 \
        }                                                                                                                     \
        float mx_ = -INFINITY;                                                                                                \
        const bool interior_ = !(PAD) && (k0) + 32 <= (Lk) && (!(causal) || (k0) + 31 <= (qbase));                            \
        if (interior_) {                                                                                                      \
            _Pragma("unroll") for (int t_ = 0; t_ < 2; ++t_)                                                                  \
                _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {                                                            \
                    s_[t_][r_] *= (a).scale;                                                                                  \
                    mx_ = fmaxf(mx_, s_[t_][r_]);                                                                             \
                }                                                                                                             \
        } else {                                                                                                              \
            _Pragma("unroll") for (int t_ = 0; t_ < 2; ++t_)                                                                  \
                _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {                                                            \
                    const int key_ = (k0) + (g) * 8 + t_ * 4 + r_;                                                            \
                    bool dead_ = key_ >= (Lk) || ((causal) && key_ > (qpos));                                                 \
                    if ((PAD) && key_ < (Lk)) dead_ = dead_ || (pad)[key_];                                                   \
                    const float v_ = dead_ ? -INFINITY : s_[t_][r_] * (a).scale;                                              \
                    s_[t_][r_] = v_;                                                                                          \
                    mx_ = fmaxf(mx_, v_);                                                                                     \
                }                                                                                                             \
        }                                                                                                                     \
        mx_ = fmaxf(mx_, __shfl_xor(mx_, 16, 64));                                                                            \
        mx_ = fmaxf(mx_, __shfl_xor(mx_, 32, 64));                                                                            \
        const float m_new_ = fmaxf(m_run, mx_);                                                                               \
        const float m_use_ = m_new_ == -INFINITY ? 0.f : m_new_;                                                              \
        const float alpha_ = __expf((m_run) - m_use_); /* m_run = -inf -> 0 */                                                \
        float psum_ = 0.f;                                                                                                    \
        float p_[8];                                                                                                          \
        _Pragma("unroll") for (int t_ = 0; t_ < 2; ++t_)                                                                      \
            _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {                                                                \
                const float e_ = __expf(s_[t_][r_] - m_use_);                                                                 \
                p_[t_ * 4 + r_] = e_;                                                                                         \
                psum_ += e_;                                                                                                  \
            }                                                                                                                 \
        l_run = (l_run) * alpha_ + psum_;                                                                                     \
        m_run = m_new_;                                                                                                       \
        union { op16x8 v; uint32_t u[4]; } pf_;                                                                               \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) pf_.u[i_] = pack_op16x2_bounded(p_[2 * i_], p_[2 * i_ + 1]);         \
        if (__builtin_amdgcn_ballot_w64(alpha_ != 1.0f) != 0) {                                                               \
            _Pragma("unroll") for (int dt_ = 0; dt_ < (DH) / 16; ++dt_) (o)[dt_] *= alpha_;                                   \
        }                                                                                                                     \
        _Pragma("unroll") for (int dt_ = 0; dt_ < (DH) / 16; ++dt_) (o)[dt_] = rv_mfma16((vf)[dt_], pf_.v, (o)[dt_]);         \
    } while (0)

// a row's l over the four lanes that hold its keys
__device__ __forceinline__ float attn_row_sum(float l) {
    l += __shfl_xor(l, 16, 64);
    return l + __shfl_xor(l, 32, 64);
}

// The end of a tile on every path without a key split: O / l to the lane's output row, and with a.out_lo its low half (LO = false: a staged form, never launched
// with split outputs - the half's code stays out of its kernels).  Whole waves call it (the row sum shuffles); the lanes of rows past the problem store nothing.
template <int DH, bool PAD, bool LO = true>
__device__ __forceinline__ void attn_store_tile(const AttnArgs& a, int h, int b, int row0, int fr, int g, float l_run, const f32x4 (&o)[DH / 16]) {
    constexpr int ND = DH / 16;
    l_run = attn_row_sum(l_run);
    if (row0 + fr >= a.Lq) return;
    const float inv = PAD && l_run == 0.f ? 0.f : 1.0f / l_run;      // (every key padded: a zero row)
    op16_t* op = (op16_t*)a.out + (int64_t)b * a.o_bs + (int64_t)(row0 + fr) * a.o_rs + h * DH + g * 4;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
        *(u32x2*)(op + dt * 16) = pack_op16x4(f32x4{o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv});
    if (LO && a.out_lo) {
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
            *(u32x2*)(op + a.out_lo + dt * 16) = u32x2{pack_op16x2_lo(o[dt][0] * inv, o[dt][1] * inv), pack_op16x2_lo(o[dt][2] * inv, o[dt][3] * inv)};
    }
}

// PER-WAVE form: every wave fetches its key blocks' fragments from L2 itself.
// SPLIT (Lq <= 16, i.e. KV-cached decode): the block's 4 waves share the same 16 queries and take key blocks
// w, w+4, ...; their (m, l, O) partials are merged through LDS.  A decode step is pure latency (one wave would
// walk all keys serially), so this cuts it ~4x.
template <int DH, bool SPLIT, bool PAD, bool QS = false>
__device__ __forceinline__ void attn_body(const AttnArgs& a, int bx, int h, int b, [[maybe_unused]] float* merge = nullptr) {
    constexpr int NC = DH / 32, ND = DH / 16;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int q0 = SPLIT ? bx * 16 : bx * 64 + wave * 16;
    if (q0 >= a.Lq) return;
    const int kb_ = b / a.kv_div;
    // per-row key count (merged decode steps): everything below uses Lk / q_pos0 of THIS batch row
    const int Lk = a.row_pos ? a.row_pos[b] + 1 : a.Lk;
    if (Lk <= 0 || (a.row_pos && Lk > a.Lk)) return;   // inactive row; a row past the pool's capacity (a.Lk = Smax) is treated like one
    const int q_pos0 = a.row_pos ? Lk - a.Lq : a.q_pos0;

    const op16_t* qp = attn_q_ptr<DH>(a, h, b, q0, fr, g);
    op16x8 qf[NC];
    attn_load_row(qp, qf);
    op16x8 ql[QS ? NC : 1];      // parity precision: the low halves of the query row
    if constexpr (QS) attn_load_row(qp + a.q_lo, ql);
    const AttnKV kv = attn_kv_ptrs(a, h, kb_, fr, g);

    // key blocks inside the prefix this row shares with a sibling row are read from the sibling's (bit-identical) cache rows: L2 hits
    int share_len = 0;
    int64_t share_k = 0, share_v = 0;       // element offsets from this row's bases to the sibling's
    if (SPLIT && a.row_share) {
        const int sv = a.row_share[b];
        const int srow = sv & 0xffff;
        share_len = sv >> 16;
        // a word that names a row outside the batch or a prefix longer than the cache is IGNORED (the row reads its own cache: always correct),
        // never followed out of bounds; rv_llm_decode_rows_shared documents the contract
        if (srow >= a.B || share_len < 0 || share_len > Lk) share_len = 0;
        share_k = (int64_t)(srow - kb_) * a.k_bs;
        share_v = (int64_t)(srow - kb_) * a.vt_bs;
    }
    const uint8_t* pad = PAD ? a.key_pad + (int64_t)kb_ * a.Lk : nullptr;

    f32x4 o[ND];
#pragma unroll
    for (int i = 0; i < ND; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const int qpos = q_pos0 + q0 + fr;
    const int kend = a.causal ? min(Lk, q_pos0 + q0 + 16) : Lk;

    for (int k0 = SPLIT ? wave * 32 : 0; k0 < kend; k0 += SPLIT ? 128 : 32) {
        // issue every load of this key block up front (K rows and V^T rows are independent of the softmax), so the
        // block costs one memory round trip instead of two
        op16x8 kf[2][NC];
        const bool shared_blk = SPLIT && k0 + 32 <= share_len;      // (wave-uniform) the whole block lies inside the shared prefix
        const int64_t sk = shared_blk ? share_k : 0, svo = shared_blk ? share_v : 0;
#pragma unroll
        for (int t = 0; t < 2; ++t) attn_load_row(kv.kbase + sk + (int64_t)min(k0 + kv.krow + t * 4, Lk - 1) * a.k_rs, kf[t]);
        op16x8 vf[ND];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) vf[dt] = *(const op16x8*)(kv.vbase + svo + (int64_t)dt * 16 * a.vt_ds + (int64_t)(k0 >> 3) * a.vt_ks);
        ATTN_BLOCK_STEP(DH, PAD, QS, a, g, kf, vf, qf, ql, k0, Lk, a.causal, q_pos0 + q0, qpos, pad, m_run, l_run, o);
    }
    if constexpr (SPLIT) {
        l_run = attn_row_sum(l_run);
        // (the merge area belongs to the KERNEL: as function-local __shared__ arrays every instantiation of this body a kernel dispatches between - with and
        // without a padding mask - got its own copy, 68.6 KB per workgroup for the decode attention instead of 34.3: two workgroups per CU instead of three)
        float (*sm_o)[16][DH + 4] = (float (*)[16][DH + 4])merge;
        float (*sm_m)[16] = (float (*)[16])(merge + 4 * 16 * (DH + 4));
        float (*sm_l)[16] = sm_m + 4;
        if (g == 0) {
            sm_m[wave][fr] = m_run;
            sm_l[wave][fr] = l_run;
        }
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) *(f32x4*)&sm_o[wave][fr][dt * 16 + g * 4] = o[dt];
        __syncthreads();
        // 256 threads: thread t -> query t / 16, d-chunk (t % 16) * (DH / 16)
        const int q = threadIdx.x >> 4, dc = (threadIdx.x & 15) * (DH / 16);
        if (q0 + q >= a.Lq) return;
        float mm = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) mm = fmaxf(mm, sm_m[w][q]);
        float sc[4], lt = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            sc[w] = sm_m[w][q] == -INFINITY ? 0.f : __expf(sm_m[w][q] - mm);
            lt += sm_l[w][q] * sc[w];
        }
        const float inv = PAD && lt == 0.f ? 0.f : 1.0f / lt;      // (every key padded: no key - a zero row, as t2v_softmax_kernel yields)
        op16_t* op = (op16_t*)a.out + (int64_t)b * a.o_bs + (int64_t)(q0 + q) * a.o_rs + h * DH + dc;
#pragma unroll
        for (int j = 0; j < DH / 16; j += 2) {
            float v0 = 0.f, v1 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                v0 += sm_o[w][q][dc + j] * sc[w];
                v1 += sm_o[w][q][dc + j + 1] * sc[w];
            }
            if (a.out_packed) *(uint32_t*)((op16_t*)a.out + rv_xp_index(b, h * DH + dc + j, a.out_packed)) = pack_op16x2(v0 * inv, v1 * inv);   // (Lq = 1)
            else *(uint32_t*)(op + j) = pack_op16x2(v0 * inv, v1 * inv);
            if (a.out_lo) *(uint32_t*)(op + a.out_lo + j) = pack_op16x2_lo(v0 * inv, v1 * inv);
        }
    } else {
        attn_store_tile<DH, PAD>(a, h, b, q0, fr, g, l_run, o);
    }
}

// STAGED form (round 6).  attn_body fetches every key block's K and V^T fragments from L2 once PER WAVE: twelve 16-byte-per-lane loads per 32 keys and wave at
// dh = 96, and the CU's vector-memory path accepts one such instruction per 16 cycles for all four SIMDs together - 768 cycles of address work per block step
// against 192 of MFMA (32 windows x 1024 frames: 308 us per layer, 0.13 of the MFMA peak).  Here a key block is staged in LDS ONCE per workgroup by LDS-DMA -
// each wave moves NF / 4 of its NF fragments, already in the lane order the MFMAs consume, so every ds_read_b128 is one conflict-free 1 KiB run -
// double-buffered: block i + 1 travels while block i is computed, one barrier per block.  No key split, no padding mask, no per-row positions.
//   NT = 2  the LONG-KEY form: the adapter's self-attention over 257 / 1025 keys, the CLIP towers.  A workgroup is 4 waves x 32 query rows: the two 16-row tiles
//           of a wave share a block's fragments in registers.  Not causal, and that is a compile-time fact: its kernels hold no masking code but the key count's.
//   NT = 1  the LLM PREFILL (causal or not, dh = 128, 171 keys at the headline): 64 query rows per workgroup - the tiling of attn_body, so a workgroup's four
//           waves (which attn_kernel_pair lets fetch the same key blocks four times) share one staged copy.  A wave computes the blocks below its own causal
//           limit and keeps staging / the barriers for the rest of the workgroup's range.
// Per tile the step is attn_body's: rows are BIT-identical to the per-wave kernels'.
typedef const __attribute__((address_space(1))) void* attn_gptr_t;
typedef __attribute__((address_space(3))) void* attn_lptr_t;
template <int DH>
constexpr int ATTN_STAGE = (2 * (DH / 32) + DH / 16) * 1024;      // bytes of one staged key block: a KiB per fragment; a staged kernel holds two
template <int DH, int NT>
__device__ __forceinline__ void attn_body_lds(const AttnArgs& a, int bx, int h, int b, char* smem) {
    constexpr int NC = DH / 32, ND = DH / 16, NF = 2 * NC + ND, STAGE = ATTN_STAGE<DH>;
    static_assert(NF % 4 == 0, "the four waves stage NF / 4 fragments each");
    static_assert(NT == 1 || NT == 2, "one or two query tiles per wave");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int q0 = (bx * 4 + wave) * 16 * NT;
    const bool active = q0 < a.Lq, two = NT == 2 && q0 + 16 < a.Lq;      // (wave-uniform) an idle wave still stages its share and keeps the barriers
    const int causal = NT == 1 ? a.causal : 0;
    const int Lk = a.Lk, q_pos0 = a.q_pos0;
    op16x8 qf[NT][NC];
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) attn_load_row(attn_q_ptr<DH>(a, h, b, q0 + qt * 16, fr, g), qf[qt]);
    const AttnKV kv = attn_kv_ptrs(a, h, b / a.kv_div, fr, g);
    // fragment f of a block: f < 2 NC: score tile t = f / NC, k-chunk c = f % NC of K; else V^T fragment dt = f - 2 NC.  The source address of a lane is the
    // address attn_body loads from; the destination is lane-linear behind the fragment's base.
    auto stage = [&](int k0, char* buf) {
#pragma unroll
        for (int i = 0; i < NF / 4; ++i) {
            const int f = wave + 4 * i;
            const op16_t* src;
            if (f < 2 * NC) {
                const int t = f / NC, c = f - t * NC;
                src = kv.kbase + (int64_t)min(k0 + kv.krow + t * 4, Lk - 1) * a.k_rs + c * 32;
            } else {
                src = kv.vbase + (int64_t)(f - 2 * NC) * 16 * a.vt_ds + (int64_t)(k0 >> 3) * a.vt_ks;
            }
            __builtin_amdgcn_global_load_lds((attn_gptr_t)src, (attn_lptr_t)(buf + f * 1024), 16, 0, 0);
        }
    };
    f32x4 o[NT][ND];
#pragma unroll
    for (int qt = 0; qt < NT; ++qt)
#pragma unroll
        for (int i = 0; i < ND; ++i) o[qt][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run[NT], l_run[NT];
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) m_run[qt] = -INFINITY, l_run[qt] = 0.f;
    // the causal limits are quantities of the NT = 1 form (one tile per wave, 64 rows per workgroup); with NT = 2 `causal` is the literal 0 and both fold to Lk
    const int kend = causal ? min(Lk, q_pos0 + q0 + 16) : Lk;                                   // this wave's keys
    const int kend_wg = causal ? min(Lk, q_pos0 + min(bx * 64 + 64, a.Lq)) : Lk;                 // the workgroup's (its last live row's)
    const int nblk = (kend_wg + 31) >> 5;
    const op16x8* const no_ql = nullptr;      // (no split queries and no padding mask in the staged forms: those arms of the step are compiled out)
    const uint8_t* const no_pad = nullptr;
    stage(0, smem);
    for (int i = 0; i < nblk; ++i) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's pieces of block i have landed ...
        __builtin_amdgcn_s_barrier();                         // ... and everyone's; and every wave is done reading the other buffer (block i - 1)
        asm volatile("" ::: "memory");
        if (i + 1 < nblk) stage((i + 1) * 32, smem + ((i + 1) & 1) * STAGE);
        const int k0 = i * 32;
        if (!active || (NT == 1 && k0 >= kend)) continue;
        const char* buf = smem + (i & 1) * STAGE + lane * 16;
        op16x8 kf[2][NC];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int c = 0; c < NC; ++c) kf[t][c] = *(const op16x8*)(buf + (t * NC + c) * 1024);
        op16x8 vf[ND];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) vf[dt] = *(const op16x8*)(buf + (2 * NC + dt) * 1024);
#pragma unroll
        for (int qt = 0; qt < NT; ++qt) {
            if (qt == 1 && !two) continue;      // (wave-uniform)
            const int qbase = q_pos0 + q0 + qt * 16, qpos = qbase + fr;
            ATTN_BLOCK_STEP(DH, false, false, a, g, kf, vf, qf[qt], no_ql, k0, Lk, causal, qbase, qpos, no_pad, m_run[qt], l_run[qt], o[qt]);
        }
    }
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) attn_store_tile<DH, false, false>(a, h, b, q0 + qt * 16, fr, g, l_run[qt], o[qt]);
}

// 1-D grid, XCD-aware: workgroup id lands on XCD id % 8 (private L2), so the query tiles of one (batch, head) - which read
// the same K / V^T - get ids that differ by multiples of 8, and an XCD only ever touches 1/8 of the (batch, head) pairs.
__device__ __forceinline__ bool attn_map(int tiles, int H, int pairs, int& bx, int& h, int& b) {
    const int id = blockIdx.x, j = id >> 3;
    const int pr = (j / tiles) * 8 + (id & 7);
    if (pr >= pairs) return false;
    bx = j % tiles;
    h = pr % H;
    b = pr / H;
    return true;
}
__host__ inline unsigned attn_grid(int tiles, int pairs) { return (unsigned)(tiles * ((pairs + 7) / 8) * 8); }

template <int DH, bool SPLIT, bool QS = false>
__global__ __launch_bounds__(256, DH <= 128 ? 3 : 1) void attn_kernel(AttnArgs a, int tiles) {
    int bx, h, b;
    if (!attn_map(tiles, a.H, a.H * a.B, bx, h, b)) return;
    __shared__ __attribute__((aligned(16))) float merge[SPLIT ? 4 * 16 * (DH + 4) + 2 * 4 * 16 : 4];   // partial (m, l, O) of the four key-split waves
    if constexpr (QS) attn_body<DH, SPLIT, false, true>(a, bx, h, b, merge);      // (the LLM has no key padding: checked by the launcher)
    else if (a.key_pad) attn_body<DH, SPLIT, true>(a, bx, h, b, merge);
    else attn_body<DH, SPLIT, false>(a, bx, h, b, merge);
}

// one problem with the key blocks staged in LDS: NT = 2, 128 query rows per workgroup (long keys, not causal); NT = 1, 64 rows (causal or not; the classic
// single-generate prefill)
template <int DH, int NT>
__global__ __launch_bounds__(256, 2) void attn_kernel_lds(AttnArgs a, int tiles) {
    __shared__ __attribute__((aligned(16))) char smem[2 * ATTN_STAGE<DH>];
    int bx, h, b;
    if (!attn_map(tiles, a.H, a.H * a.B, bx, h, b)) return;      // (workgroup-uniform)
    attn_body_lds<DH, NT>(a, bx, h, b, smem);
}

// Two attention problems of the same head geometry in one launch (the shared-prefix prefill: the prefix rows attend among
// themselves, the per-call rows attend to prefix + own keys), G times over (AttnGroups): problem z of the launch -> its group's copy of problem a
// (z < a.B within the group) or b, with the group's offsets on the four pointers; z becomes the index inside the group.
__device__ __forceinline__ AttnArgs& attn_pair_problem(AttnArgs& a, AttnArgs& b, const AttnGroups& gr, int& z) {
    const int per = a.B + b.B, g = z / per;
    z -= g * per;
    AttnArgs& p = z < a.B ? a : b;
    if (gr.G > 1) {      // (uniform per workgroup)
        p.q = (const op16_t*)p.q + gr.q_off[g];
        p.out = (op16_t*)p.out + gr.o_off[g];
        p.k = (const op16_t*)p.k + gr.kv_off[g];
        p.vt = (const op16_t*)p.vt + gr.kv_off[g];
    }
    return p;
}
template <int DH, bool QS = false>
__global__ __launch_bounds__(256, 3) void attn_kernel_pair(AttnArgs a, AttnArgs b, int tiles, AttnGroups gr) {
    int bx, h, z;
    if (!attn_map(tiles, a.H, a.H * (a.B + b.B) * gr.G, bx, h, z)) return;
    AttnArgs& p = attn_pair_problem(a, b, gr, z);
    if (z < a.B) attn_body<DH, false, false, QS>(p, bx, h, z);   // (the LLM prefill has no key padding: checked by the launcher)
    else attn_body<DH, false, false, QS>(p, bx, h, z - a.B);
}

// attn_kernel_pair with the key blocks staged in LDS (one tile per wave); no split queries
template <int DH>
__global__ __launch_bounds__(256, 2) void attn_kernel_pair_lds(AttnArgs a, AttnArgs b, int tiles, AttnGroups gr) {
    __shared__ __attribute__((aligned(16))) char smem[2 * ATTN_STAGE<DH>];
    int bx, h, z;
    if (!attn_map(tiles, a.H, a.H * (a.B + b.B) * gr.G, bx, h, z)) return;
    const AttnArgs& p = attn_pair_problem(a, b, gr, z);
    if (bx * 64 >= p.Lq) return;       // (workgroup-uniform: the two problems may differ in length, tiles counts the longer one)
    attn_body_lds<DH, 1>(p, bx, h, z < a.B ? z : z - a.B, smem);
}

// Mixed-geometry prefill passes: every group brings its own pair of problems (AttnMixed).  Workgroup -> (problem, head, query tile) as attn_map does it; the problem
// -> (group, prefix problem or sequence) through the prefix sum of the groups' problem counts.  `tiles` counts the LONGEST problem of the pass: a workgroup whose
// tile lies beyond its own problem leaves (uniformly, before any barrier).  The bodies are those of the pair kernels, fed the AttnArgs the pair launch would build
// for this group alone: a row's arithmetic does not depend on what shares the pass.
__device__ __forceinline__ void attn_mixed_problem(AttnArgs& p, const AttnMixed& mx, int z, int& b) {
    int g = 0;
    for (int i = 1; i < mx.G; ++i) g += z >= mx.first[i] ? 1 : 0;      // (z is workgroup-uniform)
    const QkvGroup e = mx.gt[g];
    const int zl = z - mx.first[g], hasp = e.P0 > 0 ? 1 : 0;
    const bool prefix = hasp && zl == 0;
    const int64_t row0 = prefix ? e.base : e.base + e.P0;
    p.q = (const op16_t*)p.q + row0 * p.q_rs;
    p.out = (op16_t*)p.out + row0 * p.o_rs;
    p.k = (const op16_t*)p.k + (int64_t)e.row * p.k_bs;
    p.vt = (const op16_t*)p.vt + (int64_t)e.row * p.vt_bs;
    if (prefix) { p.B = 1; p.Lq = p.Lk = e.P0; p.q_pos0 = 0; p.q_bs = (int64_t)e.P0 * p.q_rs; p.o_bs = (int64_t)e.P0 * p.o_rs; b = 0; }
    else { p.B = e.B; p.Lq = e.S; p.Lk = e.P0 + e.S; p.q_pos0 = e.P0; p.q_bs = (int64_t)e.S * p.q_rs; p.o_bs = (int64_t)e.S * p.o_rs; b = zl - hasp; }
}
template <int DH>
__global__ __launch_bounds__(256, 2) void attn_kernel_mixed_lds(AttnArgs a, AttnMixed mx, int tiles) {
    __shared__ __attribute__((aligned(16))) char smem[2 * ATTN_STAGE<DH>];
    int bx, h, z, b;
    if (!attn_map(tiles, a.H, a.H * mx.problems, bx, h, z)) return;
    attn_mixed_problem(a, mx, z, b);
    if (bx * 64 >= a.Lq) return;       // (workgroup-uniform)
    attn_body_lds<DH, 1>(a, bx, h, b, smem);
}
template <int DH>
__global__ __launch_bounds__(256, 3) void attn_kernel_mixed(AttnArgs a, AttnMixed mx, int tiles) {
    int bx, h, z, b;
    if (!attn_map(tiles, a.H, a.H * mx.problems, bx, h, z)) return;
    attn_mixed_problem(a, mx, z, b);
    if (bx * 64 >= a.Lq) return;
    attn_body<DH, false, false, false>(a, bx, h, b);
}
__global__ void mixed_tables_kernel(AttnMixed mx, QkvGroup* gt, int* last_rows) {
    if (threadIdx.x >= (unsigned)mx.G) return;
    const QkvGroup e = mx.gt[threadIdx.x];
    gt[threadIdx.x] = e;
    if (!last_rows) return;
    int o = 0;
    for (int i = 0; i < (int)threadIdx.x; ++i) o += mx.gt[i].B;
    for (int b = 0; b < e.B; ++b) last_rows[o + b] = e.base + e.P0 + (b + 1) * e.S - 1;
}

}  // namespace

// The launchers' argument checks, each written once.  `who` heads the message: "attention", "attention mixed".
static int attn_check_tensors(const AttnArgs& a, const char* who) {
    RV_CHECK_ARG(a.q && a.k && a.vt && a.out, "%s: null tensor", who);
    return RV_OK;
}
static int attn_check_strides(const AttnArgs& a) {
    RV_CHECK_ARG(a.q_rs % 8 == 0 && a.k_rs % 8 == 0 && a.k_hs % 8 == 0 && a.vt_ds % 8 == 0 && a.vt_hs % 8 == 0 && a.vt_bs % 8 == 0 && a.o_rs % 4 == 0,
                 "attention: stride alignment");
    return RV_OK;
}
static int attn_check_vt_rows(const AttnArgs& a, int Lk) {
    RV_CHECK_ARG(a.vt_ks != 8 || a.vt_ds >= ((Lk + 31) / 32) * 32, "attention: V^T rows must be padded to a multiple of 32 keys");
    return RV_OK;
}
static int attn_check(const AttnArgs& a) {
    if (int rc = attn_check_tensors(a, "attention")) return rc;
    RV_CHECK_ARG(a.B > 0 && a.H > 0 && a.Lq > 0 && a.Lk > 0 && a.kv_div > 0, "attention: empty problem");
    if (int rc = attn_check_strides(a)) return rc;
    return attn_check_vt_rows(a, a.Lk);
}

// The pair kernel's three forms: split queries; key blocks staged in LDS (the attn_lds option, no per-row positions, no split output); every wave from L2.
// a.B = 0 (k_attention_groups): every workgroup takes problem b.
static int attn_launch_pair(const AttnArgs& a, const AttnArgs& b, const AttnGroups& gr, const char* what, hipStream_t st) {
    const int tiles = (int)cdiv(a.Lq > b.Lq ? a.Lq : b.Lq, 64);
    const dim3 grid(attn_grid(tiles, a.H * (a.B + b.B) * gr.G));
    const bool lds = !a.q_lo && rv_cur_opts().attn_lds && !a.row_pos && !b.row_pos && !a.out_lo && !b.out_lo;
    if (a.q_lo) hipLaunchKernelGGL((attn_kernel_pair<128, true>), grid, dim3(256), 0, st, a, b, tiles, gr);
    else if (lds) hipLaunchKernelGGL((attn_kernel_pair_lds<128>), grid, dim3(256), 0, st, a, b, tiles, gr);
    else hipLaunchKernelGGL((attn_kernel_pair<128>), grid, dim3(256), 0, st, a, b, tiles, gr);
    RV_CHECK_LAUNCH(what);
    return RV_OK;
}

int k_attention_pair(const AttnArgs& a, const AttnArgs& b, hipStream_t st, const AttnGroups* groups) {
    if (int rc = attn_check(a)) return rc;
    if (int rc = attn_check(b)) return rc;
    RV_CHECK_ARG(a.dh == 128 && b.dh == 128 && a.H == b.H && a.Lq > 16 && b.Lq > 16, "attention pair: 128-wide heads, same head count, prefill lengths only");
    RV_CHECK_ARG(!a.key_pad && !b.key_pad, "attention pair: key padding is not supported");
    const AttnGroups gr = groups ? *groups : AttnGroups{};
    RV_CHECK_ARG(gr.G >= 1 && gr.G <= RV_MAX_PREFILL_GROUPS, "attention pair: 1 .. %d groups", RV_MAX_PREFILL_GROUPS);
    RV_CHECK_ARG((a.q_lo != 0) == (b.q_lo != 0), "attention pair: both problems or neither carry split queries");
    return attn_launch_pair(a, b, gr, "attention pair", st);
}

// G copies of one prefill problem (batched prefills WITHOUT a shared prefix: one-row generates, the stage-1 windows) in one launch: the pair
// kernel with an empty first problem.  Per group these were G launches of 7 - 18 us each per layer (8 x 72-row windows: 60 of a layer's 440 us).
int k_attention_groups(const AttnArgs& b, hipStream_t st, const AttnGroups& gr) {
    if (int rc = attn_check(b)) return rc;
    RV_CHECK_ARG(b.dh == 128 && b.Lq > 16 && !b.key_pad && !b.row_pos, "attention groups: 128-wide heads, prefill lengths, no key padding, no per-row positions");
    RV_CHECK_ARG(gr.G >= 1 && gr.G <= RV_MAX_PREFILL_GROUPS, "attention groups: 1 .. %d groups", RV_MAX_PREFILL_GROUPS);
    AttnArgs a = b;
    a.B = 0;      // every workgroup takes problem b
    return attn_launch_pair(a, b, gr, "attention groups", st);
}

int k_attention_mixed(const AttnArgs& a, const AttnMixed& mx, hipStream_t st) {
    if (int rc = attn_check_tensors(a, "attention mixed")) return rc;
    RV_CHECK_ARG(a.dh == 128 && a.H > 0 && !a.key_pad && !a.row_pos && !a.q_lo && !a.out_lo && a.causal && a.kv_div == 1,
                 "attention mixed: causal 128-wide heads, no key padding, no per-row positions, no split operands");
    if (int rc = attn_check_strides(a)) return rc;
    RV_CHECK_ARG(mx.G >= 1 && mx.G <= RV_MAX_PREFILL_GROUPS, "attention mixed: 1 .. %d groups", RV_MAX_PREFILL_GROUPS);
    int longest = 0, problems = 0;
    for (int g = 0; g < mx.G; ++g) {
        const QkvGroup& e = mx.gt[g];
        RV_CHECK_ARG(e.B > 0 && e.S > 16 && (e.P0 == 0 || e.P0 > 16) && e.row >= 0 && e.base >= 0, "attention mixed: group %d: prefill lengths only (S > 16, P0 == 0 or > 16)", g);
        if (int rc = attn_check_vt_rows(a, e.P0 + e.S)) return rc;
        RV_CHECK_ARG(mx.first[g] == problems, "attention mixed: group %d: first problem %d, expected %d", g, mx.first[g], problems);
        problems += (e.P0 > 0 ? 1 : 0) + e.B;
        longest = e.S > longest ? e.S : longest;
        longest = e.P0 > longest ? e.P0 : longest;
    }
    RV_CHECK_ARG(mx.problems == problems, "attention mixed: %d problems, expected %d", mx.problems, problems);
    const int tiles = (int)cdiv(longest, 64);
    const dim3 grid(attn_grid(tiles, a.H * problems));
    if (rv_cur_opts().attn_lds) hipLaunchKernelGGL((attn_kernel_mixed_lds<128>), grid, dim3(256), 0, st, a, mx, tiles);
    else hipLaunchKernelGGL((attn_kernel_mixed<128>), grid, dim3(256), 0, st, a, mx, tiles);
    RV_CHECK_LAUNCH("attention mixed");
    return RV_OK;
}

int k_mixed_tables(const AttnMixed& mx, QkvGroup* gt, int* last_rows, hipStream_t st) {
    RV_CHECK_ARG(gt && mx.G >= 1 && mx.G <= RV_MAX_PREFILL_GROUPS, "mixed tables: bad argument");
    hipLaunchKernelGGL(mixed_tables_kernel, dim3(1), dim3(64), 0, st, mx, gt, last_rows);
    RV_CHECK_LAUNCH("mixed tables");
    return RV_OK;
}

// the per-wave kernel of one head dim, key-split or not
template <int DH, bool QS = false>
static void attn_launch(const AttnArgs& a, bool split, dim3 grid, int tiles, hipStream_t st) {
    if (split) hipLaunchKernelGGL((attn_kernel<DH, true, QS>), grid, dim3(256), 0, st, a, tiles);
    else hipLaunchKernelGGL((attn_kernel<DH, false, QS>), grid, dim3(256), 0, st, a, tiles);
}

int k_attention(const AttnArgs& a, hipStream_t st) {
    if (int rc = attn_check(a)) return rc;
    const bool split = a.Lq <= 16 && !a.no_split;
    const int tiles = (int)cdiv(a.Lq, split ? 16 : 64);
    const dim3 grid(attn_grid(tiles, a.H * a.B));
    if (a.q_lo) {      // parity precision: split queries (the LLM's 128-wide heads, no key padding)
        RV_CHECK_ARG(a.dh == 128 && !a.key_pad, "attention: split queries are instantiated for 128-wide heads without key padding");
        attn_launch<128, true>(a, split, grid, tiles, st);
        RV_CHECK_LAUNCH("attention");
        return RV_OK;
    }
    // long-key problems without a mask (the adapter's self-attention, the CLIP towers): key blocks staged in LDS once per 128 query rows (attn_body_lds, two tiles)
    const bool lds = !split && !a.key_pad && !a.causal && !a.row_pos && !a.row_share && !a.out_packed && !a.out_lo && a.Lk >= 96 && a.Lq >= 48 &&
                     (a.dh == 64 || a.dh == 96) && rv_cur_opts().attn_lds;
    if (lds) {
        const int t128 = (int)cdiv(a.Lq, 128);
        const dim3 g128(attn_grid(t128, a.H * a.B));
        if (a.dh == 64) hipLaunchKernelGGL((attn_kernel_lds<64, 2>), g128, dim3(256), 0, st, a, t128);
        else hipLaunchKernelGGL((attn_kernel_lds<96, 2>), g128, dim3(256), 0, st, a, t128);
        RV_CHECK_LAUNCH("attention (LDS-staged keys)");
        return RV_OK;
    }
    if (!split && a.dh == 128 && !a.key_pad && !a.row_pos && !a.row_share && !a.out_packed && !a.out_lo && a.Lk >= 64 && a.Lq > 16 && rv_cur_opts().attn_lds) {
        hipLaunchKernelGGL((attn_kernel_lds<128, 1>), grid, dim3(256), 0, st, a, tiles);      // the LLM prefill of one generate: 64-row workgroups share a staged copy
        RV_CHECK_LAUNCH("attention (LDS-staged keys, dh 128)");
        return RV_OK;
    }
    if (a.dh == 64) attn_launch<64>(a, split, grid, tiles, st);
    else if (a.dh == 96) attn_launch<96>(a, split, grid, tiles, st);
    else if (a.dh == 128) attn_launch<128>(a, split, grid, tiles, st);
    else if (a.dh == 512) {
        // the 4096-d cross_attn ClipEncoder (8 heads of 512): the same body with 16 query / 32 output fragments per wave - 256 + 250 registers,
        // one wave per SIMD.  A coverage path (no shipped script selects this adapter), not a tuned one; short query counts take the same
        // kernel (the key-split form would need 132 KiB of static LDS for its merge)
        const int t512 = (int)cdiv(a.Lq, 64);
        hipLaunchKernelGGL((attn_kernel<512, false>), dim3(attn_grid(t512, a.H * a.B)), dim3(256), 0, st, a, t512);
    }
    else {
        rv_set_error("attention: head dim %d unsupported (64, 96, 128)", a.dh);
        return RV_ERR_ARG;
    }
    RV_CHECK_LAUNCH("attention");
    return RV_OK;
}

extern "C" int rv_attention(const void* q, int64_t q_row_stride, int64_t q_batch_stride, const void* k, int64_t k_row_stride,
                            int64_t k_batch_stride, int64_t k_head_stride, const void* vt, int64_t vt_batch_stride,
                            int64_t vt_head_stride, int64_t vt_d_stride, void* out, int64_t o_row_stride, int64_t o_batch_stride,
                            const uint8_t* key_pad, int32_t B, int32_t H, int32_t dh, int32_t Lq, int32_t Lk, int32_t causal,
                            int32_t q_pos0, int32_t kv_batch_div, float scale, void* stream) {
    AttnArgs a{q, q_row_stride, q_batch_stride, k, k_row_stride, k_batch_stride, k_head_stride, vt, vt_batch_stride,
               vt_head_stride, vt_d_stride, out, o_row_stride, o_batch_stride, key_pad, B, H, dh, Lq, Lk, causal, q_pos0,
               kv_batch_div, scale};
    // (the internal callers never ask for either; a remainder batch would read a key batch that does not exist, a query in front of key 0 has no key)
    RV_CHECK_ARG(kv_batch_div <= 0 || B % kv_batch_div == 0, "attention: B = %d is not a multiple of kv_batch_div = %d", B, kv_batch_div);
    RV_CHECK_ARG(!causal || q_pos0 >= 0, "attention: causal with q_pos0 = %d < 0 (query 0 would see no key)", q_pos0);
    return k_attention(a, as_stream(stream));
}
