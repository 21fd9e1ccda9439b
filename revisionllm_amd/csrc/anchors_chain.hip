// The chain library's second span generator (librevision_hip_chain.so, include/revision_hip_chain.h): multi-scale sliding-window proposals.
//   rvc_span_anchors   every row's sliding windows ("anchors") at up to eight (length, stride, margin) scales are scored by the mean of their usable
//                      frames, or by the contrast between that mean and the mean of the usable frames within `margin` frames outside; the local
//                      peaks of each scale come back in rv_span_propose's (centre, width) encoding with their scores, so rv_span_scores, rv_span_rank
//                      and rvc_span_refine read them - one launch
// Nothing here depends on the row's range of values, which is what rv_span_propose's relative levels depend on: one outlier frame moves no anchor's
// score but those it lies in or next to.
// Similarities are quantised to integers (2^24 steps to the unit), so every sum is exact and no result depends on the order of any scan or reduction:
// the kernel matches a numpy statement of the rule (tests/span_anchors_oracle.py) bit for bit.  The duration (span_mask_sum, duration_frames), the
// quantisation of a usable similarity (sim_usable, sim_quantise), the contrast (contrast_f64) and the span encoding (span_encode) are grounding.h's
// helpers, the ones span_refine_kernel calls.  The kernel reads f32 rows only, so one library serves both operand flavours.
#include "grounding.h"

#include "../../include/revision_hip_chain.h"

namespace {

constexpr int AN_TPB = 1024, AN_WAVES = AN_TPB / 64;
constexpr int AN_FPT = 4, AN_TILE = AN_TPB * AN_FPT;      // the prefix walk: four consecutive frames per thread, 4096 per tile
constexpr int AN_MAX_SCALES = 8, AN_MAX_PEAK = 64, AN_MAX_SPANS = 2048, AN_MAX_L = 1 << 20;

struct AnchorArgs {
    const float* sims;       // f32 [rows, L]
    const float* mask;       // f32 [rows / rpm, L]
    const float* valid;      // f32 [rows / rpv, L] or null
    float* out_spans;        // f32 [rows, N, 2]
    float* scores;           // f32 [rows, N]
    int32_t* n_spans;        // i32 [rows]
    int32_t* n_found;        // i32 [rows]
    int32_t* windows;        // i32 [rows, N, 2] or null
    int32_t* scale;          // i32 [rows, N] or null
    char* ws;                // the rows' workspaces, ws_row bytes each
    int64_t ws_row;
    int64_t cap;             // the anchors of a row of D = L frames: the length of each key array
    int rpv, rpm, L, S, mode, peak, min_usable, N;
    int len[AN_MAX_SCALES], stride[AN_MAX_SCALES], margin[AN_MAX_SCALES];
};

// a prefix point: S(0, t) and C(0, t), one 16-byte element
struct __attribute__((aligned(16))) AnPrefix {
    long long s;
    int c, pad;
};

// the anchors of one scale over D frames: floor((D - len) / stride) + 1 regular ones and, where (D - len) % stride != 0, the one flush with the end
__host__ __device__ inline int64_t an_count(int64_t D, int64_t len, int64_t stride) {
    if (len > D) return 0;
    const int64_t room = D - len;
    return room / stride + 1 + (room % stride != 0 ? 1 : 0);
}

// A key that is LARGER for the larger J, as an unsigned 64-bit number; never 0 for a number (0 is "no anchor here").  -0 counts as +0.
__device__ __forceinline__ uint64_t an_key(double j) {
    long long b = __double_as_longlong(j);
    if (j == 0.0) b = 0;
    return b < 0 ? ~(uint64_t)b : ((uint64_t)b | 0x8000000000000000ull);
}
__device__ __forceinline__ double an_value(uint64_t k) {
    return __longlong_as_double((long long)((k & 0x8000000000000000ull) ? (k ^ 0x8000000000000000ull) : ~k));
}

// exclusive prefix of v over the block's threads in thread order, and the block's total; all threads call; sc: AN_WAVES ints of LDS
__device__ __forceinline__ int an_block_scan(int v, int* sc, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(incl, o, 64);
        if (lane >= o) incl += x;
    }
    __syncthreads();                                     // the last call's loads from sc are done
    if (lane == 63) sc[wave] = incl;
    __syncthreads();
    int pre = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < AN_WAVES; ++w) {
        const int x = sc[w];
        pre += w < wave ? x : 0;
        total += x;
    }
    return pre + incl - v;
}

// One 1024-thread workgroup per row (blockIdx.x).
// (1) duration: span_mask_sum, span_refine_kernel's sum of the mask row - waves 0 to 3 add it up as that kernel's four waves do - and D.
// (2) one walk over the row's D frames in tiles of 4096, four consecutive frames per thread: (q, usable) per frame, the thread's running sums, a
//     wave-wide inclusive scan of the threads' totals, the waves' totals through LDS (two buffers in turn: one barrier per tile), and the prefix
//     pair of point t + 1 goes to the row's workspace.
// (3) every anchor of every scale (a flat index: scale-major, then the anchor index) gets its key - an_key(J), 0 when it is not admissible - from
//     two or four prefix look-ups, into the first key array.
// (4) the peak test on the keys of the <= 2 peak neighbours; a peak's key, else 0, goes to the second key array; the peaks are counted.
// (5) more peaks than N: the key V of the N-th peak in descending order by a radix descent over the second array, a byte a pass, with LDS counts, and
//     `need`, how many of the peaks with exactly that key are kept (those with the smallest flat indices).  Else V = 0, need = 0.
// (6) ordered compaction: the flat indices in chunks of 1024, one block scan per chunk over (key > V, key == V) counts; a kept peak is stored at
//     its place.  Then the padding and the two counts.
// Every barrier is reached by all threads: the loop bounds are the same in every thread.
__global__ __launch_bounds__(AN_TPB) void span_anchors_kernel(const AnchorArgs a) {
    __shared__ float red[4];
    __shared__ long long wS[2][AN_WAVES];
    __shared__ int wC[2][AN_WAVES];
    __shared__ int sc[AN_WAVES];
    __shared__ int hist[256];
    __shared__ int sLen[AN_MAX_SCALES], sStride[AN_MAX_SCALES], sMargin[AN_MAX_SCALES], sCnt[AN_MAX_SCALES], sOff[AN_MAX_SCALES + 1];
    __shared__ int pick[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    const int L = a.L, N = a.N;

    const float dur = span_mask_sum<AN_TPB>(a.mask, r, a.rpm, L, red);      // (waves 0 to 3 add; the others wait at its barrier)
    const int D = duration_frames(dur, L);

    if (tid == 0) {
        int off = 0;
#pragma unroll
        for (int k = 0; k < AN_MAX_SCALES; ++k) {
            const int n = k < a.S ? (int)an_count(D, a.len[k], a.stride[k]) : 0;
            sLen[k] = a.len[k];
            sStride[k] = a.stride[k];
            sMargin[k] = a.margin[k];
            sCnt[k] = n;
            sOff[k] = off;
            off += n;
        }
        sOff[AN_MAX_SCALES] = off;
    }

    const float* __restrict__ s = a.sims + r * L;
    const float* __restrict__ vr = a.valid ? a.valid + (r / a.rpv) * L : nullptr;
    char* ws = a.ws + r * a.ws_row;
    AnPrefix* P = (AnPrefix*)ws;                                           // L + 1 points
    uint64_t* K1 = (uint64_t*)(ws + ((int64_t)L + 1) * 16);                // cap keys: every admissible anchor
    uint64_t* K2 = K1 + a.cap;                                             // cap keys: the peaks

    // ---- (2) the prefix pairs ----
    if (tid == 0) P[0] = AnPrefix{0, 0, 0};
    {
        long long carryS = 0;
        int carryC = 0, par = 0;
        for (int base = 0; base < D; base += AN_TILE, par ^= 1) {
            const int t0 = base + tid * AN_FPT;
            long long q[AN_FPT];
            int u[AN_FPT];
#pragma unroll
            for (int e = 0; e < AN_FPT; ++e) {                              // (both loads of all four frames are in flight together; a hidden frame's
                const int t = t0 + e;                                      // similarity is loaded and dropped: it enters nothing)
                const bool in = t < D;
                const float v = in ? s[t] : 0.f;
                const float w = (in && vr) ? vr[t] : 1.f;
                const bool ok = in && w != 0.f && sim_usable(v);
                q[e] = ok ? sim_quantise(v) : 0;
                u[e] = ok ? 1 : 0;
            }
#pragma unroll
            for (int e = 1; e < AN_FPT; ++e) {
                q[e] += q[e - 1];
                u[e] += u[e - 1];
            }
            long long sq = q[AN_FPT - 1];                                  // the thread's four frames, then the wave-wide inclusive scan of those
            int su = u[AN_FPT - 1];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const long long qo = __shfl_up(sq, o, 64);
                const int uo = __shfl_up(su, o, 64);
                if (lane >= o) {
                    sq += qo;
                    su += uo;
                }
            }
            if (lane == 63) {
                wS[par][wave] = sq;
                wC[par][wave] = su;
            }
            __syncthreads();
            long long preS = carryS + (sq - q[AN_FPT - 1]), totS = 0;      // what lies in front of the thread's first frame
            int preC = carryC + (su - u[AN_FPT - 1]), totC = 0;
#pragma unroll
            for (int w = 0; w < AN_WAVES; ++w) {
                const long long xs = wS[par][w];
                const int xc = wC[par][w];
                preS += w < wave ? xs : 0;
                preC += w < wave ? xc : 0;
                totS += xs;
                totC += xc;
            }
#pragma unroll
            for (int e = 0; e < AN_FPT; ++e)
                if (t0 + e < D) P[t0 + e + 1] = AnPrefix{preS + q[e], preC + u[e], 0};
            carryS += totS;
            carryC += totC;
        }
    }
    __threadfence_block();
    __syncthreads();                                                       // the prefix pairs and the scale table are written

    const int total = sOff[AN_MAX_SCALES];
    // flat index -> scale and anchor index
    auto locate = [&](int i, int& sc_, int& idx) {
        sc_ = 0;
#pragma unroll
        for (int k = 1; k < AN_MAX_SCALES; ++k) sc_ = (k < a.S && i >= sOff[k]) ? k : sc_;
        idx = i - sOff[sc_];
    };
    // anchor idx of a scale starts at idx * stride; the flush one, whose product lies past it, at D - len
    auto start_of = [&](int idx, int len, int stride) {
        const int64_t p = (int64_t)idx * stride, last = (int64_t)D - len;
        const int64_t v = p < last ? p : last;
        return (int)(v > 0 ? v : 0);
    };

    // ---- (3) the keys ----
    for (int i = tid; i < total; i += AN_TPB) {
        int k, idx;
        locate(i, k, idx);
        const int len = sLen[k], margin = sMargin[k];
        const int x = start_of(idx, len, sStride[k]);
        const int y = x + len < D ? x + len : D;                           // (x + len <= D by the count; stated for the load, changes no value)
        const AnPrefix Px = P[x], Py = P[y];
        const long long Sin = Py.s - Px.s;
        const int Cin = Py.c - Px.c;
        bool ok = Cin >= a.min_usable;
        double j;
        if (a.mode == RVC_ANCHORS_CONTRAST) {
            const int xm = x - margin > 0 ? x - margin : 0, yp = y + margin < D ? y + margin : D;      // (margin <= L: no overflow)
            const AnPrefix Pm = P[xm], Pp = P[yp];
            const long long Sout = (Px.s - Pm.s) + (Pp.s - Py.s);
            const int Cout = (Px.c - Pm.c) + (Pp.c - Py.c);
            ok = ok && Cout > 0;
            j = contrast_f64(Sin, Cin > 0 ? Cin : 1, Sout, Cout > 0 ? Cout : 1);
        } else {
            j = __ddiv_rn((double)Sin, (double)(Cin > 0 ? Cin : 1));
        }
        K1[i] = ok ? an_key(j) : 0ull;
    }
    __threadfence_block();
    __syncthreads();

    // ---- (4) the peaks ----
    int mine = 0;
    for (int i = tid; i < total; i += AN_TPB) {
        const uint64_t key = K1[i];
        uint64_t out = 0;
        if (key) {
            int k, idx;
            locate(i, k, idx);
            const int lo = idx - a.peak > 0 ? idx - a.peak : 0, hi = idx + a.peak < sCnt[k] - 1 ? idx + a.peak : sCnt[k] - 1;
            const uint64_t* row = K1 + sOff[k];
            bool beaten = false;
            for (int j = lo; j <= hi; ++j) {
                const uint64_t kj = row[j];
                beaten = beaten || kj > key || (kj == key && j < idx);
            }
            out = beaten ? 0ull : key;
            mine += beaten ? 0 : 1;
        }
        K2[i] = out;
    }
    int found;
    an_block_scan(mine, sc, found);
    __threadfence_block();
    __syncthreads();                                                       // K2 is written

    // ---- (5) the cut ----
    uint64_t V = 0;
    int need = 0;
    if (found > N) {                                                       // (the same in every thread)
        need = N;
        for (int shift = 56; shift >= 0; shift -= 8) {
            const uint64_t hi_mask = shift == 56 ? 0ull : (~0ull << (shift + 8));
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < total; i += AN_TPB) {
                const uint64_t key = K2[i];
                if (key && (key & hi_mask) == V) atomicAdd(&hist[(int)((key >> shift) & 255u)], 1);
            }
            __syncthreads();
            const int v = tid < 256 ? hist[255 - tid] : 0;                 // from the largest byte down
            int all;
            const int above = an_block_scan(v, sc, all);
            if (tid < 256 && above < need && need <= above + v) {          // exactly one thread: the counts above reach `need` inside its bin
                pick[0] = 255 - tid;
                pick[1] = need - above;
            }
            __syncthreads();
            V |= (uint64_t)pick[0] << shift;
            need = pick[1];
            __syncthreads();                                               // pick and hist are read before the next pass writes them
        }
    }
    const bool cut = found > N;

    // ---- (6) ordered compaction ----
    int gtBase = 0, tieBase = 0;
    for (int base = 0; base < total; base += AN_TPB) {
        const int i = base + tid;
        const uint64_t key = i < total ? K2[i] : 0ull;
        const bool gt = key > V, tie = cut && key == V;
        int both;
        const int ex = an_block_scan((gt ? 1 : 0) | (tie ? 1 << 16 : 0), sc, both);
        const int gtBefore = gtBase + (ex & 0xffff), tieBefore = tieBase + (ex >> 16);
        if (gt || (tie && tieBefore < need)) {
            const int pos = gtBefore + (tieBefore < need ? tieBefore : need);
            if (pos < N) {                                                 // (the kept set has min(found, N) members; stated for the stores, changes no value)
                int k, idx;
                locate(i, k, idx);
                const int len = sLen[k];
                const int x = start_of(idx, len, sStride[k]), y = x + len;
                const int64_t o = r * N + pos;
                span_encode(x, y, dur, a.out_spans[o * 2], a.out_spans[o * 2 + 1]);      // rv_span_propose's encoding
                a.scores[o] = __double2float_rn(an_value(key));
                if (a.windows) {
                    a.windows[o * 2] = x;
                    a.windows[o * 2 + 1] = y;
                }
                if (a.scale) a.scale[o] = k;
            }
        }
        gtBase += both & 0xffff;
        tieBase += both >> 16;
    }
    const int kept = found < N ? found : N;
    for (int pos = kept + tid; pos < N; pos += AN_TPB) {
        const int64_t o = r * N + pos;
        a.out_spans[o * 2] = a.out_spans[o * 2 + 1] = qnan();
        a.scores[o] = qnan();
        if (a.windows) a.windows[o * 2] = a.windows[o * 2 + 1] = -1;
        if (a.scale) a.scale[o] = -1;
    }
    if (tid == 0) {
        a.n_spans[r] = kept;
        a.n_found[r] = found;
    }
}

// the scale table's refusals, shared by the two entries -> 0 or RV_ERR_ARG with the message set
int an_check_scales(const char* who, int32_t L, const int32_t* scales, int32_t S, int32_t rows, bool contrast) {
    RV_CHECK_ARG(scales, "%s: bad arguments (a null scales)", who);
    RV_CHECK_ARG(S >= 1 && S <= AN_MAX_SCALES, "%s: S=%d scales must be in [1, %d]", who, S, AN_MAX_SCALES);
    RV_CHECK_ARG(L >= 1 && L <= AN_MAX_L, "%s: L=%d must be in [1, %d]", who, L, AN_MAX_L);
    RV_CHECK_ARG(rows >= 1, "%s: rows=%d must be at least 1", who, rows);
    for (int k = 0; k < S; ++k) {
        const int len = scales[3 * k], stride = scales[3 * k + 1], margin = scales[3 * k + 2];
        RV_CHECK_ARG(len >= 1 && stride >= 1 && stride <= len, "%s: scale %d has len=%d, stride=%d (len >= 1, 1 <= stride <= len)", who, k, len, stride);
        RV_CHECK_ARG(!contrast || margin >= 1, "%s: scale %d has margin=%d (at least 1 in contrast mode)", who, k, margin);
    }
    return RV_OK;
}

// bytes of one row's workspace (L + 1 prefix points of 16 bytes, two arrays of `cap` 8-byte keys) and cap, the anchors of a row of D = L frames
int64_t an_row_bytes(int32_t L, const int32_t* scales, int32_t S, int64_t& cap) {
    cap = 0;
    for (int k = 0; k < S; ++k) cap += an_count(L, scales[3 * k], scales[3 * k + 1]);
    return ((int64_t)L + 1) * 16 + cap * 16;
}

}  // namespace

extern "C" int64_t rvc_span_anchors_workspace(int32_t L, const int32_t* scales, int32_t S, int32_t rows) {
    if (an_check_scales("rvc_span_anchors_workspace", L, scales, S, rows, false) != RV_OK) return RV_ERR_ARG;
    int64_t cap;
    return an_row_bytes(L, scales, S, cap) * rows;
}

extern "C" int rvc_span_anchors(const float* sims, const float* mask, const float* valid, int32_t rpv, int32_t rows, int32_t rpm, int32_t L,
                                const int32_t* scales, int32_t S, int32_t mode, int32_t peak, int32_t min_usable, int32_t max_spans, float* out_spans,
                                float* scores, int32_t* n_spans, int32_t* n_found, int32_t* windows, int32_t* scale, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    const char* who = "rvc_span_anchors";
    RV_CHECK_ARG(sims && mask && out_spans && scores && n_spans && n_found,
                 "%s: bad arguments (a null sims, mask, out_spans, scores, n_spans or n_found)", who);
    RV_CHECK_ARG(mode == RVC_ANCHORS_MEAN || mode == RVC_ANCHORS_CONTRAST, "%s: mode=%d (0: mean, 1: contrast)", who, mode);
    if (int rc = an_check_scales(who, L, scales, S, rows, mode == RVC_ANCHORS_CONTRAST)) return rc;
    RV_CHECK_ARG(rpm >= 1 && rows % rpm == 0, "%s: rows=%d with rpm=%d rows per mask row (rpm >= 1, rows a multiple of rpm)", who, rows, rpm);
    RV_CHECK_ARG(rpv >= 1 && rows % rpv == 0, "%s: rows=%d with rpv=%d rows per validity row (rpv >= 1, rows a multiple of rpv)", who, rows, rpv);
    RV_CHECK_ARG(peak >= 0 && peak <= AN_MAX_PEAK, "%s: peak=%d must be in [0, %d]", who, peak, AN_MAX_PEAK);
    RV_CHECK_ARG(min_usable >= 1, "%s: min_usable=%d must be >= 1", who, min_usable);
    RV_CHECK_ARG(max_spans >= 1 && max_spans <= AN_MAX_SPANS, "%s: max_spans=%d must be in [1, %d]", who, max_spans, AN_MAX_SPANS);
    AnchorArgs a{};
    const int64_t row_bytes = an_row_bytes(L, scales, S, a.cap);
    RV_CHECK_ARG(workspace && ((uintptr_t)workspace & 15u) == 0 && workspace_bytes >= row_bytes * rows,
                 "%s: workspace of %lld bytes (16-byte aligned, at least rvc_span_anchors_workspace() = %lld bytes)", who, (long long)workspace_bytes,
                 (long long)(row_bytes * rows));
    a.sims = sims;
    a.mask = mask;
    a.valid = valid;
    a.out_spans = out_spans;
    a.scores = scores;
    a.n_spans = n_spans;
    a.n_found = n_found;
    a.windows = windows;
    a.scale = scale;
    a.ws = (char*)workspace;
    a.ws_row = row_bytes;
    a.rpv = rpv;
    a.rpm = rpm;
    a.L = L;
    a.S = S;
    a.mode = mode;
    a.peak = peak;
    a.min_usable = min_usable;
    a.N = max_spans;
    for (int k = 0; k < AN_MAX_SCALES; ++k) {
        a.len[k] = k < S ? scales[3 * k] : 1;
        a.stride[k] = k < S ? scales[3 * k + 1] : 1;
        const int m = k < S ? scales[3 * k + 2] : 1;
        a.margin[k] = m < 1 ? 1 : (m > L ? L : m);                         // (a margin beyond the row reaches what L reaches; no index arithmetic overflows)
    }
    hipLaunchKernelGGL(span_anchors_kernel, dim3((unsigned)rows), dim3(AN_TPB), 0, as_stream(stream), a);
    RV_CHECK_LAUNCH(who);
    return RV_OK;
}
