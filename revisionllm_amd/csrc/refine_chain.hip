// The chain library's boundary refinement (librevision_hip_chain.so, include/revision_hip_chain.h): the stage behind the ranking.
//   rvc_span_refine   every span - a kept proposal, an LLM answer in (start, end) form, a retrieval log - is moved to the neighbouring start / end pair
//                     with the largest contrast between the usable frames inside and the usable frames just outside, under the chain's validity
//                     rows; the result comes back in rv_span_propose's (centre, width) encoding, so rv_span_scores / rv_span_rank read it - one launch
// Similarities are quantised to integers (2^24 steps to the unit), so every sum is exact and no result depends on the order of any scan or reduction:
// the kernel matches a numpy statement of the rule bit for bit.  The duration (span_mask_sum, duration_frames), the window rule (SPAN_NOT_FINITE, span_slice), the
// span encoding (span_encode), the quantisation (sim_usable, sim_quantise) and the contrast (contrast_f64) are grounding.h's helpers, the ones
// span_scores_kernel, span_propose_kernel and span_anchors_kernel call.  The kernel reads f32 rows only, so one library serves both operand flavours.
#include "grounding.h"

#include "../../include/revision_hip_chain.h"

namespace {

constexpr int RF_MAX_RADIUS = 64, RF_MAX_MARGIN = 128, RF_MAX_L = 1 << 20;
constexpr int RF_POINTS = 2 * (2 * RF_MAX_RADIUS + RF_MAX_MARGIN) + 2;      // 514 prefix points per span: two zones of 2 radius + margin frames, a point more than frames each

struct RefineArgs {
    const float* sims;       // f32 [rows, L]
    const float* spans;      // f32 [rows, N, 2]
    const float* mask;       // f32 [rows / rpm, L]
    const float* valid;      // f32 [rows / rpv, L] or null
    float* out_spans;        // f32 [rows, N, 2]
    int32_t* windows;        // i32 [rows, N, 2] or null
    float* contrast;         // f32 [rows, N] or null
    float* contrast0;        // f32 [rows, N] or null
    int form, rpv, rpm, L, N, radius, margin, min_len;
};

// frame t of the row (t < D): usable -> its quantised similarity and 1, hidden -> 0 and 0.  The validity entry first, the similarity only behind a
// frame it does not hide; a similarity that is not a number hides the frame as well.
__device__ __forceinline__ void rf_frame(const float* __restrict__ s, const float* __restrict__ vr, int t, long long& q, int& u) {
    q = 0;
    u = 0;
    if (vr && !(vr[t] != 0.f)) return;
    const float v = s[t];
    if (!sim_usable(v)) return;
    q = sim_quantise(v);
    u = 1;
}

// The frames [z0, z1) behind the prefix (cs, cc) of point z0, which the caller has stored at slot `at`: the prefix of point t + 1 goes to slot
// at + (t - z0) + 1, in 64-frame chunks with a wave-wide inclusive scan; on return (cs, cc) is the prefix of point z1.  All lanes call.
__device__ __forceinline__ void rf_scan(const float* __restrict__ s, const float* __restrict__ vr, int z0, int z1, long long* tS, int* tC, int at,
                                        long long& cs, int& cc, int lane) {
    for (int base = z0; base < z1; base += 64) {
        const int t = base + lane;
        long long q = 0;
        int u = 0;
        if (t < z1) rf_frame(s, vr, t, q, u);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long qo = __shfl_up(q, o, 64);
            const int uo = __shfl_up(u, o, 64);
            if (lane >= o) {
                q += qo;
                u += uo;
            }
        }
        const int slot = at + (t - z0) + 1;
        if (t < z1 && slot < RF_POINTS) {          // (slot <= 513 by the zones' lengths; stated for the store, changes no value)
            tS[slot] = cs + q;
            tC[slot] = cc + u;
        }
        cs += __shfl(q, 63, 64);
        cc += __shfl(u, 63, 64);
    }
}

struct RfBest {
    double j;
    int dist, a, b;          // a < 0: no admissible candidate yet
};
// x is chosen before y: the larger J, then the smaller distance from the original pair, then the smaller a, then the smaller b (a strict total order
// over distinct pairs, so the result does not depend on the order of the comparisons)
__device__ __forceinline__ bool rf_before(const RfBest& x, const RfBest& y) {
    if (x.a < 0 || y.a < 0) return x.a >= 0 && y.a < 0;
    if (x.j != y.j) return x.j > y.j;
    if (x.dist != y.dist) return x.dist < y.dist;
    if (x.a != y.a) return x.a < y.a;
    return x.b < y.b;
}

// One wave per span (4 spans per block, all of row blockIdx.y), as span_scores_kernel.  The block adds the row's mask row up (that kernel's sum:
// span_mask_sum), then each wave: (1) its span's window [lo, hi) by rv_span_scores' rule, cut to the D frames of the duration: (lo0, hi0); (2) the prefix
// pairs (S, C) - int64 sum of the quantised usable similarities, int32 count of usable frames - at every point of the two zones
// [lo0 - radius - margin, lo0 + radius] and [hi0 - radius, hi0 + radius + margin] cut to [0, D], into the wave's table in LDS (one zone where they
// meet; else the frames between them enter through one lane-strided integer reduction); (3) the candidate pairs dealt to the lanes, four look-ups, two
// float64 divisions and a subtraction each; (4) a wave-wide reduction in rf_before's order, and lane 0 stores.  Every read of sims and valid lies
// inside the zones or the span, in front of D.
__global__ __launch_bounds__(256) void span_refine_kernel(const RefineArgs a) {
    __shared__ float red[4];
    __shared__ long long tabS[4][RF_POINTS];
    __shared__ int tabC[4][RF_POINTS];
    const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.L;
    const float dur = span_mask_sum<256>(a.mask, r, a.rpm, L, red);
    const int n = blockIdx.x * 4 + wave;
    if (n >= a.N) return;                                          // (no block-wide barrier behind this line)
    const int D = duration_frames(dur, L);
    const int64_t sp = (int64_t)r * a.N + n;

    // ---- the window: rv_span_scores' rule (span_slice), cut to the duration ----
    float x1, x2;
    if (a.form == 1) {
        const float c = a.spans[sp * 2], hw = __fmul_rn(0.5f, a.spans[sp * 2 + 1]);
        x1 = __fsub_rn(c, hw);
        x2 = __fadd_rn(c, hw);
    } else {
        x1 = a.spans[sp * 2];
        x2 = a.spans[sp * 2 + 1];
    }
    const float p1 = __fmul_rn(x1, dur), p2 = __fmul_rn(x2, dur);
    int lo0 = 0, hi0 = 0;
    if (!SPAN_NOT_FINITE(p1, p2)) {
        int lo, hi;
        span_slice(p1, p2, L, lo, hi);
        lo0 = lo < D ? lo : D;
        hi0 = hi < D ? hi : D;
    }
    if (hi0 <= lo0) {                                              // void: a non-finite bound, an empty window, nothing inside the duration
        if (lane == 0) {
            a.out_spans[sp * 2] = a.out_spans[sp * 2 + 1] = qnan();
            if (a.windows) a.windows[sp * 2] = a.windows[sp * 2 + 1] = -1;
            if (a.contrast) a.contrast[sp] = qnan();
            if (a.contrast0) a.contrast0[sp] = qnan();
        }
        return;
    }
    // here 0 <= lo0 < hi0 <= D <= L

    // ---- the prefix table ----
    const float* __restrict__ s = a.sims + (int64_t)r * L;
    const float* __restrict__ vr = a.valid ? a.valid + (int64_t)(r / a.rpv) * L : nullptr;
    long long* tS = tabS[wave];
    int* tC = tabC[wave];
    const int radius = a.radius, margin = a.margin;
    const int zA0 = lo0 - radius - margin > 0 ? lo0 - radius - margin : 0;
    const int zA1 = lo0 + radius < D ? lo0 + radius : D;           // > lo0 >= zA0
    const int zB0 = hi0 - radius > 0 ? hi0 - radius : 0;           // <= hi0
    const int zB1 = hi0 + radius + margin < D ? hi0 + radius + margin : D;   // >= hi0
    const bool merged = zB0 <= zA1;
    const int e1 = merged ? zB1 : zA1;                             // the first zone's last point; its points zA0 .. e1 sit at slots 0 .. e1 - zA0
    const int n1 = e1 - zA0 + 1;                                   // the second zone's points zB0 .. zB1 sit at slots n1 .. n1 + zB1 - zB0
    long long cs = 0;
    int cc = 0;
    if (lane == 0) {
        tS[0] = 0;
        tC[0] = 0;
    }
    rf_scan(s, vr, zA0, e1, tS, tC, 0, cs, cc, lane);
    if (!merged) {
        long long g = 0;
        int gc = 0;
        for (int t = zA1 + lane; t < zB0; t += 64) {               // the frames between the zones: inside the span
            long long q;
            int u;
            rf_frame(s, vr, t, q, u);
            g += q;
            gc += u;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            g += __shfl_xor(g, o, 64);
            gc += __shfl_xor(gc, o, 64);
        }
        cs += g;
        cc += gc;
        if (lane == 0) {
            tS[n1] = cs;
            tC[n1] = cc;
        }
        rf_scan(s, vr, zB0, zB1, tS, tC, n1, cs, cc, lane);
    }
    // the wave's own stores to its table, then its own loads: ordered within the wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    auto slot_of = [&](int p) {                                    // p in [zA0, e1] or, apart zones, in [zB0, zB1]
        int i = p <= e1 ? p - zA0 : n1 + (p - zB0);
        return i < 0 ? 0 : (i < RF_POINTS ? i : RF_POINTS - 1);    // (inside by the candidates' ranges; stated for the load, changes no value)
    };
    // J(x, y) -> admissible
    auto contrast_of = [&](int x, int y, double& j) {
        const int xm = x - margin > 0 ? x - margin : 0, yp = y + margin < D ? y + margin : D;
        const int ix = slot_of(x), iy = slot_of(y), ixm = slot_of(xm), iyp = slot_of(yp);
        const long long Sx = tS[ix], Sy = tS[iy];
        const int Cx = tC[ix], Cy = tC[iy];
        const long long Sin = Sy - Sx, Sout = (Sx - tS[ixm]) + (tS[iyp] - Sy);
        const int Cin = Cy - Cx, Cout = (Cx - tC[ixm]) + (tC[iyp] - Cy);
        if (!(Cin > 0 && Cout > 0)) return false;
        j = contrast_f64(Sin, Cin, Sout, Cout);
        return true;
    };

    // ---- the candidates ----
    const int a_lo = lo0 - radius > 0 ? lo0 - radius : 0, a_hi = lo0 + radius < D - 1 ? lo0 + radius : D - 1;
    const int b_lo = hi0 - radius > 1 ? hi0 - radius : 1, b_hi = hi0 + radius < D ? hi0 + radius : D;
    const int na = a_hi - a_lo + 1, nb = b_hi - b_lo + 1;          // >= 1 each (the original pair lies inside), <= 2 radius + 1
    double j0 = 0.0;
    const bool ok0 = contrast_of(lo0, hi0, j0);
    RfBest best{0.0, 0, -1, -1};
    for (int p = lane; p < na * nb; p += 64) {
        const int ia = p / nb;
        const int ca = a_lo + ia, cb = b_lo + (p - ia * nb);
        if (!(cb - ca >= a.min_len || (ca == lo0 && cb == hi0))) continue;
        double j;
        if (!contrast_of(ca, cb, j)) continue;
        const int da = ca - lo0, db = cb - hi0;
        const RfBest c{j, (da < 0 ? -da : da) + (db < 0 ? -db : db), ca, cb};
        if (rf_before(c, best)) best = c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const RfBest other{__shfl_xor(best.j, o, 64), __shfl_xor(best.dist, o, 64), __shfl_xor(best.a, o, 64), __shfl_xor(best.b, o, 64)};
        if (rf_before(other, best)) best = other;
    }
    if (lane == 0) {
        const bool found = best.a >= 0;
        const int ra = found ? best.a : lo0, rb = found ? best.b : hi0;
        span_encode(ra, rb, dur, a.out_spans[sp * 2], a.out_spans[sp * 2 + 1]);      // rv_span_propose's encoding
        if (a.windows) {
            a.windows[sp * 2] = ra;
            a.windows[sp * 2 + 1] = rb;
        }
        if (a.contrast) a.contrast[sp] = found ? __double2float_rn(best.j) : qnan();
        if (a.contrast0) a.contrast0[sp] = ok0 ? __double2float_rn(j0) : qnan();
    }
}

}  // namespace

extern "C" int rvc_span_refine(const float* sims, const float* spans, int32_t form, const float* mask, const float* valid, int32_t rpv, int32_t rows,
                               int32_t rpm, int32_t L, int32_t N, int32_t radius, int32_t margin, int32_t min_len, float* out_spans, int32_t* windows,
                               float* contrast, float* contrast0, void* stream) {
    const char* who = "rvc_span_refine";
    RV_CHECK_ARG(sims && spans && mask && out_spans, "%s: bad arguments (a null sims, spans, mask or out_spans)", who);
    RV_CHECK_ARG(form == 0 || form == 1, "%s: form=%d must be 0 (start, end) or 1 (centre, width)", who, form);
    RV_CHECK_ARG(rows >= 1 && N >= 1, "%s: rows=%d, N=%d (both at least 1)", who, rows, N);
    RV_CHECK_ARG(L >= 1 && L <= RF_MAX_L, "%s: L=%d must be in [1, %d]", who, L, RF_MAX_L);
    RV_CHECK_ARG(rpm >= 1 && rows % rpm == 0, "%s: rows=%d with rpm=%d rows per mask row (rpm >= 1, rows a multiple of rpm)", who, rows, rpm);
    RV_CHECK_ARG(rpv >= 1 && rows % rpv == 0, "%s: rows=%d with rpv=%d rows per validity row (rpv >= 1, rows a multiple of rpv)", who, rows, rpv);
    RV_CHECK_ARG(rows <= 65535, "%s: at most 65535 rows per launch (rows=%d)", who, rows);
    RV_CHECK_ARG(radius >= 1 && radius <= RF_MAX_RADIUS, "%s: radius=%d must be in [1, %d]", who, radius, RF_MAX_RADIUS);
    RV_CHECK_ARG(margin >= 1 && margin <= RF_MAX_MARGIN, "%s: margin=%d must be in [1, %d]", who, margin, RF_MAX_MARGIN);
    RV_CHECK_ARG(min_len >= 1, "%s: min_len=%d must be >= 1", who, min_len);
    const RefineArgs a{sims, spans, mask, valid, out_spans, windows, contrast, contrast0, form, rpv, rpm, L, N, radius, margin, min_len};
    hipLaunchKernelGGL(span_refine_kernel, dim3((unsigned)cdiv(N, 4), (unsigned)rows), dim3(256), 0, as_stream(stream), a);
    RV_CHECK_LAUNCH(who);
    return RV_OK;
}
