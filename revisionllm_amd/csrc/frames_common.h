// What the three CLIP front-end kernels (frames.hip: uint8 RGB; frames_yuv.hip: planar and packed YCbCr surfaces) share.
//   device  the tap definition of the antialiased bicubic resampler and the tap-table routine of phase 0, the sample conversions of phase 1, and the tail of
//           phase 2: display permutation, f32 image / op16 patch stores, zero fill of the pad columns
//   host    the capacity helpers of the tile plans, the tile-plan search, the argument checks and the setup every entry point has in common, the launch helper
//           and the loop that cuts a list-form batch into launches
// The tail and the host routines are templated on the argument block: FrParams and FyParams name the fields they read alike (R, patch, g, K, Kp, top, left, ldp,
// patches, image, mirx, miry, mean, den, TY / TX / tilesX / bands), each in its own layout.
// Host and device place the taps with the same f64 expressions, so fp contraction is off from here to the end of the including translation unit; the tap loops
// ask for their fma by name.
#pragma once
#include <math.h>

#include <algorithm>
#include <atomic>
#include <tuple>
#include <type_traits>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int FR_THREADS = 256;
constexpr int FR_SR = 16;                   // source rows staged per chunk
constexpr int FR_LDS_BUDGET = 76 * 1024;    // per workgroup: two fit a CU's 160 KiB
constexpr int FR_MAX_SIDE = 8192;

// taps of an output whose centre lies at `centre` of an axis of `in` samples, filtered at `scale` (torch's antialiased resampling): [t0, t0 + nt)
__host__ __device__ inline void fr_taps_at(double centre, double scale, int in, int& t0, int& nt) {
    const double support = scale >= 1.0 ? 2.0 * scale : 2.0;
    long long lo = (long long)(centre - support + 0.5), hi = (long long)(centre + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > in) hi = in;
    t0 = (int)lo;
    nt = hi > lo ? (int)(hi - lo) : 0;
}

// One axis of a plane sampled `div` times coarser than the frame, its sample grid shifted by `off` samples: output index i of the frame's resize (scale =
// in / out of the FRAME, align_corners = False) has its centre at scale * (i + 0.5) / div + off of the plane's `in` samples and is filtered at scale / div.
// div = 1, off = 0 is the frame's own axis to the bit (x / 1 and x + 0 are exact).
struct FrAxis {
    double scale, div, off;
    int in;
};
__host__ __device__ inline double fr_axis_centre(const FrAxis& a, int i) { return a.scale * (i + 0.5) / a.div + a.off; }
__host__ __device__ inline void fr_axis_taps(const FrAxis& a, int i, int& t0, int& nt) { fr_taps_at(fr_axis_centre(a, i), a.scale / a.div, a.in, t0, nt); }

// Display orientation (include/revision_hip.h: bit 0 transpose, bit 1 mirror display x, bit 2 mirror display y, applied in that order).  The kernels stay in
// CODED orientation: each coded axis serves one display axis (the other one under transpose) and takes that axis' scale, crop offset and mirror flag; only
// the store is permuted.  mx / my: the coded x / y axis runs against the display axis it serves.
struct FrOrient {
    int tr, mx, my;
};
inline FrOrient fr_orient(int orient) {
    const int tr = orient & 1, mdx = (orient >> 1) & 1, mdy = (orient >> 2) & 1;
    return FrOrient{tr, tr ? mdy : mdx, tr ? mdx : mdy};
}
// The ORI of the instance that serves an orientation code: 0 = none, 1 = mirrors, 2 = transpose, with or without mirrors.
inline int fr_orient_class(int orient) { return orient == 0 ? 0 : (orient & 1) ? 2 : 1; }

// Resize(R): shorter side -> R, longer side -> int(R * long / short); CenterCrop(R): offset round-half-even((size - R) / 2).  sy / sx: in / out per axis.
inline void fr_resize_crop(int H, int W, int R, double& sy, double& sx, int& top, int& left) {
    const int hr = H <= W ? R : (int)((int64_t)R * H / W), wr = H <= W ? (int)((int64_t)R * W / H) : R;
    sy = (double)H / hr;
    sx = (double)W / wr;
    top = (int)nearbyint((hr - R) / 2.0);
    left = (int)nearbyint((wr - R) / 2.0);
}

// Resized index of the display axis that coded output o of the R cropped outputs computes: a mirrored axis runs backwards.  mir = 0 is first + o.
__host__ __device__ inline int fr_disp_index(int first, int R, int o, int mir) { return first + (mir ? R - 1 - o : o); }

// Taps of coded output o in CODED sample indices: the display window, reflected when the axis is mirrored.  mir = 0 is fr_axis_taps of first + o.
__host__ __device__ inline void fr_axis_taps_m(const FrAxis& a, int first, int R, int o, int mir, int& t0, int& nt) {
    fr_axis_taps(a, fr_disp_index(first, R, o, mir), t0, nt);
    if (mir) t0 = a.in - t0 - nt;
}

// Keys' cubic, a = -0.5
__device__ inline double fr_cubic(double x) {
    x = fabs(x);
    if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
    if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
    return 0.0;
}

// Phase 0, every kernel and axis: the tap-table entry of coded output o of the R cropped outputs - first tap in coded sample indices, count (clamped to the
// host's capacity) and the normalised f32 weights of the display window in coded order.  A mirrored display axis negates the siting offset a.off (the host
// does) and reflects the window.  The un-oriented instances pass the constant mir = 0: output first + o, j0 = t0, dj = 1.
__device__ inline void fr_tap_table(const FrAxis& a, int first, int R, int mir, int o, int cap, float* w, int& t0c, int& ntc) {
    const double fscale = a.scale / a.div, centre = fr_axis_centre(a, fr_disp_index(first, R, o, mir));
    int t0, nt;
    fr_taps_at(centre, fscale, a.in, t0, nt);
    nt = min(nt, cap);
    const double inv = fscale >= 1.0 ? 1.0 / fscale : 1.0;
    const int j0 = mir ? t0 + nt - 1 : t0, dj = mir ? -1 : 1;   // display sample of coded tap t: j0 + dj * t
    double tot = 0.0;
    for (int t = 0; t < nt; ++t) tot += fr_cubic((j0 + dj * t - centre + 0.5) * inv);
    const double rt = tot != 0.0 ? 1.0 / tot : 1.0;
    for (int t = 0; t < nt; ++t) w[t] = (float)(fr_cubic((j0 + dj * t - centre + 0.5) * inv) * rt);
    t0c = mir ? a.in - t0 - nt : t0;
    ntc = nt;
}

// Phase 1: a staged sample as f32.  16-bit words drop the low bits where the value sits in the high bits (shift = 0 otherwise); a 32-bit word holds three
// 10-bit fields.
__device__ inline float fr_sample(uint8_t v, int) { return (float)v; }
__device__ inline float fr_sample(uint16_t v, int shift) { return (float)(v >> shift); }
__device__ inline float fr_sample(uint32_t v, int shift) { return (float)((v >> shift) & 1023u); }

// Phase 2, behind the vertical pass and the normalisation: channel c of coded output (y, x) of frame f -> the display pixel it is -> the f32 image and / or
// the op16 patch element.
template <int ORI, class P>
__device__ inline void fr_store(const P& p, int64_t f, int c, int y, int x, float v) {
    if constexpr (ORI != 0) {
        const int dy = fr_disp_index(0, p.R, y, p.miry), dx = fr_disp_index(0, p.R, x, p.mirx);
        y = ORI == 2 ? dx : dy;
        x = ORI == 2 ? dy : dx;
    }
    if (p.image) p.image[((f * 3 + c) * p.R + y) * p.R + x] = v;
    if (p.patches)
        p.patches[((f * p.g + y / p.patch) * p.g + x / p.patch) * p.ldp + (c * p.patch + y % p.patch) * p.patch + x % p.patch] = f32_to_op16(v);
}

// ... and the zero fill of the pad columns K .. Kp - 1 of the patch rows whose first pixel lies in the tile of ty x tx coded outputs at (y0, x0).
template <int ORI, class P>
__device__ inline void fr_zero_pad(const P& p, int64_t f, int y0, int ty, int x0, int tx, int tid) {
    if (p.patches && p.Kp > p.K) {
        int py0 = y0, pty = ty, px0 = x0, ptx = tx;   // the tile's rectangle of the display image
        if constexpr (ORI != 0) {
            const int cy0 = p.miry ? p.R - y0 - ty : y0, cx0 = p.mirx ? p.R - x0 - tx : x0;
            py0 = ORI == 2 ? cx0 : cy0;
            pty = ORI == 2 ? tx : ty;
            px0 = ORI == 2 ? cy0 : cx0;
            ptx = ORI == 2 ? ty : tx;
        }
        const int gy0 = (py0 + p.patch - 1) / p.patch, gy1 = (py0 + pty + p.patch - 1) / p.patch;
        const int gx0 = (px0 + p.patch - 1) / p.patch, gx1 = (px0 + ptx + p.patch - 1) / p.patch;
        const int pad = p.Kp - p.K, ngx = gx1 - gx0;
        for (int it = tid; it < (gy1 - gy0) * ngx * pad; it += FR_THREADS) {
            const int j = it % pad, pr = it / pad;
            p.patches[((f * p.g + gy0 + pr / ngx) * p.g + gx0 + pr % ngx) * p.ldp + p.K + j] = 0;
        }
    }
}

// ---- host: tile plans -------------------------------------------------------------------------------------------------------------------------------------
// Largest tap count of an axis over the R cropped outputs.
inline int fr_max_taps(const FrAxis& a, int first, int R) {
    int cap = 0;
    for (int o = 0; o < R; ++o) {
        int lo, n;
        fr_axis_taps(a, first + o, lo, n);
        if (n > cap) cap = n;
    }
    return cap;
}

// Largest span of source rows / columns a tile of t coded outputs touches (mir: the axis is mirrored, so the tiles are cut from the far end of the crop).
inline int fr_max_span(const FrAxis& a, int first, int R, int t, int mir = 0) {
    int span = 0;
    for (int o0 = 0; o0 < R; o0 += t) {
        const int o1 = (o0 + t < R ? o0 + t : R) - 1;
        int lo, n0, hi, n1;
        fr_axis_taps_m(a, first, R, o0, mir, lo, n0);
        fr_axis_taps_m(a, first, R, o1, mir, hi, n1);
        if (hi + n1 - lo > span) span = hi + n1 - lo;
    }
    return span;
}

// The cheapest of the tile shapes ty = 16 .. 1 x tx = 256 .. 1 (clamped to R) that plan(block, ty, tx, cost) fits into the LDS budget; false = none does.
template <class P, class Plan>
bool fr_best_plan(const P& p, int R, Plan plan, P& best) {
    double best_cost = 0.0;
    bool have = false;
    for (int ty = 16; ty >= 1; ty >>= 1)
        for (int tx = 256; tx >= 1; tx >>= 1) {
            double cost;
            P q = p;
            if (plan(q, ty < R ? ty : R, tx < R ? tx : R, cost) && (!have || cost < best_cost)) best = q, best_cost = cost, have = true;
        }
    return have;
}

// ---- host: checks and setup -------------------------------------------------------------------------------------------------------------------------------
inline int fr_kp(int patch) { return (3 * patch * patch + 127) / 128 * 128; }   // K = 3 * patch^2, padded to the GEMM's 128

// The checks every entry point makes, in the order they report.  frame() and source() are the entry's own checks of the frame size and of the source pointers
// and strides, which come in between; an empty batch (n = 0) is valid without pointers, and the caller returns on it as well.
template <class Frame, class Source>
int fr_check_common(int32_t R, int32_t patch, int32_t n, const float* mean, const float* std, const void* patches, int64_t ldp, const float* image, const char* who,
                    Frame frame, Source source) {
    RV_CHECK_ARG(R >= 1 && patch >= 1 && R % patch == 0, "%s: R = %d is not a multiple of patch = %d", who, R, patch);
    if (const int rc = frame()) return rc;
    RV_CHECK_ARG(R <= FR_MAX_SIDE, "%s: R = %d above %d", who, R, FR_MAX_SIDE);
    RV_CHECK_ARG(n >= 0, "%s: n = %d", who, n);
    if (n == 0) return RV_OK;
    if (const int rc = source()) return rc;
    RV_CHECK_ARG(patches || image, "%s: both outputs null", who);
    RV_CHECK_ARG(mean && std, "%s: null mean / std", who);
    RV_CHECK_ARG(!patches || ldp >= fr_kp(patch), "%s: ldp = %lld below Kp = %d", who, (long long)ldp, fr_kp(patch));
    return RV_OK;
}

inline int fr_check_orient(int32_t orient, const char* who) {
    RV_CHECK_ARG(orient >= 0 && orient <= 7, "%s: orient %d (0 .. 7: bit 0 transpose, bit 1 mirror x, bit 2 mirror y)", who, orient);
    return RV_OK;
}

// What every block takes from the output geometry and the orientation: Resize(R) / CenterCrop(R) of the DISPLAY picture (W x H under transpose), each coded axis
// then taking the scale (sy / sx: in / out of the coded H / W), crop offset and mirror flag of the display axis it serves; the normalisation and the outputs.
template <class P>
void fr_setup(P& p, int H, int W, int32_t orient, int32_t R, int32_t patch, const float* mean, const float* std, void* patches, int64_t ldp, float* image, double& sy,
              double& sx) {
    p.R = R;
    p.patch = patch;
    p.g = R / patch;
    p.K = 3 * patch * patch;
    p.Kp = fr_kp(patch);
    const FrOrient ori = fr_orient(orient);
    double dsy, dsx;
    int dtop, dleft;
    fr_resize_crop(ori.tr ? W : H, ori.tr ? H : W, R, dsy, dsx, dtop, dleft);
    sy = ori.tr ? dsx : dsy;
    sx = ori.tr ? dsy : dsx;
    p.top = ori.tr ? dleft : dtop;
    p.left = ori.tr ? dtop : dleft;
    p.mirx = ori.mx;
    p.miry = ori.my;
    for (int c = 0; c < 3; ++c) {
        p.mean[c] = mean[c];
        p.den[c] = std[c] + 1e-8f;
    }
    p.patches = (op16_t*)patches;
    p.ldp = ldp;
    p.image = image;
}

// ---- host: launches ---------------------------------------------------------------------------------------------------------------------------------------
// fn(std::integral_constant<int, v>) for a run-time v of 0 .. N - 1: how a run-time choice names a kernel instance.
template <int N, class F>
int fr_pick(int v, F&& fn) {
    if constexpr (N == 1) return fn(std::integral_constant<int, 0>{});
    else return v == N - 1 ? fn(std::integral_constant<int, N - 1>{}) : fr_pick<N - 1>(v, fn);
}
template <int I>
using FrSample = std::tuple_element_t<I, std::tuple<uint8_t, uint16_t, uint32_t>>;   // the sample type of sample_bytes = 1 << I

// One launch of a kernel instance; `what` names the kernel in a launch error.  The dynamic-LDS opt-in is a per-device attribute of each instance: one flag word
// per instantiation of this helper, one bit per device.
template <auto Kernel, class Args>
int fr_launch(const Args& a, int64_t wgs, int lds, void* stream, const char* who, const char* what) {
    static std::atomic<uint64_t> have_lds{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = 1ull << (dev & 63);
    if (!(have_lds.load(std::memory_order_relaxed) & bit)) {
        if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FR_LDS_BUDGET) != hipSuccess) {
            rv_set_error("%s: cannot reserve %d bytes of LDS", who, FR_LDS_BUDGET);
            return RV_ERR_HIP;
        }
        have_lds.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(Kernel, dim3((unsigned)wgs), dim3(FR_THREADS), lds, as_stream(stream), a);
    RV_CHECK_LAUNCH(what);
    return RV_OK;
}

// All n frames of a call through launch(argument block, workgroups).  Contiguous frames (tab null): one launch on the planned block.  List form: launches of at
// most RV_FRAME_TABLE_MAX frames on a Tab - the block and, behind it, `tab`, the slice's entries of the caller's table; the output pointers move on with the
// slices, everything else is shared.  out(block): the part of the block that holds the plan and the outputs.
template <class Tab, class P, class Out, class Slot, class Launch>
int fr_launch_all(const P& best, Out out, const Slot* tab, int32_t n, Launch launch, const char* who) {
    const int64_t per_frame = (int64_t)out(best).bands * out(best).tilesX;
    if (!tab) {
        const int64_t wgs = n * per_frame;
        RV_CHECK_ARG(wgs < (1ll << 31), "%s: %lld workgroups (n = %d) exceed one launch", who, (long long)wgs, n);
        return launch(best, wgs);
    }
    const int64_t wmax = (n < RV_FRAME_TABLE_MAX ? n : RV_FRAME_TABLE_MAX) * per_frame;
    RV_CHECK_ARG(wmax < (1ll << 31), "%s: %lld workgroups per launch exceed one launch", who, (long long)wmax);
    for (int32_t f0 = 0; f0 < n; f0 += RV_FRAME_TABLE_MAX) {
        const int32_t nf = n - f0 < RV_FRAME_TABLE_MAX ? n - f0 : RV_FRAME_TABLE_MAX;
        Tab a{};
        static_cast<P&>(a) = best;
        auto& o = out(a);
        if (o.patches) o.patches += (int64_t)f0 * o.g * o.g * o.ldp;
        if (o.image) o.image += (int64_t)f0 * 3 * o.R * o.R;
        std::copy_n(tab + f0, nf, a.tab);
        if (const int rc = launch(a, nf * per_frame)) return rc;
    }
    return RV_OK;
}

}  // namespace
