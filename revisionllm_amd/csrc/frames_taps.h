// What the CLIP front-end kernels (frames.hip: uint8 RGB; frames_yuv.hip: YCbCr surfaces) share: the tap definition of the antialiased bicubic resampler, the
// workgroup constants and the host's capacity helpers.  Host and device place the taps with the same f64
// expressions, so fp contraction is off from here to the end of the including translation unit; the tap loops ask for their fma by name.
#pragma once
#include <math.h>

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

// taps of output index i of an axis (align_corners = False): the centre is scale * (i + 0.5)
__host__ __device__ inline void fr_taps(double scale, int in, int i, int& t0, int& nt) { fr_taps_at(scale * (i + 0.5), scale, in, t0, nt); }

// One axis of a plane sampled `div` times coarser than the frame, its sample grid shifted by `off` samples: output index i of the frame's resize (scale =
// in / out of the FRAME) has its centre at scale * (i + 0.5) / div + off of the plane's `in` samples and is filtered at scale / div.  div = 1, off = 0 is
// fr_taps to the bit (x / 1 and x + 0 are exact).
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

// The tap-table entry of coded output o of an oriented axis: first tap in coded sample indices, count (clamped to the host's capacity) and the normalised f32
// weights of the display window in coded order.  A mirrored display axis negates the siting offset a.off (the host does) and reflects the window.
__device__ inline void fr_tap_table_m(const FrAxis& a, int first, int R, int mir, int o, int cap, float* w, int& t0c, int& ntc) {
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

}  // namespace
