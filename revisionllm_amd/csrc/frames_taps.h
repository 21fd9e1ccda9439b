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

// Keys' cubic, a = -0.5
__device__ inline double fr_cubic(double x) {
    x = fabs(x);
    if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
    if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
    return 0.0;
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

// Largest span of source rows / columns a tile of t outputs touches.
inline int fr_max_span(const FrAxis& a, int first, int R, int t) {
    int span = 0;
    for (int o0 = 0; o0 < R; o0 += t) {
        const int o1 = (o0 + t < R ? o0 + t : R) - 1;
        int lo, n0, hi, n1;
        fr_axis_taps(a, first + o0, lo, n0);
        fr_axis_taps(a, first + o1, hi, n1);
        if (hi + n1 - lo > span) span = hi + n1 - lo;
    }
    return span;
}

}  // namespace
