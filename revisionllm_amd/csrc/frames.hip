// CLIP front end: decoded uint8 frames -> resize (antialiased bicubic) -> centre crop -> normalise -> patch matrix, one kernel (rv_frames_to_patches).
// What the reference does with Resize(R, BICUBIC) / CenterCrop(R) / Normalize on the decoded tensor (inference.py:108-117) followed by the
// conv1 unfold of VisualTransformer.forward (clip/model.py:223-226).  A bandwidth kernel: no MFMA, the source bytes of the cropped region are read once
// per workgroup tile (neighbouring tiles overlap by the filter support and meet in L2).
//
// One workgroup owns TY x TX output pixels of one frame, all three channels:
//   phase 0  the tile's tap tables (first tap, count, normalised f32 weights; computed in f64) for its TX columns and TY rows into LDS
//   phase 1  per chunk of FR_SR source rows: stage the bytes the tile needs in LDS (16-byte loads where the address allows, single bytes at the
//            ends of a row segment), then the horizontal pass into f32 LDS rows  inter[source row][channel][column]
//   phase 2  vertical pass over inter, normalise, then the tail all front-end kernels share (frames_common.h): store f32 image and / or op16 patch rows, zero
//            the pad columns of the patch rows the tile starts
// Tap counts depend on the geometry (4 * scale + 1 per axis): every tap loop is a runtime loop over LDS-resident weights.  The host picks TY / TX so that
// a workgroup stays under FR_LDS_BUDGET bytes (two workgroups per CU) and refuses a geometry that does not fit with TY = TX = 1.
//
// Display orientation (rv_frames_to_patches_oriented): the kernel is compiled per ORI (0 = none; 1 = mirrors; 2 = transpose, with or without mirrors).  Loads,
// staging and the LDS plan stay in CODED orientation: a coded axis takes the scale, crop offset and mirror flag of the display axis it serves, its tap table
// holds the display window reflected into coded sample indices, and only the store is permuted to image[f, c, yd, xd].
//
// Packed RGB in any byte order (rv_frames_to_patches_packed: bgr24, bgra, argb ...): compiled per PK as well.  The PK = 1 instances are the NHWC path with a
// pixel of 3 or 4 bytes and R, G, B at their own byte offsets inside it; the staged row segment covers the whole pixels, a fourth byte is staged and never read.
//
// Separately allocated frames (rv_frames_to_patches_scattered: a decoder's surface pool, a capture ring): compiled per TAB as well.  A TAB = 1 instance takes
// FrTab - FrParams and, behind it, one base pointer per frame of the launch - and reads its frame's base from that table in the argument segment (the frame
// number is uniform per workgroup: scalar loads) where the TAB = 0 instance computes src + f * fstride.  The host cuts a batch into launches of at most
// RV_FRAME_TABLE_MAX frames.
#include "frames_common.h"   // fp contraction is off from there on

namespace {

struct FrParams {
    const uint8_t* src;
    int64_t fstride, rstride, cstride;   // elements between frames, rows and channels (cstride: 1 for NHWC, frame_stride / 3 for NCHW)
    int pix;                             // elements between neighbouring pixels of a row: 3 (NHWC) or 1 (NCHW)
    int H, W, R, patch, g, K, Kp, top, left;
    double sy, sx;                       // in / out per axis (out = the resized size, before the crop)
    int TY, TX, tilesX, bands;
    int NTX, NTXp, NTY, NR, SEGPX, SEG;  // tap capacities, rows of inter, pixels / bytes (16-byte multiple + 16) of a staged row segment
    int o_wv, o_idx, o_inter, o_stage;   // LDS offsets (wh sits at 0)
    float mean[3], den[3];
    op16_t* patches;
    int64_t ldp;
    float* image;
    int mirx, miry;                      // the coded x / y axis is mirrored (read by the oriented instances only)
    int off[3];                          // PK = 1 instances only: byte offsets of R, G, B inside a pixel of `pix` bytes
};

// The argument block of the TAB = 1 instances: the frames of one launch lie where the table says (NCHW channel planes p.cstride apart; p.src / p.fstride unused).
struct FrTab : FrParams {
    const uint8_t* tab[RV_FRAME_TABLE_MAX];
};
template <int TAB>
using FrArgs = std::conditional_t<TAB != 0, FrTab, FrParams>;

template <int ORI, int PK, int TAB>
__global__ __launch_bounds__(FR_THREADS) void frames_to_patches_kernel(const FrArgs<TAB> p) {
    extern __shared__ __attribute__((aligned(16))) char fr_smem[];
    float* wh = (float*)fr_smem;                       // [TX][NTXp]
    float* wv = (float*)(fr_smem + p.o_wv);            // [TY][NTY]
    int* xmin = (int*)(fr_smem + p.o_idx);             // [TX], then nx [TX], ymin [TY], ny [TY]
    int* nx = xmin + p.TX;
    int* ymin = nx + p.TX;
    int* ny = ymin + p.TY;
    float* inter = (float*)(fr_smem + p.o_inter);      // [NR][3][TX]
    uint8_t* stage = (uint8_t*)(fr_smem + p.o_stage);  // [planes][FR_SR][SEG]
    const int tid = threadIdx.x;
    uint32_t b = blockIdx.x;
    const int tile = b % p.tilesX;
    b /= p.tilesX;
    const int band = b % p.bands;
    const int64_t f = b / p.bands;
    const int y0 = band * p.TY, x0 = tile * p.TX;
    const int ty = min(p.TY, p.R - y0), tx = min(p.TX, p.R - x0);

    // ---- phase 0: tap tables --------------------------------------------------------------------------------------------------
    for (int i = tid; i < tx + ty; i += FR_THREADS) {
        const bool isx = i < tx;
        const int o = isx ? i : i - tx;
        const int mir = ORI == 0 ? 0 : isx ? p.mirx : p.miry;
        fr_tap_table(FrAxis{isx ? p.sx : p.sy, 1.0, 0.0, isx ? p.W : p.H}, isx ? p.left : p.top, p.R, mir, (isx ? x0 : y0) + o, isx ? p.NTX : p.NTY,
                     isx ? wh + o * p.NTXp : wv + o * p.NTY, (isx ? xmin : ymin)[o], (isx ? nx : ny)[o]);
    }
    __syncthreads();
    const int rmin = ymin[0], cmin = xmin[0];
    const int nrows = min(ymin[ty - 1] + ny[ty - 1] - rmin, p.NR);
    const int segpx = min(xmin[tx - 1] + nx[tx - 1] - cmin, p.SEGPX);
    const int segbytes = segpx * p.pix;
    const int planes = PK ? 1 : p.pix == 1 ? 3 : 1;
    const int nck = p.SEG >> 4;
    const uint8_t* fsrc;
    if constexpr (TAB != 0) fsrc = p.tab[f] + (int64_t)cmin * p.pix;
    else fsrc = p.src + f * p.fstride + (int64_t)cmin * p.pix;

    // ---- phase 1: stage source bytes, horizontal pass ---------------------------------------------------------------------------
    for (int r0 = 0; r0 < nrows; r0 += FR_SR) {
        const int nr = min(FR_SR, nrows - r0);
        __syncthreads();   // the previous chunk's readers are done with `stage`
        for (int it = tid; it < nr * planes * nck; it += FR_THREADS) {
            const int k = it % nck, rr = it / nck;
            const int r = rr % nr, pl = rr / nr;
            const uint8_t* gs = fsrc + pl * p.cstride + (int64_t)(rmin + r0 + r) * p.rstride;
            const uint8_t* ge = gs + segbytes;
            const uint8_t* gc = (const uint8_t*)((uintptr_t)gs & ~(uintptr_t)15) + 16 * k;   // the segment keeps its position inside a 16-byte line
            uint8_t* d = stage + (pl * FR_SR + r) * p.SEG + 16 * k;
            if (gc >= gs && gc + 16 <= ge) {
                *(uint4*)d = *(const uint4*)gc;
            } else if (gc + 16 > gs && gc < ge) {
                for (int j = 0; j < 16; ++j)
                    if (gc + j >= gs && gc + j < ge) d[j] = gc[j];
            }
        }
        __syncthreads();
        for (int it = tid; it < nr * tx; it += FR_THREADS) {
            const int col = it % tx, r = it / tx;
            const uint8_t* gs = fsrc + (int64_t)(rmin + r0 + r) * p.rstride;
            const int xo = (xmin[col] - cmin) * p.pix;
            const uint8_t *s0, *s1, *s2;
            if constexpr (PK) {
                const uint8_t* px = stage + r * p.SEG + (int)((uintptr_t)gs & 15) + xo;
                s0 = px + p.off[0];
                s1 = px + p.off[1];
                s2 = px + p.off[2];
            } else if (planes == 1) {
                s0 = stage + r * p.SEG + (int)((uintptr_t)gs & 15) + xo;
                s1 = s0 + 1;
                s2 = s0 + 2;
            } else {
                s0 = stage + r * p.SEG + (int)((uintptr_t)gs & 15) + xo;
                s1 = stage + (FR_SR + r) * p.SEG + (int)((uintptr_t)(gs + p.cstride) & 15) + xo;
                s2 = stage + (2 * FR_SR + r) * p.SEG + (int)((uintptr_t)(gs + 2 * p.cstride) & 15) + xo;
            }
            const float* w = wh + col * p.NTXp;
            const int n = min(nx[col], segpx - (xmin[col] - cmin));
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            for (int t = 0; t < n; ++t) {
                const float wt = w[t];
                const int o = t * p.pix;
                a0 = fmaf(wt, (float)s0[o], a0);
                a1 = fmaf(wt, (float)s1[o], a1);
                a2 = fmaf(wt, (float)s2[o], a2);
            }
            float* q = inter + (r0 + r) * 3 * p.TX + col;
            q[0] = a0;
            q[p.TX] = a1;
            q[2 * p.TX] = a2;
        }
    }
    __syncthreads();

    // ---- phase 2: vertical pass, normalise, store --------------------------------------------------------------------------------
    for (int it = tid; it < ty * 3 * tx; it += FR_THREADS) {
        const int col = it % tx, c = (it / tx) % 3, yy = it / (3 * tx);
        const int rb = ymin[yy] - rmin;
        const int n = min(ny[yy], nrows - rb);
        const float* w = wv + yy * p.NTY;
        const float* q = inter + (rb * 3 + c) * p.TX + col;
        float acc = 0.f;
        for (int t = 0; t < n; ++t) acc = fmaf(w[t], q[t * 3 * p.TX], acc);
        const float v = (acc / 255.0f - (c == 0 ? p.mean[0] : c == 1 ? p.mean[1] : p.mean[2])) / (c == 0 ? p.den[0] : c == 1 ? p.den[1] : p.den[2]);
        fr_store<ORI>(p, f, c, y0 + yy, x0 + col, v);
    }
    fr_zero_pad<ORI>(p, f, y0, ty, x0, tx, tid);
}

int fr_stage_bytes(const FrParams& p) { return (p.pix == 1 ? 3 : 1) * FR_SR * p.SEG; }

// Tile plan: capacities from the exact tap placement of the crop's rows and columns (the kernel clamps to them all the same); false = over the LDS budget.
bool fr_plan(FrParams& p, int ty, int tx, double& cost) {
    p.TY = ty;
    p.TX = tx;
    p.tilesX = (p.R + tx - 1) / tx;
    p.bands = (p.R + ty - 1) / ty;
    p.NR = fr_max_span(FrAxis{p.sy, 1.0, 0.0, p.H}, p.top, p.R, ty, p.miry);
    p.SEGPX = fr_max_span(FrAxis{p.sx, 1.0, 0.0, p.W}, p.left, p.R, tx, p.mirx);
    p.SEG = ((p.SEGPX * p.pix + 15) & ~15) + 16;
    int64_t o = (int64_t)tx * p.NTXp * 4;
    p.o_wv = (int)o;
    o += (int64_t)ty * p.NTY * 4;
    p.o_idx = (int)o;
    o += (int64_t)(2 * tx + 2 * ty) * 4;
    o = (o + 15) & ~(int64_t)15;
    p.o_inter = (int)o;
    o += (int64_t)p.NR * 3 * tx * 4;
    o = (o + 15) & ~(int64_t)15;
    p.o_stage = (int)o;
    o += fr_stage_bytes(p);
    if (o > FR_LDS_BUDGET) return false;
    // source rows the horizontal pass computes per output row, plus the (cheaper) bytes staged per output pixel
    cost = (double)p.NR / ty * (3.0 + (double)p.SEGPX / (tx * (p.sx > 1.0 ? p.sx : 1.0)));
    return true;
}

// One launch of the instance for orientation class oc and pixel form pk (1: packed RGB), on the contiguous block (FrParams) or the table form (FrTab).
template <class Args>
int fr_dispatch(int oc, int pk, const Args& a, int64_t wgs, int lds, void* stream, const char* who) {
    return fr_pick<3>(oc, [&](auto ORI) {
        return fr_pick<2>(pk, [&](auto PK) {
            return fr_launch<frames_to_patches_kernel<decltype(ORI)::value, decltype(PK)::value, std::is_same_v<Args, FrTab>>>(a, wgs, lds, stream, who, "frames_to_patches");
        });
    });
}

// The packed entries' pixel: 3 or 4 bytes, R, G, B at distinct byte offsets inside it.
int fr_check_pixel(int32_t pix_bytes, int32_t r_off, int32_t g_off, int32_t b_off, const char* who) {
    RV_CHECK_ARG(pix_bytes == 3 || pix_bytes == 4, "%s: pix_bytes = %d (3, or 4 = a fourth byte that is never read)", who, pix_bytes);
    RV_CHECK_ARG(r_off >= 0 && g_off >= 0 && b_off >= 0 && r_off < pix_bytes && g_off < pix_bytes && b_off < pix_bytes && r_off != g_off && r_off != b_off &&
                     g_off != b_off,
                 "%s: r_off, g_off, b_off = %d, %d, %d (three distinct byte offsets inside the %d-byte pixel)", who, r_off, g_off, b_off, pix_bytes);
    return RV_OK;
}

// All entry points: validate, plan the tiles, launch.  `who` names the entry point in the messages; orient is validated by the caller (0 for the un-oriented
// entry).  off: null, or the packed entry's R, G, B byte offsets inside a pixel of pix_bytes bytes (layout is 1 then).  tab: the scattered entry's host array of n
// frame pointers (frames is null and frame_stride 3 * channel_stride then), else null.
int fr_run(const uint8_t* frames, const uint8_t* const* tab, int layout, int pix_bytes, const int32_t* off, int64_t frame_stride, int64_t row_stride, int32_t n, int32_t H, int32_t W,
           int32_t orient, int32_t R, int32_t patch, const float* mean, const float* std, void* patches, int64_t ldp, float* image, void* stream, const char* who) {
    RV_CHECK_ARG(layout == 0 || layout == 1, "%s: layout %d (0 = NCHW, 1 = NHWC)", who, layout);
    const int rc = fr_check_common(
        R, patch, n, mean, std, patches, ldp, image, who,
        [&]() -> int {
            RV_CHECK_ARG(H >= 1 && W >= 1 && H <= FR_MAX_SIDE && W <= FR_MAX_SIDE, "%s: frame size %d x %d outside 1 .. %d", who, H, W, FR_MAX_SIDE);
            return RV_OK;
        },
        [&]() -> int {
            RV_CHECK_ARG(frames || tab, "%s: null frames", who);
            if (tab)   // the whole table before anything is launched
                for (int32_t f = 0; f < n; ++f) RV_CHECK_ARG(tab[f], "%s: null pointer for frame %d of %d", who, f, n);
            return RV_OK;
        });
    if (rc || n == 0) return rc;
    RV_CHECK_ARG(layout == 1 || frame_stride % 3 == 0, "%s: NCHW channel planes lie frame_stride / 3 apart; frame_stride = %lld", who, (long long)frame_stride);
    FrParams p{};
    p.src = frames;
    p.fstride = frame_stride;
    p.rstride = row_stride;
    p.cstride = layout == 1 ? 1 : frame_stride / 3;
    p.pix = layout == 1 ? pix_bytes : 1;
    if (off)
        for (int c = 0; c < 3; ++c) p.off[c] = off[c];
    p.H = H;
    p.W = W;
    fr_setup(p, H, W, orient, R, patch, mean, std, patches, ldp, image, p.sy, p.sx);
    p.NTX = fr_max_taps(FrAxis{p.sx, 1.0, 0.0, W}, p.left, R);
    p.NTXp = p.NTX | 1;   // odd row pitch: the columns' weight rows start in different banks
    p.NTY = fr_max_taps(FrAxis{p.sy, 1.0, 0.0, H}, p.top, R);
    FrParams best{};
    RV_CHECK_ARG(fr_best_plan(p, R, fr_plan, best), "%s: %d x %d -> %d needs more filter taps than a workgroup's LDS holds", who, H, W, R);
    const int lds = best.o_stage + fr_stage_bytes(best), oc = fr_orient_class(orient);
    return fr_launch_all<FrTab>(
        best, [](auto& a) -> auto& { return a; }, tab, n, [&](const auto& a, int64_t wgs) { return fr_dispatch(oc, off != nullptr, a, wgs, lds, stream, who); }, who);
}

}  // namespace

extern "C" int rv_frames_to_patches(const uint8_t* frames, int layout, int64_t frame_stride, int64_t row_stride, int32_t n, int32_t H, int32_t W,
                                    int32_t R, int32_t patch, const float mean[3], const float std[3], void* patches, int64_t ldp, float* image,
                                    void* stream) {
    return fr_run(frames, nullptr, layout, 3, nullptr, frame_stride, row_stride, n, H, W, 0, R, patch, mean, std, patches, ldp, image, stream, "rv_frames_to_patches");
}

// The same front end on the picture as it is displayed: H, W and the strides describe the coded frames, orient (0 .. 7) turns and flips them.
extern "C" int rv_frames_to_patches_oriented(const uint8_t* frames, int layout, int64_t frame_stride, int64_t row_stride, int32_t n, int32_t H, int32_t W,
                                             int32_t orient, int32_t R, int32_t patch, const float mean[3], const float std[3], void* patches, int64_t ldp,
                                             float* image, void* stream) {
    const char* who = "rv_frames_to_patches_oriented";
    if (const int rc = fr_check_orient(orient, who)) return rc;
    return fr_run(frames, nullptr, layout, 3, nullptr, frame_stride, row_stride, n, H, W, orient, R, patch, mean, std, patches, ldp, image, stream, who);
}

// Packed 8-bit RGB in any byte order, 3 or 4 bytes per pixel: the oriented NHWC entry with the channels at their own offsets inside the pixel.
extern "C" int rv_frames_to_patches_packed(const uint8_t* frames, int32_t pix_bytes, int32_t r_off, int32_t g_off, int32_t b_off, int64_t frame_stride,
                                           int64_t row_stride, int32_t n, int32_t H, int32_t W, int32_t orient, int32_t R, int32_t patch, const float mean[3],
                                           const float std[3], void* patches, int64_t ldp, float* image, void* stream) {
    const char* who = "rv_frames_to_patches_packed";
    if (const int rc = fr_check_pixel(pix_bytes, r_off, g_off, b_off, who)) return rc;
    if (const int rc = fr_check_orient(orient, who)) return rc;
    const int32_t off[3] = {r_off, g_off, b_off};
    return fr_run(frames, nullptr, 1, pix_bytes, off, frame_stride, row_stride, n, H, W, orient, R, patch, mean, std, patches, ldp, image, stream, who);
}

// The packed / oriented entries on separately allocated frames: frames[f] is where frame f lies; every other argument is shared (the header has the rules).
extern "C" int rv_frames_to_patches_scattered(const uint8_t* const* frames, int layout, int32_t pix_bytes, int32_t r_off, int32_t g_off, int32_t b_off,
                                              int64_t channel_stride, int64_t row_stride, int32_t n, int32_t H, int32_t W, int32_t orient, int32_t R, int32_t patch,
                                              const float mean[3], const float std[3], void* patches, int64_t ldp, float* image, void* stream) {
    const char* who = "rv_frames_to_patches_scattered";
    RV_CHECK_ARG(layout == 0 || layout == 1, "%s: layout %d (0 = NCHW, 1 = packed pixels)", who, layout);
    if (const int rc = fr_check_orient(orient, who)) return rc;
    const int32_t off[3] = {r_off, g_off, b_off};
    if (layout == 0) {
        RV_CHECK_ARG(pix_bytes == 3 && r_off == 0 && g_off == 1 && b_off == 2, "%s: layout 0 (NCHW) takes pix_bytes 3 and offsets 0, 1, 2; got %d and %d, %d, %d", who,
                     pix_bytes, r_off, g_off, b_off);
        return fr_run(nullptr, frames, 0, 3, nullptr, 3 * channel_stride, row_stride, n, H, W, orient, R, patch, mean, std, patches, ldp, image, stream, who);
    }
    if (const int rc = fr_check_pixel(pix_bytes, r_off, g_off, b_off, who)) return rc;
    return fr_run(nullptr, frames, 1, pix_bytes, off, 0, row_stride, n, H, W, orient, R, patch, mean, std, patches, ldp, image, stream, who);
}
