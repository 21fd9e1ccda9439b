// CLIP front end on the bytes a video decoder hands over: YCbCr planes of 8-bit or 16-bit samples, 4:2:0 / 4:2:2 / 4:4:4, planar or with interleaved chroma
// (NV12 / NV21 / I420, P010 / P016, yuv420p10le, nv16, yuv444p10le ...: rv_yuv_surface) -> resize (antialiased bicubic) -> YCbCr -> RGB -> centre crop ->
// normalise -> patch matrix, one kernel (rv_yuv_surface_to_patches; rv_yuv_to_patches is the same code on an 8-bit 4:2:0 surface).  No RGB frame exists
// anywhere: resampling is linear and the colour conversion affine, so the kernel filters Y at full and Cb / Cr at their own resolution and applies the colour
// matrix once per OUTPUT pixel.
//
// The values below are those of the 8-bit 4:2:0 surface; include/revision_hip.h has the general definition (sample = word >> (16 - depth) when the value sits
// in the high bits; per axis in_c = in / sub, scale_c = scale / sub, off = 0.25 where a subsampled axis is sited on the even luma sample; s = 2^(depth - 8)
// scales 16, 128, 219, 224, and full range divides by 2^depth - 1).
//
// Values (f32 throughout, no clamp, no u8 intermediate); i = an output index of the RESIZED image (before the crop), scale = in / out per axis, the resized
// size and the crop offsets are rv_frames_to_patches' own:
//   luma     Y' = rv_frames_to_patches' resampling of the Y plane: the same taps, the same normalised f32 weights (computed in f64)
//   chroma   Cb', Cr' = the same filter in chroma-plane coordinates: in_c = in / 2, scale_c = scale / 2, centre_c = scale * (i + 0.5) / 2 + off with
//            off = 0.25 on the horizontal axis for chroma_loc 0 (left: MPEG-2 / H.264), else 0 (both sitings are vertically centred);
//            support_c = 2 * max(scale_c, 1), taps [max(0, int(centre_c - support_c + 0.5)), min(in_c, int(centre_c + support_c + 0.5))), weight
//            cubic((j - centre_c + 0.5) / max(scale_c, 1)) / (sum over the taps).  scale_c < 1 (a source below 2R per axis) interpolates chroma.
//   colour   Kr, Kb = 0.299, 0.114 (BT.601) or 0.2126, 0.0722 (BT.709), Kg = 1 - Kr - Kb;
//            studio range: yl = (Y' - 16) * 255 / 219, c = (C' - 128) * 255 / 224; full range: yl = Y', c = C' - 128;
//            Rv = yl + 2 (1 - Kr) cr,  Bv = yl + 2 (1 - Kb) cb,  Gv = yl - (2 Kb (1 - Kb) / Kg) cb - (2 Kr (1 - Kr) / Kg) cr;
//            the five coefficients (255 / 219 and the four chroma factors with 255 / 224 folded in) are computed on the host in f64 and rounded once to f32
//   norm     (v / 255 - mean[c]) / (std[c] + 1e-8); image and patches laid out, rounded and zero-padded as by rv_frames_to_patches
// This is the project's OWN definition: the chroma planes are resampled directly, which is linear and exact.  It is NOT swscale's integer conversion to
// rgb24 followed by a resize, and no parity with ffmpeg's RGB bytes is claimed.
//
//
// HDR surfaces (rv_yuv_surface_to_patches_hdr): PQ- or HLG-coded BT.2100 values are converted to SDR BT.709-coded values per OUTPUT pixel, between the colour
// matrix and the normalisation.  The library's own definition again (include/revision_hip.h has it in full); E'c = v[c] / 255 with no clamp up to here:
//   1 clamp    E' = clamp(E'c, 0, 1) per channel
//   2 transfer to display light F in nits, Lw = peak_nits
//              PQ (ST 2084)  m1 = 2610/16384, m2 = 2523/4096*128, c1 = 3424/4096, c2 = 2413/4096*32, c3 = 2392/4096*32; p = E'^(1/m2);
//                            F = 10000 (max(p - c1, 0) / (c2 - c3 p))^(1/m1), clamped to [0, Lw]
//              HLG (B67)     a = 0.17883277, b = 1 - 4a, c = 0.5 - a ln(4a); scene light E = E'^2 / 3 for E' <= 0.5, else (exp((E' - c) / a) + b) / 12;
//                            Ys = 0.2627 Er + 0.6780 Eg + 0.0593 Eb; gamma = 1.2 + 0.42 log10(Lw / 1000); F = Lw Ys^(gamma - 1) E, 0 where Ys = 0
//   3 tone map BT.2390 EETF on the brightest channel, black level 0, Lt = sdr_white_nits; PQinv(Y) = ((c1 + c2 y) / (1 + c3 y))^m2, y = (Y / 10000)^m1;
//              mx = max(Fr, Fg, Fb), e = PQinv(mx) / PQinv(Lw), maxLum = PQinv(Lt) / PQinv(Lw), KS = 1.5 maxLum - 0.5; ratio = 1 when KS >= 1, e <= KS or
//              mx = 0; else t = (e - KS) / (1 - KS), e2 = (2t^3 - 3t^2 + 1) KS + (t^3 - 2t^2 + t)(1 - KS) + (-2t^3 + 3t^2) maxLum,
//              ratio = PQ_EOTF(e2 PQinv(Lw)) / mx; L = F ratio / Lt per channel
//   4 gamut    gamut = 1: BT.2087's BT.2020 -> BT.709 matrix (1.6605 -0.5876 -0.0728 / -0.1246 1.1329 -0.0083 / -0.0182 -0.1006 1.1187), gamut = 0: none;
//              then clamp to [0, 1]
//   5 OETF     BT.709's, with its linear toe: V = 4.5 L for L < 0.018, else 1.099 L^0.45 - 0.099; v[c] = 255 V
// Powers are exp2f(k * log2f(x)); constants that are quotients are evaluated in f64 and rounded once to f32; the scalars that depend on peak_nits /
// sdr_white_nits (1 / Lt, PQinv(Lw), maxLum, KS, gamma - 1) are computed on the host in f64.  No dynamic metadata is read; peak_nits is the caller's number.
//
// The kernel follows frames_to_patches_kernel.  One workgroup owns TY x TX output pixels of one frame:
//   phase 0  four tap tables (luma x / y, chroma x / y: first tap, count, normalised f32 weights; computed in f64) into LDS
//   phase 1  per chunk of FR_SR source rows, first of the Y plane, then of the chroma planes: stage the bytes the tile needs in LDS (16-byte loads where the
//            address allows, single samples at the ends of a row segment; an interleaved chroma segment holds both planes), then the horizontal pass into
//            f32 LDS rows  interY[source row][column],  interC[chroma row][Cb | Cr][column]
//   phase 2  vertical pass over both, then fy_colour_store: colour matrix, HDR steps, normalise, and the tail all front-end kernels share (frames_common.h) -
//            store f32 image and / or op16 patch rows, zero the pad columns of the patch rows the tile starts
// At 4:2:0: half the horizontal-pass work of three RGB planes (one full plane + two quarter planes filtered with half the taps), and two thirds of its
// `inter` rows.  The kernel is compiled per sample type (uint8_t; uint16_t with a run-time shift) and per transfer (TRC: 0 = none, 1 = PQ, 2 = HLG): the HDR
// steps exist in the HDR instances only.
//
// Display orientation (rv_yuv_surface_to_patches_oriented; include/revision_hip.h has the definition): compiled per ORI as well (0 = none; 1 = mirrors;
// 2 = transpose, with or without mirrors).  Loads, staging and the LDS plan stay in CODED orientation.  Every coded axis takes the scale and
// crop offset of the display axis it serves and a mirror flag; the chroma siting offset stays with its coded axis and changes sign where that axis is
// mirrored; a tap table holds the display window reflected into coded sample indices; only the store is permuted to image[f, c, yd, xd].  So a 4:2:2
// surface turned by 90 degrees (4:4:0 on the display) is still the 2,1 surface it was coded as.
//
// Packed surfaces (rv_packed_to_patches: YUY2 / UYVY / Y210, AYUV / VUYA / Y410 / XV36 ...) have a kernel of their own behind the planar one, packed_to_patches_kernel:
// one staged segment per source row serves the Y, Cb and Cr passes; its section has the layout.  Phases 0 and 2 are the planar kernel's routines.
//
// Separately allocated surfaces (rv_yuv_surfaces_to_patches, rv_packed_surfaces_to_patches: a decoder's surface pool): both kernels are compiled per TAB as well.
// A TAB = 1 instance takes FyTab / FkTab - FyParams / FkParams and, behind them, the plane pointers of every frame of the launch - and reads its frame's base
// pointers from that table in the argument segment (the frame number is uniform per workgroup: scalar loads) where the TAB = 0 instance computes base + f *
// frame stride.  Planar Cr - Cb comes from the table too: it may differ from frame to frame.  The host cuts a batch into launches of at most RV_FRAME_TABLE_MAX
// frames.
#include "frames_common.h"   // fp contraction is off from there on

namespace {

struct FyParams {
    const uint8_t *y, *c;                 // c: the Cb plane (planar) or the lower of the two interleaved planes
    int64_t yfs, yrs, cfs, crs, cdelta;   // bytes between frames / rows of the Y and the chroma planes; cdelta: Cr plane - Cb plane (planar)
    int cpix, ocb, ocr;                   // bytes between neighbouring samples of a chroma plane; byte offsets of Cb / Cr inside an interleaved pair (planar: 0)
    int sbytes, cplanes, shift;           // bytes of a sample; planes staged apart (planar: 2, interleaved: 1); 16-bit words: sample = word >> shift
    int R, patch, g, K, Kp, top, left;
    FrAxis ax, ay, cx, cy;                // luma and chroma axes
    int TY, TX, tilesX, bands;
    int NTX, NTXp, NTY, NCX, NCXp, NCY;   // tap capacities (x rows padded to an odd pitch)
    int NRY, NRC, SPY, SPC, SEGY, SEGC;   // rows of interY / interC, samples / bytes (16-byte multiple + 16) of a staged luma / chroma row segment
    int o_wy, o_cwx, o_cwy, o_idx, o_iy, o_ic, o_stage;   // LDS offsets (the luma x weights sit at 0)
    float yoff, cmid, ky, krcr, kgcb, kgcr, kbcb;   // cmid: the chroma zero, 128 * 2^(depth - 8)
    float mean[3], den[3];
    op16_t* patches;
    int64_t ldp;
    float* image;
    // HDR instances only: Lw, 1 / Lt, PQinv(Lw), maxLum, KS, gamma - 1, the gamut matrix by rows (or the identity)
    float Lw, rLt, pqLw, maxLum, KS, gm1, gam[9];
    int mirx, miry;   // the coded x / y axis is mirrored (read by the oriented instances only)
};

// ---- HDR -> SDR per output pixel (the head of the file has the definition) ---------------------------------------------------------------------------
constexpr int FY_TRC_NONE = 0, FY_TRC_PQ = 1, FY_TRC_HLG = 2;
constexpr double PQ_M1_D = 2610.0 / 16384.0, PQ_M2_D = 2523.0 / 4096.0 * 128.0, PQ_C1_D = 3424.0 / 4096.0, PQ_C2_D = 2413.0 / 4096.0 * 32.0,
                 PQ_C3_D = 2392.0 / 4096.0 * 32.0;
constexpr float PQ_M1 = (float)PQ_M1_D, PQ_M2 = (float)PQ_M2_D, PQ_RM1 = (float)(1.0 / PQ_M1_D), PQ_RM2 = (float)(1.0 / PQ_M2_D), PQ_C1 = (float)PQ_C1_D,
                PQ_C2 = (float)PQ_C2_D, PQ_C3 = (float)PQ_C3_D;
constexpr double HLG_A_D = 0.17883277, HLG_B_D = 1.0 - 4.0 * HLG_A_D, HLG_LN4A_D = -0.3350097945111627;   // ln(4a)
constexpr float HLG_B = (float)HLG_B_D, HLG_C = (float)(0.5 - HLG_A_D * HLG_LN4A_D), HLG_K = (float)(1.4426950408889634 / HLG_A_D);   // log2(e) / a

// x^k, x >= 0 and k > 0 (0 -> 0: log2f gives -inf, exp2f of it 0)
__device__ inline float fy_pow(float x, float k) { return exp2f(k * log2f(x)); }

// ST 2084: code value in [0, 1] -> nits, and back
__device__ inline float fy_pq_eotf(float e) {
    const float p = fy_pow(e, PQ_RM2);
    return 10000.0f * fy_pow(fmaxf(p - PQ_C1, 0.0f) / (PQ_C2 - PQ_C3 * p), PQ_RM1);
}
__device__ inline float fy_pq_inv(float nits) {
    const float y = fy_pow(nits / 10000.0f, PQ_M1);
    return fy_pow((PQ_C1 + PQ_C2 * y) / (1.0f + PQ_C3 * y), PQ_M2);
}

// Steps 1 to 5 on the three values of one output pixel, in place (v / 255 = E'c on entry, the BT.709-coded SDR value on exit).
template <int TRC>
__device__ inline void fy_hdr_to_sdr(float v[3], const FyParams& p) {
    float F[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) F[c] = fminf(fmaxf(v[c] / 255.0f, 0.0f), 1.0f);
    if (TRC == FY_TRC_PQ) {
#pragma unroll
        for (int c = 0; c < 3; ++c) F[c] = fminf(fmaxf(fy_pq_eotf(F[c]), 0.0f), p.Lw);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) F[c] = F[c] <= 0.5f ? F[c] * F[c] / 3.0f : (exp2f((F[c] - HLG_C) * HLG_K) + HLG_B) / 12.0f;
        const float ys = 0.2627f * F[0] + 0.6780f * F[1] + 0.0593f * F[2];
        const float sys = ys > 0.0f ? p.Lw * fy_pow(ys, p.gm1) : 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) F[c] = sys * F[c];
    }
    const float mx = fmaxf(F[0], fmaxf(F[1], F[2]));
    float ratio = 1.0f;
    if (p.KS < 1.0f && mx > 0.0f) {
        const float e = fy_pq_inv(mx) / p.pqLw;
        if (e > p.KS) {
            const float omk = 1.0f - p.KS, t = (e - p.KS) / omk, t2 = t * t, t3 = t2 * t;
            const float e2 = (2.0f * t3 - 3.0f * t2 + 1.0f) * p.KS + (t3 - 2.0f * t2 + t) * omk + (-2.0f * t3 + 3.0f * t2) * p.maxLum;
            ratio = fy_pq_eotf(e2 * p.pqLw) / mx;
        }
    }
    float L[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) L[c] = F[c] * ratio * p.rLt;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float l = fminf(fmaxf(p.gam[3 * c] * L[0] + p.gam[3 * c + 1] * L[1] + p.gam[3 * c + 2] * L[2], 0.0f), 1.0f);
        v[c] = 255.0f * (l < 0.018f ? 4.5f * l : 1.099f * fy_pow(l, 0.45f) - 0.099f);
    }
}

// Stage `nr` rows of `planes` planes: the `segbytes` bytes from `g0` on (row r of plane pl: g0 + pl * pdelta + r * rstride) into stage[(pl * FR_SR + r) * SEG ..],
// each segment keeping its position inside a 16-byte line.  Reads [segment start, segment end) and nothing else: whole 16-byte lines inside it, single
// samples of type S (segments start and end on a sample) at its two ends.
template <typename S>
__device__ inline void fy_stage(uint8_t* stage, const uint8_t* g0, int64_t pdelta, int64_t rstride, int planes, int nr, int segbytes, int SEG, int tid) {
    const int nck = SEG >> 4;
    for (int it = tid; it < nr * planes * nck; it += FR_THREADS) {
        const int k = it % nck, rr = it / nck;
        const int r = rr % nr, pl = rr / nr;
        const uint8_t* gs = g0 + pl * pdelta + (int64_t)r * rstride;
        const uint8_t* ge = gs + segbytes;
        const uint8_t* gc = (const uint8_t*)((uintptr_t)gs & ~(uintptr_t)15) + 16 * k;
        uint8_t* d = stage + (pl * FR_SR + r) * SEG + 16 * k;
        if (gc >= gs && gc + 16 <= ge) {
            *(uint4*)d = *(const uint4*)gc;
        } else if (gc + 16 > gs && gc < ge) {
            for (int j = 0; j < 16; j += (int)sizeof(S))
                if (gc + j >= gs && gc + j < ge) *(S*)(d + j) = *(const S*)(gc + j);
        }
    }
}

// Phase 2 of both kernels, behind the vertical pass: the resampled Y', Cb', Cr' of coded output (y, x) of frame f -> colour matrix, the HDR steps of the HDR
// instances, normalise, store (fr_store has the display permutation).
template <int TRC, int ORI>
__device__ inline void fy_colour_store(const FyParams& p, float yv, float cb, float cr, int64_t f, int y, int x) {
    const float yl = (yv - p.yoff) * p.ky;
    cb -= p.cmid;
    cr -= p.cmid;
    float v[3];
    v[0] = fmaf(p.krcr, cr, yl);
    v[1] = fmaf(p.kgcr, cr, fmaf(p.kgcb, cb, yl));
    v[2] = fmaf(p.kbcb, cb, yl);
    if constexpr (TRC != FY_TRC_NONE) fy_hdr_to_sdr<TRC>(v, p);
#pragma unroll
    for (int c = 0; c < 3; ++c) fr_store<ORI>(p, f, c, y, x, (v[c] / 255.0f - p.mean[c]) / p.den[c]);
}

// The argument block of the TAB = 1 planar instances: the planes of frame f of one launch lie where tab[f] says (p.y / p.c / p.yfs / p.cfs / p.cdelta unused).
struct FyTab : FyParams {
    rv_surface_planes tab[RV_FRAME_TABLE_MAX];
};
template <int TAB>
using FyArgs = std::conditional_t<TAB != 0, FyTab, FyParams>;

template <typename S, int TRC, int ORI, int TAB>
__global__ __launch_bounds__(FR_THREADS) void yuv_to_patches_kernel(const FyArgs<TAB> p) {
    extern __shared__ __attribute__((aligned(16))) char fy_smem[];
    float* wx = (float*)fy_smem;                       // [TX][NTXp]
    float* wy = (float*)(fy_smem + p.o_wy);            // [TY][NTY]
    float* cwx = (float*)(fy_smem + p.o_cwx);          // [TX][NCXp]
    float* cwy = (float*)(fy_smem + p.o_cwy);          // [TY][NCY]
    int* xmin = (int*)(fy_smem + p.o_idx);             // [TX], then nx, cxmin, cnx [TX], ymin, ny, cymin, cny [TY]
    int* nx = xmin + p.TX;
    int* cxmin = nx + p.TX;
    int* cnx = cxmin + p.TX;
    int* ymin = cnx + p.TX;
    int* ny = ymin + p.TY;
    int* cymin = ny + p.TY;
    int* cny = cymin + p.TY;
    float* iy = (float*)(fy_smem + p.o_iy);            // [NRY][TX]
    float* ic = (float*)(fy_smem + p.o_ic);            // [NRC][2][TX]
    uint8_t* stage = (uint8_t*)(fy_smem + p.o_stage);  // [planes][FR_SR][SEG]
    const int tid = threadIdx.x;
    uint32_t b = blockIdx.x;
    const int tile = b % p.tilesX;
    b /= p.tilesX;
    const int band = b % p.bands;
    const int64_t f = b / p.bands;
    const int y0 = band * p.TY, x0 = tile * p.TX;
    const int ty = min(p.TY, p.R - y0), tx = min(p.TX, p.R - x0);

    // ---- phase 0: tap tables --------------------------------------------------------------------------------------------------
    const int mirx = ORI == 0 ? 0 : p.mirx, miry = ORI == 0 ? 0 : p.miry;
    for (int i = tid; i < 2 * (tx + ty); i += FR_THREADS) {
        int o = i;
        if (o < tx) fr_tap_table(p.ax, p.left, p.R, mirx, x0 + o, p.NTX, wx + o * p.NTXp, xmin[o], nx[o]);
        else if ((o -= tx) < tx) fr_tap_table(p.cx, p.left, p.R, mirx, x0 + o, p.NCX, cwx + o * p.NCXp, cxmin[o], cnx[o]);
        else if ((o -= tx) < ty) fr_tap_table(p.ay, p.top, p.R, miry, y0 + o, p.NTY, wy + o * p.NTY, ymin[o], ny[o]);
        else o -= ty, fr_tap_table(p.cy, p.top, p.R, miry, y0 + o, p.NCY, cwy + o * p.NCY, cymin[o], cny[o]);
    }
    __syncthreads();

    // ---- phase 1a: luma - stage source bytes, horizontal pass ---------------------------------------------------------------------
    const int rmin = ymin[0], cmin = xmin[0];
    const int nrows = min(ymin[ty - 1] + ny[ty - 1] - rmin, p.NRY);
    const int segpx = min(xmin[tx - 1] + nx[tx - 1] - cmin, p.SPY);
    constexpr int SB = (int)sizeof(S);
    const uint8_t* ysrc;
    if constexpr (TAB != 0) ysrc = (const uint8_t*)p.tab[f].y + (int64_t)rmin * p.yrs + (int64_t)cmin * SB;
    else ysrc = p.y + f * p.yfs + (int64_t)rmin * p.yrs + (int64_t)cmin * SB;
    for (int r0 = 0; r0 < nrows; r0 += FR_SR) {
        const int nr = min(FR_SR, nrows - r0);
        const uint8_t* g0 = ysrc + (int64_t)r0 * p.yrs;
        __syncthreads();   // the previous chunk's readers are done with `stage`
        fy_stage<S>(stage, g0, 0, p.yrs, 1, nr, segpx * SB, p.SEGY, tid);
        __syncthreads();
        for (int it = tid; it < nr * tx; it += FR_THREADS) {
            const int col = it % tx, r = it / tx;
            const int xo = xmin[col] - cmin;
            const S* s = (const S*)(stage + r * p.SEGY + (int)((uintptr_t)(g0 + (int64_t)r * p.yrs) & 15) + xo * SB);
            const float* w = wx + col * p.NTXp;
            const int n = min(nx[col], segpx - xo);
            float a = 0.f;
            for (int t = 0; t < n; ++t) a = fmaf(w[t], fr_sample(s[t], p.shift), a);
            iy[(r0 + r) * p.TX + col] = a;
        }
    }

    // ---- phase 1b: chroma ----------------------------------------------------------------------------------------------------------
    const int crmin = cymin[0], ccmin = cxmin[0];
    const int cnrows = min(cymin[ty - 1] + cny[ty - 1] - crmin, p.NRC);
    const int csegpx = min(cxmin[tx - 1] + cnx[tx - 1] - ccmin, p.SPC);
    const int cplanes = p.cplanes, cstep = p.cpix / SB;   // cstep: samples between neighbours of one chroma plane
    const uint8_t* csrc;
    [[maybe_unused]] int64_t tdelta = 0;   // TAB = 1: this frame's Cr plane - Cb plane (planar), in the place of p.cdelta
    if constexpr (TAB != 0) {   // interleaved: the lower of the two planes, with the shared ocb / ocr
        const uint8_t *tcb = (const uint8_t*)p.tab[f].cb, *tcr = (const uint8_t*)p.tab[f].cr;
        csrc = (cplanes == 1 && tcr < tcb ? tcr : tcb) + (int64_t)crmin * p.crs + (int64_t)ccmin * p.cpix;
        tdelta = tcr - tcb;
    } else {
        csrc = p.c + f * p.cfs + (int64_t)crmin * p.crs + (int64_t)ccmin * p.cpix;
    }
    for (int r0 = 0; r0 < cnrows; r0 += FR_SR) {
        const int nr = min(FR_SR, cnrows - r0);
        const uint8_t* g0 = csrc + (int64_t)r0 * p.crs;
        __syncthreads();
        fy_stage<S>(stage, g0, TAB != 0 ? tdelta : p.cdelta, p.crs, cplanes, nr, csegpx * p.cpix, p.SEGC, tid);
        __syncthreads();
        for (int it = tid; it < nr * tx; it += FR_THREADS) {
            const int col = it % tx, r = it / tx;
            const int xo = cxmin[col] - ccmin;
            const uint8_t* gs = g0 + (int64_t)r * p.crs;
            const uint8_t* b0 = stage + r * p.SEGC + (int)((uintptr_t)gs & 15) + xo * p.cpix;
            const S *sb, *sr;
            if (cplanes == 1) {
                sb = (const S*)(b0 + p.ocb);
                sr = (const S*)(b0 + p.ocr);
            } else {
                sb = (const S*)b0;
                sr = (const S*)(stage + (FR_SR + r) * p.SEGC + (int)((uintptr_t)(gs + (TAB != 0 ? tdelta : p.cdelta)) & 15) + xo * p.cpix);
            }
            const float* w = cwx + col * p.NCXp;
            const int n = min(cnx[col], csegpx - xo);
            float a0 = 0.f, a1 = 0.f;
            for (int t = 0; t < n; ++t) {
                const float wt = w[t];
                const int o = t * cstep;
                a0 = fmaf(wt, fr_sample(sb[o], p.shift), a0);
                a1 = fmaf(wt, fr_sample(sr[o], p.shift), a1);
            }
            float* q = ic + (r0 + r) * 2 * p.TX + col;
            q[0] = a0;
            q[p.TX] = a1;
        }
    }
    __syncthreads();

    // ---- phase 2: vertical pass, colour matrix, normalise, store -----------------------------------------------------------------------
    for (int it = tid; it < ty * tx; it += FR_THREADS) {
        const int col = it % tx, yy = it / tx;
        float yv = 0.f, cb = 0.f, cr = 0.f;
        {
            const int rb = ymin[yy] - rmin;
            const int n = min(ny[yy], nrows - rb);
            const float* w = wy + yy * p.NTY;
            const float* q = iy + rb * p.TX + col;
            for (int t = 0; t < n; ++t) yv = fmaf(w[t], q[t * p.TX], yv);
        }
        {
            const int rb = cymin[yy] - crmin;
            const int n = min(cny[yy], cnrows - rb);
            const float* w = cwy + yy * p.NCY;
            const float* q = ic + rb * 2 * p.TX + col;
            for (int t = 0; t < n; ++t) {
                cb = fmaf(w[t], q[t * 2 * p.TX], cb);
                cr = fmaf(w[t], q[(t * 2 + 1) * p.TX], cr);
            }
        }
        fy_colour_store<TRC, ORI>(p, yv, cb, cr, f, y0 + yy, x0 + col);
    }
    fr_zero_pad<ORI>(p, f, y0, ty, x0, tx, tid);
}

int fy_stage_bytes(const FyParams& p) {
    const int y = FR_SR * p.SEGY, c = p.cplanes * FR_SR * p.SEGC;   // one buffer: luma chunks first, chroma chunks after them
    return y > c ? y : c;
}

// Tile plan: capacities from the exact tap placement of the crop's rows and columns (the kernel clamps to them all the same); false = over the LDS budget.
bool fy_plan(FyParams& p, int ty, int tx, double& cost) {
    p.TY = ty;
    p.TX = tx;
    p.tilesX = (p.R + tx - 1) / tx;
    p.bands = (p.R + ty - 1) / ty;
    p.NRY = fr_max_span(p.ay, p.top, p.R, ty, p.miry);
    p.NRC = fr_max_span(p.cy, p.top, p.R, ty, p.miry);
    p.SPY = fr_max_span(p.ax, p.left, p.R, tx, p.mirx);
    p.SPC = fr_max_span(p.cx, p.left, p.R, tx, p.mirx);
    p.SEGY = ((p.SPY * p.sbytes + 15) & ~15) + 16;
    p.SEGC = ((p.SPC * p.cpix + 15) & ~15) + 16;
    int64_t o = (int64_t)tx * p.NTXp * 4;
    p.o_wy = (int)o;
    o += (int64_t)ty * p.NTY * 4;
    p.o_cwx = (int)o;
    o += (int64_t)tx * p.NCXp * 4;
    p.o_cwy = (int)o;
    o += (int64_t)ty * p.NCY * 4;
    p.o_idx = (int)o;
    o += (int64_t)(4 * tx + 4 * ty) * 4;
    o = (o + 15) & ~(int64_t)15;
    p.o_iy = (int)o;
    o += (int64_t)p.NRY * tx * 4;
    o = (o + 15) & ~(int64_t)15;
    p.o_ic = (int)o;
    o += (int64_t)p.NRC * 2 * tx * 4;
    o = (o + 15) & ~(int64_t)15;
    p.o_stage = (int)o;
    o += fy_stage_bytes(p);
    if (o > FR_LDS_BUDGET) return false;
    // per output row: the source rows the horizontal pass computes, one luma plane and two chroma planes, plus the (cheaper) staged samples per output pixel -
    // the RGB planner's measure, where staging three planes weighs SEGPX / (tx * scale): a third of that per plane here
    const double fx = p.ax.scale > 1.0 ? p.ax.scale : 1.0, fcx = p.ax.scale > p.cx.div ? p.ax.scale / p.cx.div : 1.0;
    cost = (double)p.NRY / ty * (1.0 + (double)p.SPY / (tx * fx) / 3.0) + (double)p.NRC / ty * (2.0 + 2.0 * p.SPC / (tx * fcx) / 3.0);
    return true;
}

double fy_pq_inv64(double nits) {
    const double y = pow(nits / 10000.0, PQ_M1_D);
    return pow((PQ_C1_D + PQ_C2_D * y) / (1.0 + PQ_C3_D * y), PQ_M2_D);
}

// One launch of the planar instance for a sample size, a transfer (m: null = SDR) and an orientation class, on the contiguous block (FyParams) or the table form (FyTab).
template <class Args>
int fy_dispatch(int sb, const rv_hdr_map* m, int oc, const Args& a, int64_t wgs, int lds, void* stream, const char* who) {
    return fr_pick<2>(sb >> 1, [&](auto S) {
        return fr_pick<3>(m ? m->transfer : FY_TRC_NONE, [&](auto TRC) {
            return fr_pick<3>(oc, [&](auto ORI) {
                return fr_launch<yuv_to_patches_kernel<FrSample<decltype(S)::value>, decltype(TRC)::value, decltype(ORI)::value, std::is_same_v<Args, FyTab>>>(
                    a, wgs, lds, stream, who, "yuv_to_patches");
            });
        });
    });
}

// What every entry point derives from the frame geometry, the subsampling and the colour tags: fr_setup's share, the luma and chroma axes, the
// colour coefficients, the HDR scalars (m: null = SDR) and the tap capacities.
void fy_setup(FyParams& p, int H, int W, int sub_x, int sub_y, int depth, int matrix, int full_range, int chroma_loc, const rv_hdr_map* m, int32_t orient, int32_t R,
              int32_t patch, const float* mean, const float* std, void* patches, int64_t ldp, float* image) {
    double sy, sx;
    fr_setup(p, H, W, orient, R, patch, mean, std, patches, ldp, image, sy, sx);
    p.ay = FrAxis{sy, 1.0, 0.0, H};
    p.ax = FrAxis{sx, 1.0, 0.0, W};
    // a subsampled axis whose chroma sample sits on the even luma sample lies a quarter of a chroma sample off: horizontally for left and top-left siting,
    // vertically for top-left; an axis that is not subsampled is the luma axis.  The offset belongs to the CODED axis; where that axis is mirrored the sample
    // sits on the other side of its luma pair on the display, so the offset changes sign
    const double offy = sub_y == 2 && chroma_loc == 2 ? 0.25 : 0.0, offx = sub_x == 2 && chroma_loc != 1 ? 0.25 : 0.0;
    p.cy = FrAxis{sy, (double)sub_y, p.miry ? -offy : offy, H / sub_y};
    p.cx = FrAxis{sx, (double)sub_x, p.mirx ? -offx : offx, W / sub_x};
    const double kr = matrix == 0 ? 0.299 : matrix == 1 ? 0.2126 : 0.2627, kb = matrix == 0 ? 0.114 : matrix == 1 ? 0.0722 : 0.0593, kg = 1.0 - kr - kb;
    const double sc = (double)(1 << (depth - 8)), top = (double)((1 << depth) - 1);   // 2^(depth - 8); the largest code
    const double cs = full_range ? 255.0 / top : 255.0 / (224.0 * sc);
    p.yoff = full_range ? 0.0f : (float)(16.0 * sc);
    p.cmid = (float)(128.0 * sc);
    p.ky = (float)(full_range ? 255.0 / top : 255.0 / (219.0 * sc));
    p.krcr = (float)(2.0 * (1.0 - kr) * cs);
    p.kbcb = (float)(2.0 * (1.0 - kb) * cs);
    p.kgcb = (float)(-(2.0 * kb * (1.0 - kb) / kg) * cs);
    p.kgcr = (float)(-(2.0 * kr * (1.0 - kr) / kg) * cs);
    if (m) {
        const double lw = m->peak_nits, lt = m->sdr_white_nits, max_lum = fy_pq_inv64(lt) / fy_pq_inv64(lw);
        static const double to709[9] = {1.6605, -0.5876, -0.0728, -0.1246, 1.1329, -0.0083, -0.0182, -0.1006, 1.1187};   // BT.2087
        p.Lw = m->peak_nits;
        p.rLt = (float)(1.0 / lt);
        p.pqLw = (float)fy_pq_inv64(lw);
        p.maxLum = (float)max_lum;
        p.KS = (float)(1.5 * max_lum - 0.5);
        p.gm1 = (float)(0.2 + 0.42 * log10(lw / 1000.0));
        for (int i = 0; i < 9; ++i) p.gam[i] = m->gamut ? (float)to709[i] : (i % 4 == 0 ? 1.0f : 0.0f);
    }
    p.NTX = fr_max_taps(p.ax, p.left, R);
    p.NTXp = p.NTX | 1;   // odd row pitch: the columns' weight rows start in different banks
    p.NTY = fr_max_taps(p.ay, p.top, R);
    p.NCX = fr_max_taps(p.cx, p.left, R);
    p.NCXp = p.NCX | 1;
    p.NCY = fr_max_taps(p.cy, p.top, R);
}

// The colour tags of a planar or packed surface.
int fy_check_colour(int matrix, int full_range, int chroma_loc, const char* who) {
    RV_CHECK_ARG(matrix >= 0 && matrix <= 2, "%s: matrix %d (0 = BT.601, 1 = BT.709, 2 = BT.2020 non-constant luminance)", who, matrix);
    RV_CHECK_ARG(full_range == 0 || full_range == 1, "%s: full_range %d (0 = studio, 1 = full)", who, full_range);
    RV_CHECK_ARG(chroma_loc >= 0 && chroma_loc <= 2, "%s: chroma_loc %d (0 = left, 1 = centre, 2 = top-left)", who, chroma_loc);
    return RV_OK;
}

// What an entry point checks before fy_run / fk_run: its orientation code (0 where it takes none) and its HDR map (m: null = SDR).
int fy_check_orient_map(int32_t orient, const rv_hdr_map* m, const char* who) {
    if (const int rc = fr_check_orient(orient, who)) return rc;
    if (!m) return RV_OK;
    RV_CHECK_ARG(m->transfer == FY_TRC_PQ || m->transfer == FY_TRC_HLG, "%s: transfer %d (1 = PQ, 2 = HLG)", who, m->transfer);
    RV_CHECK_ARG(m->gamut == 0 || m->gamut == 1, "%s: gamut %d (0 = none, 1 = BT.2020 -> BT.709)", who, m->gamut);
    RV_CHECK_ARG(isfinite(m->peak_nits) && m->peak_nits >= 1.0f && m->peak_nits <= 10000.0f, "%s: peak_nits %g outside 1 .. 10000", who,
                 (double)m->peak_nits);
    RV_CHECK_ARG(isfinite(m->sdr_white_nits) && m->sdr_white_nits >= 1.0f && m->sdr_white_nits <= 10000.0f, "%s: sdr_white_nits %g outside 1 .. 10000", who,
                 (double)m->sdr_white_nits);
    return RV_OK;
}

// All planar entry points: validate the surface, plan the tiles, launch.  `who` names the entry point in the messages; m (null = SDR) and orient (0 where the entry
// takes none) are validated by the caller.  tab: the scattered entry's host array of s.n plane triples (s.y / cb / cr and the two frame strides are not read
// then), else null.
int fy_run(const rv_yuv_surface& s, const rv_surface_planes* tab, const rv_hdr_map* m, int32_t orient, int32_t R, int32_t patch, const float* mean, const float* std, void* patches, int64_t ldp, float* image,
           void* stream, const char* who) {
    const int sb = s.sample_bytes, H = s.H, W = s.W, n = s.n;
    RV_CHECK_ARG(sb == 1 || sb == 2, "%s: sample_bytes = %d (1, or 2 = little-endian 16-bit words)", who, sb);
    RV_CHECK_ARG(sb == 1 ? s.depth == 8 : (s.depth >= 9 && s.depth <= 16), "%s: depth = %d does not go with sample_bytes = %d (8 with 1; 9 .. 16 with 2)", who,
                 s.depth, sb);
    RV_CHECK_ARG(s.msb_aligned == 0 || (s.msb_aligned == 1 && sb == 2), "%s: msb_aligned = %d (0 or 1, and 1 with 16-bit words only)", who, s.msb_aligned);
    RV_CHECK_ARG((s.sub_x == 2 && s.sub_y == 2) || (s.sub_x == 2 && s.sub_y == 1) || (s.sub_x == 1 && s.sub_y == 1),
                 "%s: sub_x, sub_y = %d, %d (2,2 = 4:2:0; 2,1 = 4:2:2; 1,1 = 4:4:4)", who, s.sub_x, s.sub_y);
    RV_CHECK_ARG(s.c_pix == sb || s.c_pix == 2 * sb, "%s: c_pix = %d (%d = planar, %d = interleaved)", who, s.c_pix, sb, 2 * sb);
    if (const int rc = fy_check_colour(s.matrix, s.full_range, s.chroma_loc, who)) return rc;
    const uint8_t *y = nullptr, *cb = nullptr, *cr = nullptr;
    const int rc = fr_check_common(
        R, patch, n, mean, std, patches, ldp, image, who,
        [&]() -> int {
            RV_CHECK_ARG(H >= s.sub_y && W >= s.sub_x && H <= FR_MAX_SIDE && W <= FR_MAX_SIDE, "%s: frame size %d x %d outside %d x %d .. %d", who, H, W, s.sub_y,
                         s.sub_x, FR_MAX_SIDE);
            RV_CHECK_ARG(H % s.sub_y == 0 && W % s.sub_x == 0, "%s: frame size %d x %d is odd (a chroma sample covers %d x %d luma samples)", who, H, W, s.sub_y, s.sub_x);
            return RV_OK;
        },
        [&]() -> int {
            if (tab) {   // the whole table before anything is launched; frame 0 then stands for the batch: the other frames have its interleave relation
                y = (const uint8_t*)tab[0].y, cb = (const uint8_t*)tab[0].cb, cr = (const uint8_t*)tab[0].cr;
                for (int32_t f = 0; f < n; ++f) {
                    const uint8_t *ty = (const uint8_t*)tab[f].y, *tb = (const uint8_t*)tab[f].cb, *tr = (const uint8_t*)tab[f].cr;
                    RV_CHECK_ARG(ty && tb && tr, "%s: null plane in frame %d of %d (y %p, cb %p, cr %p)", who, f, n, tab[f].y, tab[f].cb, tab[f].cr);
                    RV_CHECK_ARG(sb == 1 || (((uintptr_t)ty | (uintptr_t)tb | (uintptr_t)tr) & 1) == 0,
                                 "%s: 16-bit planes must be aligned to 2 bytes: frame %d of %d (y %p, cb %p, cr %p)", who, f, n, tab[f].y, tab[f].cb, tab[f].cr);
                    RV_CHECK_ARG(s.c_pix == sb || tr - tb == cr - cb, "%s: c_pix = %d takes interleaved planes: cr - cb = %lld bytes in frame %d of %d, %lld in frame 0", who,
                                 s.c_pix, (long long)(tr - tb), f, n, (long long)(cr - cb));
                }
                RV_CHECK_ARG(s.c_pix == sb || cr - cb == sb || cb - cr == sb, "%s: c_pix = %d takes interleaved planes (cr = cb + %d bytes or cb = cr + %d bytes): frame 0 of %d",
                             who, s.c_pix, sb, sb, n);
                RV_CHECK_ARG(sb == 1 || (((uintptr_t)s.y_row_stride | (uintptr_t)s.c_row_stride) & 1) == 0, "%s: 16-bit row strides must be aligned to 2 bytes (%lld %lld)", who,
                             (long long)s.y_row_stride, (long long)s.c_row_stride);
            } else {
                y = (const uint8_t*)s.y, cb = (const uint8_t*)s.cb, cr = (const uint8_t*)s.cr;
                RV_CHECK_ARG(y && cb && cr, "%s: null plane (y %p, cb %p, cr %p)", who, s.y, s.cb, s.cr);
                RV_CHECK_ARG(s.c_pix == sb || cr - cb == sb || cb - cr == sb, "%s: c_pix = %d takes interleaved planes (cr = cb + %d bytes or cb = cr + %d bytes)", who,
                             s.c_pix, sb, sb);
                RV_CHECK_ARG(sb == 1 || (((uintptr_t)y | (uintptr_t)cb | (uintptr_t)cr | (uintptr_t)s.y_frame_stride | (uintptr_t)s.y_row_stride |
                                           (uintptr_t)s.c_frame_stride | (uintptr_t)s.c_row_stride) & 1) == 0,
                             "%s: 16-bit planes and strides must be aligned to 2 bytes (y %p, cb %p, cr %p, strides %lld %lld %lld %lld)", who, s.y, s.cb, s.cr,
                             (long long)s.y_frame_stride, (long long)s.y_row_stride, (long long)s.c_frame_stride, (long long)s.c_row_stride);
            }
            return RV_OK;
        });
    if (rc || n == 0) return rc;
    FyParams p{};
    p.yrs = s.y_row_stride;
    p.crs = s.c_row_stride;
    p.cpix = s.c_pix;
    p.sbytes = sb;
    p.shift = s.msb_aligned ? 16 - s.depth : 0;
    const uint8_t* c = cb;   // the Cb plane (planar) or the lower of the two interleaved planes
    if (s.c_pix == sb) {
        p.cplanes = 2;
    } else {
        p.cplanes = 1;
        c = cb < cr ? cb : cr;
        p.ocb = (int)(cb - c);
        p.ocr = (int)(cr - c);
    }
    if (!tab) {   // a TAB = 1 instance takes every base, and planar Cr - Cb, from the table
        p.y = y;
        p.c = c;
        p.yfs = s.y_frame_stride;
        p.cfs = s.c_frame_stride;
        p.cdelta = s.c_pix == sb ? cr - cb : 0;
    }
    fy_setup(p, H, W, s.sub_x, s.sub_y, s.depth, s.matrix, s.full_range, s.chroma_loc, m, orient, R, patch, mean, std, patches, ldp, image);
    FyParams best{};
    RV_CHECK_ARG(fr_best_plan(p, R, fy_plan, best), "%s: %d x %d -> %d needs more filter taps than a workgroup's LDS holds", who, H, W, R);
    const int lds = best.o_stage + fy_stage_bytes(best), oc = fr_orient_class(orient);
    return fr_launch_all<FyTab>(
        best, [](auto& a) -> auto& { return a; }, tab, n, [&](const auto& a, int64_t wgs) { return fy_dispatch(sb, m, oc, a, wgs, lds, stream, who); }, who);
}

// ---- packed surfaces (rv_packed_to_patches): YUY2 / UYVY / Y210, AYUV / VUYA / Y410 / XV36 ... -------------------------------------------------------------
// One base pointer; a row is a run of units of `unit` bytes that cover `ppu` pixels each.  Pixel x has its Y sample at byte x * (unit / ppu) + oy, chroma sample j
// (one per unit) has Cb / Cr at j * unit + ocb / ocr.  The values are those of the planar surface that holds the same samples (sub_x = ppu, sub_y = 1), so the
// luma and chroma ROW windows of a tile coincide: each source row segment - the units that hold the tile's luma and chroma column windows - is staged ONCE and
// the Y, Cb and Cr horizontal passes run out of it, each with its own offset and sample step.  Tap tables, the fmaf chains per output and everything behind the
// vertical pass are the planar kernel's, so the results are its bits.  FkParams wraps FyParams: the planar instances see the argument block they always saw.
struct FkParams {
    FyParams b;               // y: the surface; yfs / yrs: its strides; ocb / ocr: the chroma byte offsets in a unit; SEGY: bytes of a staged row; NRY: rows of inter
    int unit, ppu, oy;        // bytes of a unit; pixels it covers; byte offset of its first Y sample
    int shy, shcb, shcr;      // per component: 16-bit words: sample = word >> shift; 32-bit bit-field words: sample = (word >> shift) & 1023
    int SPU;                  // units of a staged row segment
};

// The argument block of the TAB = 1 packed instances: frame f of one launch starts where tab[f] says (k.b.y / k.b.yfs unused).
struct FkTab : FkParams {
    const void* tab[RV_FRAME_TABLE_MAX];
};
template <int TAB>
using FkArgs = std::conditional_t<TAB != 0, FkTab, FkParams>;

template <typename S, int TRC, int ORI, int TAB>
__global__ __launch_bounds__(FR_THREADS) void packed_to_patches_kernel(const FkArgs<TAB> k) {
    const FyParams& p = k.b;
    extern __shared__ __attribute__((aligned(16))) char fy_smem[];
    float* wx = (float*)fy_smem;                       // [TX][NTXp]
    float* wy = (float*)(fy_smem + p.o_wy);            // [TY][NTY]
    float* cwx = (float*)(fy_smem + p.o_cwx);          // [TX][NCXp]
    int* xmin = (int*)(fy_smem + p.o_idx);             // [TX], then nx, cxmin, cnx [TX], ymin, ny [TY]
    int* nx = xmin + p.TX;
    int* cxmin = nx + p.TX;
    int* cnx = cxmin + p.TX;
    int* ymin = cnx + p.TX;
    int* ny = ymin + p.TY;
    float* inter = (float*)(fy_smem + p.o_iy);         // [NRY][Y | Cb | Cr][TX]
    uint8_t* stage = (uint8_t*)(fy_smem + p.o_stage);  // [FR_SR][SEGY]
    const int tid = threadIdx.x;
    uint32_t b = blockIdx.x;
    const int tile = b % p.tilesX;
    b /= p.tilesX;
    const int band = b % p.bands;
    const int64_t f = b / p.bands;
    const int y0 = band * p.TY, x0 = tile * p.TX;
    const int ty = min(p.TY, p.R - y0), tx = min(p.TX, p.R - x0);

    // ---- phase 0: tap tables (sub_y = 1: one row table serves luma and chroma) ---------------------------------------------------------
    const int mirx = ORI == 0 ? 0 : p.mirx, miry = ORI == 0 ? 0 : p.miry;
    for (int i = tid; i < 2 * tx + ty; i += FR_THREADS) {
        int o = i;
        if (o < tx) fr_tap_table(p.ax, p.left, p.R, mirx, x0 + o, p.NTX, wx + o * p.NTXp, xmin[o], nx[o]);
        else if ((o -= tx) < tx) fr_tap_table(p.cx, p.left, p.R, mirx, x0 + o, p.NCX, cwx + o * p.NCXp, cxmin[o], cnx[o]);
        else o -= tx, fr_tap_table(p.ay, p.top, p.R, miry, y0 + o, p.NTY, wy + o * p.NTY, ymin[o], ny[o]);
    }
    __syncthreads();

    // ---- phase 1: stage each row's units once, three horizontal passes out of them ----------------------------------------------------
    const int rmin = ymin[0];
    const int nrows = min(ymin[ty - 1] + ny[ty - 1] - rmin, p.NRY);
    const int u0 = min(xmin[0] / k.ppu, cxmin[0]);      // the units that hold the luma and the chroma column window
    const int u1 = min(max((xmin[tx - 1] + nx[tx - 1] + k.ppu - 1) / k.ppu, cxmin[tx - 1] + cnx[tx - 1]), u0 + k.SPU);
    constexpr int SB = (int)sizeof(S);
    const int ystep = k.unit / k.ppu, ys = ystep / SB, cs = k.unit / SB;   // bytes / samples between neighbouring Y samples; samples between chroma neighbours
    const uint8_t* src;
    if constexpr (TAB != 0) src = (const uint8_t*)k.tab[f] + (int64_t)rmin * p.yrs + (int64_t)u0 * k.unit;
    else src = p.y + f * p.yfs + (int64_t)rmin * p.yrs + (int64_t)u0 * k.unit;
    for (int r0 = 0; r0 < nrows; r0 += FR_SR) {
        const int nr = min(FR_SR, nrows - r0);
        const uint8_t* g0 = src + (int64_t)r0 * p.yrs;
        __syncthreads();   // the previous chunk's readers are done with `stage`
        fy_stage<S>(stage, g0, 0, p.yrs, 1, nr, (u1 - u0) * k.unit, p.SEGY, tid);
        __syncthreads();
        for (int it = tid; it < nr * tx; it += FR_THREADS) {
            const int col = it % tx, r = it / tx;
            const uint8_t* row = stage + r * p.SEGY + (int)((uintptr_t)(g0 + (int64_t)r * p.yrs) & 15);   // unit u0 of this row
            float* q = inter + (r0 + r) * 3 * p.TX + col;
            {
                const S* s = (const S*)(row + (xmin[col] - u0 * k.ppu) * ystep + k.oy);
                const float* w = wx + col * p.NTXp;
                const int n = min(nx[col], u1 * k.ppu - xmin[col]);
                float a = 0.f;
                for (int t = 0; t < n; ++t) a = fmaf(w[t], fr_sample(s[t * ys], k.shy), a);
                q[0] = a;
            }
            {
                const uint8_t* b0 = row + (cxmin[col] - u0) * k.unit;
                const S *sb = (const S*)(b0 + p.ocb), *sr = (const S*)(b0 + p.ocr);
                const float* w = cwx + col * p.NCXp;
                const int n = min(cnx[col], u1 - cxmin[col]);
                float a0 = 0.f, a1 = 0.f;
                for (int t = 0; t < n; ++t) {
                    const float wt = w[t];
                    const int o = t * cs;
                    a0 = fmaf(wt, fr_sample(sb[o], k.shcb), a0);
                    a1 = fmaf(wt, fr_sample(sr[o], k.shcr), a1);
                }
                q[p.TX] = a0;
                q[2 * p.TX] = a1;
            }
        }
    }
    __syncthreads();

    // ---- phase 2: vertical pass, then the planar kernel's colour matrix, normalisation and stores ---------------------------------------
    for (int it = tid; it < ty * tx; it += FR_THREADS) {
        const int col = it % tx, yy = it / tx;
        const int rb = ymin[yy] - rmin;
        const int n = min(ny[yy], nrows - rb);
        const float* w = wy + yy * p.NTY;
        const float* q = inter + rb * 3 * p.TX + col;
        float yv = 0.f, cb = 0.f, cr = 0.f;
        for (int t = 0; t < n; ++t) yv = fmaf(w[t], q[t * 3 * p.TX], yv);
        for (int t = 0; t < n; ++t) {
            cb = fmaf(w[t], q[(t * 3 + 1) * p.TX], cb);
            cr = fmaf(w[t], q[(t * 3 + 2) * p.TX], cr);
        }
        fy_colour_store<TRC, ORI>(p, yv, cb, cr, f, y0 + yy, x0 + col);
    }
    fr_zero_pad<ORI>(p, f, y0, ty, x0, tx, tid);
}

// Largest number of units a tile of t coded outputs stages: those that hold its luma and its chroma column window.
int fk_max_units(const FkParams& k, int t) {
    const FyParams& p = k.b;
    int span = 0;
    for (int o0 = 0; o0 < p.R; o0 += t) {
        const int o1 = (o0 + t < p.R ? o0 + t : p.R) - 1;
        int lo, n0, hi, n1, clo, cn0, chi, cn1;
        fr_axis_taps_m(p.ax, p.left, p.R, o0, p.mirx, lo, n0);
        fr_axis_taps_m(p.ax, p.left, p.R, o1, p.mirx, hi, n1);
        fr_axis_taps_m(p.cx, p.left, p.R, o0, p.mirx, clo, cn0);
        fr_axis_taps_m(p.cx, p.left, p.R, o1, p.mirx, chi, cn1);
        const int u0 = lo / k.ppu < clo ? lo / k.ppu : clo, ul = (hi + n1 + k.ppu - 1) / k.ppu, u1 = ul > chi + cn1 ? ul : chi + cn1;
        if (u1 - u0 > span) span = u1 - u0;
    }
    return span;
}

// Tile plan of the packed kernel: one staged segment of whole units (up to 8 bytes per pixel), three `inter` planes; false = over the LDS budget.
bool fk_plan(FkParams& k, int ty, int tx, double& cost) {
    FyParams& p = k.b;
    p.TY = ty;
    p.TX = tx;
    p.tilesX = (p.R + tx - 1) / tx;
    p.bands = (p.R + ty - 1) / ty;
    p.NRY = fr_max_span(p.ay, p.top, p.R, ty, p.miry);
    k.SPU = fk_max_units(k, tx);
    p.SEGY = ((k.SPU * k.unit + 15) & ~15) + 16;
    int64_t o = (int64_t)tx * p.NTXp * 4;
    p.o_wy = (int)o;
    o += (int64_t)ty * p.NTY * 4;
    p.o_cwx = (int)o;
    o += (int64_t)tx * p.NCXp * 4;
    p.o_idx = (int)o;
    o += (int64_t)(4 * tx + 2 * ty) * 4;
    o = (o + 15) & ~(int64_t)15;
    p.o_iy = (int)o;
    o += (int64_t)p.NRY * 3 * tx * 4;
    o = (o + 15) & ~(int64_t)15;
    p.o_stage = (int)o;
    o += (int64_t)FR_SR * p.SEGY;
    if (o > FR_LDS_BUDGET) return false;
    // the planar planner's measure: source rows of the horizontal pass per output row (one luma and two chroma planes), plus the staged pixels per output pixel
    const double fx = p.ax.scale > 1.0 ? p.ax.scale : 1.0;
    cost = (double)p.NRY / ty * (3.0 + (double)k.SPU * k.ppu / (tx * fx));
    return true;
}

// One launch of the packed instance for a sample size, a transfer (m: null = SDR) and an orientation class, on the contiguous block (FkParams) or the table form (FkTab).
template <class Args>
int fk_dispatch(int sb, const rv_hdr_map* m, int oc, const Args& a, int64_t wgs, int lds, void* stream, const char* who) {
    return fr_pick<3>(sb >> 1, [&](auto S) {
        return fr_pick<3>(m ? m->transfer : FY_TRC_NONE, [&](auto TRC) {
            return fr_pick<3>(oc, [&](auto ORI) {
                return fr_launch<packed_to_patches_kernel<FrSample<decltype(S)::value>, decltype(TRC)::value, decltype(ORI)::value, std::is_same_v<Args, FkTab>>>(
                    a, wgs, lds, stream, who, "packed_to_patches");
            });
        });
    });
}

// The packed entry: validate the surface (the header has the list), plan, launch.  m and orient are validated by the caller.  tab: the scattered entry's host array
// of s.n base pointers (s.base and s.frame_stride are not read then), else null.
int fk_run(const rv_packed_surface& s, const void* const* tab, const rv_hdr_map* m, int32_t orient, int32_t R, int32_t patch, const float* mean, const float* std, void* patches, int64_t ldp,
           float* image, void* stream, const char* who) {
    const int sb = s.sample_bytes, unit = s.unit_bytes, ppu = s.pix_per_unit, H = s.H, W = s.W, n = s.n;
    RV_CHECK_ARG(sb == 1 || sb == 2 || sb == 4, "%s: sample_bytes = %d (1, 2 = little-endian 16-bit words, 4 = one 32-bit word of three 10-bit fields)", who, sb);
    RV_CHECK_ARG((ppu == 1 || ppu == 2) && unit == (sb == 4 ? 4 : 4 * sb) && (sb != 4 || ppu == 1),
                 "%s: unit_bytes = %d, pix_per_unit = %d with sample_bytes = %d (a unit is 4 samples that cover 1 or 2 pixels, or one 32-bit word that covers 1)", who,
                 unit, ppu, sb);
    RV_CHECK_ARG(sb == 1 ? s.depth == 8 : sb == 2 ? (s.depth >= 9 && s.depth <= 16) : s.depth == 10,
                 "%s: depth = %d does not go with sample_bytes = %d (8 with 1; 9 .. 16 with 2; 10 with 4)", who, s.depth, sb);
    RV_CHECK_ARG(s.msb_aligned == 0 || (s.msb_aligned == 1 && sb == 2), "%s: msb_aligned = %d (0 or 1, and 1 with 16-bit words only)", who, s.msb_aligned);
    const int oy = s.y_off, ocb = s.cb_off, ocr = s.cr_off;
    if (sb == 4) {
        RV_CHECK_ARG((oy == 0 || oy == 10 || oy == 20) && (ocb == 0 || ocb == 10 || ocb == 20) && (ocr == 0 || ocr == 10 || ocr == 20) && oy != ocb && oy != ocr &&
                         ocb != ocr,
                     "%s: y_off, cb_off, cr_off = %d, %d, %d (with sample_bytes 4: three distinct bit shifts out of 0, 10, 20)", who, oy, ocb, ocr);
    } else {
        // sample slots of a unit: Y0 (and Y1 half a unit on), Cb, Cr - inside the unit, on sample boundaries, no two the same
        const int y1 = ppu == 2 ? oy + unit / 2 : oy;
        RV_CHECK_ARG(oy >= 0 && ocb >= 0 && ocr >= 0 && y1 < unit && ocb < unit && ocr < unit && oy % sb == 0 && ocb % sb == 0 && ocr % sb == 0 && ocb != ocr &&
                         ocb != oy && ocr != oy && ocb != y1 && ocr != y1,
                     "%s: y_off, cb_off, cr_off = %d, %d, %d (distinct sample offsets inside the %d-byte unit%s)", who, oy, ocb, ocr, unit,
                     ppu == 2 ? "; the second Y sample lies half a unit behind the first" : "");
    }
    if (const int rc = fy_check_colour(s.matrix, s.full_range, s.chroma_loc, who)) return rc;
    const int rc = fr_check_common(
        R, patch, n, mean, std, patches, ldp, image, who,
        [&]() -> int {
            RV_CHECK_ARG(H >= 1 && W >= ppu && H <= FR_MAX_SIDE && W <= FR_MAX_SIDE, "%s: frame size %d x %d outside 1 x %d .. %d", who, H, W, ppu, FR_MAX_SIDE);
            RV_CHECK_ARG(W % ppu == 0, "%s: frame width W = %d is odd (a unit covers %d pixels)", who, W, ppu);
            return RV_OK;
        },
        [&]() -> int {
            if (tab) {   // the whole table before anything is launched
                for (int32_t f = 0; f < n; ++f) {
                    RV_CHECK_ARG(tab[f], "%s: null base pointer for frame %d of %d", who, f, n);
                    RV_CHECK_ARG(((uintptr_t)tab[f] & (uintptr_t)(sb - 1)) == 0, "%s: %d-bit words: the base of frame %d of %d must be aligned to %d bytes (%p)", who, 8 * sb, f,
                                 n, sb, tab[f]);
                }
                RV_CHECK_ARG(((uintptr_t)s.row_stride & (uintptr_t)(sb - 1)) == 0, "%s: %d-bit words: row_stride %lld must be aligned to %d bytes", who, 8 * sb,
                             (long long)s.row_stride, sb);
            } else {
                RV_CHECK_ARG(s.base, "%s: null base pointer", who);
                RV_CHECK_ARG((((uintptr_t)s.base | (uintptr_t)s.frame_stride | (uintptr_t)s.row_stride) & (uintptr_t)(sb - 1)) == 0,
                             "%s: %d-bit words: base and strides must be aligned to %d bytes (base %p, frame_stride %lld, row_stride %lld)", who, 8 * sb, sb, s.base,
                             (long long)s.frame_stride, (long long)s.row_stride);
            }
            return RV_OK;
        });
    if (rc || n == 0) return rc;
    FkParams k{};
    FyParams& p = k.b;
    p.y = tab ? nullptr : (const uint8_t*)s.base;
    p.yfs = tab ? 0 : s.frame_stride;
    p.yrs = s.row_stride;
    p.sbytes = sb;
    k.unit = unit;
    k.ppu = ppu;
    if (sb == 4) {
        k.shy = oy, k.shcb = ocb, k.shcr = ocr;
    } else {
        k.oy = oy, p.ocb = ocb, p.ocr = ocr;
        k.shy = k.shcb = k.shcr = s.msb_aligned ? 16 - s.depth : 0;
    }
    fy_setup(p, H, W, ppu, 1, s.depth, s.matrix, s.full_range, s.chroma_loc, m, orient, R, patch, mean, std, patches, ldp, image);
    FkParams best{};
    RV_CHECK_ARG(fr_best_plan(k, R, fk_plan, best), "%s: %d x %d -> %d at %d bytes per pixel needs more filter taps and staging than a workgroup's LDS holds", who, H, W, R,
                 unit / ppu);
    const int lds = best.b.o_stage + FR_SR * best.b.SEGY, oc = fr_orient_class(orient);
    return fr_launch_all<FkTab>(
        best, [](auto& a) -> auto& { return a.b; }, tab, n, [&](const auto& a, int64_t wgs) { return fk_dispatch(sb, m, oc, a, wgs, lds, stream, who); }, who);
}

}  // namespace

extern "C" int rv_yuv_surface_to_patches(const rv_yuv_surface* s, int32_t R, int32_t patch, const float mean[3], const float std[3], void* patches, int64_t ldp,
                                         float* image, void* stream) {
    RV_CHECK_ARG(s, "rv_yuv_surface_to_patches: null surface");
    return fy_run(*s, nullptr, nullptr, 0, R, patch, mean, std, patches, ldp, image, stream, "rv_yuv_surface_to_patches");
}

// The surface entry with the HDR -> SDR steps between the colour matrix and the normalisation: the map is validated here, everything else by fy_run.
extern "C" int rv_yuv_surface_to_patches_hdr(const rv_yuv_surface* s, const rv_hdr_map* m, int32_t R, int32_t patch, const float mean[3], const float std[3],
                                             void* patches, int64_t ldp, float* image, void* stream) {
    const char* who = "rv_yuv_surface_to_patches_hdr";
    RV_CHECK_ARG(s, "%s: null surface", who);
    RV_CHECK_ARG(m, "%s: null map", who);
    if (const int rc = fy_check_orient_map(0, m, who)) return rc;
    return fy_run(*s, nullptr, m, 0, R, patch, mean, std, patches, ldp, image, stream, who);
}

// The surface entry on the picture as it is displayed: the struct describes the coded surface, orient (0 .. 7) turns and flips it; m: NULL = SDR, else the
// HDR entry's map.
extern "C" int rv_yuv_surface_to_patches_oriented(const rv_yuv_surface* s, const rv_hdr_map* m, int32_t orient, int32_t R, int32_t patch, const float mean[3],
                                                  const float std[3], void* patches, int64_t ldp, float* image, void* stream) {
    const char* who = "rv_yuv_surface_to_patches_oriented";
    RV_CHECK_ARG(s, "%s: null surface", who);
    if (const int rc = fy_check_orient_map(orient, m, who)) return rc;
    return fy_run(*s, nullptr, m, orient, R, patch, mean, std, patches, ldp, image, stream, who);
}

// The 8-bit 4:2:0 surface of the first entry point: its own two-valued matrix and chroma_loc, then the same code.
extern "C" int rv_yuv_to_patches(const uint8_t* y, int64_t y_frame_stride, int64_t y_row_stride, const uint8_t* cb, const uint8_t* cr, int64_t c_frame_stride,
                                 int64_t c_row_stride, int32_t c_pix, int32_t n, int32_t H, int32_t W, int32_t matrix, int32_t full_range, int32_t chroma_loc,
                                 int32_t R, int32_t patch, const float mean[3], const float std[3], void* patches, int64_t ldp, float* image, void* stream) {
    RV_CHECK_ARG(c_pix == 1 || c_pix == 2, "rv_yuv_to_patches: c_pix = %d (1 = planar, 2 = interleaved)", c_pix);
    RV_CHECK_ARG(matrix == 0 || matrix == 1, "rv_yuv_to_patches: matrix %d (0 = BT.601, 1 = BT.709)", matrix);
    RV_CHECK_ARG(full_range == 0 || full_range == 1, "rv_yuv_to_patches: full_range %d (0 = studio, 1 = full)", full_range);
    RV_CHECK_ARG(chroma_loc == 0 || chroma_loc == 1, "rv_yuv_to_patches: chroma_loc %d (0 = left, 1 = centre)", chroma_loc);
    rv_yuv_surface s{};
    s.y = y;
    s.cb = cb;
    s.cr = cr;
    s.y_frame_stride = y_frame_stride;
    s.y_row_stride = y_row_stride;
    s.c_frame_stride = c_frame_stride;
    s.c_row_stride = c_row_stride;
    s.sample_bytes = 1;
    s.depth = 8;
    s.msb_aligned = 0;
    s.c_pix = c_pix;
    s.sub_x = s.sub_y = 2;
    s.n = n;
    s.H = H;
    s.W = W;
    s.matrix = matrix;
    s.full_range = full_range;
    s.chroma_loc = chroma_loc;
    return fy_run(s, nullptr, nullptr, 0, R, patch, mean, std, patches, ldp, image, stream, "rv_yuv_to_patches");
}

// A packed surface (YUY2 / UYVY / Y210, AYUV / VUYA / Y410 / XV36 ...): one entry for SDR / HDR (m: NULL = SDR) and every orientation, shaped like the oriented
// surface entry.  The values are those of the planar surface that holds the same samples.
extern "C" int rv_packed_to_patches(const rv_packed_surface* s, const rv_hdr_map* m, int32_t orient, int32_t R, int32_t patch, const float mean[3], const float std[3],
                                    void* patches, int64_t ldp, float* image, void* stream) {
    const char* who = "rv_packed_to_patches";
    RV_CHECK_ARG(s, "%s: null surface", who);
    if (const int rc = fy_check_orient_map(orient, m, who)) return rc;
    return fk_run(*s, nullptr, m, orient, R, patch, mean, std, patches, ldp, image, stream, who);
}

// The oriented surface entry on separately allocated surfaces: planes[f] holds the Y, Cb and Cr pointers of frame f; the struct gives everything the frames share
// (its own plane pointers and frame strides are not read).  The header has the rules.
extern "C" int rv_yuv_surfaces_to_patches(const rv_yuv_surface* s, const rv_surface_planes* planes, const rv_hdr_map* m, int32_t orient, int32_t R, int32_t patch,
                                          const float mean[3], const float std[3], void* patches, int64_t ldp, float* image, void* stream) {
    const char* who = "rv_yuv_surfaces_to_patches";
    RV_CHECK_ARG(s, "%s: null surface", who);
    if (const int rc = fy_check_orient_map(orient, m, who)) return rc;
    RV_CHECK_ARG(planes || s->n <= 0, "%s: null array of plane pointers (n = %d)", who, s->n);
    return fy_run(*s, planes, m, orient, R, patch, mean, std, patches, ldp, image, stream, who);
}

// The packed entry on separately allocated surfaces: bases[f] is the first unit of frame f.
extern "C" int rv_packed_surfaces_to_patches(const rv_packed_surface* s, const void* const* bases, const rv_hdr_map* m, int32_t orient, int32_t R, int32_t patch,
                                             const float mean[3], const float std[3], void* patches, int64_t ldp, float* image, void* stream) {
    const char* who = "rv_packed_surfaces_to_patches";
    RV_CHECK_ARG(s, "%s: null surface", who);
    if (const int rc = fy_check_orient_map(orient, m, who)) return rc;
    RV_CHECK_ARG(bases || s->n <= 0, "%s: null array of base pointers (n = %d)", who, s->n);
    return fk_run(*s, bases, m, orient, R, patch, mean, std, patches, ldp, image, stream, who);
}
