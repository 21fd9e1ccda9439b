// Staging the stage-2 recursion's input on the device (what data/feature_store.py WindowStager.stage_windows builds on the host: a numpy fancy-index of
// the movie's features by stage2.cut_windows' linspace frame indices, a cast and an upload per query):
//   rv_window_gather        features resident on the device + rv_window_select's `select` row + the geometry -> the [R, keep, F, d] window tensor - one launch
//   rv_window_gather_rule   the same with the window rule as an argument: stage 2's shifted windows or stage 1's clipped ones (stage1.cut_windows), and a
//                           NULL select for "every window in order"
// The definition stands in include/revision_hip.h.  The duration and the window rule are grounding.h's (rv_window_select's own code), the sampled frames
// are np.linspace's float64 operations one by one (grounding.h gw_linspace: __ddiv_rn, __dmul_rn, __dadd_rn, each rounded on its own; one definition
// with the window selection that scores the sampled frames), and the rows are copied or converted element by element: a row of the result does not depend on R, on
// the row's place or on any tiling.
#include "grounding.h"

namespace {

constexpr int GW_TPB = 256;                  // 4 waves
constexpr int GW_RPW = 4;                    // output rows of a wave: their loads are in flight together before the first store
constexpr int GW_ROWS = GW_RPW * GW_TPB / 64;   // output rows of a workgroup: F = 250 gives 16 workgroups per selected window, 1600 for 100 windows
constexpr int GW_MAX_L = 1 << 20;            // = rv_window_select's limit
constexpr int GW_MAX_F = 1 << 16;            // ceil(F / GW_ROWS) rides on the grid's y dimension
constexpr int GW_MAX_ITEMS = (1 << 24) - 1;  // R * keep rides on the grid's x dimension: fewer than 2^32 threads along it

struct GatherArgs {
    const void* video;
    const float* mask;
    const int32_t* select;
    void* out;
    int32_t* frame_idx;
    int64_t ldv;
    int L, rpm, d, win, stride, keep, F;
};

// One lane's piece of a row between the load and the store.  VECTOR: 16-byte loads and 16-byte stores - 16 bytes of a copy, 8 elements of a conversion (two loads
// per store from f32 to 16 bits, two stores per load the other way); else one element.  The same type on both sides moves the bits; f32 -> 16 bits is the
// library's store conversion (round to nearest even, a NaN stays a NaN, the fp16 build saturates and reports it); 16 bits -> f32 is exact.
template <typename TI, typename TO, bool VECTOR>
struct Piece;
template <typename T>
struct Piece<T, T, true> {
    static constexpr int E = 16 / sizeof(T);
    u32x4 r;
    __device__ __forceinline__ void load(const T* p) { r = *(const u32x4*)p; }
    __device__ __forceinline__ void zero() { r = u32x4{0u, 0u, 0u, 0u}; }
    __device__ __forceinline__ void store(T* q) const { *(u32x4*)q = r; }
};
template <>
struct Piece<float, op16_t, true> {
    static constexpr int E = 8;
    f32x4 a, b;
    __device__ __forceinline__ void load(const float* p) {
        a = *(const f32x4*)p;
        b = *(const f32x4*)(p + 4);
    }
    __device__ __forceinline__ void zero() { a = b = f32x4{0.f, 0.f, 0.f, 0.f}; }
    __device__ __forceinline__ void store(op16_t* q) const {
        const u32x2 lo = pack_op16x4(a), hi = pack_op16x4(b);
        *(u32x4*)q = u32x4{lo[0], lo[1], hi[0], hi[1]};
    }
};
template <>
struct Piece<op16_t, float, true> {
    static constexpr int E = 8;
    u32x4 r;
    __device__ __forceinline__ void load(const op16_t* p) { r = *(const u32x4*)p; }
    __device__ __forceinline__ void zero() { r = u32x4{0u, 0u, 0u, 0u}; }
    __device__ __forceinline__ void store(float* q) const {
        *(f32x4*)q = op16x4_to_f32(u32x2{r[0], r[1]});
        *(f32x4*)(q + 4) = op16x4_to_f32(u32x2{r[2], r[3]});
    }
};
template <typename T>
struct Piece<T, T, false> {
    static constexpr int E = 1;
    T r;
    __device__ __forceinline__ void load(const T* p) { r = *p; }
    __device__ __forceinline__ void zero() { r = T(0); }
    __device__ __forceinline__ void store(T* q) const { *q = r; }
};
template <>
struct Piece<float, op16_t, false> {
    static constexpr int E = 1;
    float r;
    __device__ __forceinline__ void load(const float* p) { r = *p; }
    __device__ __forceinline__ void zero() { r = 0.f; }
    __device__ __forceinline__ void store(op16_t* q) const { *q = f32_to_op16(r); }
};
template <>
struct Piece<op16_t, float, false> {
    static constexpr int E = 1;
    op16_t r;
    __device__ __forceinline__ void load(const op16_t* p) { r = *p; }
    __device__ __forceinline__ void zero() { r = 0; }
    __device__ __forceinline__ void store(float* q) const { *q = op16_to_f32(r); }
};

// Workgroup (n, y): rows [y * GW_ROWS, y * GW_ROWS + GW_ROWS) of out[n], n = row * keep + slot on the grid's x dimension.  Every workgroup finds the duration
// (with a mask: the block sum of the video's mask row, again in each of them) and its window from select[n]; a wave takes GW_RPW consecutive output rows, lane q
// of it computes the source frame of row q in float64, and the wave reads the frames as scalars.  Then the lanes run over the columns, piece by piece: the
// GW_RPW loads of a step are issued before its first store.  An entry of select outside [0, W_r) loads nothing and stores zeros and -1.
// RULE: RV_WINDOWS_SHIFTED (grounding.h ws_bounds) or RV_WINDOWS_CLIPPED (ws_bounds_clipped, whose void windows are invalid entries too).  IOTA: select may
// be NULL, entry n of a row is then window n (rv_window_gather_rule's instances; rv_window_gather's own read select without looking).
template <typename TI, typename TO, bool VECTOR, int RULE, bool IOTA>
__global__ __launch_bounds__(GW_TPB) void window_gather_kernel(const GatherArgs a) {
    using P = Piece<TI, TO, VECTOR>;
    __shared__ float red[GW_TPB / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = blockIdx.x, r = n / a.keep, v = r / a.rpm;
    const int F = a.F, d = a.d;
    const int D = a.mask ? duration_frames(block_mask_sum<GW_TPB>(a.mask + v * a.L, a.L, red), a.L) : a.L;
    const int i = IOTA && !a.select ? (int)(n % a.keep) : a.select[n];
    bool valid = i >= 0 && i < ws_count(a.win, a.stride, D);
    int s = 0, e = 0;
    if (valid) {
        if constexpr (RULE == RV_WINDOWS_CLIPPED) valid = ws_bounds_clipped(i, a.win, D, s, e);
        else ws_bounds(i, a.win, a.stride, D, s, e);      // frames [s, e + 1), 0 <= s <= e <= D - 1
        e -= 1;
    }
    const int j0 = blockIdx.y * GW_ROWS + wave * GW_RPW;
    int mine = -1;
    if (lane < GW_RPW && j0 + lane < F) {
        if (valid) mine = gw_linspace(s, e, F, j0 + lane);
        if (a.frame_idx) a.frame_idx[n * F + j0 + lane] = mine;
    }
    int idx[GW_RPW];
#pragma unroll
    for (int q = 0; q < GW_RPW; ++q) idx[q] = __builtin_amdgcn_readlane(mine, q);      // -1: no source (an invalid entry, or a row past F)
    const TI* __restrict__ src = (const TI*)a.video + v * a.L * a.ldv;
    TO* __restrict__ dst = (TO*)a.out + (n * F + j0) * d;
    for (int c = lane * P::E; c < d; c += 64 * P::E) {
        P p[GW_RPW];
#pragma unroll
        for (int q = 0; q < GW_RPW; ++q) {
            if (idx[q] >= 0) p[q].load(src + idx[q] * a.ldv + c);
            else p[q].zero();
        }
#pragma unroll
        for (int q = 0; q < GW_RPW; ++q)
            if (j0 + q < F) p[q].store(dst + (int64_t)q * d + c);
    }
}

template <typename TI, typename TO, int RULE, bool IOTA>
void gw_launch(const GatherArgs& a, int64_t items, hipStream_t st) {
    constexpr int E = Piece<TI, TO, true>::E;
    const bool vector = a.d % E == 0 && (a.ldv * sizeof(TI)) % 16 == 0 && ((uintptr_t)a.video & 15u) == 0 && ((uintptr_t)a.out & 15u) == 0;
    const dim3 grid((unsigned)items, (unsigned)cdiv(a.F, GW_ROWS));
    if (vector) hipLaunchKernelGGL((window_gather_kernel<TI, TO, true, RULE, IOTA>), grid, dim3(GW_TPB), 0, st, a);
    else hipLaunchKernelGGL((window_gather_kernel<TI, TO, false, RULE, IOTA>), grid, dim3(GW_TPB), 0, st, a);
}

template <int RULE, bool IOTA>
void gw_dispatch(const GatherArgs& a, int video_dtype, int out_dtype, int64_t items, hipStream_t st) {
    if (video_dtype == RV_F32) {
        if (out_dtype == RV_F32) gw_launch<float, float, RULE, IOTA>(a, items, st);
        else gw_launch<float, op16_t, RULE, IOTA>(a, items, st);
    } else {
        if (out_dtype == RV_F32) gw_launch<op16_t, float, RULE, IOTA>(a, items, st);
        else gw_launch<op16_t, op16_t, RULE, IOTA>(a, items, st);
    }
}

}  // namespace

extern "C" int rv_window_gather(const void* video, int32_t video_dtype, int64_t ldv, const float* mask, const int32_t* select, int32_t R, int32_t rpm,
                                int32_t L, int32_t d, int32_t win, int32_t stride, int32_t keep, int32_t F, void* out, int32_t out_dtype,
                                int32_t* frame_idx, void* stream) {
    RV_CHECK_ARG(video && select && out, "rv_window_gather: bad arguments (a null video, select or out)");
    RV_CHECK_ARG(R >= 1 && rpm >= 1 && R % rpm == 0, "rv_window_gather: R=%d rows with rpm=%d rows per video (R >= 1, rpm >= 1, R a multiple of rpm)", R, rpm);
    RV_CHECK_ARG(L >= 1 && L <= GW_MAX_L, "rv_window_gather: L=%d must be in [1, %d]", L, GW_MAX_L);
    RV_CHECK_ARG(d >= 1 && ldv >= d, "rv_window_gather: d=%d columns with a frame stride of ldv=%lld elements (d >= 1, ldv >= d)", d, (long long)ldv);
    RV_CHECK_ARG(stride >= 1 && win >= stride && win <= L, "rv_window_gather: win=%d frames with stride=%d (stride >= 1, stride <= win <= L=%d)", win, stride,
                 L);
    RV_CHECK_ARG(keep >= 1, "rv_window_gather: keep=%d must be at least 1", keep);
    RV_CHECK_ARG(F >= 1 && F <= GW_MAX_F, "rv_window_gather: F=%d must be in [1, %d]", F, GW_MAX_F);
    RV_CHECK_ARG(video_dtype == RV_OP16 || video_dtype == RV_F32, "rv_window_gather: video_dtype must be f32 or %s", RV_OP16_NAME);
    RV_CHECK_ARG(out_dtype == RV_OP16 || out_dtype == RV_F32, "rv_window_gather: out_dtype must be f32 or %s", RV_OP16_NAME);
    const int64_t items = (int64_t)R * keep;
    RV_CHECK_ARG(items <= GW_MAX_ITEMS, "rv_window_gather: R=%d rows of keep=%d entries (at most %d entries per launch)", R, keep, GW_MAX_ITEMS);
    const GatherArgs a{video, mask, select, out, frame_idx, ldv, L, rpm, d, win, stride, keep, F};
    gw_dispatch<RV_WINDOWS_SHIFTED, false>(a, video_dtype, out_dtype, items, as_stream(stream));
    RV_CHECK_LAUNCH("rv_window_gather");
    return RV_OK;
}

extern "C" int rv_window_gather_rule(const void* video, int32_t video_dtype, int64_t ldv, const float* mask, const int32_t* select, int32_t R, int32_t rpm,
                                     int32_t L, int32_t d, int32_t win, int32_t stride, int32_t keep, int32_t F, void* out, int32_t out_dtype,
                                     int32_t* frame_idx, int32_t rule, void* stream) {
    RV_CHECK_ARG(video && out, "rv_window_gather_rule: bad arguments (a null video or out)");
    RV_CHECK_ARG(rule == RV_WINDOWS_SHIFTED || rule == RV_WINDOWS_CLIPPED, "rv_window_gather_rule: rule=%d (0: shifted windows, 1: clipped windows)", rule);
    RV_CHECK_ARG(R >= 1 && rpm >= 1 && R % rpm == 0, "rv_window_gather_rule: R=%d rows with rpm=%d rows per video (R >= 1, rpm >= 1, R a multiple of rpm)", R,
                 rpm);
    RV_CHECK_ARG(L >= 1 && L <= GW_MAX_L, "rv_window_gather_rule: L=%d must be in [1, %d]", L, GW_MAX_L);
    RV_CHECK_ARG(d >= 1 && ldv >= d, "rv_window_gather_rule: d=%d columns with a frame stride of ldv=%lld elements (d >= 1, ldv >= d)", d, (long long)ldv);
    RV_CHECK_ARG(stride >= 1 && win >= stride && win <= L, "rv_window_gather_rule: win=%d frames with stride=%d (stride >= 1, stride <= win <= L=%d)", win,
                 stride, L);
    RV_CHECK_ARG(rule != RV_WINDOWS_CLIPPED || stride == 2, "rv_window_gather_rule: stride=%d with the clipped rule (its windows overlap by half: stride 2)",
                 stride);
    RV_CHECK_ARG(keep >= 1, "rv_window_gather_rule: keep=%d must be at least 1", keep);
    RV_CHECK_ARG(F >= 1 && F <= GW_MAX_F, "rv_window_gather_rule: F=%d must be in [1, %d]", F, GW_MAX_F);
    RV_CHECK_ARG(video_dtype == RV_OP16 || video_dtype == RV_F32, "rv_window_gather_rule: video_dtype must be f32 or %s", RV_OP16_NAME);
    RV_CHECK_ARG(out_dtype == RV_OP16 || out_dtype == RV_F32, "rv_window_gather_rule: out_dtype must be f32 or %s", RV_OP16_NAME);
    const int64_t items = (int64_t)R * keep;
    RV_CHECK_ARG(items <= GW_MAX_ITEMS, "rv_window_gather_rule: R=%d rows of keep=%d entries (at most %d entries per launch)", R, keep, GW_MAX_ITEMS);
    const GatherArgs a{video, mask, select, out, frame_idx, ldv, L, rpm, d, win, stride, keep, F};
    if (rule == RV_WINDOWS_CLIPPED) gw_dispatch<RV_WINDOWS_CLIPPED, true>(a, video_dtype, out_dtype, items, as_stream(stream));
    else gw_dispatch<RV_WINDOWS_SHIFTED, true>(a, video_dtype, out_dtype, items, as_stream(stream));
    RV_CHECK_LAUNCH("rv_window_gather_rule");
    return RV_OK;
}
