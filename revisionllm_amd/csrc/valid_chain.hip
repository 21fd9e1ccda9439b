// The chain library's validity producer (librevision_hip_chain.so, include/revision_hip_chain.h): the joint between the coarse and the fine half of the
// grounding chain.
//   rvc_windows_valid   a window selection (rvc_window_select_frames' `select`, the LLM's answers, a retrieval log) becomes the per-row validity row
//                       the masked span entries take: 1 at the frames of the named windows' frame sets inside the duration, under an optional
//                       validity row of the caller's, 0 elsewhere; the count of ones on request - one launch
// Duration, window count, window bounds and sampled frames are grounding.h's and window_select.h's own code (block_mask_sum at WS_TPB threads,
// duration_frames, ws_rule_count, ws_rule_bounds, ws_frame_at), so an index means the same frames in the selection, in the gather and here.  The kernel
// reads and writes f32 / i32 rows only, so one library serves both operand flavours.
#include "window_select.h"

#include "../../include/revision_hip_chain.h"

namespace {

constexpr int WV_MAX_KEEP = WS_MAX_W;     // a row names at most as many windows as a row can have

struct ValidArgs {
    const int32_t* select;
    const float* mask;
    const float* valid_in;
    float* valid;
    int32_t* n_valid;
    int L, rpm, win, stride, F, keep;
};

// the row's [0, L) as a head of single elements up to the first 16-byte boundary, a body of 16-byte quads and a tail
struct RowSplit {
    int head, quads;
};
__device__ __forceinline__ RowSplit wv_split(const float* row, int L) {
    int head = (int)((4u - (unsigned)(((uintptr_t)row >> 2) & 3u)) & 3u);
    head = head < L ? head : L;
    return RowSplit{head, (L - head) >> 2};
}

// One workgroup per row.  (1) duration: the block sum of the row's mask row, as window_select_kernel takes it; (2) the whole row is set to +0, in
// 16-byte stores between the row's first and last 16-byte boundary; (3) behind a barrier the waves take the entries of `select` in turn: an entry
// outside [0, W) names nothing, another one's frame set is walked lane-strided and every frame gets its value - 1 when valid_in is null or not 0
// there, else +0.  Windows overlap and a sampled set repeats frames, so several lanes may store to one element; the value depends on the frame alone,
// so the order does not show.  Every frame of a window lies in [0, D) (ws_bounds* end at D - 1): nothing at or behind D is stored to, and valid_in is
// read at covered frames only; (4) behind another barrier the row's ones are counted, wave sums through LDS, when n_valid is asked for.
template <int RULE, int FRAMES>
__global__ __launch_bounds__(WS_TPB) void windows_valid_kernel(const ValidArgs a) {
    __shared__ float red[WS_WAVES];
    __shared__ int part[WS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    const int L = a.L;
    const float* __restrict__ m = a.mask + (r / a.rpm) * L;
    const float* __restrict__ vin = a.valid_in ? a.valid_in + (r / a.rpm) * L : nullptr;
    const int32_t* __restrict__ sel = a.select + r * a.keep;
    float* out = a.valid + r * L;

    const int D = duration_frames(block_mask_sum<WS_TPB>(m, L, red), L);
    const int W = ws_rule_count<RULE>(a.win, a.stride, D);

    const RowSplit sp = wv_split(out, L);
    const int body_end = sp.head + 4 * sp.quads;
    if (tid < sp.head) out[tid] = 0.f;
    {
        f32x4* q = (f32x4*)(out + sp.head);
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        for (int i = tid; i < sp.quads; i += WS_TPB) q[i] = zero;
    }
    for (int t = body_end + tid; t < L; t += WS_TPB) out[t] = 0.f;
    __syncthreads();

    for (int e = wave; e < a.keep; e += WS_WAVES) {
        const int i = sel[e];
        if (i < 0 || i >= W) continue;                       // the -1 padding, a void window, anything else that is no window of this row
        int lo, hi;
        ws_rule_bounds<RULE>(i, a.win, a.stride, D, lo, hi);
        lo = lo < 0 ? 0 : lo;                                // (0 <= lo < hi <= D by the rules; stated again for the stores, changes no value)
        hi = hi > D ? D : hi;
        const int n = FRAMES == WS_FRAMES_SAMPLED ? a.F : hi - lo;
        for (int j = lane; j < n; j += 64) {
            const int t = ws_frame_at<FRAMES>(lo, hi, a.F, j);
            if (t >= lo && t < hi) out[t] = (!vin || vin[t] != 0.f) ? 1.f : 0.f;
        }
    }
    if (!a.n_valid) return;
    __syncthreads();

    int c = 0;
    if (tid < sp.head) c += out[tid] != 0.f ? 1 : 0;
    {
        const f32x4* q = (const f32x4*)(out + sp.head);
        for (int i = tid; i < sp.quads; i += WS_TPB) {
            const f32x4 v = q[i];
            c += (v[0] != 0.f ? 1 : 0) + (v[1] != 0.f ? 1 : 0) + (v[2] != 0.f ? 1 : 0) + (v[3] != 0.f ? 1 : 0);
        }
    }
    for (int t = body_end + tid; t < L; t += WS_TPB) c += out[t] != 0.f ? 1 : 0;
    c = wave_sum_i32(c);
    if (lane == 0) part[wave] = c;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < WS_WAVES; ++w) total += part[w];
        a.n_valid[r] = total;
    }
}

template <int RULE>
void wv_dispatch(const ValidArgs& a, int frames, int R, hipStream_t st) {
    if (frames == RV_FRAMES_SAMPLED) hipLaunchKernelGGL((windows_valid_kernel<RULE, WS_FRAMES_SAMPLED>), dim3((unsigned)R), dim3(WS_TPB), 0, st, a);
    else hipLaunchKernelGGL((windows_valid_kernel<RULE, WS_FRAMES_ALL>), dim3((unsigned)R), dim3(WS_TPB), 0, st, a);
}

}  // namespace

extern "C" int rvc_windows_valid(const int32_t* select, const float* mask, const float* valid_in, int32_t R, int32_t rpm, int32_t L, int32_t rule,
                                 int32_t win, int32_t stride, int32_t frames, int32_t F, int32_t keep, float* valid, int32_t* n_valid, void* stream) {
    RV_CHECK_ARG(select && mask && valid, "rvc_windows_valid: bad arguments (a null select, mask or valid)");
    RV_CHECK_ARG(rule == RV_WINDOWS_SHIFTED || rule == RV_WINDOWS_CLIPPED, "rvc_windows_valid: rule=%d (0: shifted windows, 1: clipped windows)", rule);
    RV_CHECK_ARG(frames == RV_FRAMES_ALL || frames == RV_FRAMES_SAMPLED, "rvc_windows_valid: frames=%d (0: every frame, 1: the sampled frames)", frames);
    RV_CHECK_ARG(R >= 1 && rpm >= 1 && R % rpm == 0, "rvc_windows_valid: R=%d rows with rpm=%d rows per mask row (R >= 1, rpm >= 1, R a multiple of rpm)", R,
                 rpm);
    RV_CHECK_ARG(L >= 1 && L <= WS_MAX_L, "rvc_windows_valid: L=%d must be in [1, %d]", L, WS_MAX_L);
    RV_CHECK_ARG(rule != RV_WINDOWS_CLIPPED || stride == 2, "rvc_windows_valid: stride=%d with the clipped rule (its windows overlap by half: stride 2)",
                 stride);
    RV_CHECK_ARG(stride >= 1 && win >= stride && win <= L, "rvc_windows_valid: win=%d frames with stride=%d (stride >= 1, stride <= win <= L=%d)", win, stride,
                 L);
    RV_CHECK_ARG(frames != RV_FRAMES_SAMPLED || (F >= 1 && F <= RVC_MAX_SAMPLED), "rvc_windows_valid: F=%d sampled frames per window must be in [1, %d]", F,
                 RVC_MAX_SAMPLED);
    RV_CHECK_ARG(frames != RV_FRAMES_ALL || F == 0, "rvc_windows_valid: F=%d with every frame of a window (F = 0)", F);
    RV_CHECK_ARG(keep >= 1 && keep <= WV_MAX_KEEP, "rvc_windows_valid: keep=%d entries per row must be in [1, %d]", keep, WV_MAX_KEEP);
    const ValidArgs a{select, mask, valid_in, valid, n_valid, L, rpm, win, stride, F, keep};
    if (rule == RV_WINDOWS_CLIPPED) wv_dispatch<RV_WINDOWS_CLIPPED>(a, frames, R, as_stream(stream));
    else wv_dispatch<RV_WINDOWS_SHIFTED>(a, frames, R, as_stream(stream));
    RV_CHECK_LAUNCH("rvc_windows_valid");
    return RV_OK;
}
