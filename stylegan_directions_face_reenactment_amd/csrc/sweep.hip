// Direction sweeps: the ladder of shifts along one learned direction, and the frames the editing scripts make of the rendered rows.
//
// The reference walks a direction one B=1 generator call at a time (run_facial_editing.py:144-207 interpolate, libs/utilities/
// visualization.py:13-73 make_interpolation_chart): get_direction_info (libs/configs/config_directions.py:42-85) pulls the source's
// position to the host, two np.arange loops give the shifts, each shift becomes a host-built one_hot vector and an upload, and every
// 1024^2 frame goes through AdaptiveAvgPool2d, clamp, scale and cast passes of its own.  Here
//   sweep_plan    one thread per (source row, direction): start / min / max / step and the two arange lengths, on the device
//   sweep_rows    one thread per ladder row: the [R, D] one-hot matrix, the row -> direction map and the `start` flag
//   sweep_frames  one pass over the rendered rows: f x f mean, red border on the start rows, uint8 gif frames
//   video_frames  the same pass for the reenactment video: f x f mean next to up to three left panels, uint8 grid frames
//   video_px      video_frames with left panels that are float32 or uint8 and read through a row index; x may be absent
//
// The ladder arithmetic mirrors the reference's mixed NumPy / torch dtypes operation by operation -- the lengths depend on it:
//   angle directions   a 0-d float32 array times a Python number is float32, the division by the float64 angle scale and everything
//                      after it float64; np.arange computes its length, its second element and its fill in float64
//   jaw / expressions  a * x + b on a float32 tensor; the 0-d float32 array makes min, max, the length quotient and first + step
//                      float32 under NumPy's weak-scalar rule (Python numbers are rounded to float32 first); the fill is
//                      first + i * (second - first) in float64, rounded once when one_hot stores it into a float32 tensor
// One rounding per operation, no fma: each operation is a function of its own, a device intrinsic on the GPU and a lone operator on the
// host, so sgdfr_sweep_plan_host runs the same function and proves the ladder on a machine without a GPU.
#include <math.h>

#include "common.h"

namespace sgdfr {

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ float f_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float f_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float f_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ float f_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double d_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double d_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double d_sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double d_div(double a, double b) { return __ddiv_rn(a, b); }
#else
// (noinline: nothing for the host compiler to contract across)
__attribute__((noinline)) static float f_mul(float a, float b) { return a * b; }
__attribute__((noinline)) static float f_add(float a, float b) { return a + b; }
__attribute__((noinline)) static float f_sub(float a, float b) { return a - b; }
__attribute__((noinline)) static float f_div(float a, float b) { return a / b; }
__attribute__((noinline)) static double d_mul(double a, double b) { return a * b; }
__attribute__((noinline)) static double d_add(double a, double b) { return a + b; }
__attribute__((noinline)) static double d_sub(double a, double b) { return a - b; }
__attribute__((noinline)) static double d_div(double a, double b) { return a / b; }
#endif

constexpr int kSweepMaxLen = 1 << 20;      // a ladder longer than this is a NaN / zero-step accident, not a sweep

// len(np.arange(first, stop, step)) from the already rounded quotient
__host__ __device__ inline int arange_len(double q) {
    const double c = ceil(q);
    if (!(c > 0.0)) return 0;                  // negative, zero or NaN
    return c > (double)kSweepMaxLen ? kSweepMaxLen + 1 : (int)c;
}

// get_direction_info + the two arange lengths for one source value x along one direction
__host__ __device__ inline void sweep_plan_one(const sgdfr_direction& e, float x, double shift_scale, int shifts_count,
                                               sgdfr_sweep_record* r) {
    const double step = d_div(shift_scale, (double)shifts_count);
    r->step = step;
    if (e.kind == SGDFR_DIR_ANGLE) {
        const double start = d_div((double)f_mul(x, (float)shift_scale), e.b);
        const double mn = d_sub(-shift_scale, start);
        const double mx = d_add(d_sub(shift_scale, start), 1e-5);
        r->start = start;
        r->min_shift = mn;
        r->max_shift = mx;
        r->n_lo = arange_len(d_div(d_sub(start, mn), step));
        r->n_hi = arange_len(d_div(d_sub(mx, start), step));
    } else {
        const float sc = (float)shift_scale, stepf = (float)step;
        const float start = f_add(f_mul((float)e.a, x), (float)e.b);
        const float mn = f_sub(-sc, start);
        const float mx = f_add(f_sub(sc, start), (float)1e-5);
        r->start = (double)start;
        r->min_shift = (double)mn;
        r->max_shift = (double)mx;
        r->n_lo = arange_len((double)f_div(f_sub(start, mn), stepf));
        r->n_hi = arange_len((double)f_div(f_sub(mx, start), stepf));
    }
}

// element i of np.arange(first, ., step) as one_hot stores it; `first` is exact in float32 on the jaw / expression directions
__host__ __device__ inline float sweep_value(int kind, double first, double step, int i) {
    double delta;
    if (kind == SGDFR_DIR_ANGLE) {
        delta = d_sub(d_add(first, step), first);
    } else {
        const float second = f_add((float)first, (float)step);
        delta = d_sub((double)second, first);
    }
    return (float)d_add(first, d_mul((double)i, delta));
}

struct SweepDirs {
    int k[SGDFR_MAX_DIRECTIONS];
};
struct SweepTable {
    sgdfr_direction d[SGDFR_MAX_DIRECTIONS];
};
struct SweepSrc {
    const float* base[3];      // angles [N,3], pose [N,pose_dim], alpha_exp [N,exp_dim], by (kind - 1)
    int width[3];
};

__host__ __device__ inline float sweep_pick(const SweepSrc& p, const sgdfr_direction& e, int n) {
    const int k = e.kind;
    const float* b = k == SGDFR_DIR_ANGLE ? p.base[0] : (k == SGDFR_DIR_JAW ? p.base[1] : p.base[2]);
    const int w = k == SGDFR_DIR_ANGLE ? p.width[0] : (k == SGDFR_DIR_JAW ? p.width[1] : p.width[2]);
    return b[(int64_t)n * w + e.col];
}

__global__ __launch_bounds__(64) void sweep_plan_kernel(SweepSrc src, SweepTable tab, int K, double shift_scale,
                                                        int shifts_count, sgdfr_sweep_record* __restrict__ rec, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * K) return;
    const int n = i / K, j = i - n * K;
    const sgdfr_direction e = tab.d[j];               // (tab is already gathered by dirs: entry j is direction dirs.k[j])
    sweep_plan_one(e, sweep_pick(src, e, n), shift_scale, shifts_count, &rec[i]);
}

// one thread per ladder row: which (source row, direction) pair it belongs to is a binary search in the pairs' row offsets
__global__ __launch_bounds__(64) void sweep_rows_kernel(const sgdfr_sweep_record* __restrict__ rec, const int* __restrict__ offset,
                                                        SweepTable tab, SweepDirs dirs, int K, int pairs, int D, float* __restrict__ rows,
                                                        int* __restrict__ row_k, int* __restrict__ is_start, int R) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    int lo = 0, hi = pairs - 1;                        // last pair whose offset is <= r (empty ladders share an offset: the last wins)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offset[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    const sgdfr_sweep_record q = rec[lo];
    const int j = r - offset[lo], k = lo % K;
    const sgdfr_direction e = tab.d[k];
    float* row = rows + (int64_t)r * D;
    for (int d = 0; d < D; ++d) row[d] = 0.f;
    if (j < 0 || j >= q.n_lo + q.n_hi) {               // offsets that do not describe R rows: leave the row zero and say so
        row_k[r] = -1;
        is_start[r] = 0;
        return;
    }
    const bool upper = j >= q.n_lo;
    row[dirs.k[k]] = upper ? sweep_value(e.kind, q.start, q.step, j - q.n_lo) : sweep_value(e.kind, q.min_shift, q.step, j);
    row_k[r] = k;
    is_start[r] = j == q.n_lo ? 1 : 0;
}

// ---------------------------------------------------------------- frames
constexpr int kBorder = 3;                             // image_utils.py:130

__device__ __forceinline__ unsigned char to_u8(float x) {
    float v = fminf(fmaxf(x, -1.f), 1.f);              // the arithmetic of image_to_u8_kernel (elementwise.hip)
    v = (v + 1.f) / (2.f + 1e-5f) * 255.f;
    return (unsigned char)v;
}

struct FramesOut {
    float* pooled;
    float* bordered;
    unsigned char* frames;
    const float* src;
    int64_t src_bstride;
    const int* is_start;
    int panels;
};

// everything one output pixel (r, oy, ox) receives: v[c] = its pooled value per channel
__device__ __forceinline__ void put_pixel(const FramesOut& o, int r, int oy, int ox, int P, const float (&v)[3]) {
    const int64_t PP = (int64_t)P * P;
    const int64_t at = (int64_t)r * 3 * PP + (int64_t)oy * P + ox;
    if (o.pooled) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o.pooled[at + c * PP] = v[c];
    }
    if (o.bordered) {
        const bool edge = o.is_start[r] != 0 && (oy < kBorder || oy >= P - kBorder || ox < kBorder || ox >= P - kBorder);
#pragma unroll
        for (int c = 0; c < 3; ++c) o.bordered[at + c * PP] = edge ? (c == 0 ? 1.f : -1.f) : v[c];
    }
    if (o.frames) {
        unsigned char* line = o.frames + ((int64_t)r * P + oy) * (int64_t)o.panels * P * 3;
        if (o.panels == 2) {
            const float* s = o.src + (int64_t)r * o.src_bstride + (int64_t)oy * P + ox;
#pragma unroll
            for (int c = 0; c < 3; ++c) line[(int64_t)ox * 3 + c] = to_u8(s[c * PP]);
            line += (int64_t)P * 3;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) line[(int64_t)ox * 3 + c] = to_u8(v[c]);
    }
}

// 16-byte path: a lane owns four consecutive input columns of F input rows = 4 / F whole output pixels; the lanes of a wave read
// 1 KiB of one input row.  The F x F window is summed row by row, left to right, and divided by F^2 last.
template <int F>
__global__ __launch_bounds__(256) void sweep_frames_vec_kernel(const float* __restrict__ x, FramesOut o, int R, int P) {
    constexpr int NPIX = 4 / F;
    const int W = P * F, Q = W / 4;
    const int64_t items = (int64_t)R * P * Q, plane = (int64_t)W * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(i % Q);
        const int64_t t = i / Q;
        const int oy = (int)(t % P), r = (int)(t / P);
        float acc[3][NPIX];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int p = 0; p < NPIX; ++p) acc[c][p] = 0.f;
            const float* xp = x + ((int64_t)r * 3 + c) * plane + (int64_t)oy * F * W + (int64_t)q * 4;
#pragma unroll
            for (int dy = 0; dy < F; ++dy) {
                const float4 v = *reinterpret_cast<const float4*>(xp + (int64_t)dy * W);
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[c][j / F] += e[j];
            }
        }
#pragma unroll
        for (int p = 0; p < NPIX; ++p) {
            const float v[3] = {acc[0][p] / (float)(F * F), acc[1][p] / (float)(F * F), acc[2][p] / (float)(F * F)};
            put_pixel(o, r, oy, q * NPIX + p, P, v);
        }
    }
}

// dword path (P * f not a multiple of 4, or a pointer off 16 bytes): one output pixel per lane, the same order of additions
__global__ __launch_bounds__(256) void sweep_frames_scalar_kernel(const float* __restrict__ x, FramesOut o, int R, int P, int f) {
    const int W = P * f;
    const int64_t items = (int64_t)R * P * P, plane = (int64_t)W * W;
    const float ff = (float)(f * f);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % P);
        const int64_t t = i / P;
        const int oy = (int)(t % P), r = (int)(t / P);
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* xp = x + ((int64_t)r * 3 + c) * plane + (int64_t)oy * f * W + (int64_t)ox * f;
            float s = 0.f;
            for (int dy = 0; dy < f; ++dy)
                for (int dx = 0; dx < f; ++dx) s += xp[(int64_t)dy * W + dx];
            v[c] = s / ff;
        }
        put_pixel(o, r, oy, ox, P, v);
    }
}

// ---------------------------------------------------------------- video frames (pooled sessions)
// rendered rows -> [B,P,K*P,3] uint8 grid frames in one pass: up to three left panels [B or 1,3,P,P] converted as
// grid_to_u8_kernel converts them, the f x f mean of x (the arithmetic of the frames kernels above) in the last panel.
constexpr int kVideoLeft = 3;

struct VideoPanels {
    const float* x[kVideoLeft];
    int64_t bstride[kVideoLeft];
    int n;                                             // left panels; the pooled rows go into panel n
};

// one output pixel (b, oy, ox) of every panel.  Byte stores: a panel starts at a multiple of P*3 bytes, which is not a multiple of 4
// for every P (P = 7), and adjacent lanes write adjacent 3-byte pixels, so the stores of a wave still fill whole lines.
__device__ __forceinline__ void put_video_pixel(const VideoPanels& g, unsigned char* __restrict__ frames, int b, int oy, int ox, int P,
                                                int swap_rb, const float (&v)[3]) {
    const int64_t PP = (int64_t)P * P;
    unsigned char* line = frames + ((int64_t)b * P + oy) * (int64_t)(g.n + 1) * P * 3 + (int64_t)ox * 3;
#pragma unroll
    for (int k = 0; k < kVideoLeft; ++k) {
        if (k >= g.n) break;
        if (g.x[k]) {
            const float* s = g.x[k] + (int64_t)b * g.bstride[k] + (int64_t)oy * P + ox;
#pragma unroll
            for (int c = 0; c < 3; ++c) line[swap_rb ? 2 - c : c] = to_u8(s[c * PP]);
        }
        line += (int64_t)P * 3;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) line[swap_rb ? 2 - c : c] = to_u8(v[c]);
}

// the lane scheme of sweep_frames_vec_kernel: four consecutive input columns of F rows per lane, 16-byte loads
template <int F>
__global__ __launch_bounds__(256) void video_frames_vec_kernel(const float* __restrict__ x, VideoPanels g,
                                                               unsigned char* __restrict__ frames, int B, int P, int swap_rb) {
    constexpr int NPIX = 4 / F;
    const int W = P * F, Q = W / 4;
    const int64_t items = (int64_t)B * P * Q, plane = (int64_t)W * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(i % Q);
        const int64_t t = i / Q;
        const int oy = (int)(t % P), b = (int)(t / P);
        float acc[3][NPIX];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int p = 0; p < NPIX; ++p) acc[c][p] = 0.f;
            const float* xp = x + ((int64_t)b * 3 + c) * plane + (int64_t)oy * F * W + (int64_t)q * 4;
#pragma unroll
            for (int dy = 0; dy < F; ++dy) {
                const float4 v = *reinterpret_cast<const float4*>(xp + (int64_t)dy * W);
                const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[c][j / F] += e[j];
            }
        }
#pragma unroll
        for (int p = 0; p < NPIX; ++p) {
            const float v[3] = {acc[0][p] / (float)(F * F), acc[1][p] / (float)(F * F), acc[2][p] / (float)(F * F)};
            put_video_pixel(g, frames, b, oy, q * NPIX + p, P, swap_rb, v);
        }
    }
}

// dword path: one output pixel per lane, the same order of additions
__global__ __launch_bounds__(256) void video_frames_scalar_kernel(const float* __restrict__ x, VideoPanels g,
                                                                  unsigned char* __restrict__ frames, int B, int P, int f, int swap_rb) {
    const int W = P * f;
    const int64_t items = (int64_t)B * P * P, plane = (int64_t)W * W;
    const float ff = (float)(f * f);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % P);
        const int64_t t = i / P;
        const int oy = (int)(t % P), b = (int)(t / P);
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* xp = x + ((int64_t)b * 3 + c) * plane + (int64_t)oy * f * W + (int64_t)ox * f;
            float s = 0.f;
            for (int dy = 0; dy < f; ++dy)
                for (int dx = 0; dx < f; ++dx) s += xp[(int64_t)dy * W + dx];
            v[c] = s / ff;
        }
        put_video_pixel(g, frames, b, oy, ox, P, swap_rb, v);
    }
}

// ---------------------------------------------------------------- video frames from typed, indexed panels
// The pass above with left panels that are float32 planar [rows,3,P,P] or uint8 interleaved [rows,P,P,3] (the alignment crop's own
// bytes), each read at row index[b] of its table (clamped into the table), at row b, or at its only row; x may be absent.
struct PxPanels {
    const void* data[kVideoLeft];
    const int* index[kVideoLeft];
    int kind[kVideoLeft];
    int rows[kVideoLeft];
    int n;                                             // left panels; the pooled rows go into panel n
};

// the float the alignment crop hands on for byte u (resize_v_kernel, facecrop.hip): u / 255 * 2 - 1 in that float32 order
__device__ __forceinline__ float u8_to_gan(unsigned char u) { return __fdiv_rn((float)u, 255.0f) * 2.0f - 1.0f; }

__device__ __forceinline__ int panel_row(const PxPanels& g, int k, int b) {
    const int rows = g.rows[k];
    const int r = g.index[k] ? g.index[k][b] : (rows == 1 ? 0 : b);
    return min(max(r, 0), rows - 1);                   // a bad index reads a wrong row of the table, never outside it
}

// NB consecutive bytes of a uint8 panel: dwords where the lane's span is a whole number of them and starts on one, bytes otherwise.
// Adjacent lanes own adjacent spans, so a wave reads 64 * NB contiguous bytes of a panel row either way.
template <int NB>
__device__ __forceinline__ void load_span(const unsigned char* __restrict__ s, unsigned char (&u)[NB]) {
    if (NB % 4 == 0 && (reinterpret_cast<uintptr_t>(s) & 3) == 0) {
#pragma unroll
        for (int i = 0; i < NB / 4; ++i) {
            const unsigned int w = reinterpret_cast<const unsigned int*>(s)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) u[i * 4 + j] = (unsigned char)((w >> (8 * j)) & 255u);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) u[i] = s[i];
}

// NPIX consecutive output pixels (b, oy, ox0 ..) of every panel; v[c][p] = the pooled value, stored only when `last`
template <int NPIX>
__device__ __forceinline__ void put_px_pixels(const PxPanels& g, unsigned char* __restrict__ frames, int b, int oy, int ox0, int P,
                                              int swap_rb, bool last, const float (&v)[3][NPIX]) {
    const int64_t PP = (int64_t)P * P;
    unsigned char* line = frames + ((int64_t)b * P + oy) * (int64_t)(g.n + 1) * P * 3 + (int64_t)ox0 * 3;
#pragma unroll
    for (int k = 0; k < kVideoLeft; ++k) {
        if (k >= g.n) break;
        if (g.data[k]) {
            const int r = panel_row(g, k, b);
            if (g.kind[k] == SGDFR_PANEL_U8) {
                unsigned char u[3 * NPIX];
                load_span<3 * NPIX>(static_cast<const unsigned char*>(g.data[k]) + ((int64_t)r * PP + (int64_t)oy * P + ox0) * 3, u);
#pragma unroll
                for (int p = 0; p < NPIX; ++p)
#pragma unroll
                    for (int c = 0; c < 3; ++c) line[p * 3 + (swap_rb ? 2 - c : c)] = to_u8(u8_to_gan(u[p * 3 + c]));
            } else {
                const float* s = static_cast<const float*>(g.data[k]) + (int64_t)r * 3 * PP + (int64_t)oy * P + ox0;
#pragma unroll
                for (int p = 0; p < NPIX; ++p)
#pragma unroll
                    for (int c = 0; c < 3; ++c) line[p * 3 + (swap_rb ? 2 - c : c)] = to_u8(s[c * PP + p]);
            }
        }
        line += (int64_t)P * 3;
    }
    if (last) {
#pragma unroll
        for (int p = 0; p < NPIX; ++p)
#pragma unroll
            for (int c = 0; c < 3; ++c) line[p * 3 + (swap_rb ? 2 - c : c)] = to_u8(v[c][p]);
    }
}

// the lane scheme of video_frames_vec_kernel; without x (F = 1) a lane converts four pixels of every left panel and stops there
template <int F>
__global__ __launch_bounds__(256) void video_px_vec_kernel(const float* __restrict__ x, PxPanels g, unsigned char* __restrict__ frames,
                                                           int B, int P, int swap_rb) {
    constexpr int NPIX = 4 / F;
    const int W = P * F, Q = W / 4;
    const int64_t items = (int64_t)B * P * Q, plane = (int64_t)W * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(i % Q);
        const int64_t t = i / Q;
        const int oy = (int)(t % P), b = (int)(t / P);
        float v[3][NPIX] = {};
        if (x) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int p = 0; p < NPIX; ++p) v[c][p] = 0.f;
                const float* xp = x + ((int64_t)b * 3 + c) * plane + (int64_t)oy * F * W + (int64_t)q * 4;
#pragma unroll
                for (int dy = 0; dy < F; ++dy) {
                    const float4 e4 = *reinterpret_cast<const float4*>(xp + (int64_t)dy * W);
                    const float e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[c][j / F] += e[j];
                }
#pragma unroll
                for (int p = 0; p < NPIX; ++p) v[c][p] = v[c][p] / (float)(F * F);
            }
        }
        put_px_pixels<NPIX>(g, frames, b, oy, q * NPIX, P, swap_rb, x != nullptr, v);
    }
}

// dword path: one output pixel per lane, the same order of additions
__global__ __launch_bounds__(256) void video_px_scalar_kernel(const float* __restrict__ x, PxPanels g, unsigned char* __restrict__ frames,
                                                              int B, int P, int f, int swap_rb) {
    const int W = P * f;
    const int64_t items = (int64_t)B * P * P, plane = (int64_t)W * W;
    const float ff = (float)(f * f);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % P);
        const int64_t t = i / P;
        const int oy = (int)(t % P), b = (int)(t / P);
        float v[3][1] = {};
        if (x) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* xp = x + ((int64_t)b * 3 + c) * plane + (int64_t)oy * f * W + (int64_t)ox * f;
                float s = 0.f;
                for (int dy = 0; dy < f; ++dy)
                    for (int dx = 0; dx < f; ++dx) s += xp[(int64_t)dy * W + dx];
                v[c][0] = s / ff;
            }
        }
        put_px_pixels<1>(g, frames, b, oy, ox, P, swap_rb, x != nullptr, v);
    }
}

static int gather_table(const char* who, const sgdfr_direction* table, int D, const int* dirs, int K, int pose_dim, int exp_dim,
                        SweepTable* out) {
    SGDFR_REQUIRE(table && D >= 1 && D <= SGDFR_MAX_DIRECTIONS, "%s: 1..%d directions, got %d", who, SGDFR_MAX_DIRECTIONS, D);
    SGDFR_REQUIRE(dirs && K >= 1 && K <= SGDFR_MAX_DIRECTIONS, "%s: 1..%d requested directions, got %d", who, SGDFR_MAX_DIRECTIONS, K);
    for (int j = 0; j < K; ++j) {
        const int k = dirs[j];
        SGDFR_REQUIRE(k >= 0 && k < D, "%s: requested direction %d is outside 0..%d", who, k, D - 1);
        const sgdfr_direction& e = table[k];
        SGDFR_REQUIRE(e.kind != SGDFR_DIR_ZERO, "%s: direction %d is absent from this dataset's table (nothing drives it)", who, k);
        SGDFR_REQUIRE(e.kind >= SGDFR_DIR_ANGLE && e.kind <= SGDFR_DIR_EXP, "%s: direction %d has unknown kind %d", who, k, e.kind);
        const int lim = e.kind == SGDFR_DIR_ANGLE ? 3 : e.kind == SGDFR_DIR_JAW ? pose_dim : exp_dim;
        SGDFR_REQUIRE(e.col >= 0 && e.col < lim, "%s: direction %d reads column %d of %d", who, k, e.col, lim);
        SGDFR_REQUIRE(e.kind != SGDFR_DIR_ANGLE || e.b != 0.0, "%s: direction %d has a zero angle scale", who, k);
        out->d[j] = e;
    }
    return 0;
}

static int check_plan_sizes(const char* who, int N, int K, int pose_dim, int exp_dim, double shift_scale, int shifts_count) {
    SGDFR_REQUIRE(N >= 0 && pose_dim >= 1 && exp_dim >= 1, "%s: bad sizes N=%d pose_dim=%d exp_dim=%d", who, N, pose_dim, exp_dim);
    SGDFR_REQUIRE(shifts_count >= 1 && shift_scale > 0.0, "%s: shift_scale %g and shifts_count %d must be positive", who, shift_scale,
                  shifts_count);
    SGDFR_REQUIRE((int64_t)N * K <= (1 << 24), "%s: %d x %d ladders", who, N, K);
    return 0;
}

}  // namespace sgdfr

using namespace sgdfr;

extern "C" int sgdfr_sweep_plan_f32(const float* angles, const float* pose, const float* alpha_exp, int pose_dim, int exp_dim,
                                    const struct sgdfr_direction* table, int D, const int* dirs, int K, double shift_scale,
                                    int shifts_count, struct sgdfr_sweep_record* records, int N, void* stream) {
    SweepTable tab;
    if (int rc = gather_table("sweep_plan", table, D, dirs, K, pose_dim, exp_dim, &tab)) return rc;
    if (int rc = check_plan_sizes("sweep_plan", N, K, pose_dim, exp_dim, shift_scale, shifts_count)) return rc;
    if (N == 0) return 0;
    SGDFR_REQUIRE(angles && pose && alpha_exp && records, "sweep_plan: null pointer");
    SweepSrc src{{angles, pose, alpha_exp}, {3, pose_dim, exp_dim}};
    const int total = N * K;
    hipLaunchKernelGGL(sweep_plan_kernel, dim3((total + 63) / 64), dim3(64), 0, as_stream(stream), src, tab, K, shift_scale,
                       shifts_count, records, N);
    return check_launch("sweep_plan");
}

extern "C" int sgdfr_sweep_plan_host(const float* angles, const float* pose, const float* alpha_exp, int pose_dim, int exp_dim,
                                     const struct sgdfr_direction* table, int D, const int* dirs, int K, double shift_scale,
                                     int shifts_count, struct sgdfr_sweep_record* records, int N) {
    SweepTable tab;
    if (int rc = gather_table("sweep_plan_host", table, D, dirs, K, pose_dim, exp_dim, &tab)) return rc;
    if (int rc = check_plan_sizes("sweep_plan_host", N, K, pose_dim, exp_dim, shift_scale, shifts_count)) return rc;
    if (N == 0) return 0;
    SGDFR_REQUIRE(angles && pose && alpha_exp && records, "sweep_plan_host: null pointer");
    SweepSrc src{{angles, pose, alpha_exp}, {3, pose_dim, exp_dim}};
    for (int n = 0; n < N; ++n)
        for (int j = 0; j < K; ++j) sweep_plan_one(tab.d[j], sweep_pick(src, tab.d[j], n), shift_scale, shifts_count, &records[n * K + j]);
    return 0;
}

extern "C" int sgdfr_sweep_rows_host(const struct sgdfr_sweep_record* records, const struct sgdfr_direction* table, int D,
                                     const int* dirs, int K, int N, float* rows, int* row_k, int* is_start, int64_t R) {
    SweepTable tab;
    if (int rc = gather_table("sweep_rows_host", table, D, dirs, K, 1 << 30, 1 << 30, &tab)) return rc;
    SGDFR_REQUIRE(N >= 0 && R >= 0, "sweep_rows_host: bad sizes N=%d R=%lld", N, (long long)R);
    SGDFR_REQUIRE(N == 0 || (records && (R == 0 || (rows && row_k && is_start))), "sweep_rows_host: null pointer");
    int64_t r = 0;
    for (int p = 0; p < N * K; ++p) {
        const sgdfr_sweep_record& q = records[p];
        const int j = p % K, k = dirs[j];
        SGDFR_REQUIRE(q.n_lo >= 0 && q.n_hi >= 0 && r + q.n_lo + q.n_hi <= R, "sweep_rows_host: the records describe more than %lld rows",
                      (long long)R);
        for (int i = 0; i < q.n_lo + q.n_hi; ++i, ++r) {
            for (int d = 0; d < D; ++d) rows[r * D + d] = 0.f;
            rows[r * D + k] = i >= q.n_lo ? sweep_value(tab.d[j].kind, q.start, q.step, i - q.n_lo) : sweep_value(tab.d[j].kind, q.min_shift, q.step, i);
            row_k[r] = j;
            is_start[r] = i == q.n_lo ? 1 : 0;
        }
    }
    SGDFR_REQUIRE(r == R, "sweep_rows_host: the records describe %lld rows, not %lld", (long long)r, (long long)R);
    return 0;
}

extern "C" int sgdfr_sweep_rows_f32(const struct sgdfr_sweep_record* records, const int* row_offset, const struct sgdfr_direction* table,
                                    int D, const int* dirs, int K, int N, float* rows, int* row_k, int* is_start, int R, void* stream) {
    SweepTable tab;
    if (int rc = gather_table("sweep_rows", table, D, dirs, K, 1 << 30, 1 << 30, &tab)) return rc;
    SGDFR_REQUIRE(N >= 0 && R >= 0 && (int64_t)N * K <= (1 << 24), "sweep_rows: bad sizes N=%d K=%d R=%d", N, K, R);
    SGDFR_REQUIRE((int64_t)R * D < (1ll << 31), "sweep_rows: %d rows of %d", R, D);
    if (N == 0 || R == 0) return 0;
    SGDFR_REQUIRE(records && row_offset && rows && row_k && is_start, "sweep_rows: null pointer");
    SweepDirs dd;
    for (int j = 0; j < K; ++j) dd.k[j] = dirs[j];
    hipLaunchKernelGGL(sweep_rows_kernel, dim3((R + 63) / 64), dim3(64), 0, as_stream(stream), records, row_offset, tab, dd, K, N * K, D, rows,
                       row_k, is_start, R);
    return check_launch("sweep_rows");
}

extern "C" int sgdfr_sweep_frames_f32(const float* x, int R, int P, int f, const int* is_start, const float* src, int64_t src_bstride,
                                      float* pooled, float* bordered, unsigned char* frames, int panels, void* stream) {
    SGDFR_REQUIRE(f == 1 || f == 2 || f == 4, "sweep_frames: the pooling factor must be 1, 2 or 4 (256, 512, 1024 generators), got %d", f);
    SGDFR_REQUIRE(R >= 0 && P >= 1 && P <= 8192, "sweep_frames: bad shape R=%d P=%d", R, P);
    SGDFR_REQUIRE(!bordered || P >= 2 * kBorder + 1, "sweep_frames: a %d-pixel border needs P >= %d, got %d", kBorder, 2 * kBorder + 1, P);
    SGDFR_REQUIRE(!bordered || is_start, "sweep_frames: the bordered output needs the is_start flags");
    SGDFR_REQUIRE(panels == 1 || panels == 2, "sweep_frames: 1 panel, or 2 with the source, got %d", panels);
    SGDFR_REQUIRE(!frames || panels == 1 || src, "sweep_frames: two panels need the source image");
    SGDFR_REQUIRE(src_bstride == 0 || src_bstride == (int64_t)3 * P * P, "sweep_frames: the source is one image (stride 0) or one per row");
    if (R == 0 || (!pooled && !bordered && !frames)) return 0;
    SGDFR_REQUIRE(x, "sweep_frames: null input");
    FramesOut o{pooled, bordered, frames, src, src_bstride, is_start, panels};
    const int W = P * f;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const int64_t items = vec ? (int64_t)R * P * (W / 4) : (int64_t)R * P * P;
    int64_t blocks = (items + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = as_stream(stream);
    if (!vec) hipLaunchKernelGGL(sweep_frames_scalar_kernel, grid, block, 0, st, x, o, R, P, f);
    else if (f == 1) hipLaunchKernelGGL(sweep_frames_vec_kernel<1>, grid, block, 0, st, x, o, R, P);
    else if (f == 2) hipLaunchKernelGGL(sweep_frames_vec_kernel<2>, grid, block, 0, st, x, o, R, P);
    else hipLaunchKernelGGL(sweep_frames_vec_kernel<4>, grid, block, 0, st, x, o, R, P);
    return check_launch("sweep_frames");
}

extern "C" int sgdfr_video_frames_f32(const float* x, int B, int P, int f, const float* const* panels, const int64_t* bstrides, int n_left,
                                      unsigned char* frames, int swap_rb, void* stream) {
    SGDFR_REQUIRE(f == 1 || f == 2 || f == 4, "video_frames: the pooling factor must be 1, 2 or 4 (256, 512, 1024 generators), got %d", f);
    SGDFR_REQUIRE(B >= 0 && P >= 1 && P <= 8192, "video_frames: bad shape B=%d P=%d", B, P);
    SGDFR_REQUIRE(n_left >= 0 && n_left <= kVideoLeft, "video_frames: %d left panels (0..%d)", n_left, kVideoLeft);
    SGDFR_REQUIRE(n_left == 0 || (panels && bstrides), "video_frames: left panels without their pointer and stride arrays");
    VideoPanels g{};
    g.n = n_left;
    for (int k = 0; k < n_left; ++k) {
        SGDFR_REQUIRE(bstrides[k] == 0 || bstrides[k] == (int64_t)3 * P * P, "video_frames: panel %d is one image (stride 0) or one per row", k);
        g.x[k] = panels[k];
        g.bstride[k] = bstrides[k];
    }
    if (B == 0) return 0;
    SGDFR_REQUIRE(x && frames, "video_frames: null pointer");
    const int W = P * f;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const int64_t items = vec ? (int64_t)B * P * (W / 4) : (int64_t)B * P * P;
    int64_t blocks = (items + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = as_stream(stream);
    if (!vec) hipLaunchKernelGGL(video_frames_scalar_kernel, grid, block, 0, st, x, g, frames, B, P, f, swap_rb);
    else if (f == 1) hipLaunchKernelGGL(video_frames_vec_kernel<1>, grid, block, 0, st, x, g, frames, B, P, swap_rb);
    else if (f == 2) hipLaunchKernelGGL(video_frames_vec_kernel<2>, grid, block, 0, st, x, g, frames, B, P, swap_rb);
    else hipLaunchKernelGGL(video_frames_vec_kernel<4>, grid, block, 0, st, x, g, frames, B, P, swap_rb);
    return check_launch("video_frames");
}

extern "C" int sgdfr_video_frames_px(const float* x, int B, int P, int f, const struct sgdfr_video_panel* panels, int n_left,
                                     unsigned char* frames, int swap_rb, void* stream) {
    SGDFR_REQUIRE(f == 1 || f == 2 || f == 4, "video_frames_px: the pooling factor must be 1, 2 or 4 (256, 512, 1024 generators), got %d", f);
    SGDFR_REQUIRE(B >= 0 && P >= 1 && P <= 8192, "video_frames_px: bad shape B=%d P=%d", B, P);
    SGDFR_REQUIRE(n_left >= 0 && n_left <= kVideoLeft, "video_frames_px: %d left panels (0..%d)", n_left, kVideoLeft);
    SGDFR_REQUIRE(n_left == 0 || panels, "video_frames_px: left panels without their descriptor array");
    PxPanels g{};
    g.n = n_left;
    bool any = x != nullptr;
    for (int k = 0; k < n_left; ++k) {
        const sgdfr_video_panel& p = panels[k];
        g.rows[k] = 1;
        if (!p.data) continue;
        SGDFR_REQUIRE(p.kind == SGDFR_PANEL_F32 || p.kind == SGDFR_PANEL_U8, "video_frames_px: panel %d has kind %d (0 = float32 planar, 1 = uint8 interleaved)", k, p.kind);
        SGDFR_REQUIRE(p.rows >= 1, "video_frames_px: panel %d has %d rows", k, p.rows);
        SGDFR_REQUIRE(p.index || p.rows == 1 || p.rows == B, "video_frames_px: panel %d without an index has 1 or %d rows, got %d", k, B, p.rows);
        g.data[k] = p.data;
        g.index[k] = p.index;
        g.kind[k] = p.kind;
        g.rows[k] = p.rows;
        any = true;
    }
    if (B == 0 || !any) return 0;
    SGDFR_REQUIRE(frames, "video_frames_px: null frames pointer");
    if (!x) f = 1;                                      // nothing to pool: the lanes walk the output pixels
    const int W = P * f;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const int64_t items = vec ? (int64_t)B * P * (W / 4) : (int64_t)B * P * P;
    int64_t blocks = (items + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = as_stream(stream);
    if (!vec) hipLaunchKernelGGL(video_px_scalar_kernel, grid, block, 0, st, x, g, frames, B, P, f, swap_rb);
    else if (f == 1) hipLaunchKernelGGL(video_px_vec_kernel<1>, grid, block, 0, st, x, g, frames, B, P, swap_rb);
    else if (f == 2) hipLaunchKernelGGL(video_px_vec_kernel<2>, grid, block, 0, st, x, g, frames, B, P, swap_rb);
    else hipLaunchKernelGGL(video_px_vec_kernel<4>, grid, block, 0, st, x, g, frames, B, P, swap_rb);
    return check_launch("video_frames_px");
}
