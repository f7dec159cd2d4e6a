// Direction sweeps: the ladder of shifts along one learned direction, and the frames the editing scripts make of the rendered rows.
//
// The reference walks a direction one B=1 generator call at a time (run_facial_editing.py:144-207 interpolate, libs/utilities/
// visualization.py:13-73 make_interpolation_chart): get_direction_info (libs/configs/config_directions.py:42-85) pulls the source's
// position to the host, two np.arange loops give the shifts, each shift becomes a host-built one_hot vector and an upload, and every
// 1024^2 frame goes through AdaptiveAvgPool2d, clamp, scale and cast passes of its own.  Here
//   sweep_plan    one thread per (source row, direction): start / min / max / step and the two arange lengths, on the device
//   sweep_rows    one thread per ladder row: the [R, D] one-hot matrix, the row -> direction map and the `start` flag
//   pooled_walk   one pass over the rendered rows: the f x f mean of every output pixel, handed to a sink; the one walk below both
//   sweep_frames  the walk into pooled / bordered floats (red border on the start rows) and one- or two-panel uint8 gif frames
//   video_px      the walk into the reenactment video's uint8 grid frames, next to up to three left panels that are float32 or uint8
//                 and read through a row index; x may be absent.  sgdfr_video_frames_f32 is these kernels on float panels
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

#include <algorithm>

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

template <int NPIX>
__device__ __forceinline__ void put_pixels(const FramesOut& o, int r, int oy, int ox0, int P, const float (&v)[3][NPIX]) {
#pragma unroll
    for (int p = 0; p < NPIX; ++p) {
        const float w[3] = {v[0][p], v[1][p], v[2][p]};
        put_pixel(o, r, oy, ox0 + p, P, w);
    }
}

// ---------------------------------------------------------------- the pooled walk
// The one f x f window walk under every frames kernel: R rows of x [R,3,P*f,P*f], the window summed row by row, left to right, and
// divided by f^2 last.  sink(r, oy, ox0, v) receives v[c][p] = channel c of output pixel (r, oy, ox0 + p).  Without x (uniform over
// the launch) the lanes walk the same items and v is zeros.  `block` is blockDim.x, read by the KERNEL and handed in: read in here,
// a device function, it is lowered before the inlining without the kernel's uniform-block promise, to a global_load_ushort and a
// wait at the top of every kernel (+ 4.8 % on the two-panel sweep frames).
// What the sinks capture is settled per kernel by the build and the clock (profiles/frames_walk_time.txt), not by rule: the sweep
// sink copies FramesOut BY VALUE, as conv_tile.h advises; the px sink refers to the kernel's arguments, because a by-value copy of
// PxPanels is split into scalars, the float and uint8 branches of a panel are then merged behind a common conversion and store, and
// that schedule is 1 % slower at f = 4.
//
// 16-byte path: a lane owns four consecutive input columns of F input rows = 4 / F whole output pixels; the lanes of a wave read
// 1 KiB of one input row.
constexpr int kWalkBlock = 256;

template <int F, class Sink>
__device__ __forceinline__ void pooled_walk_vec(const float* __restrict__ x, int R, int P, int block, const Sink& sink) {
    constexpr int NPIX = 4 / F;
    const int W = P * F, Q = W / 4;
    const int64_t items = (int64_t)R * P * Q, plane = (int64_t)W * W;
    for (int64_t i = (int64_t)blockIdx.x * block + threadIdx.x; i < items; i += (int64_t)gridDim.x * block) {
        const int q = (int)(i % Q);
        const int64_t t = i / Q;
        const int oy = (int)(t % P), r = (int)(t / P);
        float v[3][NPIX] = {};
        if (x) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* xp = x + ((int64_t)r * 3 + c) * plane + (int64_t)oy * F * W + (int64_t)q * 4;
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
        sink(r, oy, q * NPIX, v);
    }
}

// dword path (P * f not a multiple of 4, or a pointer off 16 bytes): one output pixel per lane, the same order of additions
template <class Sink>
__device__ __forceinline__ void pooled_walk_scalar(const float* __restrict__ x, int R, int P, int f, int block, const Sink& sink) {
    const int W = P * f;
    const int64_t items = (int64_t)R * P * P, plane = (int64_t)W * W;
    const float ff = (float)(f * f);
    for (int64_t i = (int64_t)blockIdx.x * block + threadIdx.x; i < items; i += (int64_t)gridDim.x * block) {
        const int ox = (int)(i % P);
        const int64_t t = i / P;
        const int oy = (int)(t % P), r = (int)(t / P);
        float v[3][1] = {};
        if (x) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* xp = x + ((int64_t)r * 3 + c) * plane + (int64_t)oy * f * W + (int64_t)ox * f;
                float s = 0.f;
                for (int dy = 0; dy < f; ++dy)
                    for (int dx = 0; dx < f; ++dx) s += xp[(int64_t)dy * W + dx];
                v[c][0] = s / ff;
            }
        }
        sink(r, oy, ox, v);
    }
}

// The launch of a walk: 16-byte lanes where a row of x is a whole number of them and x starts on one, a grid-stride loop over at
// most 65536 blocks of kWalkBlock threads (the kernels read it as blockDim.x), the kernel picked by f.  The kernels take (x, R, P, tail...), the dword one (x, R, P, f, tail...).
constexpr int64_t kWalkMaxBlocks = 65536;
static bool walk_vec(const void* p, int P, int f) { return (P * f) % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static int64_t walk_blocks(bool vec, int R, int P, int f) {
    const int64_t items = vec ? (int64_t)R * P * (P * f / 4) : (int64_t)R * P * P;
    return std::min((items + kWalkBlock - 1) / kWalkBlock, kWalkMaxBlocks);
}
template <class... T>
static void launch_walk(void (*vec1)(const float*, int, int, T...), void (*vec2)(const float*, int, int, T...),
                        void (*vec4)(const float*, int, int, T...), void (*scalar)(const float*, int, int, int, T...), const float* x,
                        int R, int P, int f, void* stream, T... tail) {
    const bool vec = walk_vec(x, P, f);
    const dim3 grid((unsigned)walk_blocks(vec, R, P, f)), block(kWalkBlock);
    hipStream_t st = as_stream(stream);
    if (!vec) hipLaunchKernelGGL(scalar, grid, block, 0, st, x, R, P, f, tail...);
    else hipLaunchKernelGGL(f == 1 ? vec1 : f == 2 ? vec2 : vec4, grid, block, 0, st, x, R, P, tail...);
}
#define SGDFR_WALK_KERNELS(name) name##_vec_kernel<1>, name##_vec_kernel<2>, name##_vec_kernel<4>, name##_scalar_kernel

// sweep frames: the walk into put_pixel
template <int F>
__global__ __launch_bounds__(kWalkBlock) void sweep_frames_vec_kernel(const float* __restrict__ x, int R, int P, FramesOut o) {
    pooled_walk_vec<F>(x, R, P, blockDim.x, [=](int r, int oy, int ox0, const float (&v)[3][4 / F]) { put_pixels(o, r, oy, ox0, P, v); });
}

__global__ __launch_bounds__(kWalkBlock) void sweep_frames_scalar_kernel(const float* __restrict__ x, int R, int P, int f, FramesOut o) {
    pooled_walk_scalar(x, R, P, f, blockDim.x, [=](int r, int oy, int ox0, const float (&v)[3][1]) { put_pixels(o, r, oy, ox0, P, v); });
}

// ---------------------------------------------------------------- pooled image loss
// PTI above 256^2 compares the pooled image with the crop: the walk into the pooled floats and sum (pooled - real)^2, and the
// gradient of both back onto the unpooled image.  The sum has no float atomics: a lane adds its pixels in walk order, a block its
// lanes (wave_sum, then the four wave totals in wave order) into partial[blockIdx.x], one block the partials (lane t the partials
// t, t + 256, ... in double, then a pairwise tree over the lanes).  The grid follows the shape and the path alone, so mse has the same bits every call.
static_assert(kWalkBlock == 4 * kWave, "block_sum adds four wave totals");

// the sum over the block's 256 lanes, in every lane.  All lanes call it, behind their loops (wave_sum's precondition)
__device__ __forceinline__ float block_sum(float v, float (&sh)[4]) {
    v = wave_sum(v);
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

struct PoolMseOut {
    float* pooled;
    const float* real;
    float* partial;
};

template <int NPIX>
__device__ __forceinline__ void pool_mse_pixels(const PoolMseOut& o, int r, int oy, int ox0, int P, const float (&v)[3][NPIX], float& acc) {
    const int64_t PP = (int64_t)P * P;
    const int64_t at = (int64_t)r * 3 * PP + (int64_t)oy * P + ox0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int p = 0; p < NPIX; ++p) {
            o.pooled[at + c * PP + p] = v[c][p];
            const float d = v[c][p] - o.real[at + c * PP + p];
            acc = fmaf(d, d, acc);
        }
}

template <int F>
__global__ __launch_bounds__(kWalkBlock) void pool_mse_vec_kernel(const float* __restrict__ x, int R, int P, PoolMseOut o) {
    __shared__ float sh[4];
    float acc = 0.f;
    pooled_walk_vec<F>(x, R, P, blockDim.x, [=, &acc](int r, int oy, int ox0, const float (&v)[3][4 / F]) { pool_mse_pixels(o, r, oy, ox0, P, v, acc); });
    const float s = block_sum(acc, sh);
    if (threadIdx.x == 0) o.partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(kWalkBlock) void pool_mse_scalar_kernel(const float* __restrict__ x, int R, int P, int f, PoolMseOut o) {
    __shared__ float sh[4];
    float acc = 0.f;
    pooled_walk_scalar(x, R, P, f, blockDim.x, [=, &acc](int r, int oy, int ox0, const float (&v)[3][1]) { pool_mse_pixels(o, r, oy, ox0, P, v, acc); });
    const float s = block_sum(acc, sh);
    if (threadIdx.x == 0) o.partial[blockIdx.x] = s;
}

// the partials in index order per lane, then a pairwise tree over the lanes; in double, rounded once, behind the division
__global__ __launch_bounds__(kWalkBlock) void pool_mse_finish_kernel(const float* __restrict__ partial, int n, double count, float* __restrict__ mse) {
    __shared__ double sh[kWalkBlock];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kWalkBlock) s += (double)partial[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = kWalkBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) mse[0] = (float)(sh[0] / count);
}

// d(loss)/d(x) at every input pixel under output pixel `at`: one rounding per operation in both store paths, so they agree bit for bit
struct PoolMseGrad {
    const float* g_pooled;
    const float* pooled;
    const float* real;
    const float* g_mse;
    float count, ff;
};
__device__ __forceinline__ float pool_mse_grad(const PoolMseGrad& g, float gm, int64_t at) {
    const float gp = g.g_pooled ? g.g_pooled[at] : 0.f;
    const float k = g.g_mse ? __fdiv_rn(__fmul_rn(2.f, __fsub_rn(g.pooled[at], g.real[at])), g.count) : 0.f;
    return __fdiv_rn(fmaf(gm, k, gp), g.ff);
}

// 16-byte path: a lane stores four consecutive columns of one row of dx = 4 / F output pixels' values
template <int F>
__global__ __launch_bounds__(kWalkBlock) void pool_mse_bwd_vec_kernel(PoolMseGrad g, int B, int P, float* __restrict__ dx) {
    const int W = P * F, Q = W / 4;
    const int64_t items = (int64_t)B * 3 * W * Q;
    const float gm = g.g_mse ? g.g_mse[0] : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(i % Q);
        const int64_t t = i / Q;
        const int Y = (int)(t % W);
        const int64_t bc = t / W;
        const int64_t at = (bc * P + Y / F) * P + (q * 4) / F;
        float v[4];
#pragma unroll
        for (int p = 0; p < 4 / F; ++p) {
            const float e = pool_mse_grad(g, gm, at + p);
#pragma unroll
            for (int j = 0; j < F; ++j) v[p * F + j] = e;
        }
        *reinterpret_cast<float4*>(dx + (bc * W + Y) * W + (int64_t)q * 4) = float4{v[0], v[1], v[2], v[3]};
    }
}

// dword path: one element of dx per lane
__global__ __launch_bounds__(kWalkBlock) void pool_mse_bwd_scalar_kernel(PoolMseGrad g, int B, int P, int f, float* __restrict__ dx) {
    const int W = P * f;
    const int64_t items = (int64_t)B * 3 * W * W;
    const float gm = g.g_mse ? g.g_mse[0] : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        const int X = (int)(i % W);
        const int64_t t = i / W;
        const int Y = (int)(t % W);
        const int64_t bc = t / W;
        dx[i] = pool_mse_grad(g, gm, (bc * P + Y / f) * P + X / f);
    }
}

// ---------------------------------------------------------------- video frames
// rendered rows -> [B,P,K*P,3] uint8 grid frames in one pass: up to three left panels converted as grid_to_u8_kernel converts them,
// the f x f mean of x (the walk above) in the last panel.  A left panel is float32 planar [rows,3,P,P] or uint8 interleaved
// [rows,P,P,3] (the alignment crop's own bytes), read at row index[b] of its table (clamped into the table), at row b, or at its only
// row; x may be absent.  Both video entries launch these kernels: sgdfr_video_frames_f32 describes its float panels as such tables.
constexpr int kVideoLeft = 3;

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

// the walk into put_px_pixels; without x (F = 1) a lane converts four pixels of every left panel and stops there.  The sink lives
// inside the kernel and refers to its arguments (see the walk's header for why not a copy)
template <int F>
__global__ __launch_bounds__(kWalkBlock) void video_px_vec_kernel(const float* __restrict__ x, int B, int P, PxPanels g,
                                                           unsigned char* __restrict__ frames, int swap_rb) {
    const bool last = x != nullptr;
    pooled_walk_vec<F>(x, B, P, blockDim.x, [&](int b, int oy, int ox0, const float (&v)[3][4 / F]) {
        put_px_pixels<4 / F>(g, frames, b, oy, ox0, P, swap_rb, last, v);
    });
}

__global__ __launch_bounds__(kWalkBlock) void video_px_scalar_kernel(const float* __restrict__ x, int B, int P, int f, PxPanels g,
                                                              unsigned char* __restrict__ frames, int swap_rb) {
    const bool last = x != nullptr;
    pooled_walk_scalar(x, B, P, f, blockDim.x, [&](int b, int oy, int ox0, const float (&v)[3][1]) {
        put_px_pixels<1>(g, frames, b, oy, ox0, P, swap_rb, last, v);
    });
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
    launch_walk(SGDFR_WALK_KERNELS(sweep_frames), x, R, P, f, stream, o);
    return check_launch("sweep_frames");
}

constexpr int kPoolMseMaxRows = 4096;
static bool pool_mse_ok(int B, int P) { return B >= 1 && B <= kPoolMseMaxRows && P >= 1 && P <= 8192; }
// one float per block of the widest walk, the dword one: B * P * P items
static int64_t pool_mse_partials(int B, int P) { return walk_blocks(false, B, P, 1); }

extern "C" int64_t sgdfr_pool_mse_workspace_bytes(int B, int P) {
    return pool_mse_ok(B, P) ? pool_mse_partials(B, P) * (int64_t)sizeof(float) : -1;
}

extern "C" int sgdfr_pool_mse_f32(const float* x, const float* real, int B, int P, int f, float* pooled, float* mse, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(f == 1 || f == 2 || f == 4, "pool_mse: the pooling factor must be 1, 2 or 4 (256, 512, 1024 generators), got %d", f);
    SGDFR_REQUIRE(pool_mse_ok(B, P), "pool_mse: bad shape B=%d P=%d (1..%d rows, P in 1..8192)", B, P, kPoolMseMaxRows);
    SGDFR_REQUIRE(x && real && pooled && mse && workspace, "pool_mse: null pointer");
    SGDFR_REQUIRE(workspace_bytes >= pool_mse_partials(B, P) * (int64_t)sizeof(float), "pool_mse: workspace of %lld bytes, B=%d P=%d need %lld",
                  (long long)workspace_bytes, B, P, (long long)(pool_mse_partials(B, P) * (int64_t)sizeof(float)));
    PoolMseOut o{pooled, real, reinterpret_cast<float*>(workspace)};
    const int blocks = (int)walk_blocks(walk_vec(x, P, f), B, P, f);       // the grid launch_walk gives the walk
    launch_walk(SGDFR_WALK_KERNELS(pool_mse), x, B, P, f, stream, o);
    if (check_launch("pool_mse")) return 2;
    hipLaunchKernelGGL(pool_mse_finish_kernel, dim3(1), dim3(kWalkBlock), 0, as_stream(stream), (const float*)o.partial, blocks,
                       3.0 * B * P * P, mse);
    return check_launch("pool_mse finish");
}

extern "C" int sgdfr_pool_mse_bwd_f32(const float* g_pooled, const float* pooled, const float* real, const float* g_mse, int B, int P,
                                      int f, float* dx, void* stream) {
    SGDFR_REQUIRE(f == 1 || f == 2 || f == 4, "pool_mse_bwd: the pooling factor must be 1, 2 or 4 (256, 512, 1024 generators), got %d", f);
    SGDFR_REQUIRE(pool_mse_ok(B, P), "pool_mse_bwd: bad shape B=%d P=%d (1..%d rows, P in 1..8192)", B, P, kPoolMseMaxRows);
    SGDFR_REQUIRE(dx && (!g_mse || (pooled && real)), "pool_mse_bwd: null pointer");
    const PoolMseGrad g{g_pooled, pooled, real, g_mse, (float)(3.0 * B * P * P), (float)(f * f)};
    const int W = P * f;
    const bool vec = walk_vec(dx, P, f);
    const int64_t items = (int64_t)B * 3 * W * (vec ? W / 4 : W);
    const dim3 grid((unsigned)std::min((items + kWalkBlock - 1) / kWalkBlock, kWalkMaxBlocks)), block(kWalkBlock);
    hipStream_t st = as_stream(stream);
    if (!vec) hipLaunchKernelGGL(pool_mse_bwd_scalar_kernel, grid, block, 0, st, g, B, P, f, dx);
    else if (f == 1) hipLaunchKernelGGL(pool_mse_bwd_vec_kernel<1>, grid, block, 0, st, g, B, P, dx);
    else if (f == 2) hipLaunchKernelGGL(pool_mse_bwd_vec_kernel<2>, grid, block, 0, st, g, B, P, dx);
    else hipLaunchKernelGGL(pool_mse_bwd_vec_kernel<4>, grid, block, 0, st, g, B, P, dx);
    return check_launch("pool_mse_bwd");
}

// the float panels of this entry as the tables of the next: stride 0 is a table of one row, stride 3 * P * P one of B rows
extern "C" int sgdfr_video_frames_f32(const float* x, int B, int P, int f, const float* const* panels, const int64_t* bstrides, int n_left,
                                      unsigned char* frames, int swap_rb, void* stream) {
    SGDFR_REQUIRE(f == 1 || f == 2 || f == 4, "video_frames: the pooling factor must be 1, 2 or 4 (256, 512, 1024 generators), got %d", f);
    SGDFR_REQUIRE(B >= 0 && P >= 1 && P <= 8192, "video_frames: bad shape B=%d P=%d", B, P);
    SGDFR_REQUIRE(n_left >= 0 && n_left <= kVideoLeft, "video_frames: %d left panels (0..%d)", n_left, kVideoLeft);
    SGDFR_REQUIRE(n_left == 0 || (panels && bstrides), "video_frames: left panels without their pointer and stride arrays");
    PxPanels g{};
    g.n = n_left;
    for (int k = 0; k < n_left; ++k) {
        SGDFR_REQUIRE(bstrides[k] == 0 || bstrides[k] == (int64_t)3 * P * P, "video_frames: panel %d is one image (stride 0) or one per row", k);
        g.data[k] = panels[k];
        g.kind[k] = SGDFR_PANEL_F32;
        g.rows[k] = bstrides[k] == 0 ? 1 : B;
    }
    if (B == 0) return 0;
    SGDFR_REQUIRE(x && frames, "video_frames: null pointer");
    launch_walk(SGDFR_WALK_KERNELS(video_px), x, B, P, f, stream, g, frames, swap_rb);
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
    launch_walk(SGDFR_WALK_KERNELS(video_px), x, B, P, f, stream, g, frames, swap_rb);
    return check_launch("video_frames_px");
}
