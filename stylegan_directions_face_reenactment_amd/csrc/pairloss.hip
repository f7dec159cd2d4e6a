// The loss arithmetic that only the paired training step has (libs/utilities/utils_train.py:435-499 calculate_losses_paired):
// the [-1,1] -> [0,255] image transform (libs/utilities/image_utils.py:87-94 torch_range_1_to_255), the pixel-wise L1 on the
// transformed images (libs/criteria/losses.py:14-18) and the latent regulariser L1Loss(shifted_latents, target_w).
//
// Stock torch spends about a dozen elementwise and reduction launches on these, and as many again in the backward.  Here the
// forward is one streaming pass (both transforms, both optional image stores and the block partials of the mean) plus a finish
// launch that sums the partials in a fixed order; the backward is one launch that recomputes the transform and folds the
// optional upstream gradient of the materialised t(x) -- LPIPS's dL/dx in the paired step -- into the same store.
//
// Element -> thread assignment.  A tile is kTile = 256 threads x 4 groups x 4 floats; thread `tid` of the block that owns tile
// `k` takes the four floats at k*kTile + j*1024 + tid*4 for j = 0..3, so that a wave reads 1 KiB of contiguous memory per
// instruction.  The assignment, the grid and the partial layout depend on n alone -- NOT on the pointers: where a pointer
// breaks 16-byte alignment the same four floats are moved by dword accesses, they are added in the same order, and the result
// has the same bits.  Sums: float within a tile (16 terms), double across the tiles of a thread (a grid-stride loop, entered
// above 2048 tiles only), a float tree over the block, and a float tree over the partials in the finish kernel.  No atomics.
#include "common.h"

namespace sgdfr {

constexpr int kPlThreads = 256, kPlGroups = 4, kPlTile = kPlThreads * kPlGroups * 4, kPlMaxBlocks = 2048;
constexpr float kPlSpan = 2.00001f;             // max_val - min_val + 1e-5 of torch_range_1_to_255, as the float32 torch divides by

static inline int pl_blocks(int64_t n) {
    const int64_t tiles = (n + kPlTile - 1) / kPlTile;
    return (int)(tiles < 1 ? 1 : tiles > kPlMaxBlocks ? kPlMaxBlocks : tiles);
}

// clone, clamp_(-1, 1), add_(1), div_(2 + 1e-5), mul(255): one float32 rounding each, in that order (a NaN stays a NaN, as in torch)
__device__ __forceinline__ float pl_clamp(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }
__device__ __forceinline__ float pl_t(float v) { return __fmul_rn(__fdiv_rn(__fadd_rn(pl_clamp(v), 1.f), kPlSpan), 255.f); }
__device__ __forceinline__ float pl_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }      // torch.sign: sign(0) = 0

// (a float4 is a struct of four floats to the optimiser, which splits its store and sinks the last dword into the tail path:
// dwordx3 + dword.  A vector-typed access stays one 16-byte instruction.)
typedef float pl_f4 __attribute__((ext_vector_type(4)));

// four floats at p[0..3]; lanes at or beyond `left` are not touched (loads give 0)
template <bool VEC>
__device__ __forceinline__ float4 pl_load4(const float* __restrict__ p, int64_t left) {
    if (VEC && left >= 4) {
        const pl_f4 q = *reinterpret_cast<const pl_f4*>(p);
        return make_float4(q.x, q.y, q.z, q.w);
    }
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (left > 0) v.x = p[0];
    if (left > 1) v.y = p[1];
    if (left > 2) v.z = p[2];
    if (left > 3) v.w = p[3];
    return v;
}
template <bool VEC>
__device__ __forceinline__ void pl_store4(float* __restrict__ p, int64_t left, float4 v) {
    if (VEC && left >= 4) {
        *reinterpret_cast<pl_f4*>(p) = pl_f4{v.x, v.y, v.z, v.w};
        return;
    }
    if (left > 0) p[0] = v.x;
    if (left > 1) p[1] = v.y;
    if (left > 2) p[2] = v.z;
    if (left > 3) p[3] = v.w;
}

// sum over the block, valid in thread 0; every thread of the block calls it (wave_sum needs all 64 lanes)
__device__ __forceinline__ float pl_block_sum(float v) {
    __shared__ float part[kPlThreads / kWave];
    v = wave_sum(v);
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = v;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(kPlThreads) void pairloss_forward_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t n,
                                                                     float* __restrict__ x255, float* __restrict__ y255,
                                                                     float* __restrict__ partials) {
    const int64_t tiles = (n + kPlTile - 1) / kPlTile;
    double acc = 0.0;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < kPlGroups; ++j) {
            const int64_t e = tile * kPlTile + (int64_t)j * (kPlThreads * 4) + (int64_t)threadIdx.x * 4;
            const int64_t left = n - e;
            if (left <= 0) continue;
            float4 a = pl_load4<VEC>(x + e, left), b = pl_load4<VEC>(y + e, left);
            if (MODE == SGDFR_PAIRLOSS_RANGE255) {
                a = make_float4(pl_t(a.x), pl_t(a.y), pl_t(a.z), pl_t(a.w));
                b = make_float4(pl_t(b.x), pl_t(b.y), pl_t(b.z), pl_t(b.w));
                if (x255) pl_store4<VEC>(x255 + e, left, a);
                if (y255) pl_store4<VEC>(y255 + e, left, b);
            }
            // (lanes beyond n hold the same value in a and b: they add an exact 0)
            s += fabsf(b.x - a.x);
            s += fabsf(b.y - a.y);
            s += fabsf(b.z - a.z);
            s += fabsf(b.w - a.w);
        }
        acc += (double)s;
    }
    const float total = pl_block_sum((float)acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// loss[0] = (sum of the partials, in a fixed order) / n
__global__ __launch_bounds__(kPlThreads) void pairloss_finish_kernel(const float* __restrict__ partials, int count, int64_t n,
                                                                    float* __restrict__ loss) {
    float s = 0.f;
    for (int i = threadIdx.x; i < count; i += kPlThreads) s += partials[i];
    const float total = pl_block_sum(s);
    if (threadIdx.x == 0) loss[0] = __fdiv_rn(total, (float)n);
}

// plain:    dx = sign(x - y) * (g / n)
// range255: dx = m(x) * ((g255 + sign(t(x) - t(y)) * (g / n)) * 255 / (2 + 1e-5)), m(x) = 1 on -1 <= x <= 1 and exactly 0 elsewhere
template <int MODE, bool VEC>
__global__ __launch_bounds__(kPlThreads) void pairloss_backward_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t n,
                                                                      const float* __restrict__ grad_loss,
                                                                      const float* __restrict__ grad_x255, float* __restrict__ dx) {
    const float gn = grad_loss ? __fdiv_rn(grad_loss[0], (float)n) : 0.f;
    const int64_t tiles = (n + kPlTile - 1) / kPlTile;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
        for (int j = 0; j < kPlGroups; ++j) {
            const int64_t e = tile * kPlTile + (int64_t)j * (kPlThreads * 4) + (int64_t)threadIdx.x * 4;
            const int64_t left = n - e;
            if (left <= 0) continue;
            const float4 a = pl_load4<VEC>(x + e, left), b = pl_load4<VEC>(y + e, left);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
            float r[4];
            if (MODE == SGDFR_PAIRLOSS_RANGE255) {
                float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
                if (grad_x255) u = pl_load4<VEC>(grad_x255 + e, left);
                const float uv[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float up = __fadd_rn(uv[k], __fmul_rn(pl_sign(pl_t(av[k]) - pl_t(bv[k])), gn));
                    const bool inside = av[k] >= -1.f && av[k] <= 1.f;              // torch's clamp backward: the bounds pass
                    r[k] = inside ? __fdiv_rn(__fmul_rn(up, 255.f), kPlSpan) : 0.f;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = __fmul_rn(pl_sign(av[k] - bv[k]), gn);
            }
            pl_store4<VEC>(dx + e, left, make_float4(r[0], r[1], r[2], r[3]));
        }
    }
}

static inline bool pl_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace sgdfr

using namespace sgdfr;

extern "C" int64_t sgdfr_pairloss_workspace_bytes(int n) {
    if (n < 1) return -1;
    return (int64_t)pl_blocks(n) * (int64_t)sizeof(float);
}

extern "C" int sgdfr_pairloss_forward_f32(const float* x, const float* y, int64_t n, int mode, float* x255, float* y255, float* loss,
                                          void* workspace, int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(n >= 1, "pairloss: n must be at least 1, got %lld", (long long)n);
    SGDFR_REQUIRE(mode == SGDFR_PAIRLOSS_PLAIN || mode == SGDFR_PAIRLOSS_RANGE255, "pairloss: unknown mode %d", mode);
    SGDFR_REQUIRE(x && y && loss && workspace, "pairloss: null pointer");
    SGDFR_REQUIRE(mode == SGDFR_PAIRLOSS_RANGE255 || (!x255 && !y255), "pairloss: the plain mode writes no images");
    SGDFR_REQUIRE((!x255 || (x255 != x && x255 != y)) && (!y255 || (y255 != x && y255 != y)) && (!x255 || x255 != y255),
                  "pairloss: the 0..255 images must not alias the inputs or each other");
    const int blocks = pl_blocks(n);
    SGDFR_REQUIRE(workspace_bytes >= (int64_t)blocks * (int64_t)sizeof(float), "pairloss: workspace of %lld bytes, need %lld",
                  (long long)workspace_bytes, (long long)blocks * (long long)sizeof(float));
    SGDFR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, "pairloss: the workspace must be 4-byte aligned");
    float* partials = static_cast<float*>(workspace);
    const bool vec = pl_aligned(x) && pl_aligned(y) && pl_aligned(x255) && pl_aligned(y255);
    hipStream_t st = as_stream(stream);
    if (mode == SGDFR_PAIRLOSS_PLAIN) {
        if (vec) hipLaunchKernelGGL((pairloss_forward_kernel<SGDFR_PAIRLOSS_PLAIN, true>), dim3(blocks), dim3(kPlThreads), 0, st, x, y, n, x255, y255, partials);
        else hipLaunchKernelGGL((pairloss_forward_kernel<SGDFR_PAIRLOSS_PLAIN, false>), dim3(blocks), dim3(kPlThreads), 0, st, x, y, n, x255, y255, partials);
    } else {
        if (vec) hipLaunchKernelGGL((pairloss_forward_kernel<SGDFR_PAIRLOSS_RANGE255, true>), dim3(blocks), dim3(kPlThreads), 0, st, x, y, n, x255, y255, partials);
        else hipLaunchKernelGGL((pairloss_forward_kernel<SGDFR_PAIRLOSS_RANGE255, false>), dim3(blocks), dim3(kPlThreads), 0, st, x, y, n, x255, y255, partials);
    }
    if (int rc = check_launch("pairloss_forward")) return rc;
    hipLaunchKernelGGL(pairloss_finish_kernel, dim3(1), dim3(kPlThreads), 0, st, partials, blocks, n, loss);
    return check_launch("pairloss_finish");
}

extern "C" int sgdfr_pairloss_backward_f32(const float* x, const float* y, int64_t n, int mode, const float* grad_loss,
                                           const float* grad_x255, float* dx, void* stream) {
    SGDFR_REQUIRE(n >= 1, "pairloss: n must be at least 1, got %lld", (long long)n);
    SGDFR_REQUIRE(mode == SGDFR_PAIRLOSS_PLAIN || mode == SGDFR_PAIRLOSS_RANGE255, "pairloss: unknown mode %d", mode);
    SGDFR_REQUIRE(x && y && dx, "pairloss: null pointer");
    SGDFR_REQUIRE(mode == SGDFR_PAIRLOSS_RANGE255 || !grad_x255, "pairloss: the plain mode has no image gradient");
    const int blocks = pl_blocks(n);
    const bool vec = pl_aligned(x) && pl_aligned(y) && pl_aligned(grad_x255) && pl_aligned(dx);
    hipStream_t st = as_stream(stream);
    if (mode == SGDFR_PAIRLOSS_PLAIN) {
        if (vec) hipLaunchKernelGGL((pairloss_backward_kernel<SGDFR_PAIRLOSS_PLAIN, true>), dim3(blocks), dim3(kPlThreads), 0, st, x, y, n, grad_loss, grad_x255, dx);
        else hipLaunchKernelGGL((pairloss_backward_kernel<SGDFR_PAIRLOSS_PLAIN, false>), dim3(blocks), dim3(kPlThreads), 0, st, x, y, n, grad_loss, grad_x255, dx);
    } else {
        if (vec) hipLaunchKernelGGL((pairloss_backward_kernel<SGDFR_PAIRLOSS_RANGE255, true>), dim3(blocks), dim3(kPlThreads), 0, st, x, y, n, grad_loss, grad_x255, dx);
        else hipLaunchKernelGGL((pairloss_backward_kernel<SGDFR_PAIRLOSS_RANGE255, false>), dim3(blocks), dim3(kPlThreads), 0, st, x, y, n, grad_loss, grad_x255, dx);
    }
    return check_launch("pairloss_backward");
}
