// The three per-pixel helpers the mesh kernels share (shaperender.hip, texture.hip, detail.hip): grid_sample of a three-channel map,
// add_SHlight at one normal, and the guarded barycentric gather through a (pix_to_face, bary) table.  Each is compared bit for bit
// with a restatement that does not fuse, so each body turns floating-point contraction OFF for itself, whatever the includer has set.
#pragma once
#include <stddef.h>

#include <hip/hip_runtime.h>

namespace sgdfr {

// F.grid_sample(bilinear, zeros, align_corners=False) of one [3,H,W] map at (gx, gy): a neighbour outside the map adds nothing
__device__ __forceinline__ void grid_sample3(const float* __restrict__ map, int H, int W, float gx, float gy, float (&r)[3]) {
#pragma clang fp contract(off)
    const float ix = ((gx + 1.0f) * (float)W - 1.0f) * 0.5f, iy = ((gy + 1.0f) * (float)H - 1.0f) * 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    const float ax = ix - fx, ay = iy - fy, bx = (fx + 1.0f) - ix, by = (fy + 1.0f) - iy;
    r[0] = r[1] = r[2] = 0.f;
    // a coordinate that is not finite or far outside fails every test below (the casts are then never made)
    if (!(fx >= -1.0f && fx < (float)W && fy >= -1.0f && fy < (float)H)) return;
    const int x0 = (int)fx, y0 = (int)fy;
    const size_t plane = (size_t)H * W;
    const float w[4] = {bx * by, ax * by, bx * ay, ax * ay};      // nw, ne, sw, se
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + (k & 1), y = y0 + (k >> 1);
        if (x < 0 || x >= W || y < 0 || y >= H) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] += map[c * plane + (size_t)y * W + x] * w[k];
    }
}

// SRenderY.add_SHlight at one normal: sum_k coeff[k][c] (basis_k(n) constants[k]), k ascending; coeff [9][3]
__device__ __forceinline__ void sh_light(const float (&constants)[9], const float* coeff, const float (&n)[3], float (&r)[3]) {
#pragma clang fp contract(off)
    const float basis[9] = {1.0f, n[0], n[1], n[2], n[0] * n[1], n[0] * n[2], n[1] * n[2], n[0] * n[0] - n[1] * n[1],
                            3.0f * (n[2] * n[2]) - 1.0f};
    r[0] = r[1] = r[2] = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float v = basis[k] * constants[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] += coeff[k * 3 + c] * v;
    }
}

// world2uv at one texel: r = w0 a + w1 b + w2 c over the corners of pix_to_face[texel], values [V,3] of one image.  False, and r = 0,
// where no face covers or an index points outside the tables.
__device__ __forceinline__ bool bary_gather3(const float* __restrict__ values, int V, const int* __restrict__ faces, int F,
                                             const int* __restrict__ pix_to_face, const float* __restrict__ bary, int texel, float (&r)[3]) {
#pragma clang fp contract(off)
    r[0] = r[1] = r[2] = 0.f;
    const unsigned f = (unsigned)pix_to_face[texel];
    if (f >= (unsigned)F) return false;
    const unsigned i0 = (unsigned)faces[f * 3], i1 = (unsigned)faces[f * 3 + 1], i2 = (unsigned)faces[f * 3 + 2];
    if (i0 >= (unsigned)V || i1 >= (unsigned)V || i2 >= (unsigned)V) return false;
    const float w0 = bary[texel * 3], w1 = bary[texel * 3 + 1], w2 = bary[texel * 3 + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = w0 * values[i0 * 3 + c] + w1 * values[i1 * 3 + c] + w2 * values[i2 * 3 + c];
    return true;
}

}  // namespace sgdfr
