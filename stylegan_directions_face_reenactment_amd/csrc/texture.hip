// DECA's texture side, forward only (libs/DECA/decalib/models/FLAME.py:216-262 FLAMETex, deca.py:180-181 and 193-199 with
// utils/renderer.py:193-206 add_SHlight and 331-340 world2uv).  Contract: include/sgdfr.h.
//
// FLAMETex.  The reference forms mean + basis . code at the source size (512 x 512 x 3), keeps every second texel (F.interpolate,
// nearest) and flips the channels: three quarters of the basis are never used.  The pack holds the kept texels only, already in the
// output's order: mean [3][uv][uv], then basis [n_tex][3][uv][uv]; the nearest-neighbour source index of every output row and column
// comes from the host.
//   prepack   1 thread / output element    gathers mean and the n_tex basis values of its source texel
//   forward   1 thread / 4 (or 1) elements the codes of up to 32 rows sit in LDS, eight accumulators per element in registers (four
//              of 8 rows                   waves of a block share the elements and split the rows); k runs ascending with one fmaf per
//                                          (row, k), then mean + sum.  The pack is streamed from memory once per group of 32 rows with
//                                          16-byte loads (4-byte when 3 uv^2 is no multiple of 4), eight planes in flight; a row's
//                                          result does not depend on the rows beside it.
// The UV texture pass is one launch, 1 thread / (row, texel): add_SHlight of the UV normal map, albedo . shading, world2uv of the
// projected vertices' x, y through the layout's table, grid_sample of the input image there and the blend with face_eye_mask.  The
// maps in between (uv_pverts, uv_gt) are written only when asked for.
//
// Floating-point contraction is OFF for the whole file (the UV pass is compared with a restatement that does not fuse); the texture
// sum names its fmaf.
#include <math.h>

#include "common.h"
#include "mesh_sample.h"

#pragma clang fp contract(off)

namespace sgdfr {
namespace {

constexpr int kMaxTex = 200, kMaxUv = 1024, kMaxSource = 4096, kMaxRows = 4096;
constexpr int kThreads = 256;

bool tex_sizes_ok(int uv, int n_tex) { return uv >= 1 && uv <= kMaxUv && n_tex >= 1 && n_tex <= kMaxTex; }

__global__ __launch_bounds__(kThreads) void flametex_prepack_kernel(const float* __restrict__ mean, const float* __restrict__ basis,
                                                                    const int* __restrict__ index_y, const int* __restrict__ index_x, int Hs,
                                                                    int Ws, int uv, int n_tex, float* __restrict__ pack) {
    const int P = 3 * uv * uv, e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= P) return;
    const int c = e / (uv * uv), y = (e - c * uv * uv) / uv, x = e - c * uv * uv - y * uv;
    const unsigned sy = (unsigned)index_y[y], sx = (unsigned)index_x[x];
    const bool ok = sy < (unsigned)Hs && sx < (unsigned)Ws;               // the host checks the table; nothing is read outside anyway
    const size_t src = ((size_t)sy * Ws + sx) * 3 + (2 - c);              // texture[:, [2,1,0]]
    pack[e] = ok ? mean[src] : 0.f;
    for (int k = 0; k < n_tex; ++k) pack[(size_t)(1 + k) * P + e] = ok ? basis[src * n_tex + k] : 0.f;
}

template <int VEC>
struct Vec;
template <>
struct Vec<4> {
    using T = float4;
};
template <>
struct Vec<1> {
    using T = float;
};

__device__ __forceinline__ float fma_v(float b, float c, float a) { return fmaf(b, c, a); }
__device__ __forceinline__ float4 fma_v(float4 b, float c, float4 a) {
    return make_float4(fmaf(b.x, c, a.x), fmaf(b.y, c, a.y), fmaf(b.z, c, a.z), fmaf(b.w, c, a.w));
}
__device__ __forceinline__ float add_v(float m, float a) { return m + a; }
__device__ __forceinline__ float4 add_v(float4 m, float4 a) { return make_float4(m.x + a.x, m.y + a.y, m.z + a.z, m.w + a.w); }
__device__ __forceinline__ void zero_v(float& a) { a = 0.f; }
__device__ __forceinline__ void zero_v(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }

// A block is WAVES waves over the same 64 x VEC output elements; wave w takes rows 8 w .. 8 w + 7 of every group of 8 WAVES rows, so its
// eight accumulators stay in registers.  The waves of a block ask for the same planes at about the same time: the pack comes from
// memory once and from the compute unit's cache for the other waves.  At the real size (192 K elements, float4) that is 768 blocks
// and, from 17 rows up, 12 waves a compute unit; kAhead planes are fetched before the first is used.
constexpr int kRB = 8, kAhead = 8;

template <int VEC, int WAVES>
__global__ __launch_bounds__(kWave* WAVES) void flametex_kernel(const float* __restrict__ code, int rows, const float* __restrict__ pack, int P,
                                                                int n_tex, float* __restrict__ out) {
    using T = typename Vec<VEC>::T;
    constexpr int GROUP = kRB * WAVES;
    __shared__ float s_code[GROUP][kMaxTex];
    const int t = threadIdx.x, wave = t / kWave;
    const int64_t e = ((int64_t)blockIdx.x * kWave + (t & (kWave - 1))) * VEC;
    const bool live = e < P;                                              // VEC = 4 only where P is a multiple of 4: e + 3 < P too
    for (int r0 = 0; r0 < rows; r0 += GROUP) {
        __syncthreads();                                                  // the previous group of rows is through with s_code
        for (int i = t; i < GROUP * n_tex; i += kWave * WAVES) {
            const int r = i / n_tex, k = i - r * n_tex;
            s_code[r][k] = r0 + r < rows ? code[(size_t)(r0 + r) * n_tex + k] : 0.f;
        }
        __syncthreads();
        const int row0 = r0 + wave * kRB;                                 // this wave's first row
        if (!live || row0 >= rows) continue;
        const float(*c)[kMaxTex] = s_code + wave * kRB;
        T acc[kRB];
#pragma unroll
        for (int r = 0; r < kRB; ++r) zero_v(acc[r]);
        for (int k0 = 0; k0 < n_tex; k0 += kAhead) {
            T b[kAhead];
#pragma unroll
            for (int j = 0; j < kAhead; ++j)
                if (k0 + j < n_tex) b[j] = *(const T*)(pack + (size_t)(1 + k0 + j) * P + e);
#pragma unroll
            for (int j = 0; j < kAhead; ++j) {                            // k = k0 + j ascending: the order of the sum is fixed
                if (k0 + j >= n_tex) break;
#pragma unroll
                for (int r = 0; r < kRB; ++r) acc[r] = fma_v(b[j], c[r][k0 + j], acc[r]);
            }
        }
        const T m = *(const T*)(pack + e);
#pragma unroll
        for (int r = 0; r < kRB; ++r)
            if (row0 + r < rows) *(T*)(out + (size_t)(row0 + r) * P + e) = add_v(m, acc[r]);
    }
}

template <int VEC>
int launch_flametex(const float* code, int rows, const float* pack, int P, int n_tex, float* out, hipStream_t st) {
    const int blocks = (int)(((int64_t)P + (int64_t)kWave * VEC - 1) / ((int64_t)kWave * VEC));
    if (rows <= kRB)
        flametex_kernel<VEC, 1><<<blocks, kWave, 0, st>>>(code, rows, pack, P, n_tex, out);
    else if (rows <= 2 * kRB)
        flametex_kernel<VEC, 2><<<blocks, 2 * kWave, 0, st>>>(code, rows, pack, P, n_tex, out);
    else
        flametex_kernel<VEC, 4><<<blocks, 4 * kWave, 0, st>>>(code, rows, pack, P, n_tex, out);
    return check_launch("texture flametex_kernel");
}

// ---------------------------------------------------------------------------------------------------------------- the UV pass
struct UvTexIO {
    const float* albedo;       // [B,3,S,S] or NULL (use_tex False)
    const float* uv_normals;   // [B,3,S,S]
    const float* light;        // [B,9,3]
    float sh[9];
    const float* trans_verts;  // [B,V,3]
    const float* images;       // [B,3,H,W]
    int H, W;
    const int* faces;          // [F,3]
    const int* pix_to_face;    // [S,S]
    const float* bary;         // [S,S,3]
    const float* mask;         // [S,S]
    float* uv_shading;         // [B,3,S,S] or NULL
    float* uv_texture;         // [B,3,S,S] or NULL
    float* uv_texture_gt;      // [B,3,S,S] or NULL
    float* uv_pverts;          // [B,3,S,S] or NULL
    float* uv_gt;              // [B,3,S,S] or NULL
};

__global__ __launch_bounds__(kThreads) void uvtexture_kernel(int V, int F, int S, UvTexIO io) {
    const int b = blockIdx.y, t = blockIdx.x * kThreads + threadIdx.x, plane = S * S;
    if (t >= plane) return;
    const size_t o = (size_t)b * 3 * plane + t;
    float n[3], sh[3], p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] = io.uv_normals[o + (size_t)c * plane];
    sh_light(io.sh, io.light + (size_t)b * 27, n, sh);
    // world2uv(trans_verts): (0, 0) where no face covers
    bary_gather3(io.trans_verts + (size_t)b * V * 3, V, io.faces, F, io.pix_to_face, io.bary, t, p);
    float gt[3] = {0.f, 0.f, 0.f};
    if (io.uv_texture_gt || io.uv_gt) grid_sample3(io.images + (size_t)b * 3 * io.H * io.W, io.H, io.W, p[0], p[1], gt);
    const float m = io.mask[t];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t at = o + (size_t)c * plane;
        const float tex = io.albedo ? io.albedo[at] * sh[c] : 1.0f;
        if (io.uv_shading) io.uv_shading[at] = sh[c];
        if (io.uv_texture && io.albedo) io.uv_texture[at] = tex;
        if (io.uv_texture_gt) io.uv_texture_gt[at] = gt[c] * m + tex * (1.0f - m) * 0.7f;
        if (io.uv_pverts) io.uv_pverts[at] = p[c];
        if (io.uv_gt) io.uv_gt[at] = gt[c];
    }
}

}  // namespace
}  // namespace sgdfr

using namespace sgdfr;

extern "C" int64_t sgdfr_flametex_pack_elems(int uv, int n_tex) {
    if (!tex_sizes_ok(uv, n_tex)) return -1;
    return (int64_t)(1 + n_tex) * 3 * uv * uv;
}

extern "C" int sgdfr_flametex_prepack_f32(const void* const* params, int Hs, int Ws, int uv, int n_tex, float* pack, void* stream) {
    SGDFR_REQUIRE(params && params[0] && params[1] && params[2] && params[3] && pack, "flametex_prepack: null pointer");
    SGDFR_REQUIRE(tex_sizes_ok(uv, n_tex), "flametex_prepack: uv_size=%d n_tex=%d (1..%d, 1..%d)", uv, n_tex, kMaxUv, kMaxTex);
    SGDFR_REQUIRE(Hs >= 1 && Hs <= kMaxSource && Ws >= 1 && Ws <= kMaxSource, "flametex_prepack: source %d x %d (1..%d)", Hs, Ws, kMaxSource);
    const int P = 3 * uv * uv;
    flametex_prepack_kernel<<<(P + kThreads - 1) / kThreads, kThreads, 0, as_stream(stream)>>>(
        (const float*)params[0], (const float*)params[1], (const int*)params[2], (const int*)params[3], Hs, Ws, uv, n_tex, pack);
    return check_launch("texture flametex_prepack_kernel");
}

extern "C" int sgdfr_flametex_forward_f32(const float* code, int rows, const float* pack, int uv, int n_tex, float* albedo, void* stream) {
    SGDFR_REQUIRE(code && pack && albedo, "flametex_forward: null pointer");
    SGDFR_REQUIRE(tex_sizes_ok(uv, n_tex), "flametex_forward: uv_size=%d n_tex=%d (1..%d, 1..%d)", uv, n_tex, kMaxUv, kMaxTex);
    SGDFR_REQUIRE(rows >= 1 && rows <= kMaxRows, "flametex_forward: rows=%d (1..%d)", rows, kMaxRows);
    const int P = 3 * uv * uv;
    // 16-byte loads need every plane of the pack, and every row of the output, to start on a 16-byte boundary
    if (P % 4 == 0 && ((uintptr_t)pack & 15) == 0 && ((uintptr_t)albedo & 15) == 0)
        return launch_flametex<4>(code, rows, pack, P, n_tex, albedo, as_stream(stream));
    return launch_flametex<1>(code, rows, pack, P, n_tex, albedo, as_stream(stream));
}

extern "C" int sgdfr_texture_uv_f32(const float* albedo, const float* uv_normals, const float* light, const float* sh_constants,
                                    const float* trans_verts, const float* images, int rows, int V, int H, int W, const int* faces, int F,
                                    const int* pix_to_face, const float* bary, const float* mask, int S, float* uv_shading, float* uv_texture,
                                    float* uv_texture_gt, float* uv_pverts, float* uv_gt, void* stream) {
    SGDFR_REQUIRE(uv_normals && light && sh_constants && trans_verts && images && faces && pix_to_face && bary && mask,
                  "texture_uv: null pointer");
    SGDFR_REQUIRE(uv_shading || uv_texture || uv_texture_gt || uv_pverts || uv_gt, "texture_uv: no output");
    SGDFR_REQUIRE(!uv_texture || albedo, "texture_uv: uv_texture needs an albedo");
    SGDFR_REQUIRE(rows >= 1 && rows <= kMaxRows && V >= 1 && V <= (1 << 24) && F >= 1 && F <= (1 << 24) && S >= 1 && S <= kMaxUv,
                  "texture_uv: rows=%d V=%d F=%d uv_size=%d (rows 1..%d, V and F 1..2^24, uv_size 1..%d)", rows, V, F, S, kMaxRows, kMaxUv);
    SGDFR_REQUIRE(H >= 1 && H <= kMaxSource && W >= 1 && W <= kMaxSource, "texture_uv: image %d x %d (1..%d)", H, W, kMaxSource);
    UvTexIO io{albedo, uv_normals, light, {}, trans_verts, images, H, W, faces, pix_to_face, bary, mask, uv_shading, uv_texture, uv_texture_gt,
               uv_pverts, uv_gt};
    for (int k = 0; k < 9; ++k) io.sh[k] = sh_constants[k];
    uvtexture_kernel<<<dim3((S * S + kThreads - 1) / kThreads, rows), kThreads, 0, as_stream(stream)>>>(V, F, S, io);
    return check_launch("texture uvtexture_kernel");
}
