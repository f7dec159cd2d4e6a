// DECA's shape renderer (libs/DECA/decalib/utils/renderer.py:237-293 SRenderY.render_shape with util.vertex_normals and the fixed
// settings of Pytorch3dRasterizer): projection, vertex normals, a tiled z-buffer rasteriser and the lit grey panel, forward only, on the
// caller's stream with no host round trip.  Contract: include/sgdfr.h.
//   project    1 thread / vertex        batch_orth_proj, the y / z flip and the z offset -> projected vertices
//   normals    1 thread / vertex        gather over the vertex -> (face, corner) table in (face, corner) order, then n / max(|n|, 1e-6);
//                                       once for the world vertices (three components), once for the projected ones (z only)
//   setup      1 thread / (image, face) the face record (corners, area + 1e-8) and its pixel bounding box as four 16-bit ints; an
//                                       empty box (x0 > x1) marks a face that is skipped or wholly outside
//   raster     1 block / 16 x 16 tile   walks the faces in chunks of 256: one bounding-box test per thread, the hits compacted in face
//                                       order (wave ballot, popcount prefix, cross-wave offset in LDS), their records copied to LDS,
//                                       then every thread tests its own pixel against the compacted list; the epilogue interpolates,
//                                       lights and blends the winner, so no attribute image exists
// No global bins, no atomics, a fixed face order: the result does not depend on scheduling.  All 256 threads read the same LDS record
// at the same time (three ds_read_b128 of one address: a broadcast, no bank conflict).
//
// sgdfr_shaperender_detail_f32 is the same five launches with raster_kernel<true>: one rasterisation serves the smooth panel and the
// detail panel, whose shading normal is the UV normal map sampled at the pixel's interpolated UV coordinate (grid_sample rules).  The
// reference renders three times and adds z_offset = 10 to the caller's projected vertices in place each time (renderer.py:255); the
// projection is orthographic, so a constant shift of z changes no coverage, no barycentric and no depth order, and every |z| < 10
// stays in front of the z >= 0 cut whether 10, 20 or 30 was added: z_offset stays 10 here and no argument is modified.
//
// sgdfr_shaperender_texture_f32 is the third instance, raster_kernel<kTexture>: SRenderY.forward (renderer.py:121-191), the albedo map
// sampled at the pixel's UV coordinate, add_SHlight on the interpolated world normal, the coverage and the z < -0.05 mask of the
// projected normals.  sgdfr_shaperender_attr_f32 is the fourth, raster_kernel<kAttr>: D <= 3 per-vertex values interpolated, 0 where no
// face covers (render_normal, render_depth; no normals are computed: three launches).
//
// Floating-point contraction is OFF for the whole file: coverage is a sign test on differences of products, and the tests compare
// it with a restatement that does not fuse.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace sgdfr {
namespace {

constexpr int kTile = 16;                    // raster tile side; kTile * kTile = the block
constexpr int kChunk = kTile * kTile;        // faces per chunk: one bounding-box test per thread
constexpr int kMaxLights = 8;
constexpr int kMaxSize = 4096;               // the bounding box is stored in 16 bits per bound
constexpr float kAreaEps = 1e-8f;            // pytorch3d's kEpsilon: |area| <= eps is skipped, the barycentrics divide by area + eps
constexpr float kAlbedo = 180.0f / 255.0f;   // renderer.py:110
constexpr float kFrontZ = 0.15f;             // renderer.py:276

struct FaceRec {                             // 48 bytes: three 16-byte LDS reads
    float ax, ay, bx, by;
    float cx, cy, za, zb;
    float zc, denom;
    int face, pad;
};
static_assert(sizeof(FaceRec) == 48, "FaceRec is read as three float4");

struct Workspace {
    float* proj;                             // [B,V,3]
    float* wn;                               // [B,V,3]  world normals
    float* tz;                               // [B,V]    z of the projected normals
    FaceRec* rec;                            // [B,F]
    ushort4* box;                            // [B,F]    x0, y0, x1, y1 (inclusive); x0 > x1: no pixel
};

inline int64_t align256(int64_t v) { return (v + 255) & ~255ll; }

bool sizes_ok(int B, int V, int F) { return B >= 1 && B <= 4096 && V >= 1 && V <= (1 << 24) && F >= 1 && F <= (1 << 24); }

int64_t layout(int B, int V, int F, char* base, Workspace* ws) {
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t at = o; o += align256(bytes); return at; };
    const int64_t o_proj = take((int64_t)B * V * 3 * 4);
    const int64_t o_wn = take((int64_t)B * V * 3 * 4);
    const int64_t o_tz = take((int64_t)B * V * 4);
    const int64_t o_rec = take((int64_t)B * F * (int64_t)sizeof(FaceRec));
    const int64_t o_box = take((int64_t)B * F * (int64_t)sizeof(ushort4));
    if (ws) {
        ws->proj = (float*)(base + o_proj);
        ws->wn = (float*)(base + o_wn);
        ws->tz = (float*)(base + o_tz);
        ws->rec = (FaceRec*)(base + o_rec);
        ws->box = (ushort4*)(base + o_box);
    }
    return o;
}

// ---------------------------------------------------------------------------------------------------------------- projection
// cam: X = s (x + tx), Y = -s (y + ty), Z = -s z + z_offset (util.batch_orth_proj, deca.py:175, renderer.py:255);  no cam: the vertices
// are projected already and only Z moves
__global__ __launch_bounds__(256) void project_kernel(const float* __restrict__ verts, const float* __restrict__ cam, float z_offset, int V,
                                                      float* __restrict__ proj) {
    const int b = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const size_t at = ((size_t)b * V + v) * 3;
    const float x = verts[at], y = verts[at + 1], z = verts[at + 2];
    if (cam) {
        const float s = cam[b * 3], tx = cam[b * 3 + 1], ty = cam[b * 3 + 2];
        proj[at] = s * (x + tx);
        proj[at + 1] = -(s * (y + ty));
        proj[at + 2] = -(s * z) + z_offset;
    } else {
        proj[at] = x;
        proj[at + 1] = y;
        proj[at + 2] = z + z_offset;
    }
}

// ---------------------------------------------------------------------------------------------------------------- vertex normals
// util.vertex_normals with the index_add_ turned into a gather: entry e of vertex v is face * 3 + corner, ascending.  Corner k
// contributes (v[k+1] - v[k]) x (v[k+2] - v[k]), the reference's per-corner form.  An entry that points outside the tables adds nothing.
__global__ __launch_bounds__(256) void normals_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                      const int* __restrict__ offsets, const int* __restrict__ entries, int z_only,
                                                      float* __restrict__ out) {
    const int b = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const float* p = verts + (size_t)b * V * 3;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    const int e0 = offsets[v], e1 = offsets[v + 1];
    for (int e = e0; e < e1; ++e) {
        const unsigned entry = (unsigned)entries[e];
        const unsigned f = entry / 3u, k = entry - f * 3u;
        if (f >= (unsigned)F) continue;
        const unsigned i0 = (unsigned)faces[f * 3 + k], i1 = (unsigned)faces[f * 3 + (k + 1) % 3], i2 = (unsigned)faces[f * 3 + (k + 2) % 3];
        if (i0 >= (unsigned)V || i1 >= (unsigned)V || i2 >= (unsigned)V) continue;
        const float ox = p[i0 * 3], oy = p[i0 * 3 + 1], oz = p[i0 * 3 + 2];
        const float ux = p[i1 * 3] - ox, uy = p[i1 * 3 + 1] - oy, uz = p[i1 * 3 + 2] - oz;
        const float wx = p[i2 * 3] - ox, wy = p[i2 * 3 + 1] - oy, wz = p[i2 * 3 + 2] - oz;
        nx += uy * wz - uz * wy;
        ny += uz * wx - ux * wz;
        nz += ux * wy - uy * wx;
    }
    const float len = fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), 1e-6f);       // F.normalize(eps=1e-6)
    if (z_only) {
        out[(size_t)b * V + v] = __fdiv_rn(nz, len);
    } else {
        float* o = out + ((size_t)b * V + v) * 3;
        o[0] = __fdiv_rn(nx, len), o[1] = __fdiv_rn(ny, len), o[2] = __fdiv_rn(nz, len);
    }
}

// ---------------------------------------------------------------------------------------------------------------- face setup
// continuous pixel index of an NDC coordinate: pixel j has its centre at (2 j + 1) / S - 1
__device__ __forceinline__ float pixel_of(float x, int S) { return (x + 1.0f) * (0.5f * (float)S) - 0.5f; }

__global__ __launch_bounds__(256) void setup_kernel(const float* __restrict__ proj, int V, const int* __restrict__ faces, int F, int S,
                                                    FaceRec* __restrict__ rec, ushort4* __restrict__ box) {
    const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const size_t at = (size_t)b * F + f;
    const ushort4 none = make_ushort4(1, 1, 0, 0);
    const unsigned i0 = (unsigned)faces[f * 3], i1 = (unsigned)faces[f * 3 + 1], i2 = (unsigned)faces[f * 3 + 2];
    if (i0 >= (unsigned)V || i1 >= (unsigned)V || i2 >= (unsigned)V) {
        box[at] = none;
        return;
    }
    const float* p = proj + (size_t)b * V * 3;
    FaceRec r;
    r.ax = p[i0 * 3], r.ay = p[i0 * 3 + 1], r.za = p[i0 * 3 + 2];
    r.bx = p[i1 * 3], r.by = p[i1 * 3 + 1], r.zb = p[i1 * 3 + 2];
    r.cx = p[i2 * 3], r.cy = p[i2 * 3 + 1], r.zc = p[i2 * 3 + 2];
    const float area = (r.cx - r.ax) * (r.by - r.ay) - (r.cy - r.ay) * (r.bx - r.ax);        // edge(c; a, b)
    r.denom = area + kAreaEps;
    r.face = f, r.pad = 0;
    const float x0 = fminf(fminf(r.ax, r.bx), r.cx), x1 = fmaxf(fmaxf(r.ax, r.bx), r.cx);
    const float y0 = fminf(fminf(r.ay, r.by), r.cy), y1 = fmaxf(fmaxf(r.ay, r.by), r.cy);
    // a NaN or infinite corner fails the first comparison; the bounds below are then never turned into integers
    const bool finite = fabsf(x0) < 1e30f && fabsf(x1) < 1e30f && fabsf(y0) < 1e30f && fabsf(y1) < 1e30f;
    const bool keep = finite && fabsf(area) > kAreaEps && !(r.za < 0.f && r.zb < 0.f && r.zc < 0.f);
    ushort4 bb = none;
    if (keep) {
        const float hi = (float)S;
        // a covered centre lies strictly inside the triangle, so inside [x0, x1] x [y0, y1]: floor / ceil of the continuous index
        // keep every such pixel (the rounding of pixel_of is far below one pixel at S <= 4096)
        const int px0 = (int)floorf(fminf(fmaxf(pixel_of(x0, S), -1.0f), hi)), px1 = (int)ceilf(fminf(fmaxf(pixel_of(x1, S), -1.0f), hi));
        const int py0 = (int)floorf(fminf(fmaxf(pixel_of(y0, S), -1.0f), hi)), py1 = (int)ceilf(fminf(fmaxf(pixel_of(y1, S), -1.0f), hi));
        const int cx0 = max(px0, 0), cx1 = min(px1, S - 1), cy0 = max(py0, 0), cy1 = min(py1, S - 1);
        if (cx0 <= cx1 && cy0 <= cy1) bb = make_ushort4((unsigned short)cx0, (unsigned short)cy0, (unsigned short)cx1, (unsigned short)cy1);
    }
    rec[at] = r;
    box[at] = bb;
}

// ---------------------------------------------------------------------------------------------------------------- raster + shade
struct RasterOut {
    float* shape;            // [B,3,S,S] or NULL
    float* alpha;            // [B,1,S,S] or NULL
    int* pix_to_face;        // [B,S,S] or NULL
    float* zbuf;             // [B,S,S] or NULL
    float* bary;             // [B,S,S,3] or NULL
};

// the detail panel's inputs and outputs (sgdfr_shaperender_detail_f32); unused by raster_kernel<false>
struct DetailIO {
    const float* face_uv;    // [F,3,2]
    const float* uv_normals; // [B,3,Su,Su]
    int Su;
    float* shape_detail;     // [B,3,S,S] or NULL
    float* grid;             // [B,S,S,2] or NULL
    float* normal_images;    // [B,3,S,S] or NULL
};

// the textured render's inputs and outputs (sgdfr_shaperender_texture_f32); every output may be NULL
struct TexIO {
    const float* face_uv;    // [F,3,2]
    const float* albedo;     // [B,3,Su,Su]
    int Su;
    float sh[9];             // renderer.py:114-119, rounded to float once on the host
    float* images;           // [B,3,S,S]
    float* albedo_images;    // [B,3,S,S]
    float* alpha;            // [B,1,S,S]
    float* pos_mask;         // [B,1,S,S]
    float* shading;          // [B,3,S,S]
    float* grid;             // [B,S,S,2]
    float* normal_images;    // [B,3,S,S]
};

// the attribute mode (sgdfr_shaperender_attr_f32)
struct AttrIO {
    const float* values;     // [B,V,D]
    int D;                   // 1..3
    float* out;              // [B,D,S,S]
};

constexpr int kShape = 0, kDetail = 1, kTexture = 2, kAttr = 3;      // raster_kernel's modes
constexpr float kPosZ = -0.05f;              // renderer.py:159

// F.grid_sample(bilinear, zeros, align_corners=False) of one [3,Su,Su] map at g: a neighbour outside the map adds nothing
__device__ __forceinline__ void sample_uv(const float* __restrict__ map, int Su, float gx, float gy, float (&r)[3]) {
    const float ix = ((gx + 1.0f) * (float)Su - 1.0f) * 0.5f, iy = ((gy + 1.0f) * (float)Su - 1.0f) * 0.5f;
    const float fx = floorf(ix), fy = floorf(iy);
    const float ax = ix - fx, ay = iy - fy, bx = (fx + 1.0f) - ix, by = (fy + 1.0f) - iy;
    r[0] = r[1] = r[2] = 0.f;
    // a coordinate that is not finite or far outside fails every test below (the casts are then never made)
    if (!(fx >= -1.0f && fx < (float)Su && fy >= -1.0f && fy < (float)Su)) return;
    const int x0 = (int)fx, y0 = (int)fy;
    const size_t plane = (size_t)Su * Su;
    const float w[4] = {bx * by, ax * by, bx * ay, ax * ay};      // nw, ne, sw, se
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + (k & 1), y = y0 + (k >> 1);
        if (x < 0 || x >= Su || y < 0 || y >= Su) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] += map[c * plane + (size_t)y * Su + x] * w[k];
    }
}

// SRenderY.add_SHlight at one normal: sum_k coeff[k][c] (basis_k(n) constant_k), k ascending; coeff [9][3]
__device__ __forceinline__ void sh_light(const float (&c)[9], const float* coeff, float nx, float ny, float nz, float (&r)[3]) {
    const float basis[9] = {1.0f, nx, ny, nz, nx * ny, nx * nz, ny * nz, nx * nx - ny * ny, 3.0f * (nz * nz) - 1.0f};
    r[0] = r[1] = r[2] = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float sh = basis[k] * c[k];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) r[ch] += coeff[k * 3 + ch] * sh;
    }
}

template <int MODE, typename IO>
__global__ __launch_bounds__(kChunk) void raster_kernel(const FaceRec* __restrict__ rec, const ushort4* __restrict__ box, int F, int S, int V,
                                                        const int* __restrict__ faces, const float* __restrict__ wn,
                                                        const float* __restrict__ tz, const float* __restrict__ lights, int light_rows, int L,
                                                        const float* __restrict__ background, int gan_range, RasterOut out, IO det) {
    constexpr bool DETAIL = MODE == kDetail;
    __shared__ float4 s_rec[kChunk][3];
    __shared__ float s_light[kMaxLights][6];
    __shared__ int s_wave[kChunk / kWave];
    const int t = threadIdx.x, b = blockIdx.z;
    const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
    const int j = tx0 + (t & (kTile - 1)), i = ty0 + t / kTile;
    const bool live = j < S && i < S;
    const float px = __fdiv_rn((float)(2 * j + 1), (float)S) - 1.0f, py = __fdiv_rn((float)(2 * i + 1), (float)S) - 1.0f;
    if constexpr (MODE == kTexture) {
        if (lights && t < 27) (&s_light[0][0])[t] = lights[(size_t)b * 27 + t];       // this image's SH coefficients [9][3]
    } else if ((DETAIL || (MODE == kShape && out.shape)) && t < L) {
        // F.normalize(direction, eps=1e-12) and the intensities of this image's light t
        const float* l = lights + ((size_t)(light_rows == 1 ? 0 : b) * L + t) * 6;
        const float n = fmaxf(sqrtf(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]), 1e-12f);
        s_light[t][0] = __fdiv_rn(l[0], n), s_light[t][1] = __fdiv_rn(l[1], n), s_light[t][2] = __fdiv_rn(l[2], n);
        s_light[t][3] = l[3], s_light[t][4] = l[4], s_light[t][5] = l[5];
    }
    const FaceRec* rec_b = rec + (size_t)b * F;
    const ushort4* box_b = box + (size_t)b * F;
    const int lane = t & (kWave - 1), wave = t / kWave;
    const int tx1 = tx0 + kTile - 1, ty1 = ty0 + kTile - 1;
    float best_z = INFINITY, w0 = 0.f, w1 = 0.f, w2 = 0.f;
    int best = -1;
    for (int f0 = 0; f0 < F; f0 += kChunk) {
        const int f = f0 + t;
        bool hit = false;
        if (f < F) {
            const ushort4 bb = box_b[f];
            hit = bb.x <= bb.z && (int)bb.x <= tx1 && (int)bb.z >= tx0 && (int)bb.y <= ty1 && (int)bb.w >= ty0;
        }
        const unsigned long long vote = __ballot(hit);
        if (lane == 0) s_wave[wave] = __popcll(vote);
        __syncthreads();                       // also: every thread has left the previous chunk's pixel loop
        int slot = __popcll(vote & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < kChunk / kWave; ++w) {
            const int n = s_wave[w];
            slot += w < wave ? n : 0;
            total += n;
        }
        if (hit) {
            const float4* src = (const float4*)(rec_b + f);
            s_rec[slot][0] = src[0], s_rec[slot][1] = src[1], s_rec[slot][2] = src[2];
        }
        __syncthreads();
        if (live) {
            for (int k = 0; k < total; ++k) {
                const float4 r0 = s_rec[k][0], r1 = s_rec[k][1], r2 = s_rec[k][2];
                const float ax = r0.x, ay = r0.y, bx = r0.z, by = r0.w, cx = r1.x, cy = r1.y, denom = r2.y;
                // edge(p; u, v) = (p.x - u.x)(v.y - u.y) - (p.y - u.y)(v.x - u.x), the differences first
                const float e0 = (px - bx) * (cy - by) - (py - by) * (cx - bx);
                const float e1 = (px - cx) * (ay - cy) - (py - cy) * (ax - cx);
                const float e2 = (px - ax) * (by - ay) - (py - ay) * (bx - ax);
                // a positive quotient needs the sign of the divisor: three divisions only for the faces that pass
                const bool pos = denom > 0.f;
                if ((pos ? (e0 > 0.f && e1 > 0.f && e2 > 0.f) : (e0 < 0.f && e1 < 0.f && e2 < 0.f))) {
                    const float q0 = __fdiv_rn(e0, denom), q1 = __fdiv_rn(e1, denom), q2 = __fdiv_rn(e2, denom);
                    const float z = q0 * r1.z + q1 * r1.w + q2 * r2.x;
                    // strictly nearer only: the list is in face order, so on equal z the lower face index stays
                    if (q0 > 0.f && q1 > 0.f && q2 > 0.f && z >= 0.f && z < best_z) {
                        best_z = z, best = __float_as_int(r2.z), w0 = q0, w1 = q1, w2 = q2;
                    }
                }
            }
        }
        // the barrier at the top of the next chunk keeps s_rec until every thread is through this loop
    }
    if (!live) return;
    const size_t pix = ((size_t)b * S + i) * S + j;
    const bool covered = best >= 0;
    if (out.pix_to_face) out.pix_to_face[pix] = best;
    if (out.zbuf) out.zbuf[pix] = covered ? best_z : -1.0f;
    if (out.bary) {
        out.bary[pix * 3] = covered ? w0 : -1.0f;
        out.bary[pix * 3 + 1] = covered ? w1 : -1.0f;
        out.bary[pix * 3 + 2] = covered ? w2 : -1.0f;
    }
    if constexpr (MODE == kAttr) {
        float r[3] = {0.f, 0.f, 0.f};
        if (covered) {
            const int i0 = faces[best * 3], i1 = faces[best * 3 + 1], i2 = faces[best * 3 + 2];
            const float* a = det.values + (size_t)b * V * det.D;
            for (int c = 0; c < det.D; ++c) r[c] = w0 * a[i0 * det.D + c] + w1 * a[i1 * det.D + c] + w2 * a[i2 * det.D + c];
        }
        for (int c = 0; c < det.D; ++c) det.out[((size_t)b * det.D + c) * S * S + (size_t)i * S + j] = r[c];
    } else if constexpr (MODE == kTexture) {
        // SRenderY.forward: an uncovered pixel has every attribute 0, so its shading is add_SHlight(0) and everything else 0
        float n[3] = {0.f, 0.f, 0.f}, al[3] = {0.f, 0.f, 0.f}, sh[3] = {0.f, 0.f, 0.f}, tzp = 0.f, gx = 0.f, gy = 0.f;
        const float a = covered ? 1.0f : 0.0f;
        if (covered) {
            const int i0 = faces[best * 3], i1 = faces[best * 3 + 1], i2 = faces[best * 3 + 2];
            const float* nw = wn + (size_t)b * V * 3;
            const float* z = tz + (size_t)b * V;
#pragma unroll
            for (int c = 0; c < 3; ++c) n[c] = w0 * nw[i0 * 3 + c] + w1 * nw[i1 * 3 + c] + w2 * nw[i2 * 3 + c];
            tzp = w0 * z[i0] + w1 * z[i1] + w2 * z[i2];
            const float* uv = det.face_uv + (size_t)best * 6;
            gx = w0 * uv[0] + w1 * uv[2] + w2 * uv[4];
            gy = w0 * uv[1] + w1 * uv[3] + w2 * uv[5];
            if (det.images || det.albedo_images) sample_uv(det.albedo + (size_t)b * 3 * det.Su * det.Su, det.Su, gx, gy, al);
        }
        if (lights) sh_light(det.sh, &s_light[0][0], n[0], n[1], n[2], sh);
        if (det.grid) det.grid[pix * 2] = gx, det.grid[pix * 2 + 1] = gy;
        if (det.alpha) det.alpha[pix] = a;
        if (det.pos_mask) det.pos_mask[pix] = tzp < kPosZ ? 1.0f : 0.0f;
        const size_t plane = (size_t)S * S;
        const size_t o = (size_t)b * 3 * plane + (size_t)i * S + j;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (det.images) det.images[o + c * plane] = (lights ? al[c] * sh[c] : al[c]) * a;
            if (det.albedo_images) det.albedo_images[o + c * plane] = al[c] * a;
            if (det.shading) det.shading[o + c * plane] = sh[c];
            if (det.normal_images) det.normal_images[o + c * plane] = n[c] * a;
        }
    } else {
        if (!DETAIL && !out.shape) return;
        float shade[3] = {0.f, 0.f, 0.f}, albedo = 0.f, a = 0.f;
        float dshade[3] = {0.f, 0.f, 0.f}, dn[3] = {0.f, 0.f, 0.f}, gx = 0.f, gy = 0.f;
        if (covered) {
            const int i0 = faces[best * 3], i1 = faces[best * 3 + 1], i2 = faces[best * 3 + 2];      // in range: setup skipped the others
            const float* n = wn + (size_t)b * V * 3;
            const float* z = tz + (size_t)b * V;
            const float nx = w0 * n[i0 * 3] + w1 * n[i1 * 3] + w2 * n[i2 * 3];
            const float ny = w0 * n[i0 * 3 + 1] + w1 * n[i1 * 3 + 1] + w2 * n[i2 * 3 + 1];
            const float nz = w0 * n[i0 * 3 + 2] + w1 * n[i1 * 3 + 2] + w2 * n[i2 * 3 + 2];
            const float tzp = w0 * z[i0] + w1 * z[i1] + w2 * z[i2];
            albedo = (w0 + w1 + w2) * kAlbedo;
            for (int l = 0; l < L; ++l) {
                const float d = fminf(fmaxf(nx * s_light[l][0] + ny * s_light[l][1] + nz * s_light[l][2], 0.0f), 1.0f);
                shade[0] += d * s_light[l][3], shade[1] += d * s_light[l][4], shade[2] += d * s_light[l][5];
            }
            a = tzp < kFrontZ ? 1.0f : 0.0f;
            if constexpr (DETAIL) {
                // ops['grid'] and the UV normal map sampled there: the detail panel's shading normal (covered = 1 here)
                const float* uv = det.face_uv + (size_t)best * 6;
                gx = w0 * uv[0] + w1 * uv[2] + w2 * uv[4];
                gy = w0 * uv[1] + w1 * uv[3] + w2 * uv[5];
                sample_uv(det.uv_normals + (size_t)b * 3 * det.Su * det.Su, det.Su, gx, gy, dn);
                for (int l = 0; l < L; ++l) {
                    const float d = fminf(fmaxf(dn[0] * s_light[l][0] + dn[1] * s_light[l][1] + dn[2] * s_light[l][2], 0.0f), 1.0f);
                    dshade[0] += d * s_light[l][3], dshade[1] += d * s_light[l][4], dshade[2] += d * s_light[l][5];
                }
            }
        }
        if constexpr (DETAIL) {
            if (det.grid) det.grid[pix * 2] = gx, det.grid[pix * 2 + 1] = gy;
        }
        if (out.alpha) out.alpha[pix] = a;
        const size_t plane = (size_t)S * S;
        const size_t o = (size_t)b * 3 * plane + (size_t)i * S + j;
    #pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float bg = background ? background[o + c * plane] : 0.0f;
            if (!DETAIL || out.shape) {
                const float shading = __fdiv_rn(shade[c], (float)L);
                float v = albedo * shading * a + bg * (1.0f - a);
                if (gan_range) v = fminf(fmaxf(v, 0.0f), 1.0f) * 2.0f - 1.0f;
                out.shape[o + c * plane] = v;
            }
            if constexpr (DETAIL) {
                if (det.normal_images) det.normal_images[o + c * plane] = dn[c];
                if (det.shape_detail) {
                    const float shading = __fdiv_rn(dshade[c], (float)L);
                    float v = albedo * shading * a + bg * (1.0f - a);
                    if (gan_range) v = fminf(fmaxf(v, 0.0f), 1.0f) * 2.0f - 1.0f;
                    det.shape_detail[o + c * plane] = v;
                }
            }
        }
    }
}

int launch_normals(const float* verts, int rows, int V, const int* faces, int F, const int* offsets, const int* entries, int z_only,
                   float* out, hipStream_t st) {
    normals_kernel<<<dim3((V + 255) / 256, rows), 256, 0, st>>>(verts, V, faces, F, offsets, entries, z_only, out);
    return check_launch("shaperender normals_kernel");
}

}  // namespace
}  // namespace sgdfr

using namespace sgdfr;

extern "C" int64_t sgdfr_shaperender_workspace_bytes(int rows, int V, int F) {
    if (!sizes_ok(rows, V, F)) return -1;
    return layout(rows, V, F, nullptr, nullptr);
}

extern "C" int sgdfr_shaperender_normals_f32(const float* vertices, int rows, int V, const int* faces, int F, const int* csr_offsets,
                                             const int* csr_entries, float* normals, void* stream) {
    SGDFR_REQUIRE(vertices && faces && csr_offsets && csr_entries && normals, "shaperender_normals: null pointer");
    SGDFR_REQUIRE(sizes_ok(rows, V, F), "shaperender_normals: rows=%d V=%d F=%d (rows 1..4096, V and F 1..2^24)", rows, V, F);
    return launch_normals(vertices, rows, V, faces, F, csr_offsets, csr_entries, 0, normals, as_stream(stream));
}

static int forward(const float* vertices, const float* projected, const float* cam, float z_offset, int rows, int V, const int* faces, int F,
                   const int* csr_offsets, const int* csr_entries, int S, const float* lights, int light_rows, int L, const float* background,
                   int gan_range, float* shape, float* alpha, int* pix_to_face, float* zbuf, float* bary, const DetailIO* det, void* workspace,
                   int64_t workspace_bytes, void* stream, const TexIO* tex = nullptr, float* normals = nullptr, float* tnormals = nullptr,
                   const AttrIO* attr = nullptr) {
    SGDFR_REQUIRE(faces, "shaperender_forward: null faces");
    SGDFR_REQUIRE(sizes_ok(rows, V, F), "shaperender_forward: rows=%d V=%d F=%d (rows 1..4096, V and F 1..2^24)", rows, V, F);
    SGDFR_REQUIRE(S >= 1 && S <= kMaxSize, "shaperender_forward: size=%d (1..%d)", S, kMaxSize);
    SGDFR_REQUIRE((projected != nullptr) != (cam != nullptr), "shaperender_forward: exactly one of projected / cam");
    SGDFR_REQUIRE(!cam || vertices, "shaperender_forward: cam needs the world vertices");
    const bool shade = shape != nullptr || det != nullptr || tex != nullptr;
    if (tex) {
        SGDFR_REQUIRE(vertices && csr_offsets && csr_entries, "shaperender_texture: vertices and the vertex table are needed");
    } else if (attr) {
        SGDFR_REQUIRE(attr->values && attr->out && attr->D >= 1 && attr->D <= 3, "shaperender_attr: values [rows,V,D] with D 1..3 and out");
    } else if (shade) {
        SGDFR_REQUIRE(vertices && csr_offsets && csr_entries && lights, "shaperender_forward: shading needs vertices, the vertex table and lights");
        SGDFR_REQUIRE(L >= 1 && L <= kMaxLights, "shaperender_forward: %d lights (1..%d)", L, kMaxLights);
        SGDFR_REQUIRE(light_rows == 1 || light_rows == rows, "shaperender_forward: lights for %d rows (1 or %d)", light_rows, rows);
    } else {
        SGDFR_REQUIRE(!alpha && !background, "shaperender_forward: alpha and background belong to the shaded output");
        SGDFR_REQUIRE(pix_to_face || zbuf || bary, "shaperender_forward: no output");
    }
    Workspace ws;
    const int64_t need = layout(rows, V, F, (char*)workspace, &ws);
    SGDFR_REQUIRE(workspace && workspace_bytes >= need, "shaperender_forward: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)need);
    hipStream_t st = as_stream(stream);
    project_kernel<<<dim3((V + 255) / 256, rows), 256, 0, st>>>(cam ? vertices : projected, cam, z_offset, V, ws.proj);
    if (check_launch("shaperender project_kernel")) return 1;
    float* wn = normals ? normals : ws.wn;             // the textured render writes the world normals where the caller wants them
    if (shade) {
        if (launch_normals(vertices, rows, V, faces, F, csr_offsets, csr_entries, 0, wn, st)) return 1;
        if (launch_normals(ws.proj, rows, V, faces, F, csr_offsets, csr_entries, 1, ws.tz, st)) return 1;
        if (tnormals && launch_normals(ws.proj, rows, V, faces, F, csr_offsets, csr_entries, 0, tnormals, st)) return 1;
    }
    setup_kernel<<<dim3((F + 255) / 256, rows), 256, 0, st>>>(ws.proj, V, faces, F, S, ws.rec, ws.box);
    if (check_launch("shaperender setup_kernel")) return 1;
    RasterOut out{shape, alpha, pix_to_face, zbuf, bary};
    const int tiles = (S + kTile - 1) / kTile;
    const dim3 grid(tiles, tiles, rows);
    if (tex)
        raster_kernel<kTexture, TexIO><<<grid, kChunk, 0, st>>>(ws.rec, ws.box, F, S, V, faces, wn, ws.tz, lights, rows, 0, nullptr, 0, out, *tex);
    else if (attr)
        raster_kernel<kAttr, AttrIO><<<grid, kChunk, 0, st>>>(ws.rec, ws.box, F, S, V, faces, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, out,
                                                             *attr);
    else if (det)
        raster_kernel<kDetail, DetailIO><<<grid, kChunk, 0, st>>>(ws.rec, ws.box, F, S, V, faces, ws.wn, ws.tz, lights, light_rows, L, background,
                                                                 gan_range, out, *det);
    else
        raster_kernel<kShape, DetailIO><<<grid, kChunk, 0, st>>>(ws.rec, ws.box, F, S, V, faces, ws.wn, ws.tz, lights, light_rows, L, background,
                                                                gan_range, out, DetailIO{});
    return check_launch("shaperender raster_kernel");
}

extern "C" int sgdfr_shaperender_forward_f32(const float* vertices, const float* projected, const float* cam, float z_offset, int rows, int V,
                                             const int* faces, int F, const int* csr_offsets, const int* csr_entries, int S,
                                             const float* lights, int light_rows, int L, const float* background, int gan_range,
                                             float* shape, float* alpha, int* pix_to_face, float* zbuf, float* bary, void* workspace,
                                             int64_t workspace_bytes, void* stream) {
    return forward(vertices, projected, cam, z_offset, rows, V, faces, F, csr_offsets, csr_entries, S, lights, light_rows, L, background,
                   gan_range, shape, alpha, pix_to_face, zbuf, bary, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int sgdfr_shaperender_detail_f32(const float* vertices, const float* projected, const float* cam, float z_offset, int rows, int V,
                                            const int* faces, int F, const int* csr_offsets, const int* csr_entries, int S,
                                            const float* lights, int light_rows, int L, const float* background, int gan_range,
                                            const float* face_uv, const float* uv_normals, int Su, float* shape, float* shape_detail,
                                            float* grid, float* detail_normal_images, float* alpha, int* pix_to_face, float* zbuf, float* bary,
                                            void* workspace, int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(face_uv && uv_normals, "shaperender_detail: null face_uv or uv_normals");
    SGDFR_REQUIRE(Su >= 1 && Su <= kMaxSize, "shaperender_detail: uv_size=%d (1..%d)", Su, kMaxSize);
    const DetailIO det{face_uv, uv_normals, Su, shape_detail, grid, detail_normal_images};
    return forward(vertices, projected, cam, z_offset, rows, V, faces, F, csr_offsets, csr_entries, S, lights, light_rows, L, background,
                   gan_range, shape, alpha, pix_to_face, zbuf, bary, &det, workspace, workspace_bytes, stream);
}

extern "C" int sgdfr_shaperender_texture_f32(const float* vertices, const float* projected, const float* cam, float z_offset, int rows, int V,
                                             const int* faces, int F, const int* csr_offsets, const int* csr_entries, int S,
                                             const float* sh_lights, const float* sh_constants, const float* face_uv, const float* albedo,
                                             int Su, float* images, float* albedo_images, float* alpha_images, float* pos_mask,
                                             float* shading_images, float* grid, float* normal_images, float* normals,
                                             float* transformed_normals, int* pix_to_face, float* zbuf, float* bary, void* workspace,
                                             int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(face_uv && sh_constants, "shaperender_texture: null face_uv or sh_constants");
    SGDFR_REQUIRE(albedo || (!images && !albedo_images), "shaperender_texture: images and albedo_images need an albedo");
    SGDFR_REQUIRE(Su >= 1 && Su <= kMaxSize, "shaperender_texture: uv_size=%d (1..%d)", Su, kMaxSize);
    SGDFR_REQUIRE(images || albedo_images || alpha_images || pos_mask || shading_images || grid || normal_images || normals ||
                      transformed_normals || pix_to_face || zbuf || bary,
                  "shaperender_texture: no output");
    TexIO tex{face_uv, albedo, Su, {}, images, albedo_images, alpha_images, pos_mask, shading_images, grid, normal_images};
    for (int k = 0; k < 9; ++k) tex.sh[k] = sh_constants[k];
    return forward(vertices, projected, cam, z_offset, rows, V, faces, F, csr_offsets, csr_entries, S, sh_lights, rows, 0, nullptr, 0, nullptr,
                   nullptr, pix_to_face, zbuf, bary, nullptr, workspace, workspace_bytes, stream, &tex, normals, transformed_normals);
}

extern "C" int sgdfr_shaperender_attr_f32(const float* projected, float z_offset, int rows, int V, const int* faces, int F, int S,
                                          const float* values, int D, float* out, int* pix_to_face, float* zbuf, float* bary, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(projected, "shaperender_attr: null projected");
    const AttrIO attr{values, D, out};
    return forward(nullptr, projected, nullptr, z_offset, rows, V, faces, F, nullptr, nullptr, S, nullptr, 0, 0, nullptr, 0, nullptr, nullptr,
                   pix_to_face, zbuf, bary, nullptr, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr, &attr);
}
