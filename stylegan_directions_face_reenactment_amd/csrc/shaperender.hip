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
//                                       then every thread tests its own pixel against the compacted list; a shader interpolates,
//                                       lights and blends the winner, so no attribute image exists
// No global bins, no atomics, a fixed face order: the result does not depend on scheduling.  All 256 threads read the same LDS record
// at the same time (three ds_read_b128 of one address: a broadcast, no bank conflict).
//
// The raster kernel is one walk and four shaders: raster_kernel<Shader> = the shader's prologue (lights into LDS), cover() (the walk
// above, which knows nothing of shading and returns the pixel's Hit), write_raster (pix_to_face, zbuf, bary) and the shader on the
// Hit.  A shader (ShapeShader, DetailShader, TextureShader, AttrShader below) is a struct of its own inputs and outputs, passed by
// value as a kernel argument; what more than one needs (corners, mix3, normal_at, face_uv_at, directional; grid_sample3 and sh_light
// of mesh_sample.h) is written once.  The host side is as it was: forward() with the entries' common checks and launches; z_offset
// stays 10 however often the reference adds it in place (orthographic: a shift of |z| < 10 changes nothing).
//
// Floating-point contraction is OFF for the whole file: coverage is a sign test on differences of products, and the tests compare
// it with a restatement that does not fuse.
#include <math.h>

#include "common.h"
#include "mesh_sample.h"

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
constexpr float kPosZ = -0.05f;              // renderer.py:159

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

// ---------------------------------------------------------------------------------------------------------------- raster: the cover
struct RasterOut {
    int* pix_to_face;        // [B,S,S] or NULL
    float* zbuf;             // [B,S,S] or NULL
    float* bary;             // [B,S,S,3] or NULL
};
struct Hit { int face; float z, w0, w1, w2; };       // the nearest face over one pixel centre and its barycentrics; face < 0: none
// what forward() tells every shader of the mesh and the image; wn, tz [B,V,3], [B,V]: only where the entry computes the normals
struct Mesh { const int* faces; int V, S; const float *wn, *tz; };

// One tile's walk over the faces of its image in chunks of kChunk; p = the centre of this thread's pixel, live = it lies in the image.
__device__ __forceinline__ Hit cover(const FaceRec* __restrict__ rec_b, const ushort4* __restrict__ box_b, int F, int t, int tx0, int ty0,
                                     bool live, float px, float py, float4 (&s_rec)[kChunk][3], int (&s_wave)[kChunk / kWave]) {
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
    return Hit{best, best_z, w0, w1, w2};
}

__device__ __forceinline__ void write_raster(const RasterOut& out, size_t pix, const Hit& h) {
    const bool covered = h.face >= 0;
    if (out.pix_to_face) out.pix_to_face[pix] = h.face;
    if (out.zbuf) out.zbuf[pix] = covered ? h.z : -1.0f;
    if (out.bary) {
        out.bary[pix * 3] = covered ? h.w0 : -1.0f;
        out.bary[pix * 3 + 1] = covered ? h.w1 : -1.0f;
        out.bary[pix * 3 + 2] = covered ? h.w2 : -1.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- what the shaders share
// the three vertices k of a face that won a pixel (in range: setup skipped the others), and component c of a per-vertex table of
// `stride` floats a vertex interpolated over them: w0 a + w1 b + w2 c in this association
__device__ __forceinline__ const int* corners(const int* __restrict__ faces, int face) { return faces + face * 3; }
__device__ __forceinline__ float mix3(const Hit& h, const float* __restrict__ a, const int* __restrict__ k, int stride, int c) {
    return h.w0 * a[k[0] * stride + c] + h.w1 * a[k[1] * stride + c] + h.w2 * a[k[2] * stride + c];
}

// the interpolated world normal under a hit (not renormalised); returns the interpolated z of the projected normals
__device__ __forceinline__ float normal_at(const Mesh& m, int b, const Hit& h, float (&n)[3]) {
    const int* k = corners(m.faces, h.face);
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] = mix3(h, m.wn + (size_t)b * m.V * 3, k, 3, c);
    return mix3(h, m.tz + (size_t)b * m.V, k, 1, 0);
}

// the pixel's UV coordinate (ops['grid']); face_uv [F,3,2]
__device__ __forceinline__ void face_uv_at(const float* __restrict__ face_uv, const Hit& h, float& gx, float& gy) {
    const float* uv = face_uv + (size_t)h.face * 6;
    gx = h.w0 * uv[0] + h.w1 * uv[2] + h.w2 * uv[4], gy = h.w0 * uv[1] + h.w1 * uv[3] + h.w2 * uv[5];
}

// sum over the staged lights [L][6] = unit direction, intensity: clamp(n . direction, 0, 1) intensity (renderer.py:226-235)
__device__ __forceinline__ void directional(const float* s_light, int L, const float (&n)[3], float (&shade)[3]) {
    shade[0] = shade[1] = shade[2] = 0.f;
    for (int l = 0; l < L; ++l, s_light += 6) {
        const float d = fminf(fmaxf(n[0] * s_light[0] + n[1] * s_light[1] + n[2] * s_light[2], 0.0f), 1.0f);
        shade[0] += d * s_light[3], shade[1] += d * s_light[4], shade[2] += d * s_light[5];
    }
}

// ---------------------------------------------------------------------------------------------------------------- the four shaders
// A shader has kLightFloats (the LDS it stages into), prologue(t, b, s_light) for thread t of a block of image b before the cover and
// operator()(mesh, b, pix, hit, s_light) for one live pixel after it: pix = (b S + i) S + j, [B,C,S,S] at pix + ((C - 1) b + c) S S.
struct DetailIO {            // what the detail panel adds to the grey one (sgdfr_shaperender_detail_f32)
    const float* face_uv;    // [F,3,2]
    const float* uv_normals; // [B,3,Su,Su]
    int Su;
    float *shape_detail, *normal_images, *grid;      // [B,3,S,S], [B,3,S,S], [B,S,S,2] or NULL
};
struct ShapeShader {         // sgdfr_shaperender_forward_f32 (SRenderY.render_shape); shape NULL: the cover alone (rasterize)
    const float* lights;     // [light_rows,L,6] direction, intensity
    int light_rows, L;
    const float* background; // [B,3,S,S] or NULL
    int gan_range;
    float *shape, *alpha;    // [B,3,S,S], [B,1,S,S] or NULL
    static constexpr int kLightFloats = kMaxLights * 6;

    // F.normalize(direction, eps=1e-12) and the intensities of this image's light t (forward() sets L = 0 where nothing is lit)
    __device__ __forceinline__ void prologue(int t, int b, float* s_light) const {
        if (t >= L) return;
        const float* l = lights + ((size_t)(light_rows == 1 ? 0 : b) * L + t) * 6;
        const float n = fmaxf(sqrtf(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]), 1e-12f);
        float* s = s_light + t * 6;
        s[0] = __fdiv_rn(l[0], n), s[1] = __fdiv_rn(l[1], n), s[2] = __fdiv_rn(l[2], n), s[3] = l[3], s[4] = l[4], s[5] = l[5];
    }
    // albedo . mean shading . alpha over the background (renderer.py:283-291)
    __device__ __forceinline__ float blend(float shade, float albedo, float a, float bg) const {
        const float v = albedo * __fdiv_rn(shade, (float)L) * a + bg * (1.0f - a);
        return gan_range ? fminf(fmaxf(v, 0.0f), 1.0f) * 2.0f - 1.0f : v;
    }
    // One live pixel of the grey panel and, with d, of the detail panel, which shares its albedo, alpha and background and takes its
    // shading normal from the UV normal map at the pixel's UV coordinate (ops['grid']).  d is a constant of the instance: NULL folds away.
    __device__ __forceinline__ void pixel(const Mesh& m, int b, size_t pix, const Hit& h, const float* s_light, const DetailIO* d) const {
        float n[3], shade[3] = {0.f, 0.f, 0.f}, albedo = 0.f, a = 0.f, dn[3] = {0.f, 0.f, 0.f}, dshade[3] = {0.f, 0.f, 0.f}, gx = 0.f, gy = 0.f;
        if (h.face >= 0) {
            albedo = (h.w0 + h.w1 + h.w2) * kAlbedo;
            a = normal_at(m, b, h, n) < kFrontZ ? 1.0f : 0.0f;       // renderer.py:272-277
            directional(s_light, L, n, shade);
            if (d) {
                face_uv_at(d->face_uv, h, gx, gy);
                grid_sample3(d->uv_normals + (size_t)b * 3 * d->Su * d->Su, d->Su, d->Su, gx, gy, dn);
                directional(s_light, L, dn, dshade);
            }
        }
        if (d && d->grid) d->grid[pix * 2] = gx, d->grid[pix * 2 + 1] = gy;
        if (alpha) alpha[pix] = a;
        const size_t plane = (size_t)m.S * m.S, o = pix + 2 * b * plane;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float bg = background ? background[o + c * plane] : 0.0f;
            if (shape) shape[o + c * plane] = blend(shade[c], albedo, a, bg);
            if (d) {
                if (d->normal_images) d->normal_images[o + c * plane] = dn[c];
                if (d->shape_detail) d->shape_detail[o + c * plane] = blend(dshade[c], albedo, a, bg);
            }
        }
    }
    __device__ __forceinline__ void operator()(const Mesh& m, int b, size_t pix, const Hit& h, const float* s_light) const {
        if (shape) pixel(m, b, pix, h, s_light, nullptr);
    }
};

struct DetailShader : ShapeShader {      // sgdfr_shaperender_detail_f32: the grey panel (shape may be NULL) and the detail panel
    DetailIO io;
    __device__ __forceinline__ void operator()(const Mesh& m, int b, size_t pix, const Hit& h, const float* s_light) const {
        pixel(m, b, pix, h, s_light, &io);
    }
};

struct TextureShader {       // sgdfr_shaperender_texture_f32 (SRenderY.forward); every output may be NULL
    const float* sh_coeff;   // [B,9,3] spherical-harmonic coefficients, or NULL: no shading
    float sh[9];             // renderer.py:114-119, rounded to float once on the host
    const float* face_uv;    // [F,3,2]
    const float* albedo;     // [B,3,Su,Su]
    int Su;
    float *images, *albedo_images, *shading, *normal_images, *alpha, *pos_mask, *grid;       // four [B,3,S,S], two [B,1,S,S], [B,S,S,2]
    static constexpr int kLightFloats = 27;

    __device__ __forceinline__ void prologue(int t, int b, float* s_light) const {      // this image's coefficients [9][3]
        if (sh_coeff && t < 27) s_light[t] = sh_coeff[(size_t)b * 27 + t];
    }
    // an uncovered pixel has every attribute 0, so its shading is add_SHlight(0) and everything else 0
    __device__ __forceinline__ void operator()(const Mesh& m, int b, size_t pix, const Hit& h, const float* s_light) const {
        float n[3] = {0.f, 0.f, 0.f}, al[3] = {0.f, 0.f, 0.f}, shd[3] = {0.f, 0.f, 0.f}, tzp = 0.f, gx = 0.f, gy = 0.f;
        const float a = h.face >= 0 ? 1.0f : 0.0f;
        if (h.face >= 0) {
            tzp = normal_at(m, b, h, n);
            face_uv_at(face_uv, h, gx, gy);
            if (images || albedo_images) grid_sample3(albedo + (size_t)b * 3 * Su * Su, Su, Su, gx, gy, al);
        }
        if (sh_coeff) sh_light(sh, s_light, n, shd);
        if (grid) grid[pix * 2] = gx, grid[pix * 2 + 1] = gy;
        if (alpha) alpha[pix] = a;
        if (pos_mask) pos_mask[pix] = tzp < kPosZ ? 1.0f : 0.0f;
        const size_t plane = (size_t)m.S * m.S, o = pix + 2 * b * plane;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (images) images[o + c * plane] = (sh_coeff ? al[c] * shd[c] : al[c]) * a;
            if (albedo_images) albedo_images[o + c * plane] = al[c] * a;
            if (shading) shading[o + c * plane] = shd[c];
            if (normal_images) normal_images[o + c * plane] = n[c] * a;
        }
    }
};

struct AttrShader {          // sgdfr_shaperender_attr_f32 (render_normal, render_depth): no normals, no lights
    const float* values;     // [B,V,D]
    int D;                   // 1..3
    float* out;              // [B,D,S,S]; 0 where no face covers
    static constexpr int kLightFloats = 0;

    __device__ __forceinline__ void prologue(int, int, float*) const {}
    __device__ __forceinline__ void operator()(const Mesh& m, int b, size_t pix, const Hit& h, const float*) const {
        const size_t plane = (size_t)m.S * m.S, o = pix + (size_t)(D - 1) * b * plane;
        for (int c = 0; c < D; ++c)
            out[o + c * plane] = h.face >= 0 ? mix3(h, values + (size_t)b * m.V * D, corners(m.faces, h.face), D, c) : 0.f;
    }
};

template <typename Shader>
__global__ __launch_bounds__(kChunk) void raster_kernel(const FaceRec* __restrict__ rec, const ushort4* __restrict__ box, int F, Mesh mesh,
                                                        RasterOut out, Shader shader) {
    __shared__ float4 s_rec[kChunk][3];
    __shared__ int s_wave[kChunk / kWave];
    float* s_light = nullptr;
    if constexpr (Shader::kLightFloats > 0) {        // the shader's own light table: an instance that stages none holds none
        __shared__ float s[Shader::kLightFloats];
        s_light = s;
    }
    const int t = threadIdx.x, b = blockIdx.z, S = mesh.S;
    const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
    const int j = tx0 + (t & (kTile - 1)), i = ty0 + t / kTile;
    const bool live = j < S && i < S;
    const float px = __fdiv_rn((float)(2 * j + 1), (float)S) - 1.0f, py = __fdiv_rn((float)(2 * i + 1), (float)S) - 1.0f;
    shader.prologue(t, b, s_light);                  // the cover's first barrier orders it before every pixel's read
    const Hit hit = cover(rec + (size_t)b * F, box + (size_t)b * F, F, t, tx0, ty0, live, px, py, s_rec, s_wave);
    if (!live) return;
    const size_t pix = ((size_t)b * S + i) * S + j;
    write_raster(out, pix, hit);
    shader(mesh, b, pix, hit, s_light);
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
                   int gan_range, float* shape, float* alpha, int* pix_to_face, float* zbuf, float* bary, const DetailShader* det, void* workspace,
                   int64_t workspace_bytes, void* stream, const TextureShader* tex = nullptr, float* normals = nullptr, float* tnormals = nullptr,
                   const AttrShader* attr = nullptr) {
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
    const int tiles = (S + kTile - 1) / kTile;
    const dim3 grid(tiles, tiles, rows);
    const Mesh mesh{faces, V, S, wn, ws.tz};
    const RasterOut out{pix_to_face, zbuf, bary};
    DetailShader lit = det ? *det : DetailShader{};    // the grey panel's arguments are the detail shader's base
    lit.lights = lights, lit.light_rows = light_rows, lit.L = shade ? L : 0, lit.background = background, lit.gan_range = gan_range;
    lit.shape = shape, lit.alpha = alpha;
    if (tex)
        raster_kernel<TextureShader><<<grid, kChunk, 0, st>>>(ws.rec, ws.box, F, mesh, out, *tex);
    else if (attr)
        raster_kernel<AttrShader><<<grid, kChunk, 0, st>>>(ws.rec, ws.box, F, mesh, out, *attr);
    else if (det)
        raster_kernel<DetailShader><<<grid, kChunk, 0, st>>>(ws.rec, ws.box, F, mesh, out, lit);
    else
        raster_kernel<ShapeShader><<<grid, kChunk, 0, st>>>(ws.rec, ws.box, F, mesh, out, lit);
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
    DetailShader det{};
    det.io.face_uv = face_uv, det.io.uv_normals = uv_normals, det.io.Su = Su;
    det.io.shape_detail = shape_detail, det.io.grid = grid, det.io.normal_images = detail_normal_images;
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
    TextureShader tex{};
    tex.sh_coeff = sh_lights, tex.face_uv = face_uv, tex.albedo = albedo, tex.Su = Su;
    for (int k = 0; k < 9; ++k) tex.sh[k] = sh_constants[k];
    tex.images = images, tex.albedo_images = albedo_images, tex.alpha = alpha_images, tex.pos_mask = pos_mask, tex.shading = shading_images;
    tex.grid = grid, tex.normal_images = normal_images;
    return forward(vertices, projected, cam, z_offset, rows, V, faces, F, csr_offsets, csr_entries, S, nullptr, 0, 0, nullptr, 0, nullptr,
                   nullptr, pix_to_face, zbuf, bary, nullptr, workspace, workspace_bytes, stream, &tex, normals, transformed_normals);
}

extern "C" int sgdfr_shaperender_attr_f32(const float* projected, float z_offset, int rows, int V, const int* faces, int F, int S,
                                          const float* values, int D, float* out, int* pix_to_face, float* zbuf, float* bary, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(projected, "shaperender_attr: null projected");
    const AttrShader attr{values, D, out};
    return forward(nullptr, projected, nullptr, z_offset, rows, V, faces, F, nullptr, nullptr, S, nullptr, 0, 0, nullptr, 0, nullptr, nullptr,
                   pix_to_face, zbuf, bary, nullptr, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr, &attr);
}
