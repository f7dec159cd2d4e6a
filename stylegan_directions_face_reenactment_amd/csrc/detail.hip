// DECA's detail path in eval mode, forward only (libs/DECA/decalib/models/decoders.py Generator with sample_mode 'bilinear',
// deca.py:114-141 displacement2normal / displacement2vertex, utils/renderer.py:331-340 world2uv).  Contract: include/sgdfr.h.
//
// D_detail: latent [rows,181] -> Linear 181->8192 with the first BatchNorm folded in, seen as [rows,128,8,8] -> five times (2x bilinear
// upsample, conv3x3 pad 1 with its BatchNorm folded in, LeakyReLU 0.2): 128@16^2, 64@32^2, 64@64^2, 32@128^2, 16@256^2 -> conv3x3 16->1,
// tanh, * out_scale.  Every layer is ONE implicit-GEMM launch on exact-f32 MFMA, the tile of conv_tile.h with its split over K and
// fixed-order finish.  What this network adds is the gather: for output pixel (y, x) and tap (dy, dx) a thread computes the value of
// the 2x upsampled map at (y + dy - 1, x + dx - 1) from four values of the low-resolution map (upsample_bilinear2d, align_corners
// False: source coordinate max(0, (i + 0.5) / 2 - 0.5), upper neighbour clamped to h - 1), zero outside the UPSAMPLED map (the conv's
// padding).  The upsampled tensors (up to 8.4 MB a row) never exist in memory; the four values of neighbouring lanes fall into the
// same cache lines of a map that is a quarter of the output's size.  Channel tiles: BN = 64, and BN = 16 for N <= 16 (32->16, 16->1).
//
// UV space: a per-layout table (pix_to_face, bary at S x S, rasterised once by shaperender.hip) turns per-vertex values into maps.
//   world2uv   1 thread / texel          sum_k bary_k value[faces[f][k]], 0 where no face covers
//   uvnormals  1 block / 16 x 16 texels  the dense vertex P = (uv_v + (uv_z mask) uv_n) + fixed_dis uv_n of the tile and a one-texel
//                                        halo goes to LDS; each texel then sums the corners of its (at most six) incident triangles of
//                                        util.generate_triangles(S, S) in ascending (face, corner) order and normalises.  No atomics.
// Floating-point contraction is OFF for the whole file: the UV pass is compared with a restatement that does not fuse.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "conv_tile.h"
#include "mesh_sample.h"

#pragma clang fp contract(off)

namespace sgdfr {
namespace {

constexpr int kLatent = 181, kBase = 8, kBaseC = 128, kFeat = kBaseC * kBase * kBase;
constexpr int kLayers = 5;                                   // up + conv + BN + LeakyReLU
constexpr int kCin[kLayers + 1] = {128, 128, 64, 64, 32, 16};   // the last entry: conv 16 -> 1
constexpr int kCout[kLayers + 1] = {128, 64, 64, 32, 16, 1};
constexpr int kUvSize = kBase << kLayers;                    // 256
constexpr float kSlope = 0.2f;
constexpr int kParams = 2 + 2 * (kLayers + 1);               // pointers sgdfr_detail_prepack_f32 takes
constexpr int kMaxRows = 256;
constexpr int kMaxC = 1024, kMaxHW = 256;                    // sgdfr_detail_upconv_f32
// split K only below 512 output tiles, at most 512 / tiles slices: S * (output elements) <= 512 tiles of 64 x 64
constexpr int64_t kPartElems = 512LL * BM * 64;

// ------------------------------------------------------------------ weight pack
struct PackLayout {
    int64_t w_fc, b_fc, w[kLayers + 1], b[kLayers + 1], total;
};
static PackLayout pack_layout() {
    PackLayout p;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    p.w_fc = take((int64_t)kLatent * kFeat), p.b_fc = take(kFeat);
    for (int i = 0; i <= kLayers; ++i) p.w[i] = take(9LL * kCin[i] * kCout[i]), p.b[i] = take(kCout[i]);
    p.total = o;
    return p;
}

// copy: dst[j] = src[j].  Else [k = ci*kk + r][co] <- W[co][ci][r]
__global__ __launch_bounds__(kThreads) void detail_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t count, int copy,
                                                               int cin, int cout, int kk) {
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < count; j += (int64_t)gridDim.x * kThreads) {
        float v;
        if (copy) {
            v = src[j];
        } else {
            const int64_t K = (int64_t)cin * kk, k = j / cout, co = j - k * cout;
            v = src[co * K + k];
        }
        dst[j] = v;
    }
}

static int launch_pack(const float* src, float* dst, int64_t count, int copy, int cin, int cout, int kk, hipStream_t st) {
    hipLaunchKernelGGL(detail_pack_kernel, dim3(grid_1d(count)), dim3(kThreads), 0, st, src, dst, count, copy, cin, cout, kk);
    return check_launch("detail pack");
}

// ------------------------------------------------------------------ implicit-GEMM conv behind a 2x bilinear upsample
// every tensor is dense [R, C, H, W]
struct ConvArgs {
    const float* src;        // [R, C, Hs, Ws], C = K / (KS*KS): the LOW-resolution map when UP
    const float* wp;         // [K][N]
    const float* bias;       // + bias[n]
    float* out;              // [R, N, Ho, Wo]; UP: Ho = 2 Hs, Wo = 2 Ws, else Ho = Hs, Wo = Ws
    float* part;             // split K: [S][R*N*Ho*Wo]
    int64_t part_elems;
    int R, Hs, Ws, N, Ho, Wo, K, cps, tanh_out;
    float slope, scale;      // v > 0 ? v : v * slope; tanh_out: tanh(v) * scale instead
};

__device__ __forceinline__ void epilogue(const ConvArgs& a, int b, int n, int p, float v) {
    const int64_t o = ((int64_t)b * a.N + n) * (a.Ho * a.Wo) + p;
    v += a.bias[n];
    a.out[o] = a.tanh_out ? tanhf(v) * a.scale : (v > 0.f ? v : v * a.slope);
}

// upsample_bilinear2d at scale 2, align_corners False: output index u of 2n -> lower and upper source index and the upper one's weight
// (0.25 or 0.75; 0 at u = 0).  (u + 0.5) / 2 - 0.5 is exact in fp32 for u < 2^22.
__device__ __forceinline__ void up_coord(int u, int n, int& i0, int& i1, float& l1) {
    const float s = fmaxf(((float)u + 0.5f) * 0.5f - 0.5f, 0.f);
    i0 = (int)s;
    i1 = min(i0 + 1, n - 1);
    l1 = s - (float)i0;
}

template <int BN, int KS, bool UP>
__global__ __launch_bounds__(kThreads) void detail_conv_kernel(ConvArgs a) {
    __shared__ ConvLds<BN> lds;
    constexpr int PAD = KS / 2;
    const int t = threadIdx.x, wv = t >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int HWo = a.Ho * a.Wo, M = a.R * HWo;
    const int plane = a.Hs * a.Ws;

    // the pixel this thread gathers (fixed over K)
    const int gm = m0 + (t & (BM - 1));
    const bool mvalid = gm < M;
    int b = 0, oh = 0, ow = 0;
    if (mvalid) {
        b = gm / HWo;
        const int p = gm - b * HWo;
        oh = p / a.Wo;
        ow = p - oh * a.Wo;
    }
    const float* srcb = a.src + (int64_t)b * (a.K / (KS * KS)) * plane;

    const int nchunks = (a.K + BK - 1) / BK;
    const int c0 = blockIdx.z * a.cps, c1 = min(nchunks, c0 + a.cps);
    float xr[4], wr[Tile<BN>::WL];
    auto gload = [&](int c) {
        const int k0 = c * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + wv + 4 * i;
            float v = 0.f;
            if (k < a.K) {
                const int ci = k / (KS * KS), r = k - ci * (KS * KS), kh = r / KS, kw = r - kh * KS;
                const int ih = oh - PAD + kh, iw = ow - PAD + kw;      // in the conv's input: the upsampled map when UP
                if (mvalid && ih >= 0 && ih < a.Ho && iw >= 0 && iw < a.Wo) {
                    const float* pl = srcb + ci * plane;               // ci is uniform over the wave
                    if (UP) {
                        int y0, y1, x0, x1;
                        float ly, lx;
                        up_coord(ih, a.Hs, y0, y1, ly);
                        up_coord(iw, a.Ws, x0, x1, lx);
                        const float v00 = pl[y0 * a.Ws + x0], v01 = pl[y0 * a.Ws + x1];
                        const float v10 = pl[y1 * a.Ws + x0], v11 = pl[y1 * a.Ws + x1];
                        const float hy = 1.f - ly, hx = 1.f - lx;
                        v = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
                    } else {
                        v = pl[ih * a.Ws + iw];
                    }
                }
            }
            xr[i] = v;
        }
        load_w<BN>(wr, a.wp, a.K, a.N, k0, n0);
    };
    auto sstore = [&](int buf) {
        store_x(lds.xs[buf], xr);
        store_w<BN>(lds.ws[buf], wr);
    };

    floatx4 acc[Tile<BN>::TN][Tile<BN>::TM];
    k_loop<BN>(lds, c0, c1, gload, sstore, acc);

    float* const slice = slice_of(a.part, a.part_elems);
    for_each_output<BN>(acc, m0, n0, M, a.N, HWo, [=](int bb, int gn, int p, float v) {
        if (slice)
            slice[((int64_t)bb * a.N + gn) * HWo + p] = v;
        else
            epilogue(a, bb, gn, p, v);
    });
}

// sum of the K slices in fixed order + the conv's epilogue
__global__ __launch_bounds__(kThreads) void detail_finish_kernel(ConvArgs a, int S) {
    finish_slices(a.part, a.part_elems, S, a.N, a.Ho * a.Wo, [=](int b, int n, int p, float v) { epilogue(a, b, n, p, v); });
}

// ------------------------------------------------------------------ host side
static int launch_conv(const ConvArgs& a0, int ks, bool up, float* part, hipStream_t st) {
    ConvArgs a = a0;
    // The channel tile follows N, the number of K slices the output tiles, i.e. the layer and the row count, nothing else.
    const int bn = a.N <= 16 ? 16 : 64;
    const int M = a.R * a.Ho * a.Wo;
    const ConvPlan p = plan_conv(M, a.N, a.K, bn, conv_tiles(M, a.N, bn));
    SGDFR_REQUIRE(p.S == 1 || p.S * p.out_elems <= kPartElems, "detail: split-K partials of %lld floats exceed the workspace",
                  (long long)(p.S * p.out_elems));
    a.cps = p.cps;
    a.part = part;
    a.part_elems = p.out_elems;
    const dim3 grid(p.mt, p.nt, p.S);
    if (ks == 3 && up && bn == 64)
        hipLaunchKernelGGL((detail_conv_kernel<64, 3, true>), grid, dim3(kThreads), 0, st, a);
    else if (ks == 3 && up)
        hipLaunchKernelGGL((detail_conv_kernel<16, 3, true>), grid, dim3(kThreads), 0, st, a);
    else if (ks == 3 && bn == 64)
        hipLaunchKernelGGL((detail_conv_kernel<64, 3, false>), grid, dim3(kThreads), 0, st, a);
    else if (ks == 3)
        hipLaunchKernelGGL((detail_conv_kernel<16, 3, false>), grid, dim3(kThreads), 0, st, a);
    else if (ks == 1 && !up && bn == 64)
        hipLaunchKernelGGL((detail_conv_kernel<64, 1, false>), grid, dim3(kThreads), 0, st, a);       // the linear layer
    else
        SGDFR_REQUIRE(false, "detail: no conv instance for k=%d up=%d bn=%d", ks, (int)up, bn);
    if (check_launch("detail conv")) return 2;
    if (p.S > 1) {
        hipLaunchKernelGGL(detail_finish_kernel, dim3(grid_1d(p.out_elems)), dim3(kThreads), 0, st, a, p.S);
        if (check_launch("detail finish")) return 2;
    }
    return 0;
}

static ConvArgs conv_args(const float* src, int Hs, int Ws, const float* wp, const float* bias, int K, int N, bool up, float slope, float* out,
                          int R) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src, a.wp = wp, a.bias = bias, a.out = out;
    a.R = R, a.Hs = Hs, a.Ws = Ws, a.N = N, a.K = K, a.slope = slope, a.scale = 1.f;
    a.Ho = up ? 2 * Hs : Hs, a.Wo = up ? 2 * Ws : Ws;
    return a;
}

// per row: the linear layer's output and the five layers' outputs, in this order (what `taps` receives)
struct TapLayout {
    int64_t at[kLayers + 1], total;
};
static TapLayout tap_layout(int rows) {
    TapLayout t;
    int64_t o = 0;
    t.at[0] = o, o += (int64_t)rows * kFeat;
    for (int i = 0; i < kLayers; ++i) {
        const int s = kBase << (i + 1);
        t.at[i + 1] = o, o += (int64_t)rows * kCout[i] * s * s;
    }
    t.total = o;
    return t;
}

constexpr int64_t kMaxAct = 16LL * kUvSize * kUvSize;    // the largest activation of a row (the fifth layer's output)
struct WsLayout {
    int64_t part, act[2], total;      // float offsets
};
static WsLayout ws_layout(int rows) {
    WsLayout w;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    w.part = take(kPartElems);
    w.act[0] = take((int64_t)rows * kMaxAct);            // stages 1, 3, 5 write here (stage 0 = the linear layer, 5 = the fifth layer)
    w.act[1] = take((int64_t)rows * kMaxAct / 2);        // stages 0, 2, 4: the fourth layer's output is half the fifth's
    w.total = o;
    return w;
}

static bool rows_ok(int rows) { return rows >= 1 && rows <= kMaxRows; }

// ------------------------------------------------------------------ UV space
constexpr int kUvMin = 13, kUvMax = 1024;
constexpr int kTile = 16, kHalo = kTile + 2;

// the quads of util.generate_triangles(S, S): x in [2, S-3), y in [5, S-6)
__device__ __forceinline__ bool quad_ok(int qy, int qx, int S) { return qx >= 2 && qx < S - 3 && qy >= 5 && qy < S - 6; }

__global__ __launch_bounds__(256) void world2uv_kernel(const float* __restrict__ values, int V, const int* __restrict__ faces, int F,
                                                       const int* __restrict__ pix_to_face, const float* __restrict__ bary, int S,
                                                       float* __restrict__ out) {
    const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x, plane = S * S;
    if (t >= plane) return;
    float r[3];
    bary_gather3(values + (size_t)b * V * 3, V, faces, F, pix_to_face, bary, t, r);
    float* o = out + (size_t)b * 3 * plane + t;
    o[0] = r[0], o[plane] = r[1], o[2 * (size_t)plane] = r[2];
}

// corner contribution (u - o) x (w - o) of util.vertex_normals, added to n
__device__ __forceinline__ void add_corner(const float* o, const float* u, const float* w, float (&n)[3]) {
    const float ux = u[0] - o[0], uy = u[1] - o[1], uz = u[2] - o[2];
    const float wx = w[0] - o[0], wy = w[1] - o[1], wz = w[2] - o[2];
    n[0] += uy * wz - uz * wy;
    n[1] += uz * wx - ux * wz;
    n[2] += ux * wy - uy * wx;
}

__global__ __launch_bounds__(kTile * kTile) void uvnormals_kernel(const float* __restrict__ uv_z, const float* __restrict__ verts,
                                                                  const float* __restrict__ normals, int V, const int* __restrict__ faces, int F,
                                                                  const int* __restrict__ pix_to_face, const float* __restrict__ bary,
                                                                  const float* __restrict__ mask, const float* __restrict__ fixed_dis, int S,
                                                                  float* __restrict__ out, float* __restrict__ dense) {
    __shared__ float s_p[kHalo * kHalo][3];
    const int t = threadIdx.x, b = blockIdx.z, plane = S * S;
    const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
    const float* pv = verts + (size_t)b * V * 3;
    const float* pn = normals + (size_t)b * V * 3;
    for (int cell = t; cell < kHalo * kHalo; cell += kTile * kTile) {
        const int cy = cell / kHalo, cx = cell - cy * kHalo;
        const int y = ty0 - 1 + cy, x = tx0 - 1 + cx;
        float P[3] = {0.f, 0.f, 0.f};
        if (y >= 0 && y < S && x >= 0 && x < S) {
            const int tex = y * S + x;
            float v[3], n[3];
            // the second gather is made only under a covered texel, so an uncovered one stays exactly 0 whatever z and d hold
            if (bary_gather3(pv, V, faces, F, pix_to_face, bary, tex, v) && bary_gather3(pn, V, faces, F, pix_to_face, bary, tex, n)) {
                const float z = uv_z[(size_t)b * plane + tex] * mask[tex], d = fixed_dis[tex];
#pragma unroll
                for (int c = 0; c < 3; ++c) P[c] = (v[c] + z * n[c]) + d * n[c];
            }
            if (dense && cy >= 1 && cy <= kTile && cx >= 1 && cx <= kTile) {
                float* o = dense + ((size_t)b * plane + tex) * 3;
                o[0] = P[0], o[1] = P[1], o[2] = P[2];
            }
        }
        s_p[cell][0] = P[0], s_p[cell][1] = P[1], s_p[cell][2] = P[2];
    }
    __syncthreads();
    const int ly = t / kTile, lx = t - ly * kTile;
    const int y = ty0 + ly, x = tx0 + lx;
    if (y >= S || x >= S) return;
    // the vertex (y, x) is corner a of quad (y, x), b of quad (y, x-1), c of quad (y-1, x), d of quad (y-1, x-1); a quad is the faces
    // T0 = (a, c, b), T1 = (b, c, d), quads ordered by x, then y.  Ascending (face, corner):
    auto at = [&](int dy, int dx) -> const float* { return s_p[(ly + 1 + dy) * kHalo + lx + 1 + dx]; };
    const float* o = at(0, 0);
    float n[3] = {0.f, 0.f, 0.f};
    if (quad_ok(y - 1, x - 1, S)) add_corner(o, at(-1, 0), at(0, -1), n);      // T1 = (b, c, d), corner 2: (b - d) x (c - d)
    if (quad_ok(y, x - 1, S)) {
        add_corner(o, at(0, -1), at(1, -1), n);                                // T0 = (a, c, b), corner 2: (a - b) x (c - b)
        add_corner(o, at(1, -1), at(1, 0), n);                                 // T1 = (b, c, d), corner 0: (c - b) x (d - b)
    }
    if (quad_ok(y - 1, x, S)) {
        add_corner(o, at(-1, 1), at(-1, 0), n);                                // T0 = (a, c, b), corner 1: (b - c) x (a - c)
        add_corner(o, at(0, 1), at(-1, 1), n);                                 // T1 = (b, c, d), corner 1: (d - c) x (b - c)
    }
    if (quad_ok(y, x, S)) add_corner(o, at(1, 0), at(0, 1), n);                // T0 = (a, c, b), corner 0: (c - a) x (b - a)
    const float len = fmaxf(sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-6f);       // F.normalize(eps=1e-6)
    float* q = out + (size_t)b * 3 * plane + y * S + x;
    q[0] = __fdiv_rn(n[0], len), q[plane] = __fdiv_rn(n[1], len), q[2 * (size_t)plane] = __fdiv_rn(n[2], len);
}

static bool uv_sizes_ok(int rows, int V, int F, int S) {
    return rows >= 1 && rows <= 4096 && V >= 1 && V <= (1 << 24) && F >= 1 && F <= (1 << 24) && S >= kUvMin && S <= kUvMax;
}

}  // namespace
}  // namespace sgdfr

using namespace sgdfr;

extern "C" int64_t sgdfr_detail_pack_elems(void) { return pack_layout().total; }

extern "C" int64_t sgdfr_detail_workspace_bytes(int rows) {
    if (!rows_ok(rows)) return -1;
    return ws_layout(rows).total * (int64_t)sizeof(float);
}

extern "C" int64_t sgdfr_detail_upconv_workspace_bytes(int Cin, int Cout) {
    if (Cin < 1 || Cin > kMaxC || Cout < 1 || Cout > kMaxC) return -1;
    return (kPartElems + align64(9LL * Cin * Cout)) * (int64_t)sizeof(float);
}

extern "C" int sgdfr_detail_prepack_f32(const float* const* params, float* pack, void* stream) {
    SGDFR_REQUIRE(params && pack, "detail_prepack: null pointer");
    for (int i = 0; i < kParams; ++i) SGDFR_REQUIRE(params[i], "detail_prepack: parameter %d is null", i);
    const PackLayout pl = pack_layout();
    hipStream_t st = as_stream(stream);
    if (launch_pack(params[0], pack + pl.w_fc, (int64_t)kLatent * kFeat, 0, kLatent, kFeat, 1, st)) return 2;
    if (launch_pack(params[1], pack + pl.b_fc, kFeat, 1, 0, 0, 0, st)) return 2;
    for (int i = 0; i <= kLayers; ++i) {
        if (launch_pack(params[2 + 2 * i], pack + pl.w[i], 9LL * kCin[i] * kCout[i], 0, kCin[i], kCout[i], 9, st)) return 2;
        if (launch_pack(params[3 + 2 * i], pack + pl.b[i], kCout[i], 1, 0, 0, 0, st)) return 2;
    }
    return 0;
}

extern "C" int sgdfr_detail_upconv_f32(const float* x, const float* w, const float* bias, int rows, int Cin, int Cout, int h, int wd, float slope,
                                       int up, float* y, void* workspace, int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(x && w && bias && y && workspace, "detail_upconv: null pointer");
    SGDFR_REQUIRE(rows >= 1 && rows <= 4096 && Cin >= 1 && Cin <= kMaxC && Cout >= 1 && Cout <= kMaxC && h >= 1 && h <= kMaxHW && wd >= 1 &&
                      wd <= kMaxHW,
                  "detail_upconv: rows=%d Cin=%d Cout=%d h=%d w=%d (rows 1..4096, channels 1..%d, sides 1..%d)", rows, Cin, Cout, h, wd, kMaxC,
                  kMaxHW);
    const int64_t pixels = (int64_t)rows * h * wd * (up ? 4 : 1);
    SGDFR_REQUIRE(pixels <= (1LL << 28), "detail_upconv: %lld output pixels (at most 2^28)", (long long)pixels);
    const int64_t need = sgdfr_detail_upconv_workspace_bytes(Cin, Cout);
    SGDFR_REQUIRE(workspace_bytes >= need, "detail_upconv: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    float* wsf = reinterpret_cast<float*>(workspace);
    float* wp = wsf + kPartElems;
    hipStream_t st = as_stream(stream);
    if (launch_pack(w, wp, 9LL * Cin * Cout, 0, Cin, Cout, 9, st)) return 2;
    const ConvArgs a = conv_args(x, h, wd, wp, bias, 9 * Cin, Cout, up != 0, slope, y, rows);
    return launch_conv(a, 3, up != 0, wsf, st);
}

extern "C" int sgdfr_detail_decode_f32(const float* latent, int rows, const float* pack, float out_scale, float* uv_z, float* taps,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(rows_ok(rows), "detail_decode: unsupported size (%d rows, 1..%d)", rows, kMaxRows);
    SGDFR_REQUIRE(latent && pack && uv_z && workspace, "detail_decode: null pointer");
    const WsLayout wl = ws_layout(rows);
    SGDFR_REQUIRE(wl.total * (int64_t)sizeof(float) <= workspace_bytes, "detail_decode: workspace of %lld bytes, %d rows need %lld",
                  (long long)workspace_bytes, rows, (long long)(wl.total * (int64_t)sizeof(float)));
    const PackLayout pl = pack_layout();
    const TapLayout tl = tap_layout(rows);
    float* wsf = reinterpret_cast<float*>(workspace);
    float* part = wsf + wl.part;
    hipStream_t st = as_stream(stream);
    // stage i's output: straight into the caller's taps, else the two workspace buffers in turn (stage 0 = the linear layer)
    auto buffer = [&](int i) { return taps ? taps + tl.at[i] : wsf + wl.act[(i + 1) & 1]; };

    ConvArgs a = conv_args(latent, 1, 1, pack + pl.w_fc, pack + pl.b_fc, kLatent, kFeat, false, 1.f, buffer(0), rows);
    if (launch_conv(a, 1, false, part, st)) return 2;
    for (int i = 0; i < kLayers; ++i) {
        const int s = kBase << i;
        a = conv_args(buffer(i), s, s, pack + pl.w[i], pack + pl.b[i], 9 * kCin[i], kCout[i], true, kSlope, buffer(i + 1), rows);
        if (launch_conv(a, 3, true, part, st)) return 2;
    }
    a = conv_args(buffer(kLayers), kUvSize, kUvSize, pack + pl.w[kLayers], pack + pl.b[kLayers], 9 * kCin[kLayers], 1, false, 1.f, uv_z, rows);
    a.tanh_out = 1, a.scale = out_scale;
    return launch_conv(a, 3, false, part, st);
}

extern "C" int sgdfr_detail_world2uv_f32(const float* values, int rows, int V, const int* faces, int F, const int* pix_to_face,
                                         const float* bary, int S, float* out, void* stream) {
    SGDFR_REQUIRE(values && faces && pix_to_face && bary && out, "detail_world2uv: null pointer");
    SGDFR_REQUIRE(uv_sizes_ok(rows, V, F, S), "detail_world2uv: rows=%d V=%d F=%d uv_size=%d (rows 1..4096, V and F 1..2^24, uv_size %d..%d)", rows,
                  V, F, S, kUvMin, kUvMax);
    world2uv_kernel<<<dim3((S * S + 255) / 256, rows), 256, 0, as_stream(stream)>>>(values, V, faces, F, pix_to_face, bary, S, out);
    return check_launch("detail world2uv_kernel");
}

extern "C" int sgdfr_detail_uvnormals_f32(const float* uv_z, const float* vertices, const float* normals, int rows, int V, const int* faces, int F,
                                          const int* pix_to_face, const float* bary, const float* mask, const float* fixed_dis, int S,
                                          float* uv_normals, float* dense_vertices, void* stream) {
    SGDFR_REQUIRE(uv_z && vertices && normals && faces && pix_to_face && bary && mask && fixed_dis && uv_normals, "detail_uvnormals: null pointer");
    SGDFR_REQUIRE(uv_sizes_ok(rows, V, F, S), "detail_uvnormals: rows=%d V=%d F=%d uv_size=%d (rows 1..4096, V and F 1..2^24, uv_size %d..%d)", rows,
                  V, F, S, kUvMin, kUvMax);
    const int tiles = (S + kTile - 1) / kTile;
    uvnormals_kernel<<<dim3(tiles, tiles, rows), kTile * kTile, 0, as_stream(stream)>>>(uv_z, vertices, normals, V, faces, F, pix_to_face, bary,
                                                                                     mask, fixed_dis, S, uv_normals, dense_vertices);
    return check_launch("detail uvnormals_kernel");
}
