// DECA's coefficient encoder in eval mode (decalib/models/encoders.py ResnetEncoder(outsize=236), models/resnet.py:21-118,
// datasets.py:57-82, image_utils.py:87-94, rotation_converter.py:312-360): [-1,1] image -> [0,255] -> affine 224x224 crop / 255 ->
// ResNet-50 trunk (conv7x7/2 + BN + ReLU, max-pool 3x3/2, 16 bottlenecks, 7x7 average pool) -> Linear 2048->1024 + ReLU ->
// Linear 1024->236, and the Euler angles in degrees of pose[:3]; and dL/dx of the 236 parameters (the weights are frozen: no
// weight gradients).
//
// Every conv, every input-gradient conv and the four head GEMMs are one implicit-GEMM kernel on exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32), tiled and split over K like idloss.hip's: rows = output channels, columns = pixels, the K loop
// double-buffered through registers.  All 53 BatchNorms are folded into filters + bias on the host (deca.py, once per weight
// version).  The backward needs only the forward's decisions: one byte per ReLU decision and per max-pool choice is saved (and
// nothing at all when `saved` is NULL).  No float atomics, no host synchronisation, everything on the given stream.
#include <string.h>

#include <algorithm>

#include "conv_tile.h"

namespace sgdfr {
namespace {

constexpr int kBlocks = 16;
constexpr int kCrop = 224, kCropPlane = kCrop * kCrop;
constexpr int kStem = 112, kPool = 56;
constexpr int kFeat = 2048, kHidden = 1024, kOut = 236;
constexpr int kParams = 2 + 8 * kBlocks + 4;     // pointers sgdfr_deca_prepack_f32 takes
constexpr int kMaxRows = 1024;
constexpr int BN = 64;
// split K only below 512 output tiles, at most 512 / tiles slices: S * (output elements) <= 512 tiles
constexpr int64_t kPartElems = 512LL * BM * BN;

enum { TAP_FWD = 0, TAP_DGRAD = 1 };
enum { EP_RAW = 0, EP_BIAS = 1, EP_BIAS_RELU = 2, EP_BIAS_ADD_RELU = 3, EP_MASK = 4, EP_ADD_MASK = 5 };

// ------------------------------------------------------------------ network geometry
struct Block {
    int cin, p, stride, h, ho;   // input [cin, h, h] -> conv1 [p, h, h] -> conv2 [p, ho, ho] -> conv3 [4p, ho, ho]
    bool ds;                     // projection shortcut conv1x1 at the stride + BN; else identity
};
static void make_blocks(Block* b) {
    const int planes[4] = {64, 128, 256, 512}, count[4] = {3, 4, 6, 3};
    int c = 64, h = kPool, i = 0;
    for (int s = 0; s < 4; ++s)
        for (int k = 0; k < count[s]; ++k, ++i) {
            Block& x = b[i];
            x.cin = c, x.p = planes[s], x.stride = (k == 0 && s > 0) ? 2 : 1, x.h = h;
            x.ho = (h - 1) / x.stride + 1;
            x.ds = k == 0;
            c = 4 * planes[s], h = x.ho;
        }
}

// ------------------------------------------------------------------ weight pack
struct BlockPack {
    int64_t wf1, b1, wf2, wd2, b2, wf3, wd3, b3, wfd, bd, wdx;
};
struct PackLayout {
    int64_t wf0, w0, b0;
    BlockPack u[kBlocks];
    int64_t wf_fc1, wd_fc1, b_fc1, wf_fc2, wd_fc2, b_fc2, total;
};
static PackLayout pack_layout() {
    Block bs[kBlocks];
    make_blocks(bs);
    PackLayout p;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    p.wf0 = take(147 * 64), p.w0 = take(147 * 64), p.b0 = take(64);
    for (int i = 0; i < kBlocks; ++i) {
        const Block& u = bs[i];
        BlockPack& q = p.u[i];
        const int64_t c4 = 4LL * u.p;
        q.wf1 = take((int64_t)u.cin * u.p), q.b1 = take(u.p);
        q.wf2 = take(9LL * u.p * u.p), q.wd2 = take(9LL * u.p * u.p), q.b2 = take(u.p);
        q.wf3 = take(u.p * c4), q.wd3 = take(u.p * c4), q.b3 = take(c4);
        q.wfd = u.ds ? take(u.cin * c4) : -1;
        q.bd = u.ds ? take(c4) : -1;
        q.wdx = take((u.p + (u.ds ? c4 : 0)) * u.cin);
    }
    p.wf_fc1 = take((int64_t)kFeat * kHidden), p.wd_fc1 = take((int64_t)kFeat * kHidden), p.b_fc1 = take(kHidden);
    p.wf_fc2 = take((int64_t)kHidden * kOut), p.wd_fc2 = take((int64_t)kHidden * kOut), p.b_fc2 = take(kOut);
    p.total = o;
    return p;
}

enum { SEG_COPY = 0, SEG_FWD = 1, SEG_DGRAD = 2 };
// COPY: dst[j] = src[j] (also the input-gradient weights [co][ci] of a 1x1 conv).  FWD: [k = ci*kk + r][co] <- W[co][ci][r].
// DGRAD: [co*kk + r][ci] <- W[co][ci][r]: the input-gradient conv gathers dO at (o + pad - kh) / stride, so its weights are
// transposed, not flipped.
__global__ __launch_bounds__(kThreads) void deca_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t count,
                                                             int kind, int cin, int cout, int kk) {
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < count; j += (int64_t)gridDim.x * kThreads) {
        float v;
        if (kind == SEG_COPY) {
            v = src[j];
        } else if (kind == SEG_FWD) {
            const int64_t K = (int64_t)cin * kk, k = j / cout, co = j - k * cout;
            v = src[co * K + k];
        } else {
            const int64_t row = j / cin, ci = j - row * cin, co = row / kk, r = row - co * kk;
            v = src[(co * cin + ci) * kk + r];
        }
        dst[j] = v;
    }
}

// ------------------------------------------------------------------ implicit-GEMM conv
// every tensor is dense [R, C, H, W]
struct ConvArgs {
    const float* src;        // [R, Cs, Hs, Ws], Cs = K1 / (KS*KS)
    const float* ext;        // EXT, k >= K1: a second operand [R, K - K1, He, We] read at (oh/es, ow/es) where es divides both (else 0)
    const float* wp;         // [K][N]
    const float* bias;       // EP_BIAS*
    const float* aux;        // EP_BIAS_ADD_RELU, EP_ADD_MASK: addend [R, N, Ho, Wo]
    const uint8_t* mask_in;  // EP_MASK, EP_ADD_MASK: the result passes where the byte is set (NULL: everywhere)
    uint8_t* mask_out;       // EP_BIAS_RELU, EP_BIAS_ADD_RELU: receives (pre-activation > 0) (NULL: not kept)
    float* out;              // [R, N, Ho, Wo]
    float* part;             // split K: [S][R*N*Ho*Wo]
    int64_t part_elems;
    int R, Hs, Ws, N, Ho, Wo, K, K1, stride, pad, cps, epi, He, We, es;
};

__device__ __forceinline__ void epilogue(const ConvArgs& a, int b, int n, int p, float v) {
    const int64_t o = ((int64_t)b * a.N + n) * (a.Ho * a.Wo) + p;
    float r;
    switch (a.epi) {
        case EP_RAW: r = v; break;
        case EP_BIAS: r = v + a.bias[n]; break;
        case EP_BIAS_RELU:
        case EP_BIAS_ADD_RELU: {
            float pre = v + a.bias[n];
            if (a.epi == EP_BIAS_ADD_RELU) pre += a.aux[o];
            const bool on = pre > 0.f;
            if (a.mask_out) a.mask_out[o] = on ? 1 : 0;
            r = on ? pre : 0.f;
            break;
        }
        default: {   // EP_MASK, EP_ADD_MASK
            r = a.epi == EP_ADD_MASK ? v + a.aux[o] : v;
            if (a.mask_in && !a.mask_in[o]) r = 0.f;
        }
    }
    a.out[o] = r;
}

template <int TAP, int KS, bool EXT>
__global__ __launch_bounds__(kThreads) void deca_conv_kernel(ConvArgs a) {
    __shared__ ConvLds<BN> lds;
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
    const float* srcb = a.src + (int64_t)b * (a.K1 / (KS * KS)) * plane;
    const float* extb = EXT ? a.ext + (int64_t)b * (a.K - a.K1) * (a.He * a.We) : nullptr;

    const int nchunks = (a.K + BK - 1) / BK;
    const int c0 = blockIdx.z * a.cps, c1 = min(nchunks, c0 + a.cps);
    float xr[4], wr[4];
    auto gload = [&](int c) {
        const int k0 = c * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + wv + 4 * i;
            float v = 0.f;
            if (k < a.K) {
                if (EXT && k >= a.K1) {
                    const int sh = a.es - 1;   // es is 1 or 2
                    if (mvalid && !((oh | ow) & sh)) v = extb[((k - a.K1) * a.He + (oh >> sh)) * a.We + (ow >> sh)];
                } else {
                    const int ci = k / (KS * KS), r = k - ci * (KS * KS), kh = r / KS, kw = r - kh * KS;
                    int ih, iw;
                    bool ok;
                    if (TAP == TAP_FWD) {
                        ih = oh * a.stride - a.pad + kh, iw = ow * a.stride - a.pad + kw;
                        ok = ih >= 0 && ih < a.Hs && iw >= 0 && iw < a.Ws;
                    } else if (a.stride == 1) {
                        ih = oh + a.pad - kh, iw = ow + a.pad - kw;
                        ok = ih >= 0 && ih < a.Hs && iw >= 0 && iw < a.Ws;
                    } else {           // stride 2: only the taps of this output's parity meet a dO sample
                        ih = oh + a.pad - kh, iw = ow + a.pad - kw;
                        ok = ih >= 0 && iw >= 0 && !((ih | iw) & 1);
                        ih >>= 1, iw >>= 1;
                        ok = ok && ih < a.Hs && iw < a.Ws;
                    }
                    if (mvalid && ok) v = srcb[ci * plane + ih * a.Ws + iw];
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

    floatx4 acc[2][2];
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
__global__ __launch_bounds__(kThreads) void deca_finish_kernel(ConvArgs a, int S) {
    finish_slices(a.part, a.part_elems, S, a.N, a.Ho * a.Wo, [=](int b, int n, int p, float v) { epilogue(a, b, n, p, v); });
}

// ------------------------------------------------------------------ front: [-1,1] -> [0,255], affine bilinear crop, / 255
// source position of output pixel (u, v) under the row's 2x3 matrix; the forward and the adjoint share these bits.  In fp64: a
// position near 256 carries an fp32 rounding of 1.5e-5 pixels, which would reach the bilinear weights (and through them the stem's
// near-tied max-pool choices) at 100 times the rounding of everything else; the two fused multiply-adds per pixel cost nothing.
__device__ __forceinline__ void src_pos(const float* m, int u, int v, double& sx, double& sy) {
    sx = fma((double)m[0], (double)u, fma((double)m[1], (double)v, (double)m[2]));
    sy = fma((double)m[3], (double)u, fma((double)m[4], (double)v, (double)m[5]));
}
__device__ __forceinline__ float to_255(float t) {
    return (fminf(fmaxf(t, -1.f), 1.f) + 1.f) / 2.00001f * 255.f;
}

__global__ __launch_bounds__(kThreads) void deca_front_kernel(const float* __restrict__ x, const float* __restrict__ mat, int B, int H,
                                                              int W, float* __restrict__ out) {
    const int64_t n = (int64_t)B * 3 * kCropPlane;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int u = (int)(idx % kCrop), v = (int)((idx / kCrop) % kCrop);
        const int bc = (int)(idx / kCropPlane), b = bc / 3;
        double sx, sy;
        src_pos(mat + 6 * b, u, v, sx, sy);
        float r = 0.f;
        if (sx > -1.0 && sx < (double)W && sy > -1.0 && sy < (double)H) {     // false for NaN as well
            const double fx0 = floor(sx), fy0 = floor(sy);
            const float fx = (float)(sx - fx0), fy = (float)(sy - fy0);
            const int x0 = (int)fx0, y0 = (int)fy0;
            const float* pl = x + (int64_t)bc * H * W;
            auto tap = [&](int yy, int xx) { return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? to_255(pl[(int64_t)yy * W + xx]) : 0.f; };
            const float v00 = tap(y0, x0), v01 = tap(y0, x0 + 1), v10 = tap(y0 + 1, x0), v11 = tap(y0 + 1, x0 + 1);
            r = (v00 * ((1.f - fx) * (1.f - fy)) + v01 * (fx * (1.f - fy))) + (v10 * ((1.f - fx) * fy) + v11 * (fx * fy));
        }
        out[idx] = r / 255.f;
    }
}

// dL/dx [B,3,H,W]: a gather per source pixel over the output pixels whose 2x2 footprint can contain it -- the bounding box of the
// inverse-mapped square |sx - w| < 1, |sy - h| < 1, every candidate tested with the forward's own arithmetic -- in row-major
// order; then the adjoint of the range map with torch.clamp's mask (the gradient passes where -1 <= x <= 1).
__global__ __launch_bounds__(kThreads) void deca_front_bwd_kernel(const float* __restrict__ dcrop, const float* __restrict__ x,
                                                                  const float* __restrict__ mat, int B, int H, int W,
                                                                  float* __restrict__ dx) {
    const int64_t n = (int64_t)B * H * W;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int w = (int)(idx % W), h = (int)((idx / W) % H), b = (int)(idx / ((int64_t)H * W));
        const float* m = mat + 6 * b;
        int u0 = 0, u1 = kCrop - 1, v0 = 0, v1 = kCrop - 1;     // a singular matrix: every output pixel is a candidate
        const float det = m[0] * m[4] - m[1] * m[3];
        if (fabsf(det) > 1e-12f) {
            const float i00 = m[4] / det, i01 = -m[1] / det, i10 = -m[3] / det, i11 = m[0] / det;
            const float ds = (float)w - m[2], dt = (float)h - m[5];
            const float uc = i00 * ds + i01 * dt, vc = i10 * ds + i11 * dt;
            const float ru = fabsf(i00) + fabsf(i01) + 0.01f + 1e-5f * fabsf(uc), rv = fabsf(i10) + fabsf(i11) + 0.01f + 1e-5f * fabsf(vc);
            u0 = (int)floorf(fminf(fmaxf(uc - ru, 0.f), (float)kCrop));
            u1 = (int)ceilf(fminf(fmaxf(uc + ru, -1.f), (float)(kCrop - 1)));
            v0 = (int)floorf(fminf(fmaxf(vc - rv, 0.f), (float)kCrop));
            v1 = (int)ceilf(fminf(fmaxf(vc + rv, -1.f), (float)(kCrop - 1)));
        }
        float g[3] = {0.f, 0.f, 0.f};
        const float* dc = dcrop + (int64_t)b * 3 * kCropPlane;
        for (int v = v0; v <= v1; ++v)
            for (int u = u0; u <= u1; ++u) {
                double sx, sy;
                src_pos(m, u, v, sx, sy);
                if (!(sx > -1.0 && sx < (double)W && sy > -1.0 && sy < (double)H)) continue;
                const double fx0 = floor(sx), fy0 = floor(sy);
                const float fx = (float)(sx - fx0), fy = (float)(sy - fy0);
                const int x0 = (int)fx0, y0 = (int)fy0;
                float wx, wy;
                if (x0 == w) wx = 1.f - fx;
                else if (x0 + 1 == w) wx = fx;
                else continue;
                if (y0 == h) wy = 1.f - fy;
                else if (y0 + 1 == h) wy = fy;
                else continue;
                const float wgt = wx * wy;
                const int o = v * kCrop + u;
#pragma unroll
                for (int c = 0; c < 3; ++c) g[c] = fmaf(dc[c * kCropPlane + o], wgt, g[c]);
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t o = (((int64_t)b * 3 + c) * H + h) * W + w;
            const float t = x[o];
            dx[o] = (t >= -1.f && t <= 1.f) ? g[c] / 255.f * 255.f / 2.00001f : 0.f;
        }
    }
}

// ------------------------------------------------------------------ max-pool 3x3 / 2, pad 1 (112 -> 56) and its adjoint
// the first maximum in row-major order wins, as in torch; arg = kh*3 + kw of the winner
__global__ __launch_bounds__(kThreads) void deca_pool_kernel(const float* __restrict__ in, float* __restrict__ out, uint8_t* __restrict__ arg,
                                                             int64_t planes) {
    const int64_t n = planes * kPool * kPool;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(idx % kPool), i = (int)((idx / kPool) % kPool);
        const float* pl = in + (idx / (kPool * kPool)) * (kStem * kStem);
        float best = -INFINITY;
        int at = 0;
        bool any = false;
        for (int kh = 0; kh < 3; ++kh) {
            const int y = 2 * i - 1 + kh;
            if (y < 0 || y >= kStem) continue;
            for (int kw = 0; kw < 3; ++kw) {
                const int xx = 2 * j - 1 + kw;
                if (xx < 0 || xx >= kStem) continue;
                const float v = pl[y * kStem + xx];
                if (!any || v > best) best = v, at = kh * 3 + kw, any = true;
            }
        }
        out[idx] = best;
        if (arg) arg[idx] = (uint8_t)at;
    }
}

// gradient at the stem's pre-activation: the pooled windows that chose this pixel, in row-major order, times the stem's ReLU mask
__global__ __launch_bounds__(kThreads) void deca_pool_bwd_kernel(const float* __restrict__ dpool, const uint8_t* __restrict__ arg,
                                                                 const uint8_t* __restrict__ mask, float* __restrict__ dstem, int64_t planes) {
    const int64_t n = planes * kStem * kStem;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int xx = (int)(idx % kStem), y = (int)((idx / kStem) % kStem);
        const int64_t pl = idx / (kStem * kStem);
        float g = 0.f;
        if (mask[idx]) {
            const int i1 = min(kPool - 1, (y + 1) / 2), j1 = min(kPool - 1, (xx + 1) / 2);
            for (int i = y / 2; i <= i1; ++i)
                for (int j = xx / 2; j <= j1; ++j) {
                    const int64_t o = pl * (kPool * kPool) + i * kPool + j;
                    if (arg[o] == (y - (2 * i - 1)) * 3 + (xx - (2 * j - 1))) g += dpool[o];
                }
        }
        dstem[idx] = g;
    }
}

// stem adjoint: conv7x7/2 pad 3, 3 <- 64, as a gather per crop pixel (only the taps of the pixel's parity meet an output)
__global__ __launch_bounds__(kThreads) void deca_stem_bwd_kernel(const float* __restrict__ dstem, const float* __restrict__ w0,
                                                                 float* __restrict__ dcrop, int B) {
    const int64_t n = (int64_t)B * kCropPlane;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int xx = (int)(idx % kCrop), y = (int)((idx / kCrop) % kCrop), b = (int)(idx / kCropPlane);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        const float* d = dstem + (int64_t)b * 64 * kStem * kStem;
        for (int co = 0; co < 64; ++co)
            for (int kh = (y + 3) & 1; kh < 7; kh += 2) {
                const int oh = (y + 3 - kh) >> 1;
                if (y + 3 - kh < 0 || oh >= kStem) continue;
                for (int kw = (xx + 3) & 1; kw < 7; kw += 2) {
                    const int ow = (xx + 3 - kw) >> 1;
                    if (xx + 3 - kw < 0 || ow >= kStem) continue;
                    const float v = d[(co * kStem + oh) * kStem + ow];
                    const float* wp = w0 + co * 147 + kh * 7 + kw;
                    s0 = fmaf(wp[0], v, s0);
                    s1 = fmaf(wp[49], v, s1);
                    s2 = fmaf(wp[98], v, s2);
                }
            }
        const int64_t o = (int64_t)b * 3 * kCropPlane + y * kCrop + xx;
        dcrop[o] = s0;
        dcrop[o + kCropPlane] = s1;
        dcrop[o + 2 * kCropPlane] = s2;
    }
}

// ------------------------------------------------------------------ 7x7 average pool and its adjoint
__global__ __launch_bounds__(kThreads) void deca_avg_kernel(const float* __restrict__ in, float* __restrict__ feat, int64_t n) {
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const float* p = in + idx * 49;
        float s = 0.f;
        for (int i = 0; i < 49; ++i) s += p[i];
        feat[idx] = s / 49.f;
    }
}
// gradient at the last bottleneck's pre-activation sum
__global__ __launch_bounds__(kThreads) void deca_avg_bwd_kernel(const float* __restrict__ dfeat, const uint8_t* __restrict__ mask,
                                                                float* __restrict__ out, int64_t n) {
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads)
        out[idx] = mask[idx] ? dfeat[idx / 49] / 49.f : 0.f;
}

// ------------------------------------------------------------------ Euler angles in degrees of pose[:3] (parameters 200..202)
// rad2deg(batch_axis2euler): axis-angle -> quaternion -> rotation matrix -> (x, y, z).  Beyond |R20| > 0.998 the reference's
// first branch names an undefined bare atan2; both branches are taken as written otherwise (z = 0).
__global__ void deca_angles_kernel(const float* __restrict__ params, float* __restrict__ angles, int B) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B) return;
    const float* a = params + (int64_t)r * kOut + 200;
    const float a0 = a[0], a1 = a[1], a2 = a[2];
    const float t2 = a0 * a0 + a1 * a1 + a2 * a2, th = sqrtf(t2);
    const bool nz = t2 > 0.f;
    const float k = nz ? sinf(0.5f * th) / th : 0.5f;
    float w = nz ? cosf(0.5f * th) : 1.f, qx = a0 * k, qy = a1 * k, qz = a2 * k;
    const float nrm = sqrtf(w * w + qx * qx + qy * qy + qz * qz);
    w /= nrm, qx /= nrm, qy /= nrm, qz /= nrm;
    const float w2 = w * w, x2 = qx * qx, y2 = qy * qy, z2 = qz * qz;
    const float r00 = w2 + x2 - y2 - z2, r01 = 2.f * qx * qy - 2.f * w * qz, r02 = 2.f * w * qy + 2.f * qx * qz;
    const float r10 = 2.f * w * qz + 2.f * qx * qy;
    const float r20 = 2.f * qx * qz - 2.f * w * qy, r21 = 2.f * w * qx + 2.f * qy * qz, r22 = w2 - x2 - y2 + z2;
    float ex, ey, ez;
    const float half_pi = 1.57079632679489662f;
    if (r20 > 0.998f) {
        ez = 0.f, ex = half_pi, ey = atan2f(-r01, -r02);
    } else if (r20 < -0.998f) {
        ez = 0.f, ex = -half_pi, ey = atan2f(r01, r02);
    } else {
        ex = asinf(r20);
        const float c = cosf(ex);
        ey = atan2f(r21 / c, r22 / c);
        ez = atan2f(r10 / c, r00 / c);
    }
    const float pi = 3.14159265358979323846f;
    angles[3 * r + 0] = 180.f * ex / pi;
    angles[3 * r + 1] = 180.f * ey / pi;
    angles[3 * r + 2] = 180.f * ez / pi;
}

// ------------------------------------------------------------------ host side
static int launch_conv(const ConvArgs& a0, int tap, int ks, bool ext, float* part, hipStream_t st) {
    ConvArgs a = a0;
    // The number of K slices follows the output tiles, i.e. the layer and the row count, nothing else.
    const int M = a.R * a.Ho * a.Wo;
    const ConvPlan p = plan_conv(M, a.N, a.K, BN, conv_tiles(M, a.N, BN));
    SGDFR_REQUIRE(p.S == 1 || p.S * p.out_elems <= kPartElems, "deca: split-K partials of %lld floats exceed the workspace",
                  (long long)(p.S * p.out_elems));
    a.cps = p.cps;
    a.part = part;
    a.part_elems = p.out_elems;
    const dim3 grid(p.mt, p.nt, p.S);
    bool done = false;
#define SGDFR_DECA_CONV(T_, KS_, EXT_)                                                    \
    if (!done && tap == T_ && ks == KS_ && ext == EXT_) {                                  \
        hipLaunchKernelGGL((deca_conv_kernel<T_, KS_, EXT_>), grid, dim3(kThreads), 0, st, a); \
        done = true;                                                                       \
    }
    SGDFR_DECA_CONV(TAP_FWD, 7, false)     // stem
    SGDFR_DECA_CONV(TAP_FWD, 1, false)     // conv1, conv3, projection, the head GEMMs, every 1x1 input gradient
    SGDFR_DECA_CONV(TAP_FWD, 3, false)     // conv2
    SGDFR_DECA_CONV(TAP_FWD, 1, true)      // conv1 + projection input gradient
    SGDFR_DECA_CONV(TAP_DGRAD, 3, false)   // conv2 input gradient
#undef SGDFR_DECA_CONV
    SGDFR_REQUIRE(done, "deca: no conv instance for tap=%d k=%d ext=%d", tap, ks, (int)ext);
    if (check_launch("deca conv")) return 2;
    if (p.S > 1) {
        hipLaunchKernelGGL(deca_finish_kernel, dim3(grid_1d(p.out_elems)), dim3(kThreads), 0, st, a, p.S);
        if (check_launch("deca finish")) return 2;
    }
    return 0;
}

// saved bytes per row: the stem's ReLU mask, the max-pool choices, per bottleneck the three ReLU masks, the regressor's mask
struct SavedLayout {
    int64_t stem, arg, m1[kBlocks], m2[kBlocks], m3[kBlocks], fc, total;
};
static SavedLayout saved_layout(int rows) {
    Block bs[kBlocks];
    make_blocks(bs);
    SavedLayout s;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    s.stem = take((int64_t)rows * 64 * kStem * kStem);
    s.arg = take((int64_t)rows * 64 * kPool * kPool);
    for (int i = 0; i < kBlocks; ++i) {
        const Block& u = bs[i];
        s.m1[i] = take((int64_t)rows * u.p * u.h * u.h);
        s.m2[i] = take((int64_t)rows * u.p * u.ho * u.ho);
        s.m3[i] = take((int64_t)rows * 4 * u.p * u.ho * u.ho);
    }
    s.fc = take((int64_t)rows * kHidden);
    s.total = o;
    return s;
}

constexpr int64_t kMaxAct = 64LL * kStem * kStem;   // largest activation per row (stem output = layer1's outputs)
struct WsLayout {
    int64_t part, crop, act[5], feat, hid, total;   // float offsets
};
static WsLayout ws_layout(int rows) {
    WsLayout w;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    w.part = take(kPartElems);
    w.crop = take((int64_t)rows * 3 * kCropPlane);
    for (int i = 0; i < 5; ++i) w.act[i] = take((int64_t)rows * kMaxAct);
    w.feat = take((int64_t)rows * kFeat);
    w.hid = take((int64_t)rows * kHidden);
    w.total = o;
    return w;
}

// debug stage outputs, each [rows, ...]: stem, pool, per stage the first and the last bottleneck's output, pooled features
struct DebugLayout {
    int64_t stem, pool, first[4], last[4], feat, total;
};
static DebugLayout debug_layout(int rows) {
    DebugLayout d;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o += n; return r; };
    d.stem = take((int64_t)rows * 64 * kStem * kStem);
    d.pool = take((int64_t)rows * 64 * kPool * kPool);
    int h = kPool;
    for (int s = 0; s < 4; ++s) {
        if (s) h /= 2;
        const int64_t n = (int64_t)rows * (256 << s) * h * h;
        d.first[s] = take(n), d.last[s] = take(n);
    }
    d.feat = take((int64_t)rows * kFeat);
    d.total = o;
    return d;
}

static bool size_ok(int rows, int H, int W) { return rows >= 1 && rows <= kMaxRows && H >= 1 && W >= 1 && H <= 8192 && W <= 8192; }

static ConvArgs conv_args(const float* src, int Hs, const float* wp, int K, int N, int Ho, int stride, int pad, int epi, float* out, int R) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src, a.wp = wp, a.out = out;
    a.R = R, a.Hs = a.Ws = Hs, a.N = N, a.Ho = a.Wo = Ho, a.K = a.K1 = K, a.stride = stride, a.pad = pad, a.epi = epi, a.es = 1;
    return a;
}

}  // namespace
}  // namespace sgdfr

using namespace sgdfr;

extern "C" int64_t sgdfr_deca_pack_elems(void) { return pack_layout().total; }

extern "C" int64_t sgdfr_deca_saved_elems(int rows) {
    if (rows < 1 || rows > kMaxRows) return -1;
    return saved_layout(rows).total;
}

extern "C" int64_t sgdfr_deca_debug_elems(int rows) {
    if (rows < 1 || rows > kMaxRows) return -1;
    return debug_layout(rows).total;
}

extern "C" int64_t sgdfr_deca_workspace_bytes(int rows, int H, int W) {
    if (!size_ok(rows, H, W)) return -1;
    return ws_layout(rows).total * (int64_t)sizeof(float);
}

extern "C" int sgdfr_deca_prepack_f32(const float* const* params, float* pack, void* stream) {
    SGDFR_REQUIRE(params && pack, "deca_prepack: null pointer");
    Block bs[kBlocks];
    make_blocks(bs);
    for (int i = 0; i < kParams; ++i) {
        const int u = (i - 2) / 8, j = (i - 2) % 8;
        const bool optional = i >= 2 && i < 2 + 8 * kBlocks && j >= 6 && !bs[u].ds;   // projection of an identity block
        SGDFR_REQUIRE(optional || params[i], "deca_prepack: parameter %d is null", i);
    }
    const PackLayout pl = pack_layout();
    hipStream_t st = as_stream(stream);
    auto seg = [&](const float* src, int64_t dst, int64_t count, int kind, int cin, int cout, int kk) {
        hipLaunchKernelGGL(deca_pack_kernel, dim3(grid_1d(count)), dim3(kThreads), 0, st, src, pack + dst, count, kind, cin, cout, kk);
        return check_launch("deca prepack");
    };
    int rc = 0;
    rc |= seg(params[0], pl.wf0, 147 * 64, SEG_FWD, 3, 64, 49);
    rc |= seg(params[0], pl.w0, 147 * 64, SEG_COPY, 0, 0, 0);
    rc |= seg(params[1], pl.b0, 64, SEG_COPY, 0, 0, 0);
    for (int i = 0; i < kBlocks && !rc; ++i) {
        const Block& u = bs[i];
        const BlockPack& q = pl.u[i];
        const float* const* P = params + 2 + 8 * i;   // w1, b1, w2, b2, w3, b3, wd, bd
        const int c4 = 4 * u.p;
        const int64_t n1 = (int64_t)u.cin * u.p, n2 = 9LL * u.p * u.p, n3 = (int64_t)u.p * c4, nd = (int64_t)u.cin * c4;
        rc |= seg(P[0], q.wf1, n1, SEG_FWD, u.cin, u.p, 1);
        rc |= seg(P[0], q.wdx, n1, SEG_COPY, 0, 0, 0);
        rc |= seg(P[1], q.b1, u.p, SEG_COPY, 0, 0, 0);
        rc |= seg(P[2], q.wf2, n2, SEG_FWD, u.p, u.p, 9);
        rc |= seg(P[2], q.wd2, n2, SEG_DGRAD, u.p, u.p, 9);
        rc |= seg(P[3], q.b2, u.p, SEG_COPY, 0, 0, 0);
        rc |= seg(P[4], q.wf3, n3, SEG_FWD, u.p, c4, 1);
        rc |= seg(P[4], q.wd3, n3, SEG_COPY, 0, 0, 0);
        rc |= seg(P[5], q.b3, c4, SEG_COPY, 0, 0, 0);
        if (u.ds) {
            rc |= seg(P[6], q.wfd, nd, SEG_FWD, u.cin, c4, 1);
            rc |= seg(P[6], q.wdx + n1, nd, SEG_COPY, 0, 0, 0);   // extra K rows of conv1's input gradient
            rc |= seg(P[7], q.bd, c4, SEG_COPY, 0, 0, 0);
        }
    }
    const float* const* Hd = params + 2 + 8 * kBlocks;
    if (!rc) rc |= seg(Hd[0], pl.wf_fc1, (int64_t)kFeat * kHidden, SEG_FWD, kFeat, kHidden, 1);
    if (!rc) rc |= seg(Hd[0], pl.wd_fc1, (int64_t)kFeat * kHidden, SEG_COPY, 0, 0, 0);
    if (!rc) rc |= seg(Hd[1], pl.b_fc1, kHidden, SEG_COPY, 0, 0, 0);
    if (!rc) rc |= seg(Hd[2], pl.wf_fc2, (int64_t)kHidden * kOut, SEG_FWD, kHidden, kOut, 1);
    if (!rc) rc |= seg(Hd[2], pl.wd_fc2, (int64_t)kHidden * kOut, SEG_COPY, 0, 0, 0);
    if (!rc) rc |= seg(Hd[3], pl.b_fc2, kOut, SEG_COPY, 0, 0, 0);
    return rc ? 2 : 0;
}

extern "C" int sgdfr_deca_crop_f32(const float* x, const float* mat, int rows, int H, int W, float* crop, void* stream) {
    SGDFR_REQUIRE(size_ok(rows, H, W), "deca_crop: unsupported size (%d rows of %dx%d)", rows, H, W);
    SGDFR_REQUIRE(x && mat && crop, "deca_crop: null pointer");
    hipLaunchKernelGGL(deca_front_kernel, dim3(grid_1d((int64_t)rows * 3 * kCropPlane)), dim3(kThreads), 0, as_stream(stream), x, mat, rows,
                       H, W, crop);
    return check_launch("deca crop");
}

extern "C" int sgdfr_deca_crop_backward_f32(const float* grad_crop, const float* x, const float* mat, int rows, int H, int W, float* dx,
                                            void* stream) {
    SGDFR_REQUIRE(size_ok(rows, H, W), "deca_crop_backward: unsupported size (%d rows of %dx%d)", rows, H, W);
    SGDFR_REQUIRE(grad_crop && x && mat && dx, "deca_crop_backward: null pointer");
    hipLaunchKernelGGL(deca_front_bwd_kernel, dim3(grid_1d((int64_t)rows * H * W)), dim3(kThreads), 0, as_stream(stream), grad_crop, x, mat,
                       rows, H, W, dx);
    return check_launch("deca crop backward");
}

extern "C" int sgdfr_deca_forward_f32(const float* x, const float* mat, int rows, int H, int W, const float* pack, float* crop,
                                      float* params, float* angles, uint8_t* saved, float* debug, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(size_ok(rows, H, W), "deca_forward: unsupported size (%d rows of %dx%d)", rows, H, W);
    SGDFR_REQUIRE(x && mat && pack && crop && params && angles && workspace, "deca_forward: null pointer");
    const int R = rows;
    const WsLayout wl = ws_layout(R);
    SGDFR_REQUIRE(wl.total * (int64_t)sizeof(float) <= workspace_bytes, "deca_forward: workspace of %lld bytes, %d rows need %lld",
                  (long long)workspace_bytes, R, (long long)(wl.total * (int64_t)sizeof(float)));
    Block bs[kBlocks];
    make_blocks(bs);
    const PackLayout pl = pack_layout();
    const SavedLayout sl = saved_layout(R);
    const DebugLayout dl = debug_layout(R);
    float* wsf = reinterpret_cast<float*>(workspace);
    float* part = wsf + wl.part;
    hipStream_t st = as_stream(stream);
    auto mask = [&](int64_t off) { return saved ? saved + off : nullptr; };
    auto dump = [&](int64_t off, const float* src, int64_t n) {
        if (!debug) return 0;
        if (hipMemcpyAsync(debug + off, src, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
            set_error("deca_forward: debug copy failed");
            return 2;
        }
        return 0;
    };

    hipLaunchKernelGGL(deca_front_kernel, dim3(grid_1d((int64_t)R * 3 * kCropPlane)), dim3(kThreads), 0, st, x, mat, R, H, W, crop);
    if (check_launch("deca front")) return 2;

    float* A[5];
    for (int i = 0; i < 5; ++i) A[i] = wsf + wl.act[i];
    ConvArgs a = conv_args(crop, kCrop, pack + pl.wf0, 147, 64, kStem, 2, 3, EP_BIAS_RELU, A[0], R);
    a.bias = pack + pl.b0, a.mask_out = mask(sl.stem);
    if (launch_conv(a, TAP_FWD, 7, false, part, st)) return 2;
    if (dump(dl.stem, A[0], (int64_t)R * 64 * kStem * kStem)) return 2;
    hipLaunchKernelGGL(deca_pool_kernel, dim3(grid_1d((int64_t)R * 64 * kPool * kPool)), dim3(kThreads), 0, st, A[0], A[1], mask(sl.arg),
                       (int64_t)R * 64);
    if (check_launch("deca pool")) return 2;
    if (dump(dl.pool, A[1], (int64_t)R * 64 * kPool * kPool)) return 2;

    int cur = 1, stage = -1;
    for (int i = 0; i < kBlocks; ++i) {
        const Block& u = bs[i];
        const BlockPack& q = pl.u[i];
        const int c4 = 4 * u.p;
        float* in = A[cur];
        float* out = A[cur ^ 1];
        float *t1 = A[2], *t2 = A[3], *res = A[4];
        a = conv_args(in, u.h, pack + q.wf1, u.cin, u.p, u.h, 1, 0, EP_BIAS_RELU, t1, R);
        a.bias = pack + q.b1, a.mask_out = mask(sl.m1[i]);
        if (launch_conv(a, TAP_FWD, 1, false, part, st)) return 2;
        a = conv_args(t1, u.h, pack + q.wf2, 9 * u.p, u.p, u.ho, u.stride, 1, EP_BIAS_RELU, t2, R);
        a.bias = pack + q.b2, a.mask_out = mask(sl.m2[i]);
        if (launch_conv(a, TAP_FWD, 3, false, part, st)) return 2;
        if (u.ds) {
            a = conv_args(in, u.h, pack + q.wfd, u.cin, c4, u.ho, u.stride, 0, EP_BIAS, res, R);
            a.bias = pack + q.bd;
            if (launch_conv(a, TAP_FWD, 1, false, part, st)) return 2;
        }
        a = conv_args(t2, u.ho, pack + q.wf3, u.p, c4, u.ho, 1, 0, EP_BIAS_ADD_RELU, out, R);
        a.bias = pack + q.b3, a.aux = u.ds ? res : in, a.mask_out = mask(sl.m3[i]);
        if (launch_conv(a, TAP_FWD, 1, false, part, st)) return 2;
        cur ^= 1;
        const int64_t n = (int64_t)R * c4 * u.ho * u.ho;
        if (u.ds) {
            ++stage;
            if (dump(dl.first[stage], out, n)) return 2;
        }
        if (i + 1 == kBlocks || bs[i + 1].ds)
            if (dump(dl.last[stage], out, n)) return 2;
    }

    float* feat = wsf + wl.feat;
    float* hid = wsf + wl.hid;
    hipLaunchKernelGGL(deca_avg_kernel, dim3(grid_1d((int64_t)R * kFeat)), dim3(kThreads), 0, st, A[cur], feat, (int64_t)R * kFeat);
    if (check_launch("deca average pool")) return 2;
    if (dump(dl.feat, feat, (int64_t)R * kFeat)) return 2;
    a = conv_args(feat, 1, pack + pl.wf_fc1, kFeat, kHidden, 1, 1, 0, EP_BIAS_RELU, hid, R);
    a.bias = pack + pl.b_fc1, a.mask_out = mask(sl.fc);
    if (launch_conv(a, TAP_FWD, 1, false, part, st)) return 2;
    a = conv_args(hid, 1, pack + pl.wf_fc2, kHidden, kOut, 1, 1, 0, EP_BIAS, params, R);
    a.bias = pack + pl.b_fc2;
    if (launch_conv(a, TAP_FWD, 1, false, part, st)) return 2;
    hipLaunchKernelGGL(deca_angles_kernel, dim3((R + 63) / 64), dim3(64), 0, st, params, angles, R);
    return check_launch("deca angles");
}

extern "C" int sgdfr_deca_backward_f32(const float* grad_params, const float* x, const float* mat, const uint8_t* saved, int rows, int H,
                                       int W, const float* pack, float* dx, void* workspace, int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(size_ok(rows, H, W), "deca_backward: unsupported size (%d rows of %dx%d)", rows, H, W);
    SGDFR_REQUIRE(grad_params && x && mat && saved && pack && dx && workspace, "deca_backward: null pointer");
    const int R = rows;
    const WsLayout wl = ws_layout(R);
    SGDFR_REQUIRE(wl.total * (int64_t)sizeof(float) <= workspace_bytes, "deca_backward: workspace of %lld bytes, %d rows need %lld",
                  (long long)workspace_bytes, R, (long long)(wl.total * (int64_t)sizeof(float)));
    Block bs[kBlocks];
    make_blocks(bs);
    const PackLayout pl = pack_layout();
    const SavedLayout sl = saved_layout(R);
    float* wsf = reinterpret_cast<float*>(workspace);
    float* part = wsf + wl.part;
    hipStream_t st = as_stream(stream);
    float* A[5];
    for (int i = 0; i < 5; ++i) A[i] = wsf + wl.act[i];

    // regressor: dh = W2^T g [h > 0]; dfeat = W1^T dh
    float* hid = wsf + wl.hid;
    float* feat = wsf + wl.feat;
    ConvArgs a = conv_args(grad_params, 1, pack + pl.wd_fc2, kOut, kHidden, 1, 1, 0, EP_MASK, hid, R);
    a.mask_in = saved + sl.fc;
    if (launch_conv(a, TAP_FWD, 1, false, part, st)) return 2;
    a = conv_args(hid, 1, pack + pl.wd_fc1, kHidden, kFeat, 1, 1, 0, EP_RAW, feat, R);
    if (launch_conv(a, TAP_FWD, 1, false, part, st)) return 2;
    int cur = 0;
    hipLaunchKernelGGL(deca_avg_bwd_kernel, dim3(grid_1d((int64_t)R * kFeat * 49)), dim3(kThreads), 0, st, feat, saved + sl.m3[kBlocks - 1],
                       A[cur], (int64_t)R * kFeat * 49);
    if (check_launch("deca average pool backward")) return 2;

    // per bottleneck, G = the gradient at the pre-activation of the block's output (already masked by its ReLU)
    for (int i = kBlocks - 1; i >= 0; --i) {
        const Block& u = bs[i];
        const BlockPack& q = pl.u[i];
        const int c4 = 4 * u.p;
        const float* G = A[cur];
        float *t1 = A[2], *t2 = A[3];
        a = conv_args(G, u.ho, pack + q.wd3, c4, u.p, u.ho, 1, 0, EP_MASK, t2, R);
        a.mask_in = saved + sl.m2[i];
        if (launch_conv(a, TAP_FWD, 1, false, part, st)) return 2;
        a = conv_args(t2, u.ho, pack + q.wd2, 9 * u.p, u.p, u.h, u.stride, 1, EP_MASK, t1, R);
        a.mask_in = saved + sl.m1[i];
        if (launch_conv(a, TAP_DGRAD, 3, false, part, st)) return 2;
        // dx_block = conv1^T dt1 + the shortcut's adjoint, masked by the previous block's ReLU (the pooled input has none)
        a = conv_args(t1, u.h, pack + q.wdx, u.p, u.cin, u.h, 1, 0, u.ds ? EP_MASK : EP_ADD_MASK, A[cur ^ 1], R);
        a.mask_in = i > 0 ? saved + sl.m3[i - 1] : nullptr;
        if (u.ds) {
            a.K = u.p + c4, a.ext = G, a.He = a.We = u.ho, a.es = u.stride;
        } else {
            a.aux = G;
        }
        if (launch_conv(a, TAP_FWD, 1, u.ds, part, st)) return 2;
        cur ^= 1;
    }

    float* dstem = A[cur ^ 1];
    hipLaunchKernelGGL(deca_pool_bwd_kernel, dim3(grid_1d((int64_t)R * 64 * kStem * kStem)), dim3(kThreads), 0, st, A[cur], saved + sl.arg,
                       saved + sl.stem, dstem, (int64_t)R * 64);
    if (check_launch("deca pool backward")) return 2;
    float* dcrop = wsf + wl.crop;
    hipLaunchKernelGGL(deca_stem_bwd_kernel, dim3(grid_1d((int64_t)R * kCropPlane)), dim3(kThreads), 0, st, dstem, pack + pl.w0, dcrop, R);
    if (check_launch("deca stem backward")) return 2;
    hipLaunchKernelGGL(deca_front_bwd_kernel, dim3(grid_1d((int64_t)R * H * W)), dim3(kThreads), 0, st, dcrop, x, mat, R, H, W, dx);
    return check_launch("deca front backward");
}
