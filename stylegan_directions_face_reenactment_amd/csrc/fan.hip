// The 2D-FAN-4 landmark detector in eval mode (libs/face_models/fan_model/models.py:145-202 FAN(4), landmarks_estimation.py:50-88 and
// :143-185, fan_model/utils.py:63-97 and :140-165): image + face box -> integer window, zero padding, bilinear resize to 256x256, / 255
// -> stem conv7x7/2 + BN + ReLU -> ConvBlock 64->128, average pool, ConvBlock 128->128, ConvBlock 128->256 -> four stacks of
// (hourglass of depth 4, ConvBlock, conv1x1 + BN + ReLU, conv1x1 -> 68 heatmaps of 64x64, and between stacks previous + bl + al)
// -> per heatmap the first maximum, the quarter-pixel step, the crop-pixel and the image-pixel coordinates -> the 'kpt68' box.
// Forward only: nothing is kept for a backward.
//
// Every one of the 194 convs is one implicit-GEMM kernel on exact-f32 MFMA (v_mfma_f32_16x16x4_f32), the 64 x 64 x 16 tile of
// deca.hip with its split over K and fixed-order finish.  What this network adds lies in the loader and the epilogue:
//   * ConvBlock is BN -> ReLU -> conv3x3 three times, so its BatchNorms cannot be folded into filters.  The loader applies
//     max(0, x g[c] + h[c]) to every tap INSIDE the map; a tap outside loads 0 (the conv pads behind the activation).
//   * the block's output cat(out1, out2, out3) + residual is written by the three convs themselves: each adds the residual's slice and
//     stores at its channel offset of the block output, and conv1 / conv2 also store the raw value for the conv that follows.
//   * up1 + nearest_upsample(low3) of an hourglass level rides in the same epilogue (b1 runs after the lower branch).
//   * previous + bl(ll) + al(heatmaps) is one launch: al's 68 channels are concatenated behind bl's 256 in K.
// avg_pool2d(2) is a bandwidth kernel of its own: its output is read four times (conv1's loader and three residual slices).
// No float atomics, no host synchronisation, everything on the given stream.
#include <string.h>

#include <algorithm>

#include "conv_tile.h"

namespace sgdfr {
namespace {

constexpr int kStacks = 4, kDepth = 4;
constexpr int kIn = 256, kInPlane = kIn * kIn;       // the network's input crop
constexpr int kStem = 128, kMap = 64, kMapPlane = kMap * kMap;
constexpr int kFeat = 256, kPts = 68;
constexpr int kHgBlocks = 3 * kDepth + 1;            // b1, b2, b3 per level, b2_plus of the last
constexpr int kStackBlocks = kHgBlocks + 1;          // + top_m
constexpr int kBlocks = 3 + kStacks * kStackBlocks;  // conv2, conv3, conv4 in front
constexpr int kBlockParams = 12;                     // g1 h1 w1 g2 h2 w2 g3 h3 w3 gd hd wd
constexpr int kParams = 2 + kBlocks * kBlockParams + 4 * kStacks + 3 * (kStacks - 1);
constexpr int kMaxRows = 256;
constexpr int BN = 64;
// split K only below 512 output tiles, at most 512 / tiles slices: S * (output elements) <= 512 tiles
constexpr int64_t kPartElems = 512LL * BM * BN;

// ------------------------------------------------------------------ network geometry
struct Block {
    int cin, cout;
};
static Block block_of(int i) {
    if (i == 0) return {64, 128};
    if (i == 1) return {128, 128};
    if (i == 2) return {128, 256};
    return {kFeat, kFeat};
}
static int hg_block(int stack, int level, int which) { return 3 + stack * kStackBlocks + (kDepth - level) * 3 + which; }   // which: b1 b2 b3
static int hg_plus(int stack) { return 3 + stack * kStackBlocks + 3 * kDepth; }
static int top_block(int stack) { return 3 + stack * kStackBlocks + kHgBlocks; }

// ------------------------------------------------------------------ weight pack
struct BlockPack {
    int64_t g[3], h[3], w[3], gd, hd, wd;
};
struct PackLayout {
    int64_t w0, b0;
    BlockPack u[kBlocks];
    int64_t w_last[kStacks], b_last[kStacks], w_l[kStacks], b_l[kStacks], w_mix[kStacks - 1], b_mix[kStacks - 1], total;
};
static PackLayout pack_layout() {
    PackLayout p;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    p.w0 = take(147 * 64), p.b0 = take(64);
    for (int i = 0; i < kBlocks; ++i) {
        const Block u = block_of(i);
        BlockPack& q = p.u[i];
        const int ci[3] = {u.cin, u.cout / 2, u.cout / 4}, co[3] = {u.cout / 2, u.cout / 4, u.cout / 4};
        for (int j = 0; j < 3; ++j) q.g[j] = take(ci[j]), q.h[j] = take(ci[j]), q.w[j] = take(9LL * ci[j] * co[j]);
        const bool ds = u.cin != u.cout;
        q.gd = ds ? take(u.cin) : -1, q.hd = ds ? take(u.cin) : -1, q.wd = ds ? take((int64_t)u.cin * u.cout) : -1;
    }
    for (int s = 0; s < kStacks; ++s) {
        p.w_last[s] = take(kFeat * kFeat), p.b_last[s] = take(kFeat);
        p.w_l[s] = take(kFeat * kPts), p.b_l[s] = take(kPts);
    }
    for (int s = 0; s + 1 < kStacks; ++s) p.w_mix[s] = take((kFeat + kPts) * kFeat), p.b_mix[s] = take(kFeat);
    p.total = o;
    return p;
}

// copy: dst[j] = src[j].  Else [k = ci*kk + r][co] <- W[co][ci][r]
__global__ __launch_bounds__(kThreads) void fan_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t count,
                                                            int copy, int cin, int cout, int kk) {
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

// ------------------------------------------------------------------ implicit-GEMM conv
// every tensor is dense [R, C, H, W]
struct ConvArgs {
    const float* src;        // [R, Cs, Hs, Ws], Cs = K1 / (KS*KS)
    const float* ext;        // EXT, k >= K1: a second operand [R, K - K1, Ho, Wo] read at the output pixel
    const float* wp;         // [K][N]
    const float* pre_g;      // loader: max(0, x * pre_g[ci] + pre_h[ci]) on every tap inside the map (NULL: the plain value)
    const float* pre_h;
    const float* bias;       // epilogue: + bias[n] (NULL: none), then ReLU if `relu`
    float* raw;              // the value so far, dense [R, N, Ho, Wo], for the conv that follows (NULL: not kept)
    const float* res;        // + res at the output's own index (NULL: none)
    const float* up;         // + up [R, outC, Ho/2, Wo/2] at (oh/2, ow/2), channel c0 + n (NULL: none)
    float* out;              // [R, outC, Ho, Wo], this conv's channels at c0 .. c0 + N
    float* part;             // split K: [S][R*N*Ho*Wo]
    int64_t part_elems;
    int R, Hs, Ws, N, Ho, Wo, K, K1, stride, pad, cps, relu, outC, c0;
};

__device__ __forceinline__ void epilogue(const ConvArgs& a, int b, int n, int p, float v) {
    const int HWo = a.Ho * a.Wo;
    if (a.bias) v += a.bias[n];
    if (a.relu) v = fmaxf(v, 0.f);
    if (a.raw) a.raw[((int64_t)b * a.N + n) * HWo + p] = v;
    const int64_t ch = (int64_t)b * a.outC + a.c0 + n, o = ch * HWo + p;
    if (a.res) v += a.res[o];
    if (a.up) {
        const int oh = p / a.Wo, ow = p - oh * a.Wo;
        v += a.up[(ch * (a.Ho >> 1) + (oh >> 1)) * (a.Wo >> 1) + (ow >> 1)];
    }
    a.out[o] = v;
}

template <int KS, bool EXT>
__global__ __launch_bounds__(kThreads) void fan_conv_kernel(ConvArgs a) {
    __shared__ ConvLds<BN> lds;
    const int t = threadIdx.x, wv = t >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int HWo = a.Ho * a.Wo, M = a.R * HWo;
    const int plane = a.Hs * a.Ws;

    // the pixel this thread gathers (fixed over K)
    const int gm = m0 + (t & (BM - 1));
    const bool mvalid = gm < M;
    int b = 0, oh = 0, ow = 0, pix = 0;
    if (mvalid) {
        b = gm / HWo;
        pix = gm - b * HWo;
        oh = pix / a.Wo;
        ow = pix - oh * a.Wo;
    }
    const float* srcb = a.src + (int64_t)b * (a.K1 / (KS * KS)) * plane;
    const float* extb = EXT ? a.ext + (int64_t)b * (a.K - a.K1) * HWo : nullptr;
    const bool pre = a.pre_g != nullptr;

    const int nchunks = (a.K + BK - 1) / BK;
    const int c0 = blockIdx.z * a.cps, c1 = min(nchunks, c0 + a.cps);
    float xr[4], wr[4];
    auto gload = [&](int c) {
        const int k0 = c * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + wv + 4 * i;      // uniform over the wave: the channel's g, h are scalar loads
            float v = 0.f;
            if (k < a.K) {
                if (EXT && k >= a.K1) {
                    if (mvalid) v = extb[(int64_t)(k - a.K1) * HWo + pix];
                } else {
                    const int ci = k / (KS * KS), r = k - ci * (KS * KS), kh = r / KS, kw = r - kh * KS;
                    const int ih = oh * a.stride - a.pad + kh, iw = ow * a.stride - a.pad + kw;
                    if (mvalid && ih >= 0 && ih < a.Hs && iw >= 0 && iw < a.Ws) {
                        v = srcb[ci * plane + ih * a.Ws + iw];
                        if (pre) v = fmaxf(fmaf(v, a.pre_g[ci], a.pre_h[ci]), 0.f);
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
__global__ __launch_bounds__(kThreads) void fan_finish_kernel(ConvArgs a, int S) {
    finish_slices(a.part, a.part_elems, S, a.N, a.Ho * a.Wo, [=](int b, int n, int p, float v) { epilogue(a, b, n, p, v); });
}

// ------------------------------------------------------------------ avg_pool2d(2): [planes, 2h, 2w] -> [planes, h, w]
__global__ __launch_bounds__(kThreads) void fan_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t planes, int h, int w) {
    const int64_t n = planes * h * w;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(idx % w), i = (int)((idx / w) % h);
        const float* p = in + (idx / ((int64_t)h * w)) * (4LL * h * w) + (2 * i) * (2 * w) + 2 * j;
        out[idx] = (((p[0] + p[1]) + p[2 * w]) + p[2 * w + 1]) * 0.25f;
    }
}

// ------------------------------------------------------------------ centre, scale and transform(..., invert=True)
// landmarks_estimation.py:145-150 in float32, every operation rounded on its own (no contraction into an fma)
struct Face {
    float cx, cy, scale;
};
__device__ __forceinline__ Face face_of(const float* f) {
    Face r;
    r.cx = __fdiv_rn(__fadd_rn(f[2], f[0]), 2.0f);
    r.cy = __fsub_rn(__fdiv_rn(__fadd_rn(f[3], f[1]), 2.0f), __fmul_rn(__fsub_rn(f[3], f[1]), 0.12f));
    r.scale = __fdiv_rn(__fsub_rn(__fadd_rn(__fsub_rn(f[2], f[0]), f[3]), f[1]), 195.0f);
    return r;
}
// fan_model/utils.py:63-97 with invert=True: t = [[a, 0, tx], [0, a, ty], [0, 0, 1]], a = res / (200 scale), tx = res (-cx / h + 0.5);
// the inverse in closed form (the reference inverts numerically), then .int(): truncation toward zero
__device__ __forceinline__ void inv_transform(const Face& f, float px, float py, float res, int& x, int& y) {
    const float h = __fmul_rn(200.0f, f.scale), a = __fdiv_rn(res, h);
    const float tx = __fmul_rn(res, __fadd_rn(__fdiv_rn(-f.cx, h), 0.5f)), ty = __fmul_rn(res, __fadd_rn(__fdiv_rn(-f.cy, h), 0.5f));
    const float ia = __fdiv_rn(1.0f, a);
    const float fx = __fadd_rn(__fmul_rn(ia, px), __fmul_rn(-tx, ia)), fy = __fadd_rn(__fmul_rn(ia, py), __fmul_rn(-ty, ia));
    // a degenerate box (scale 0, NaN) gives no window instead of an undefined conversion
    x = (fx > -1e9f && fx < 1e9f) ? (int)fx : 0;
    y = (fy > -1e9f && fy < 1e9f) ? (int)fy : 0;
}

__device__ __forceinline__ float to_255(float t) {
    return (fminf(fmaxf(t, -1.f), 1.f) + 1.f) / 2.00001f * 255.f;
}

// ------------------------------------------------------------------ front: window, zero padding, bilinear resize to 256x256, / 255
// crop_torch (fan_model/utils.py:140-165): the window [l1, l2) of the image with zeros outside the image, resized as
// F.interpolate(mode='bilinear', align_corners=False) does, without antialiasing
__global__ __launch_bounds__(kThreads) void fan_front_kernel(const float* __restrict__ x, const float* __restrict__ faces, int B, int H, int W,
                                                             int gan, float* __restrict__ out) {
    const int64_t n = (int64_t)B * 3 * kInPlane;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int u = (int)(idx % kIn), v = (int)((idx / kIn) % kIn);
        const int bc = (int)(idx / kInPlane), b = bc / 3;
        const Face f = face_of(faces + 4 * b);
        int l1x, l1y, l2x, l2y;
        inv_transform(f, 1.f, 1.f, 256.f, l1x, l1y);
        inv_transform(f, 256.f, 256.f, 256.f, l2x, l2y);
        const int ww = l2x - l1x, wh = l2y - l1y;
        float r = 0.f;
        if (ww > 0 && wh > 0 && ww <= (1 << 20) && wh <= (1 << 20)) {
            const float sx = fmaxf(__fsub_rn(__fmul_rn((float)ww / 256.f, (float)u + 0.5f), 0.5f), 0.f);
            const float sy = fmaxf(__fsub_rn(__fmul_rn((float)wh / 256.f, (float)v + 0.5f), 0.5f), 0.f);
            const int x0 = min((int)sx, ww - 1), y0 = min((int)sy, wh - 1);
            const int x1 = x0 + (x0 < ww - 1 ? 1 : 0), y1 = y0 + (y0 < wh - 1 ? 1 : 0);
            const float lx = sx - (float)x0, ly = sy - (float)y0;
            const float* pl = x + (int64_t)bc * H * W;
            auto tap = [&](int wy, int wx) {
                const int iy = wy + l1y, ix = wx + l1x;
                if (iy < 0 || iy >= H || ix < 0 || ix >= W) return 0.f;
                const float t = pl[(int64_t)iy * W + ix];
                return gan ? to_255(t) : t;
            };
            const float v00 = tap(y0, x0), v01 = tap(y0, x1), v10 = tap(y1, x0), v11 = tap(y1, x1);
            r = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
        }
        out[idx] = r / 255.f;
    }
}

// ------------------------------------------------------------------ decode: one block per heatmap
// landmarks_estimation.py:50-88: the first maximum in row-major order, +-0.25 by the sign of the neighbour differences for an interior
// maximum, - 0.5; pts = preds * 4 (crop pixels), pts_img = transform(preds, centre, scale, 64, invert=True).int() (image pixels)
__global__ __launch_bounds__(kThreads) void fan_decode_kernel(const float* __restrict__ hm, const float* __restrict__ faces,
                                                              float* __restrict__ pts, float* __restrict__ pts_img) {
    __shared__ float sv[kThreads];
    __shared__ int si[kThreads];
    const int t = threadIdx.x, map = blockIdx.x, b = map / kPts;
    const float* m = hm + (int64_t)map * kMapPlane;
    float best = m[t];
    int at = t;
    for (int i = t + kThreads; i < kMapPlane; i += kThreads) {
        const float v = m[i];
        if (v > best) best = v, at = i;
    }
    sv[t] = best, si[t] = at;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            const float v = sv[t + s];
            const int i = si[t + s];
            if (v > sv[t] || (v == sv[t] && i < si[t])) sv[t] = v, si[t] = i;
        }
        __syncthreads();
    }
    if (t == 0) {
        at = si[0];
        const int px = at % kMap, py = at / kMap;
        float fx = (float)(px + 1), fy = (float)(py + 1);
        if (px > 0 && px < kMap - 1 && py > 0 && py < kMap - 1) {
            const float dx = m[py * kMap + px + 1] - m[py * kMap + px - 1], dy = m[(py + 1) * kMap + px] - m[(py - 1) * kMap + px];
            fx += dx > 0.f ? 0.25f : dx < 0.f ? -0.25f : 0.f;
            fy += dy > 0.f ? 0.25f : dy < 0.f ? -0.25f : 0.f;
        }
        fx -= 0.5f, fy -= 0.5f;
        pts[2 * map] = fx * 4.f, pts[2 * map + 1] = fy * 4.f;
        int ix, iy;
        inv_transform(face_of(faces + 4 * b), fx, fy, 64.f, ix, iy);
        pts_img[2 * map] = (float)ix, pts_img[2 * map + 1] = (float)iy;
    }
}

// [left, top, right, bottom] = min x, min y, max x, max y of a row's 68 points: one wave per row
__global__ __launch_bounds__(64) void fan_boxes_kernel(const float* __restrict__ pts, float* __restrict__ boxes) {
    const int b = blockIdx.x, t = threadIdx.x;
    const float* p = pts + (int64_t)b * kPts * 2;
    float x0 = p[2 * t], y0 = p[2 * t + 1], x1 = x0, y1 = y0;
    if (t + 64 < kPts) {
        const float xx = p[2 * (t + 64)], yy = p[2 * (t + 64) + 1];
        x0 = fminf(x0, xx), x1 = fmaxf(x1, xx), y0 = fminf(y0, yy), y1 = fmaxf(y1, yy);
    }
    x1 = wave_max(x1), y1 = wave_max(y1);
    x0 = -wave_max(-x0), y0 = -wave_max(-y0);
    if (t == 0) boxes[4 * b] = x0, boxes[4 * b + 1] = y0, boxes[4 * b + 2] = x1, boxes[4 * b + 3] = y1;
}

// ------------------------------------------------------------------ flip_input (landmarks_estimation.py:157-159)
// rows B..2B-1 of the crop buffer = rows 0..B-1 mirrored along x: flip(inp), a copy
__global__ __launch_bounds__(kThreads) void fan_mirror_kernel(float* __restrict__ crop, int B) {
    const int64_t n = (int64_t)B * 3 * kInPlane;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int u = (int)(idx % kIn);
        crop[n + idx] = crop[idx - u + (kIn - 1 - u)];
    }
}

// shuffle_lr's table (fan_model/utils.py:256-260)
struct Pairs {
    unsigned char at[kPts];
};
static Pairs flip_pairs() {
    static const unsigned char t[kPts] = {16, 15, 14, 13, 12, 11, 10, 9,  8,  7,  6,  5,  4,  3,  2,  1,  0,  26, 25, 24, 23, 22, 21,
                                          20, 19, 18, 17, 27, 28, 29, 30, 35, 34, 33, 32, 31, 45, 44, 43, 42, 47, 46, 39, 38, 37, 36,
                                          41, 40, 54, 53, 52, 51, 50, 49, 48, 59, 58, 57, 56, 55, 64, 63, 62, 61, 60, 67, 66, 65};
    Pairs p;
    memcpy(p.at, t, sizeof(t));
    return p;
}

// out[b,c,y,x] = hm2[b,c,y,x] + hm2[B+b, pairs[c], y, 63-x]: net(inp) + flip(net(flip(inp)), is_label=True)
__global__ __launch_bounds__(kThreads) void fan_flip_add_kernel(const float* __restrict__ hm2, int B, Pairs pairs, float* __restrict__ out) {
    const int64_t n = (int64_t)B * kPts * kMapPlane;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int x = (int)(idx % kMap), y = (int)((idx / kMap) % kMap);
        const int bc = (int)(idx / kMapPlane), b = bc / kPts, c = bc - b * kPts;
        const int64_t other = ((int64_t)(B + b) * kPts + pairs.at[c]) * kMapPlane + y * kMap + (kMap - 1 - x);
        out[idx] = hm2[idx] + hm2[other];
    }
}

// ------------------------------------------------------------------ draw_gaussian (fan_model/utils.py:13-60, sigma = 2)
constexpr int kGauss = 13;
struct GaussTable {
    float g[kGauss * kGauss];
};
// _gaussian(13): sigma 0.25 of the width, centre 7, evaluated in double and rounded to float once, as the store into the
// reference's float32 array does
static const GaussTable& gauss_table() {
    static const GaussTable t = [] {
        GaussTable r;
        for (int i = 0; i < kGauss; ++i)
            for (int j = 0; j < kGauss; ++j)
                r.g[i * kGauss + j] = (float)(1 * exp(-(pow((j + 1 - 7.0) / (0.25 * kGauss), 2) / 2.0 + pow((i + 1 - 7.0) / (0.25 * kGauss), 2) / 2.0)));
        return r;
    }();
    return t;
}

// the reference's 1-based ranges along one axis for ul = floor(p - 6), br = floor(p + 6) on a 256 map: image pixels i0 .. i1 take
// table entries from g0 on (all 1-based, i1 < i0: nothing)
__device__ __forceinline__ bool draw_range(float p, int& i0, int& i1, int& g0) {
    const float lo = floorf(__fsub_rn(p, 6.0f)), hi = floorf(__fadd_rn(p, 6.0f));
    if (!(lo > -1e6f && hi < 1e6f)) return false;      // also NaN; such a window is rejected below anyway
    const int ul = (int)lo, br = (int)hi;
    if (ul > kIn || br < 1) return false;
    g0 = max(1, -ul), i0 = max(1, ul), i1 = min(br, kIn);
    return true;
}

// one block per map: zeros, then the Gaussian.  Only one Gaussian lands in a map, so the clamp at 1 is a min.
__global__ __launch_bounds__(kThreads) void fan_draw_kernel(const float* __restrict__ pts, GaussTable tab, float* __restrict__ maps) {
    const int map = blockIdx.x, t = threadIdx.x;
    float* m = maps + (int64_t)map * kInPlane;
    for (int i = t; i < kInPlane; i += kThreads) m[i] = 0.f;
    const float px = pts[2 * map], py = pts[2 * map + 1];
    int x0, x1, gx, y0, y1, gy;
    if (!(px > 0.f) || !draw_range(px, x0, x1, gx) || !draw_range(py, y0, y1, gy)) return;
    __syncthreads();
    if (t < kGauss * kGauss) {
        const int dy = t / kGauss, dx = t - dy * kGauss;
        const int iy = y0 + dy, ix = x0 + dx, jy = gy + dy, jx = gx + dx;      // 1-based
        if (iy <= y1 && ix <= x1 && jy <= kGauss && jx <= kGauss) m[(iy - 1) * kIn + (ix - 1)] = fminf(tab.g[(jy - 1) * kGauss + (jx - 1)], 1.f);
    }
}

// ------------------------------------------------------------------ pts_img3 (landmarks_estimation.py:179-181)
// (pts_img.x, pts_img.y, depth * (1.0 / (256.0 / (200.0 * scale)))) in float32, every operation rounded on its own
__global__ __launch_bounds__(kThreads) void fan_assemble_kernel(const float* __restrict__ pts_img, const float* __restrict__ depth,
                                                                const float* __restrict__ faces, int B, float* __restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= B * kPts) return;
    const float scale = face_of(faces + 4 * (i / kPts)).scale;
    const float k = __fdiv_rn(1.0f, __fdiv_rn(256.0f, __fmul_rn(200.0f, scale)));
    out[3 * i] = pts_img[2 * i], out[3 * i + 1] = pts_img[2 * i + 1], out[3 * i + 2] = __fmul_rn(depth[i], k);
}

// ------------------------------------------------------------------ host side
static int launch_conv(const ConvArgs& a0, int ks, bool ext, float* part, hipStream_t st) {
    ConvArgs a = a0;
    // The number of K slices follows the output tiles, i.e. the layer and the row count, nothing else.
    const int M = a.R * a.Ho * a.Wo;
    const ConvPlan p = plan_conv(M, a.N, a.K, BN, conv_tiles(M, a.N, BN));
    SGDFR_REQUIRE(p.S == 1 || p.S * p.out_elems <= kPartElems, "fan: split-K partials of %lld floats exceed the workspace",
                  (long long)(p.S * p.out_elems));
    a.cps = p.cps;
    a.part = part;
    a.part_elems = p.out_elems;
    const dim3 grid(p.mt, p.nt, p.S);
    if (ks == 7 && !ext)
        hipLaunchKernelGGL((fan_conv_kernel<7, false>), grid, dim3(kThreads), 0, st, a);      // stem
    else if (ks == 3 && !ext)
        hipLaunchKernelGGL((fan_conv_kernel<3, false>), grid, dim3(kThreads), 0, st, a);      // the ConvBlock convs
    else if (ks == 1 && !ext)
        hipLaunchKernelGGL((fan_conv_kernel<1, false>), grid, dim3(kThreads), 0, st, a);      // projections, conv_last, l
    else if (ks == 1 && ext)
        hipLaunchKernelGGL((fan_conv_kernel<1, true>), grid, dim3(kThreads), 0, st, a);       // bl + al
    else
        SGDFR_REQUIRE(false, "fan: no conv instance for k=%d ext=%d", ks, (int)ext);
    if (check_launch("fan conv")) return 2;
    if (p.S > 1) {
        hipLaunchKernelGGL(fan_finish_kernel, dim3(grid_1d(p.out_elems)), dim3(kThreads), 0, st, a, p.S);
        if (check_launch("fan finish")) return 2;
    }
    return 0;
}

// workspace, float offsets.  Per row about 16.4 M floats (66 MB), most of it the four 128x128 maps in front of the first pool.
struct WsLayout {
    int64_t part, crop, stem, y2, res, t1, t2, pool, y3, prev[2], hg, top, ll, hm;
    int64_t pooled[kDepth], low1[kDepth], low2[kDepth], low3[kDepth];   // index level - 1, maps of (64 >> (4 - level)) / 2
    int64_t total;
};
static WsLayout ws_layout(int rows) {
    WsLayout w;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n * rows); return r; };
    const int64_t F = (int64_t)kFeat * kMapPlane;
    o = align64(kPartElems);
    w.part = 0;
    w.crop = take(3 * kInPlane);
    w.stem = take(64LL * kStem * kStem);
    w.y2 = take(128LL * kStem * kStem), w.res = take(128LL * kStem * kStem);
    w.t1 = take(64LL * kStem * kStem), w.t2 = take(32LL * kStem * kStem);
    w.pool = take(128LL * kMapPlane), w.y3 = take(128LL * kMapPlane);
    w.prev[0] = take(F), w.prev[1] = take(F), w.hg = take(F), w.top = take(F), w.ll = take(F);
    w.hm = take((int64_t)kPts * kMapPlane);
    for (int level = kDepth; level >= 1; --level) {
        const int h = (kMap >> (kDepth - level)) / 2;
        const int64_t n = (int64_t)kFeat * h * h;
        w.pooled[level - 1] = take(n), w.low1[level - 1] = take(n), w.low2[level - 1] = take(n), w.low3[level - 1] = take(n);
    }
    w.total = o;
    return w;
}

// debug stage outputs, each [rows, ...]: stem, conv4, per stack the hourglass output and the heatmaps
struct DebugLayout {
    int64_t stem, conv4, hg[kStacks], hm[kStacks], total;
};
static DebugLayout debug_layout(int rows) {
    DebugLayout d;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o += n * rows; return r; };
    d.stem = take(64LL * kStem * kStem);
    d.conv4 = take((int64_t)kFeat * kMapPlane);
    for (int s = 0; s < kStacks; ++s) d.hg[s] = take((int64_t)kFeat * kMapPlane), d.hm[s] = take((int64_t)kPts * kMapPlane);
    d.total = o;
    return d;
}

static bool rows_ok(int rows) { return rows >= 1 && rows <= kMaxRows; }
static bool size_ok(int rows, int H, int W) { return rows_ok(rows) && H >= 1 && W >= 1 && H <= 8192 && W <= 8192; }

struct Net {
    const float* pack;
    PackLayout pl;
    WsLayout wl;
    float* wsf;
    float* part;
    int R;
    hipStream_t st;
};

static ConvArgs conv_args(const float* src, int Hs, const float* wp, int K, int N, int Ho, int stride, int pad, float* out, int outC, int c0, int R) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src, a.wp = wp, a.out = out;
    a.R = R, a.Hs = a.Ws = Hs, a.N = N, a.Ho = a.Wo = Ho, a.K = a.K1 = K, a.stride = stride, a.pad = pad, a.outC = outC, a.c0 = c0;
    return a;
}

// ConvBlock i on in [R, cin, h, h] -> out [R, cout, h, h] (+ nearest_upsample(up) when up is given): 3 launches, 4 with a projection
static int run_block(const Net& n, int i, const float* in, int h, float* out, const float* up) {
    const Block u = block_of(i);
    const BlockPack& q = n.pl.u[i];
    const float* P = n.pack;
    float* t1 = n.wsf + n.wl.t1;
    float* t2 = n.wsf + n.wl.t2;
    const float* res = in;
    if (u.cin != u.cout) {
        float* r = n.wsf + n.wl.res;
        ConvArgs a = conv_args(in, h, P + q.wd, u.cin, u.cout, h, 1, 0, r, u.cout, 0, n.R);
        a.pre_g = P + q.gd, a.pre_h = P + q.hd;
        if (launch_conv(a, 1, false, n.part, n.st)) return 2;
        res = r;
    }
    const int ci[3] = {u.cin, u.cout / 2, u.cout / 4}, co[3] = {u.cout / 2, u.cout / 4, u.cout / 4}, c0[3] = {0, u.cout / 2, 3 * u.cout / 4};
    const float* src[3] = {in, t1, t2};
    float* raw[3] = {t1, t2, nullptr};
    for (int j = 0; j < 3; ++j) {
        ConvArgs a = conv_args(src[j], h, P + q.w[j], 9 * ci[j], co[j], h, 1, 1, out, u.cout, c0[j], n.R);
        a.pre_g = P + q.g[j], a.pre_h = P + q.h[j], a.raw = raw[j], a.res = res, a.up = up;
        if (launch_conv(a, 3, false, n.part, n.st)) return 2;
    }
    return 0;
}

static int run_pool(const Net& n, const float* in, float* out, int c, int h) {
    const int64_t planes = (int64_t)n.R * c;
    hipLaunchKernelGGL(fan_pool_kernel, dim3(grid_1d(planes * h * h)), dim3(kThreads), 0, n.st, in, out, planes, h, h);
    return check_launch("fan pool");
}

// HourGlass._forward(level, inp) on inp [R, 256, h, h] -> out: the lower branch first, so that b1's epilogue can add its upsampled end
static int run_hourglass(const Net& n, int stack, int level, const float* inp, int h, float* out) {
    float* pooled = n.wsf + n.wl.pooled[level - 1];
    float* low1 = n.wsf + n.wl.low1[level - 1];
    float* low2 = n.wsf + n.wl.low2[level - 1];
    float* low3 = n.wsf + n.wl.low3[level - 1];
    if (run_pool(n, inp, pooled, kFeat, h / 2)) return 2;
    if (run_block(n, hg_block(stack, level, 1), pooled, h / 2, low1, nullptr)) return 2;
    if (level > 1) {
        if (run_hourglass(n, stack, level - 1, low1, h / 2, low2)) return 2;
    } else {
        if (run_block(n, hg_plus(stack), low1, h / 2, low2, nullptr)) return 2;
    }
    if (run_block(n, hg_block(stack, level, 2), low2, h / 2, low3, nullptr)) return 2;
    return run_block(n, hg_block(stack, level, 0), inp, h, out, low3);
}

static int run_network(const float* crop, int R, const float* pack, float* heatmaps, float* debug, float* wsf, hipStream_t st) {
    Net n;
    n.pack = pack, n.pl = pack_layout(), n.wl = ws_layout(R), n.wsf = wsf, n.part = wsf + n.wl.part, n.R = R, n.st = st;
    const PackLayout& pl = n.pl;
    const WsLayout& wl = n.wl;
    const DebugLayout dl = debug_layout(R);
    auto dump = [&](int64_t off, const float* src, int64_t count) {
        if (!debug) return 0;
        if (hipMemcpyAsync(debug + off, src, count * R * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
            set_error("fan_forward: debug copy failed");
            return 2;
        }
        return 0;
    };
    const int64_t F = (int64_t)kFeat * kMapPlane, HM = (int64_t)kPts * kMapPlane;

    float* stem = wsf + wl.stem;
    ConvArgs a = conv_args(crop, kIn, pack + pl.w0, 147, 64, kStem, 2, 3, stem, 64, 0, R);
    a.bias = pack + pl.b0, a.relu = 1;
    if (launch_conv(a, 7, false, n.part, st)) return 2;
    if (dump(dl.stem, stem, 64LL * kStem * kStem)) return 2;
    if (run_block(n, 0, stem, kStem, wsf + wl.y2, nullptr)) return 2;
    if (run_pool(n, wsf + wl.y2, wsf + wl.pool, 128, kMap)) return 2;
    if (run_block(n, 1, wsf + wl.pool, kMap, wsf + wl.y3, nullptr)) return 2;
    if (run_block(n, 2, wsf + wl.y3, kMap, wsf + wl.prev[0], nullptr)) return 2;
    if (dump(dl.conv4, wsf + wl.prev[0], F)) return 2;

    int cur = 0;
    for (int s = 0; s < kStacks; ++s) {
        float* prev = wsf + wl.prev[cur];
        float* hg = wsf + wl.hg;
        float* top = wsf + wl.top;
        float* ll = wsf + wl.ll;
        float* hm = s + 1 == kStacks ? heatmaps : wsf + wl.hm;
        if (run_hourglass(n, s, kDepth, prev, kMap, hg)) return 2;
        if (dump(dl.hg[s], hg, F)) return 2;
        if (run_block(n, top_block(s), hg, kMap, top, nullptr)) return 2;
        a = conv_args(top, kMap, pack + pl.w_last[s], kFeat, kFeat, kMap, 1, 0, ll, kFeat, 0, R);
        a.bias = pack + pl.b_last[s], a.relu = 1;
        if (launch_conv(a, 1, false, n.part, st)) return 2;
        a = conv_args(ll, kMap, pack + pl.w_l[s], kFeat, kPts, kMap, 1, 0, hm, kPts, 0, R);
        a.bias = pack + pl.b_l[s];
        if (launch_conv(a, 1, false, n.part, st)) return 2;
        if (dump(dl.hm[s], hm, HM)) return 2;
        if (s + 1 < kStacks) {
            a = conv_args(ll, kMap, pack + pl.w_mix[s], kFeat, kFeat, kMap, 1, 0, wsf + wl.prev[cur ^ 1], kFeat, 0, R);
            a.K = kFeat + kPts, a.ext = hm, a.bias = pack + pl.b_mix[s], a.res = prev;
            if (launch_conv(a, 1, true, n.part, st)) return 2;
            cur ^= 1;
        }
    }
    return 0;
}

static int run_decode(const float* heatmaps, const float* faces, int rows, float* pts, float* pts_img, float* boxes, hipStream_t st) {
    hipLaunchKernelGGL(fan_decode_kernel, dim3(rows * kPts), dim3(kThreads), 0, st, heatmaps, faces, pts, pts_img);
    if (check_launch("fan decode")) return 2;
    if (boxes) {
        hipLaunchKernelGGL(fan_boxes_kernel, dim3(rows), dim3(64), 0, st, pts_img, boxes);
        if (check_launch("fan boxes")) return 2;
    }
    return 0;
}

}  // namespace
}  // namespace sgdfr

using namespace sgdfr;

extern "C" int64_t sgdfr_fan_pack_elems(void) { return pack_layout().total; }

extern "C" int64_t sgdfr_fan_debug_elems(int rows) {
    if (!rows_ok(rows)) return -1;
    return debug_layout(rows).total;
}

extern "C" int64_t sgdfr_fan_workspace_bytes(int rows, int H, int W) {
    if (!size_ok(rows, H, W)) return -1;
    return ws_layout(rows).total * (int64_t)sizeof(float);
}

extern "C" int sgdfr_fan_prepack_f32(const float* const* params, float* pack, void* stream) {
    SGDFR_REQUIRE(params && pack, "fan_prepack: null pointer");
    for (int i = 0; i < kParams; ++i) {
        bool optional = false;
        if (i >= 2 && i < 2 + kBlocks * kBlockParams) {
            const Block u = block_of((i - 2) / kBlockParams);
            optional = (i - 2) % kBlockParams >= 9 && u.cin == u.cout;      // projection of an identity block
        }
        SGDFR_REQUIRE(optional || params[i], "fan_prepack: parameter %d is null", i);
    }
    const PackLayout pl = pack_layout();
    hipStream_t st = as_stream(stream);
    auto seg = [&](const float* src, int64_t dst, int64_t count, int copy, int cin, int cout, int kk) {
        hipLaunchKernelGGL(fan_pack_kernel, dim3(grid_1d(count)), dim3(kThreads), 0, st, src, pack + dst, count, copy, cin, cout, kk);
        return check_launch("fan prepack");
    };
    int rc = 0;
    rc |= seg(params[0], pl.w0, 147 * 64, 0, 3, 64, 49);
    rc |= seg(params[1], pl.b0, 64, 1, 0, 0, 0);
    for (int i = 0; i < kBlocks && !rc; ++i) {
        const Block u = block_of(i);
        const BlockPack& q = pl.u[i];
        const float* const* P = params + 2 + kBlockParams * i;
        const int ci[3] = {u.cin, u.cout / 2, u.cout / 4}, co[3] = {u.cout / 2, u.cout / 4, u.cout / 4};
        for (int j = 0; j < 3; ++j) {
            rc |= seg(P[3 * j], q.g[j], ci[j], 1, 0, 0, 0);
            rc |= seg(P[3 * j + 1], q.h[j], ci[j], 1, 0, 0, 0);
            rc |= seg(P[3 * j + 2], q.w[j], 9LL * ci[j] * co[j], 0, ci[j], co[j], 9);
        }
        if (u.cin != u.cout) {
            rc |= seg(P[9], q.gd, u.cin, 1, 0, 0, 0);
            rc |= seg(P[10], q.hd, u.cin, 1, 0, 0, 0);
            rc |= seg(P[11], q.wd, (int64_t)u.cin * u.cout, 0, u.cin, u.cout, 1);
        }
    }
    const float* const* T = params + 2 + kBlockParams * kBlocks;      // per stack: conv_last w, b, l w, b
    for (int s = 0; s < kStacks && !rc; ++s) {
        rc |= seg(T[4 * s], pl.w_last[s], kFeat * kFeat, 0, kFeat, kFeat, 1);
        rc |= seg(T[4 * s + 1], pl.b_last[s], kFeat, 1, 0, 0, 0);
        rc |= seg(T[4 * s + 2], pl.w_l[s], kFeat * kPts, 0, kFeat, kPts, 1);
        rc |= seg(T[4 * s + 3], pl.b_l[s], kPts, 1, 0, 0, 0);
    }
    const float* const* X = T + 4 * kStacks;                          // per stack but the last: bl w, al w, bl b + al b
    for (int s = 0; s + 1 < kStacks && !rc; ++s) {
        rc |= seg(X[3 * s], pl.w_mix[s], kFeat * kFeat, 0, kFeat, kFeat, 1);
        rc |= seg(X[3 * s + 1], pl.w_mix[s] + kFeat * kFeat, kPts * kFeat, 0, kPts, kFeat, 1);   // al's rows behind bl's in K
        rc |= seg(X[3 * s + 2], pl.b_mix[s], kFeat, 1, 0, 0, 0);
    }
    return rc ? 2 : 0;
}

extern "C" int sgdfr_fan_crop_f32(const float* x, const float* faces, int rows, int H, int W, int input_range, float* crop, void* stream) {
    SGDFR_REQUIRE(size_ok(rows, H, W), "fan_crop: unsupported size (%d rows of %dx%d)", rows, H, W);
    SGDFR_REQUIRE(input_range == SGDFR_FAN_RANGE_255 || input_range == SGDFR_FAN_RANGE_GAN, "fan_crop: unknown input_range %d", input_range);
    SGDFR_REQUIRE(x && faces && crop, "fan_crop: null pointer");
    hipLaunchKernelGGL(fan_front_kernel, dim3(grid_1d((int64_t)rows * 3 * kInPlane)), dim3(kThreads), 0, as_stream(stream), x, faces, rows, H,
                       W, input_range == SGDFR_FAN_RANGE_GAN ? 1 : 0, crop);
    return check_launch("fan crop");
}

extern "C" int sgdfr_fan_network_f32(const float* crop, int rows, const float* pack, float* heatmaps, float* debug, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(rows_ok(rows), "fan_network: unsupported size (%d rows)", rows);
    SGDFR_REQUIRE(crop && pack && heatmaps && workspace, "fan_network: null pointer");
    const int64_t need = ws_layout(rows).total * (int64_t)sizeof(float);
    SGDFR_REQUIRE(need <= workspace_bytes, "fan_network: workspace of %lld bytes, %d rows need %lld", (long long)workspace_bytes, rows,
                  (long long)need);
    return run_network(crop, rows, pack, heatmaps, debug, reinterpret_cast<float*>(workspace), as_stream(stream));
}

extern "C" int sgdfr_fan_decode_f32(const float* heatmaps, const float* faces, int rows, float* pts, float* pts_img, float* boxes,
                                    void* stream) {
    SGDFR_REQUIRE(rows_ok(rows), "fan_decode: unsupported size (%d rows)", rows);
    SGDFR_REQUIRE(heatmaps && faces && pts && pts_img, "fan_decode: null pointer");
    return run_decode(heatmaps, faces, rows, pts, pts_img, boxes, as_stream(stream));
}

extern "C" int sgdfr_fan_boxes_f32(const float* pts_img, int rows, float* boxes, void* stream) {
    SGDFR_REQUIRE(rows >= 1, "fan_boxes: unsupported size (%d rows)", rows);
    SGDFR_REQUIRE(pts_img && boxes, "fan_boxes: null pointer");
    hipLaunchKernelGGL(fan_boxes_kernel, dim3(rows), dim3(64), 0, as_stream(stream), pts_img, boxes);
    return check_launch("fan boxes");
}

extern "C" int sgdfr_fan_forward_f32(const float* x, const float* faces, int rows, int H, int W, int input_range, const float* pack,
                                     float* heatmaps, float* pts, float* pts_img, float* boxes, float* debug, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(size_ok(rows, H, W), "fan_forward: unsupported size (%d rows of %dx%d)", rows, H, W);
    SGDFR_REQUIRE(input_range == SGDFR_FAN_RANGE_255 || input_range == SGDFR_FAN_RANGE_GAN, "fan_forward: unknown input_range %d",
                  input_range);
    SGDFR_REQUIRE(x && faces && pack && heatmaps && pts && pts_img && workspace, "fan_forward: null pointer");
    const WsLayout wl = ws_layout(rows);
    SGDFR_REQUIRE(wl.total * (int64_t)sizeof(float) <= workspace_bytes, "fan_forward: workspace of %lld bytes, %d rows need %lld",
                  (long long)workspace_bytes, rows, (long long)(wl.total * (int64_t)sizeof(float)));
    float* wsf = reinterpret_cast<float*>(workspace);
    hipStream_t st = as_stream(stream);
    float* crop = wsf + wl.crop;
    hipLaunchKernelGGL(fan_front_kernel, dim3(grid_1d((int64_t)rows * 3 * kInPlane)), dim3(kThreads), 0, st, x, faces, rows, H, W,
                       input_range == SGDFR_FAN_RANGE_GAN ? 1 : 0, crop);
    if (check_launch("fan front")) return 2;
    if (run_network(crop, rows, pack, heatmaps, debug, wsf, st)) return 2;
    return run_decode(heatmaps, faces, rows, pts, pts_img, boxes, st);
}

extern "C" int sgdfr_fan_flip_add_f32(const float* hm2, int rows, float* out, void* stream) {
    SGDFR_REQUIRE(rows >= 1 && 2 * rows <= kMaxRows, "fan_flip_add: unsupported size (%d rows)", rows);
    SGDFR_REQUIRE(hm2 && out, "fan_flip_add: null pointer");
    hipLaunchKernelGGL(fan_flip_add_kernel, dim3(grid_1d((int64_t)rows * kPts * kMapPlane)), dim3(kThreads), 0, as_stream(stream), hm2, rows,
                       flip_pairs(), out);
    return check_launch("fan flip add");
}

extern "C" int sgdfr_fan_draw_f32(const float* pts, int rows, float* maps, void* stream) {
    SGDFR_REQUIRE(rows_ok(rows), "fan_draw: unsupported size (%d rows)", rows);
    SGDFR_REQUIRE(pts && maps, "fan_draw: null pointer");
    hipLaunchKernelGGL(fan_draw_kernel, dim3(rows * kPts), dim3(kThreads), 0, as_stream(stream), pts, gauss_table(), maps);
    return check_launch("fan draw");
}

extern "C" int sgdfr_fan_forward3d_f32(const float* x, const float* faces, int rows, int H, int W, int input_range, int flip,
                                       const float* pack, const float* depth_pack, float* hm2, float* heatmaps, float* pts, float* pts_img,
                                       float* boxes, float* maps, float* depth, float* pts_img3, float* debug, void* workspace,
                                       int64_t workspace_bytes, void* depth_workspace, int64_t depth_workspace_bytes, void* stream) {
    const int net_rows = flip ? 2 * rows : rows;      // the mirrors ride behind the crops: a flip call takes half the rows
    SGDFR_REQUIRE(rows >= 1 && size_ok(net_rows, H, W), "fan_forward3d: unsupported size (%d rows of %dx%d, flip %d)", rows, H, W, flip);
    SGDFR_REQUIRE(input_range == SGDFR_FAN_RANGE_255 || input_range == SGDFR_FAN_RANGE_GAN, "fan_forward3d: unknown input_range %d",
                  input_range);
    SGDFR_REQUIRE(x && faces && pack && heatmaps && pts && pts_img && workspace && (!flip || hm2), "fan_forward3d: null pointer");
    SGDFR_REQUIRE(!depth_pack || (maps && depth && pts_img3 && depth_workspace), "fan_forward3d: null pointer (3D outputs)");
    const WsLayout wl = ws_layout(net_rows);
    SGDFR_REQUIRE(wl.total * (int64_t)sizeof(float) <= workspace_bytes, "fan_forward3d: workspace of %lld bytes, %d rows need %lld",
                  (long long)workspace_bytes, net_rows, (long long)(wl.total * (int64_t)sizeof(float)));
    float* wsf = reinterpret_cast<float*>(workspace);
    hipStream_t st = as_stream(stream);
    float* crop = wsf + wl.crop;
    hipLaunchKernelGGL(fan_front_kernel, dim3(grid_1d((int64_t)rows * 3 * kInPlane)), dim3(kThreads), 0, st, x, faces, rows, H, W,
                       input_range == SGDFR_FAN_RANGE_GAN ? 1 : 0, crop);
    if (check_launch("fan front")) return 2;
    if (flip) {
        hipLaunchKernelGGL(fan_mirror_kernel, dim3(grid_1d((int64_t)rows * 3 * kInPlane)), dim3(kThreads), 0, st, crop, rows);
        if (check_launch("fan mirror")) return 2;
        if (run_network(crop, net_rows, pack, hm2, debug, wsf, st)) return 2;
        hipLaunchKernelGGL(fan_flip_add_kernel, dim3(grid_1d((int64_t)rows * kPts * kMapPlane)), dim3(kThreads), 0, st, hm2, rows, flip_pairs(),
                           heatmaps);
        if (check_launch("fan flip add")) return 2;
    } else if (run_network(crop, rows, pack, heatmaps, debug, wsf, st)) {
        return 2;
    }
    if (run_decode(heatmaps, faces, rows, pts, pts_img, boxes, st)) return 2;
    if (!depth_pack) return 0;
    hipLaunchKernelGGL(fan_draw_kernel, dim3(rows * kPts), dim3(kThreads), 0, st, pts, gauss_table(), maps);
    if (check_launch("fan draw")) return 2;
    // the crop rows 0..rows-1 are read by the stem only and are still the front's
    if (sgdfr_fandepth_network_f32(crop, maps, rows, depth_pack, depth, nullptr, depth_workspace, depth_workspace_bytes, stream)) return 2;
    hipLaunchKernelGGL(fan_assemble_kernel, dim3((rows * kPts + kThreads - 1) / kThreads), dim3(kThreads), 0, st, pts_img, depth, faces, rows,
                       pts_img3);
    return check_launch("fan assemble");
}
