// The S3FD face detector in eval mode (libs/face_models/sfd/net_s3fd.py s3fd, detect.py:36-81 batch_detect, bbox.py:44-66 nms and
// :93-111 decode, sfd_detector.py:31-47 detect_from_batch): image -> VGG-16 trunk (conv3x3 + bias + ReLU, 2x2 max-pool with floor
// after conv1_2, conv2_2, conv3_3, conv4_3, conv5_3) -> fc6 (3x3, padding 3: the map grows by 4), fc7, conv6_1, conv6_2 (stride 2),
// conv7_1, conv7_2 (stride 2) -> L2Norm on conv3_3, conv4_3, conv5_3 -> per level one conv3x3 for conf and loc together -> max-out of
// level 0's three background logits, softmax score, threshold, box decode against the prior (stride 2^(i+2), size 4 strides),
// compacted in (level, y, x) order -> greedy NMS at IoU 0.3 in descending score order, boxes above 0.5 kept.
// Forward only: a box is a decision, nothing differentiates it.
//
// Every conv is one implicit-GEMM kernel on exact-f32 MFMA (v_mfma_f32_16x16x4_f32) with the split over K and fixed-order finish
// of deca.hip / fan.hip.  What this network adds:
//   * two tiles: 64 pixels x 64 channels for the trunk (four waves as 2 x 2, each 32 x 32) and 64 pixels x 16 channels for the six
//     head convs (four waves along the pixels, one MFMA block each), so that N = 6 or 8 fills half of one 16-wide block and not an
//     eighth of a 64-wide tile;
//   * L2Norm is a per-pixel reciprocal norm (one bandwidth kernel per tap) that the head conv's loader multiplies onto every tap at
//     the tap's pixel; the per-channel L2Norm weight is folded into the head filters on the host;
//   * the mean subtraction of detect() is a loader option of the first conv (a tap outside the image stays 0: the reference pads
//     behind the subtraction).
// The max-pool is a kernel of its own: levels 0-2 keep the unpooled map for their head.
// No float atomics, no host synchronisation, everything on the given stream: candidate and box counts stay on the device.
#include <string.h>

#include <algorithm>

#include "conv_tile.h"

namespace sgdfr {
namespace {

constexpr int kTrunk = 19, kLevels = 6;
constexpr int kParams = 2 * (kTrunk + kLevels);
constexpr int kMaxRows = 256, kMaxSide = 4096, kMinSide = 32, kMaxCapacity = 16384;
constexpr int64_t kMaxPixels = 1LL << 24;           // rows * H * W: every element index of a 64-channel map stays below 2^31
// split K only below 512 output tiles, at most 512 / tiles slices: S * (output elements) <= 512 tiles of 64 x 64
constexpr int64_t kPartElems = 512LL * BM * 64;

// ------------------------------------------------------------------ network geometry
struct Layer {
    int cin, cout, ks, stride, pad, pool, level;    // pool: a 2x2 max-pool follows; level: the head this output feeds (-1: none)
};
const Layer kNet[kTrunk] = {
    {3, 64, 3, 1, 1, 0, -1},     {64, 64, 3, 1, 1, 1, -1},                                     // conv1_1 conv1_2
    {64, 128, 3, 1, 1, 0, -1},   {128, 128, 3, 1, 1, 1, -1},                                   // conv2_1 conv2_2
    {128, 256, 3, 1, 1, 0, -1},  {256, 256, 3, 1, 1, 0, -1},  {256, 256, 3, 1, 1, 1, 0},       // conv3_1 conv3_2 conv3_3
    {256, 512, 3, 1, 1, 0, -1},  {512, 512, 3, 1, 1, 0, -1},  {512, 512, 3, 1, 1, 1, 1},       // conv4_1 conv4_2 conv4_3
    {512, 512, 3, 1, 1, 0, -1},  {512, 512, 3, 1, 1, 0, -1},  {512, 512, 3, 1, 1, 1, 2},       // conv5_1 conv5_2 conv5_3
    {512, 1024, 3, 1, 3, 0, -1}, {1024, 1024, 1, 1, 0, 0, 3},                                  // fc6 fc7
    {1024, 256, 1, 1, 0, 0, -1}, {256, 512, 3, 2, 1, 0, 4},                                    // conv6_1 conv6_2
    {512, 128, 1, 1, 0, 0, -1},  {128, 256, 3, 2, 1, 0, 5},                                    // conv7_1 conv7_2
};
const int kHeadC[kLevels] = {256, 512, 512, 1024, 512, 256};
const int kHeadConf[kLevels] = {4, 2, 2, 2, 2, 2};                 // + 4 loc channels behind them
const int kDebugLayers[] = {1, 3, 6, 9, 12, 13, 14, 16, 18};       // conv1_2 conv2_2 conv3_3 conv4_3 conv5_3 fc6 fc7 conv6_2 conv7_2
constexpr int kDebugTaps = 9;

struct Geo {
    int hi[kTrunk], wi[kTrunk], ho[kTrunk], wo[kTrunk], lh[kLevels], lw[kLevels];
};
static Geo geometry(int H, int W) {
    Geo g;
    int h = H, w = W;
    for (int i = 0; i < kTrunk; ++i) {
        const Layer& l = kNet[i];
        g.hi[i] = h, g.wi[i] = w;
        h = (h + 2 * l.pad - l.ks) / l.stride + 1, w = (w + 2 * l.pad - l.ks) / l.stride + 1;
        g.ho[i] = h, g.wo[i] = w;
        if (l.level >= 0) g.lh[l.level] = h, g.lw[l.level] = w;
        if (l.pool) h /= 2, w /= 2;
    }
    return g;
}

static bool rows_ok(int rows) { return rows >= 1 && rows <= kMaxRows; }
static bool size_ok(int rows, int H, int W) {
    return rows_ok(rows) && H >= kMinSide && W >= kMinSide && H <= kMaxSide && W <= kMaxSide && (int64_t)rows * H * W <= kMaxPixels;
}

// ------------------------------------------------------------------ weight pack
struct PackLayout {
    int64_t w[kTrunk], b[kTrunk], hw[kLevels], hb[kLevels], total;
};
static PackLayout pack_layout() {
    PackLayout p;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    for (int i = 0; i < kTrunk; ++i) {
        const Layer& l = kNet[i];
        p.w[i] = take((int64_t)l.cin * l.ks * l.ks * l.cout), p.b[i] = take(l.cout);
    }
    for (int l = 0; l < kLevels; ++l) p.hw[l] = take(9LL * kHeadC[l] * (kHeadConf[l] + 4)), p.hb[l] = take(kHeadConf[l] + 4);
    p.total = o;
    return p;
}

// copy: dst[j] = src[j].  Else [k = ci*kk + r][co] <- W[co][ci][r]
__global__ __launch_bounds__(kThreads) void s3fd_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t count,
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
    const float* src;        // [R, K / (KS*KS), Hs, Ws]
    const float* wp;         // [K][N]
    const float* bias;       // epilogue: + bias[n], then ReLU if `relu`
    const float* rn;         // loader: x * rn[b, ih, iw] on every tap inside the map (NULL: the plain value)
    float* out;              // [R, N, Ho, Wo]
    float* part;             // split K: [S][R*N*Ho*Wo]
    int64_t part_elems;
    float sub0, sub1, sub2;  // loader: x - sub[ci] on every tap inside the map when has_sub (the first conv: ci < 3)
    int has_sub;
    int R, Hs, Ws, N, Ho, Wo, K, stride, pad, cps, relu;
};

__device__ __forceinline__ void epilogue(const ConvArgs& a, int b, int n, int p, float v) {
    v += a.bias[n];
    if (a.relu) v = fmaxf(v, 0.f);
    a.out[((int64_t)b * a.N + n) * (a.Ho * a.Wo) + p] = v;
}

// BN = 64: the trunk's tile.  BN = 16: the heads' (conv_tile.h Tile<BN>).
template <int KS, int BN>
__global__ __launch_bounds__(kThreads) void s3fd_conv_kernel(ConvArgs a) {
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
        const int pix = gm - b * HWo;
        oh = pix / a.Wo;
        ow = pix - oh * a.Wo;
    }
    const float* srcb = a.src + (int64_t)b * (a.K / (KS * KS)) * plane;
    const float* rnb = a.rn ? a.rn + (int64_t)b * plane : nullptr;

    const int nchunks = (a.K + BK - 1) / BK;
    const int c0 = blockIdx.z * a.cps, c1 = min(nchunks, c0 + a.cps);
    float xr[4], wr[Tile<BN>::WL];
    auto gload = [&](int c) {
        const int k0 = c * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + wv + 4 * i;      // uniform over the wave
            float v = 0.f;
            if (k < a.K) {
                const int ci = k / (KS * KS), r = k - ci * (KS * KS), kh = r / KS, kw = r - kh * KS;
                const int ih = oh * a.stride - a.pad + kh, iw = ow * a.stride - a.pad + kw;
                if (mvalid && ih >= 0 && ih < a.Hs && iw >= 0 && iw < a.Ws) {
                    v = srcb[(int64_t)ci * plane + ih * a.Ws + iw];
                    if (rnb) v *= rnb[ih * a.Ws + iw];
                    if (a.has_sub) v -= ci == 0 ? a.sub0 : ci == 1 ? a.sub1 : a.sub2;
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
__global__ __launch_bounds__(kThreads) void s3fd_finish_kernel(ConvArgs a, int S) {
    finish_slices(a.part, a.part_elems, S, a.N, a.Ho * a.Wo, [=](int b, int n, int p, float v) { epilogue(a, b, n, p, v); });
}

// ------------------------------------------------------------------ max_pool2d(2, 2), floor: [planes, hi, wi] -> [planes, hi/2, wi/2]
__global__ __launch_bounds__(kThreads) void s3fd_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t planes, int hi,
                                                             int wi) {
    const int ho = hi / 2, wo = wi / 2;
    const int64_t n = planes * ho * wo;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(idx % wo), i = (int)((idx / wo) % ho);
        const float* p = in + (idx / ((int64_t)ho * wo)) * ((int64_t)hi * wi) + (int64_t)(2 * i) * wi + 2 * j;
        out[idx] = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[wi], p[wi + 1]));
    }
}

// ------------------------------------------------------------------ L2Norm: rn[b, p] = 1 / (sqrt(sum_c x[b, c, p]^2) + 1e-10)
__global__ __launch_bounds__(kThreads) void s3fd_rnorm_kernel(const float* __restrict__ x, float* __restrict__ rn, int rows, int C, int plane) {
    const int64_t n = (int64_t)rows * plane;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int b = (int)(idx / plane), p = (int)(idx - (int64_t)b * plane);
        const float* q = x + (int64_t)b * C * plane + p;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;          // C is a multiple of 4
        for (int c = 0; c < C; c += 4) {
            const float v0 = q[(int64_t)c * plane], v1 = q[(int64_t)(c + 1) * plane], v2 = q[(int64_t)(c + 2) * plane],
                        v3 = q[(int64_t)(c + 3) * plane];
            s0 = fmaf(v0, v0, s0), s1 = fmaf(v1, v1, s1), s2 = fmaf(v2, v2, s2), s3 = fmaf(v3, v3, s3);
        }
        rn[idx] = 1.f / (sqrtf((s0 + s1) + (s2 + s3)) + 1e-10f);
    }
}

// ------------------------------------------------------------------ the head outputs of every level, as the decode reads them
struct Heads {
    const float* p[kLevels];       // level l: [rows, conf_l + 4, h_l, w_l], conf channels first
    int h[kLevels], w[kLevels];
    int start[kLevels + 1];        // positions of one image in front of level l
};
static Heads make_heads(const float* const* ptrs, const int* hw) {
    Heads hd;
    hd.start[0] = 0;
    for (int l = 0; l < kLevels; ++l) {
        hd.p[l] = ptrs[l], hd.h[l] = hw[2 * l], hd.w[l] = hw[2 * l + 1];
        hd.start[l + 1] = hd.start[l] + hd.h[l] * hd.w[l];
    }
    return hd;
}

// the twelve maps of s3fd.forward: per level cls [rows, 2, h, w] (level 0 after the max-out) and reg [rows, 4, h, w]
__global__ __launch_bounds__(kThreads) void s3fd_maps_kernel(const float* __restrict__ head, int rows, int conf, int plane,
                                                             float* __restrict__ cls, float* __restrict__ reg) {
    const int64_t n = (int64_t)rows * 6 * plane;
    const int C = conf + 4;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int p = (int)(idx % plane), c = (int)((idx / plane) % 6), b = (int)(idx / (6LL * plane));
        const float* q = head + (int64_t)b * C * plane + p;
        if (c == 0) {
            float v = q[0];
            for (int k = 1; k < conf - 1; ++k) v = fmaxf(v, q[(int64_t)k * plane]);
            cls[((int64_t)b * 2) * plane + p] = v;
        } else if (c == 1) {
            cls[((int64_t)b * 2 + 1) * plane + p] = q[(int64_t)(conf - 1) * plane];
        } else {
            reg[((int64_t)b * 4 + (c - 2)) * plane + p] = q[(int64_t)(conf + c - 2) * plane];
        }
    }
}

// ------------------------------------------------------------------ candidates: one block per image
// detect.py:48-72 and bbox.py:93-111 in float32, every operation rounded on its own.  The positions of an image are walked in
// (level, y, x) order in chunks of one block; a ballot and the four wave totals give every passing position its place, so the list
// has the reference's order whatever order the waves run in.
__global__ __launch_bounds__(kThreads) void s3fd_candidates_kernel(Heads hd, float threshold, int capacity, float* __restrict__ cand,
                                                                   int* __restrict__ count, int* __restrict__ valid) {
    __shared__ int wsum[kThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, b = blockIdx.x;
    const int total = hd.start[kLevels];
    float* out = cand + (int64_t)b * capacity * 5;
    int base = 0;
    for (int p0 = 0; p0 < total; p0 += kThreads) {
        const int pos = p0 + t;
        bool flag = false;
        float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, score = 0.f;
        if (pos < total) {
            int l = 0;
#pragma unroll
            for (int k = 1; k < kLevels; ++k) l += pos >= hd.start[k] ? 1 : 0;
            const float* hp = hd.p[0];
            int h = hd.h[0], w = hd.w[0], st = hd.start[0];
#pragma unroll
            for (int k = 1; k < kLevels; ++k)
                if (l == k) hp = hd.p[k], h = hd.h[k], w = hd.w[k], st = hd.start[k];
            const int plane = h * w, p = pos - st, conf = l == 0 ? 4 : 2;
            const int y = p / w, x = p - y * w;
            const float* q = hp + (int64_t)b * (conf + 4) * plane + p;
            float bg = q[0];
            if (l == 0) bg = fmaxf(fmaxf(bg, q[plane]), q[2 * plane]);
            const float fg = q[(int64_t)(conf - 1) * plane];
            const float m = fmaxf(bg, fg), e0 = expf(bg - m), e1 = expf(fg - m);
            score = __fdiv_rn(e1, __fadd_rn(e0, e1));
            flag = score > threshold;
            if (flag) {
                const float* loc = q + (int64_t)conf * plane;
                const float s = (float)(4 << l), a4 = 4.f * s;
                const float cx = __fadd_rn(s * 0.5f + (float)x * s, __fmul_rn(__fmul_rn(loc[0], 0.1f), a4));
                const float cy = __fadd_rn(s * 0.5f + (float)y * s, __fmul_rn(__fmul_rn(loc[plane], 0.1f), a4));
                const float bw = __fmul_rn(a4, expf(__fmul_rn(loc[2 * plane], 0.2f)));
                const float bh = __fmul_rn(a4, expf(__fmul_rn(loc[3 * plane], 0.2f)));
                x1 = __fsub_rn(cx, __fdiv_rn(bw, 2.f)), y1 = __fsub_rn(cy, __fdiv_rn(bh, 2.f));
                x2 = __fadd_rn(bw, x1), y2 = __fadd_rn(bh, y1);
            }
        }
        const unsigned long long mask = __ballot(flag);
        if (lane == 0) wsum[wv] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kThreads / 64; ++k) {
            const int v = wsum[k];
            before += k < wv ? v : 0;
            all += v;
        }
        if (flag) {
            const int at = base + before + __popcll(mask & ((1ull << lane) - 1ull));
            if (at < capacity) {
                float* o = out + (int64_t)at * 5;
                o[0] = x1, o[1] = y1, o[2] = x2, o[3] = y2, o[4] = score;
            }
        }
        base += all;
        __syncthreads();
    }
    if (t == 0) count[b] = base, valid[b] = base <= capacity ? 1 : 0;
}

// ------------------------------------------------------------------ selection: one block per image
// bbox.py:44-66 with sfd_detector.py:42: the candidates above 0.5 (a box is never suppressed by a lower-scoring one, so those at or
// below 0.5 cannot change what survives the final filter) ranked by score descending, ties by candidate index ascending, then the
// greedy pass with the reference's float32 arithmetic ("+ 1" areas, suppressed when IoU > 0.3), then the survivors moved up in order.
__device__ __forceinline__ float box_area(const float* q) {
    return __fmul_rn(__fadd_rn(__fsub_rn(q[2], q[0]), 1.f), __fadd_rn(__fsub_rn(q[3], q[1]), 1.f));
}

__global__ __launch_bounds__(kThreads) void s3fd_nms_kernel(const float* __restrict__ cand, const int* __restrict__ count, int capacity,
                                                            float* __restrict__ boxes, int* __restrict__ index, int* __restrict__ kept) {
    __shared__ unsigned sup[kMaxCapacity / 32];
    __shared__ int wsum[kThreads / 64];
    __shared__ int n2s;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, b = blockIdx.x;
    const float* in = cand + (int64_t)b * capacity * 5;
    float* out = boxes + (int64_t)b * capacity * 5;
    int* idx = index + (int64_t)b * capacity;
    const int n = min(max(count[b], 0), capacity);
    for (int i = t; i < kMaxCapacity / 32; i += kThreads) sup[i] = 0u;
    if (t == 0) n2s = 0;
    __syncthreads();

    // rank sort of the candidates above 0.5
    for (int i = t; i < n; i += kThreads) {
        const float s = in[(int64_t)i * 5 + 4];
        if (!(s > 0.5f)) continue;
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float u = in[(int64_t)j * 5 + 4];
            rank += (u > 0.5f && (u > s || (u == s && j < i))) ? 1 : 0;
        }
        float* o = out + (int64_t)rank * 5;
#pragma unroll
        for (int k = 0; k < 5; ++k) o[k] = in[(int64_t)i * 5 + k];
        idx[rank] = i;
        atomicAdd(&n2s, 1);
    }
    __syncthreads();
    const int n2 = n2s;

    // greedy pass: box i is kept unless an earlier kept box marked it
    for (int i = 0; i < n2; ++i) {
        if ((sup[i >> 5] >> (i & 31)) & 1u) continue;        // uniform over the block
        const float* q = out + (int64_t)i * 5;
        const float ax1 = q[0], ay1 = q[1], ax2 = q[2], ay2 = q[3], aa = box_area(q);
        for (int j = i + 1 + t; j < n2; j += kThreads) {
            const float* r = out + (int64_t)j * 5;
            const float w = fmaxf(0.f, __fadd_rn(__fsub_rn(fminf(ax2, r[2]), fmaxf(ax1, r[0])), 1.f));
            const float h = fmaxf(0.f, __fadd_rn(__fsub_rn(fminf(ay2, r[3]), fmaxf(ay1, r[1])), 1.f));
            const float inter = __fmul_rn(w, h);
            const float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(aa, box_area(r)), inter));
            if (ovr > 0.3f) atomicOr(&sup[j >> 5], 1u << (j & 31));
        }
        __syncthreads();
    }
    __syncthreads();

    // the survivors move up in order: a chunk is read whole before any of it is written, and lands at or in front of itself
    int base = 0;
    for (int p0 = 0; p0 < n2; p0 += kThreads) {
        const int i = p0 + t;
        const bool keep = i < n2 && !((sup[i >> 5] >> (i & 31)) & 1u);
        float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        int src = 0;
        if (keep) {
#pragma unroll
            for (int k = 0; k < 5; ++k) v[k] = out[(int64_t)i * 5 + k];
            src = idx[i];
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wsum[wv] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kThreads / 64; ++k) {
            const int c = wsum[k];
            before += k < wv ? c : 0;
            all += c;
        }
        if (keep) {
            const int at = base + before + __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
            for (int k = 0; k < 5; ++k) out[(int64_t)at * 5 + k] = v[k];
            idx[at] = src;
        }
        base += all;
        __syncthreads();
    }
    // the rest of the row is defined: zero boxes, index -1
    for (int i = base + t; i < capacity; i += kThreads) {
#pragma unroll
        for (int k = 0; k < 5; ++k) out[(int64_t)i * 5 + k] = 0.f;
        idx[i] = -1;
    }
    if (t == 0) kept[b] = base;
}

// ------------------------------------------------------------------ host side
static int launch_conv(const ConvArgs& a0, int ks, bool head, float* part, hipStream_t st) {
    ConvArgs a = a0;
    // The number of K slices follows the output tiles, i.e. the layer, the image size and the row count, nothing else.
    const int M = a.R * a.Ho * a.Wo, bn = head ? 16 : 64;
    const ConvPlan p = plan_conv(M, a.N, a.K, bn, conv_tiles(M, a.N, bn));
    SGDFR_REQUIRE(p.S == 1 || p.S * p.out_elems <= kPartElems, "s3fd: split-K partials of %lld floats exceed the workspace",
                  (long long)(p.S * p.out_elems));
    a.cps = p.cps;
    a.part = part;
    a.part_elems = p.out_elems;
    const dim3 grid(p.mt, p.nt, p.S);
    if (ks == 3 && !head)
        hipLaunchKernelGGL((s3fd_conv_kernel<3, 64>), grid, dim3(kThreads), 0, st, a);
    else if (ks == 1 && !head)
        hipLaunchKernelGGL((s3fd_conv_kernel<1, 64>), grid, dim3(kThreads), 0, st, a);
    else if (ks == 3 && head)
        hipLaunchKernelGGL((s3fd_conv_kernel<3, 16>), grid, dim3(kThreads), 0, st, a);
    else
        SGDFR_REQUIRE(false, "s3fd: no conv instance for k=%d head=%d", ks, (int)head);
    if (check_launch("s3fd conv")) return 2;
    if (p.S > 1) {
        hipLaunchKernelGGL(s3fd_finish_kernel, dim3(grid_1d(p.out_elems)), dim3(kThreads), 0, st, a, p.S);
        if (check_launch("s3fd finish")) return 2;
    }
    return 0;
}

// workspace, float offsets: the split-K partials, two ping-pong maps of the largest layer output, the six head inputs, the three
// reciprocal norms, the six head outputs, and (for sgdfr_s3fd_forward_f32) nothing else: lists and counts are the caller's
struct WsLayout {
    int64_t part, a, b, tap[kLevels], rn[3], head[kLevels], total;
};
static WsLayout ws_layout(int rows, const Geo& g) {
    WsLayout w;
    int64_t o = align64(kPartElems);
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n * rows); return r; };
    w.part = 0;
    int64_t big = 0;
    for (int i = 0; i < kTrunk; ++i)
        if (kNet[i].level < 0) big = std::max(big, (int64_t)kNet[i].cout * g.ho[i] * g.wo[i]);
    w.a = take(big), w.b = take(big);
    for (int l = 0; l < kLevels; ++l) w.tap[l] = take((int64_t)kHeadC[l] * g.lh[l] * g.lw[l]);
    for (int l = 0; l < 3; ++l) w.rn[l] = take((int64_t)g.lh[l] * g.lw[l]);
    for (int l = 0; l < kLevels; ++l) w.head[l] = take((int64_t)(kHeadConf[l] + 4) * g.lh[l] * g.lw[l]);
    w.total = o;
    return w;
}

// debug stage outputs, each [rows, ...]: conv1_2, conv2_2, conv3_3, conv4_3, conv5_3, fc6, fc7, conv6_2, conv7_2 (all behind their
// ReLU, in front of a pool), then the reciprocal norms of conv3_3, conv4_3, conv5_3 [rows, h, w]
struct DebugLayout {
    int64_t tap[kDebugTaps], rn[3], total;
};
static DebugLayout debug_layout(int rows, const Geo& g) {
    DebugLayout d;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o += n * rows; return r; };
    for (int k = 0; k < kDebugTaps; ++k) {
        const int i = kDebugLayers[k];
        d.tap[k] = take((int64_t)kNet[i].cout * g.ho[i] * g.wo[i]);
    }
    for (int l = 0; l < 3; ++l) d.rn[l] = take((int64_t)g.lh[l] * g.lw[l]);
    d.total = o;
    return d;
}

static int64_t map_elems(int rows, const Geo& g) {
    int64_t n = 0;
    for (int l = 0; l < kLevels; ++l) n += 6LL * rows * g.lh[l] * g.lw[l];
    return n;
}

// image -> the six head outputs in the workspace (and the twelve maps / the debug taps when asked for)
static int run_network(const float* x, int R, int H, int W, int subtract_mean, const float* pack, float* maps, float* debug, float* wsf,
                       hipStream_t st) {
    const Geo g = geometry(H, W);
    const PackLayout pl = pack_layout();
    const WsLayout wl = ws_layout(R, g);
    const DebugLayout dl = debug_layout(R, g);
    float* part = wsf + wl.part;
    float* A = wsf + wl.a;
    float* B = wsf + wl.b;
    auto dump = [&](int64_t off, const float* src, int64_t count) {
        if (!debug) return 0;
        if (hipMemcpyAsync(debug + off, src, count * R * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
            set_error("s3fd_forward: debug copy failed");
            return 2;
        }
        return 0;
    };
    const float* cur = x;
    int dbg = 0;
    for (int i = 0; i < kTrunk; ++i) {
        const Layer& l = kNet[i];
        float* dst = l.level >= 0 ? wsf + wl.tap[l.level] : (cur == A ? B : A);
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.src = cur, a.wp = pack + pl.w[i], a.bias = pack + pl.b[i], a.out = dst;
        a.R = R, a.Hs = g.hi[i], a.Ws = g.wi[i], a.N = l.cout, a.Ho = g.ho[i], a.Wo = g.wo[i], a.K = l.cin * l.ks * l.ks;
        a.stride = l.stride, a.pad = l.pad, a.relu = 1;
        if (i == 0 && subtract_mean) a.has_sub = 1, a.sub0 = 104.f, a.sub1 = 117.f, a.sub2 = 123.f;
        if (launch_conv(a, l.ks, false, part, st)) return 2;
        cur = dst;
        if (dbg < kDebugTaps && kDebugLayers[dbg] == i) {
            if (dump(dl.tap[dbg], cur, (int64_t)l.cout * g.ho[i] * g.wo[i])) return 2;
            ++dbg;
        }
        if (l.pool) {
            float* pd = cur == A ? B : A;
            const int64_t planes = (int64_t)R * l.cout;
            hipLaunchKernelGGL(s3fd_pool_kernel, dim3(grid_1d(planes * (g.ho[i] / 2) * (g.wo[i] / 2))), dim3(kThreads), 0, st, cur, pd, planes,
                               g.ho[i], g.wo[i]);
            if (check_launch("s3fd pool")) return 2;
            cur = pd;
        }
    }
    int64_t mo = 0;
    for (int l = 0; l < kLevels; ++l) {
        const int plane = g.lh[l] * g.lw[l], N = kHeadConf[l] + 4;
        const float* tap = wsf + wl.tap[l];
        float* rn = nullptr;
        if (l < 3) {
            rn = wsf + wl.rn[l];
            hipLaunchKernelGGL(s3fd_rnorm_kernel, dim3(grid_1d((int64_t)R * plane)), dim3(kThreads), 0, st, tap, rn, R, kHeadC[l], plane);
            if (check_launch("s3fd rnorm")) return 2;
            if (dump(dl.rn[l], rn, plane)) return 2;
        }
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.src = tap, a.wp = pack + pl.hw[l], a.bias = pack + pl.hb[l], a.rn = rn, a.out = wsf + wl.head[l];
        a.R = R, a.Hs = a.Ho = g.lh[l], a.Ws = a.Wo = g.lw[l], a.N = N, a.K = 9 * kHeadC[l], a.stride = 1, a.pad = 1, a.relu = 0;
        if (launch_conv(a, 3, true, part, st)) return 2;
        if (maps) {
            float* cls = maps + mo;
            float* reg = cls + 2LL * R * plane;
            hipLaunchKernelGGL(s3fd_maps_kernel, dim3(grid_1d(6LL * R * plane)), dim3(kThreads), 0, st, wsf + wl.head[l], R, kHeadConf[l], plane,
                               cls, reg);
            if (check_launch("s3fd maps")) return 2;
            mo += 6LL * R * plane;
        }
    }
    return 0;
}

static int run_candidates(const Heads& hd, int rows, float threshold, int capacity, float* cand, int* count, int* valid, hipStream_t st) {
    hipLaunchKernelGGL(s3fd_candidates_kernel, dim3(rows), dim3(kThreads), 0, st, hd, threshold, capacity, cand, count, valid);
    return check_launch("s3fd candidates");
}

static int run_nms(const float* cand, const int* count, int rows, int capacity, float* boxes, int* index, int* kept, hipStream_t st) {
    hipLaunchKernelGGL(s3fd_nms_kernel, dim3(rows), dim3(kThreads), 0, st, cand, count, capacity, boxes, index, kept);
    return check_launch("s3fd nms");
}

static bool capacity_ok(int capacity) { return capacity >= 1 && capacity <= kMaxCapacity; }

}  // namespace
}  // namespace sgdfr

using namespace sgdfr;

extern "C" int64_t sgdfr_s3fd_pack_elems(void) { return pack_layout().total; }

extern "C" int sgdfr_s3fd_level_dims(int H, int W, int* hw) {
    SGDFR_REQUIRE(size_ok(1, H, W), "s3fd_level_dims: unsupported size %dx%d (each side 32..4096)", H, W);
    SGDFR_REQUIRE(hw, "s3fd_level_dims: null pointer");
    const Geo g = geometry(H, W);
    for (int l = 0; l < kLevels; ++l) hw[2 * l] = g.lh[l], hw[2 * l + 1] = g.lw[l];
    return 0;
}

extern "C" int64_t sgdfr_s3fd_debug_elems(int rows, int H, int W) {
    if (!size_ok(rows, H, W)) return -1;
    return debug_layout(rows, geometry(H, W)).total;
}

extern "C" int64_t sgdfr_s3fd_map_elems(int rows, int H, int W) {
    if (!size_ok(rows, H, W)) return -1;
    return map_elems(rows, geometry(H, W));
}

extern "C" int64_t sgdfr_s3fd_workspace_bytes(int rows, int H, int W) {
    if (!size_ok(rows, H, W)) return -1;
    return ws_layout(rows, geometry(H, W)).total * (int64_t)sizeof(float);
}

extern "C" int sgdfr_s3fd_prepack_f32(const float* const* params, float* pack, void* stream) {
    SGDFR_REQUIRE(params && pack, "s3fd_prepack: null pointer");
    for (int i = 0; i < kParams; ++i) SGDFR_REQUIRE(params[i], "s3fd_prepack: parameter %d is null", i);
    const PackLayout pl = pack_layout();
    hipStream_t st = as_stream(stream);
    auto seg = [&](const float* src, int64_t dst, int64_t count, int copy, int cin, int cout, int kk) {
        hipLaunchKernelGGL(s3fd_pack_kernel, dim3(grid_1d(count)), dim3(kThreads), 0, st, src, pack + dst, count, copy, cin, cout, kk);
        return check_launch("s3fd prepack");
    };
    int rc = 0;
    for (int i = 0; i < kTrunk && !rc; ++i) {
        const Layer& l = kNet[i];
        rc |= seg(params[2 * i], pl.w[i], (int64_t)l.cin * l.ks * l.ks * l.cout, 0, l.cin, l.cout, l.ks * l.ks);
        rc |= seg(params[2 * i + 1], pl.b[i], l.cout, 1, 0, 0, 0);
    }
    const float* const* T = params + 2 * kTrunk;
    for (int l = 0; l < kLevels && !rc; ++l) {
        const int N = kHeadConf[l] + 4;
        rc |= seg(T[2 * l], pl.hw[l], 9LL * kHeadC[l] * N, 0, kHeadC[l], N, 9);
        rc |= seg(T[2 * l + 1], pl.hb[l], N, 1, 0, 0, 0);
    }
    return rc ? 2 : 0;
}

#define S3FD_CHECK_SIZE(what)                                                                                                        \
    SGDFR_REQUIRE(size_ok(rows, H, W), what ": unsupported size (%d rows of %dx%d; 1..256 rows, each side 32..4096, rows*H*W <= 2^24)", \
                  rows, H, W)

extern "C" int sgdfr_s3fd_network_f32(const float* x, int rows, int H, int W, int subtract_mean, const float* pack, float* maps,
                                      float* debug, void* workspace, int64_t workspace_bytes, void* stream) {
    S3FD_CHECK_SIZE("s3fd_network");
    SGDFR_REQUIRE(x && pack && maps && workspace, "s3fd_network: null pointer");
    const int64_t need = ws_layout(rows, geometry(H, W)).total * (int64_t)sizeof(float);
    SGDFR_REQUIRE(need <= workspace_bytes, "s3fd_network: workspace of %lld bytes, %d rows of %dx%d need %lld", (long long)workspace_bytes,
                  rows, H, W, (long long)need);
    return run_network(x, rows, H, W, subtract_mean, pack, maps, debug, reinterpret_cast<float*>(workspace), as_stream(stream));
}

extern "C" int sgdfr_s3fd_candidates_f32(const float* const* heads, const int* hw, int rows, float threshold, int capacity, float* cand,
                                         int* count, int* valid, void* stream) {
    SGDFR_REQUIRE(rows_ok(rows), "s3fd_candidates: unsupported size (%d rows)", rows);
    SGDFR_REQUIRE(capacity_ok(capacity), "s3fd_candidates: capacity %d outside 1..%d", capacity, kMaxCapacity);
    SGDFR_REQUIRE(heads && hw && cand && count && valid, "s3fd_candidates: null pointer");
    int64_t total = 0;
    for (int l = 0; l < kLevels; ++l) {
        SGDFR_REQUIRE(heads[l], "s3fd_candidates: level %d is null", l);
        SGDFR_REQUIRE(hw[2 * l] >= 1 && hw[2 * l + 1] >= 1 && hw[2 * l] <= kMaxSide && hw[2 * l + 1] <= kMaxSide,
                      "s3fd_candidates: level %d has a map of %dx%d", l, hw[2 * l], hw[2 * l + 1]);
        total += (int64_t)hw[2 * l] * hw[2 * l + 1];
    }
    SGDFR_REQUIRE(total * rows <= kMaxPixels, "s3fd_candidates: %lld positions per image are too many", (long long)total);
    return run_candidates(make_heads(heads, hw), rows, threshold, capacity, cand, count, valid, as_stream(stream));
}

extern "C" int sgdfr_s3fd_nms_f32(const float* cand, const int* count, int rows, int capacity, float* boxes, int* index, int* kept,
                                  void* stream) {
    SGDFR_REQUIRE(rows_ok(rows), "s3fd_nms: unsupported size (%d rows)", rows);
    SGDFR_REQUIRE(capacity_ok(capacity), "s3fd_nms: capacity %d outside 1..%d", capacity, kMaxCapacity);
    SGDFR_REQUIRE(cand && count && boxes && index && kept, "s3fd_nms: null pointer");
    SGDFR_REQUIRE(cand != boxes, "s3fd_nms: boxes must not alias the candidates");
    return run_nms(cand, count, rows, capacity, boxes, index, kept, as_stream(stream));
}

extern "C" int sgdfr_s3fd_forward_f32(const float* x, int rows, int H, int W, int subtract_mean, const float* pack, float threshold,
                                      int capacity, float* cand, int* count, int* valid, float* boxes, int* index, int* kept, float* maps,
                                      float* debug, void* workspace, int64_t workspace_bytes, void* stream) {
    S3FD_CHECK_SIZE("s3fd_forward");
    SGDFR_REQUIRE(capacity_ok(capacity), "s3fd_forward: capacity %d outside 1..%d", capacity, kMaxCapacity);
    SGDFR_REQUIRE(x && pack && cand && count && valid && workspace, "s3fd_forward: null pointer");
    SGDFR_REQUIRE((boxes && index && kept) || (!boxes && !index && !kept), "s3fd_forward: boxes, index and kept come together");
    const Geo g = geometry(H, W);
    const WsLayout wl = ws_layout(rows, g);
    SGDFR_REQUIRE(wl.total * (int64_t)sizeof(float) <= workspace_bytes, "s3fd_forward: workspace of %lld bytes, %d rows of %dx%d need %lld",
                  (long long)workspace_bytes, rows, H, W, (long long)(wl.total * (int64_t)sizeof(float)));
    float* wsf = reinterpret_cast<float*>(workspace);
    hipStream_t st = as_stream(stream);
    if (run_network(x, rows, H, W, subtract_mean, pack, maps, debug, wsf, st)) return 2;
    const float* ptrs[kLevels];
    int hw[2 * kLevels];
    for (int l = 0; l < kLevels; ++l) ptrs[l] = wsf + wl.head[l], hw[2 * l] = g.lh[l], hw[2 * l + 1] = g.lw[l];
    if (run_candidates(make_heads(ptrs, hw), rows, threshold, capacity, cand, count, valid, st)) return 2;
    if (!boxes) return 0;
    return run_nms(cand, count, rows, capacity, boxes, index, kept, st);
}
