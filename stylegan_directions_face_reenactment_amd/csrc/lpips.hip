// LPIPS (AlexNet, v0.1) distance and its input gradient (libs/criteria/lpips/lpips.py:28-34, networks.py:53-63,78-85,
// utils.py:6-12): z-score, conv0 k11 s4 p2 + ReLU (tap 1), pool 3/2, conv3 k5 p2 + ReLU (tap 2), pool 3/2, conv6/8/10 k3 p1
// + ReLU (taps 3-5); per tap the channel-normalised squared difference weighted by the 1x1 `lin` heads, spatial mean, sum.
//
// Every conv (and every stride-1 input-gradient conv) is one implicit GEMM on exact-f32 MFMA (v_mfma_f32_16x16x4_f32): rows =
// output channels, columns = pixels, K = Cin*k*k gathered straight from the activation (z-score or the 3/2 max-pool fused into
// the load, zero padding after the z-score).  Layers with few output tiles split K; the slices land in a partial buffer and are
// summed in fixed order by the finish / pool-backward kernels.  No float atomics, no host sync, everything on the given stream.
#include <string.h>

#include <algorithm>

#include "common.h"

namespace sgdfr {
namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kLayers = 5;
constexpr int kCin[kLayers] = {3, 64, 192, 384, 256};
constexpr int kCout[kLayers] = {64, 192, 384, 256, 256};
constexpr int kKs[kLayers] = {11, 5, 3, 3, 3};
constexpr int kPad[kLayers] = {2, 2, 1, 1, 1};

constexpr int BM = 64, BN = 64, BK = 16, kThreads = 256;
enum { LOAD_PLAIN = 0, LOAD_ZSCORE = 1, LOAD_POOL = 2 };
enum { EPI_BIAS_RELU = 0, EPI_GRAD = 1, EPI_RAW = 2 };

// ------------------------------------------------------------------ geometry
struct Geom {
    int H, W;       // input image
    int h[kLayers], w[kLayers];   // tap t output size (taps 3..5 share the second pooled size)
    int ph1, pw1;   // pooled tap 1 (= tap 2 size)
    int ph2, pw2;   // pooled tap 2 (= taps 3-5 size)
};

static bool make_geom(int H, int W, Geom& g) {
    if (H < 31 || W < 31 || H > 4096 || W > 4096) return false;
    g.H = H, g.W = W;
    g.h[0] = (H + 4 - 11) / 4 + 1, g.w[0] = (W + 4 - 11) / 4 + 1;
    g.ph1 = (g.h[0] - 3) / 2 + 1, g.pw1 = (g.w[0] - 3) / 2 + 1;
    g.h[1] = g.ph1, g.w[1] = g.pw1;
    g.ph2 = (g.h[1] - 3) / 2 + 1, g.pw2 = (g.w[1] - 3) / 2 + 1;
    for (int t = 2; t < kLayers; ++t) g.h[t] = g.ph2, g.w[t] = g.pw2;
    return g.ph2 >= 1 && g.pw2 >= 1;
}

static int64_t tap_elems(const Geom& g, int t) { return (int64_t)kCout[t] * g.h[t] * g.w[t]; }   // per image
static int64_t feat_elems_per_row(const Geom& g) {
    int64_t s = 0;
    for (int t = 0; t < kLayers; ++t) s += tap_elems(g, t);
    return s;
}
// tap t of a feature buffer of `rows` images: [rows, C_t, h_t, w_t], taps one after the other
static int64_t tap_offset(const Geom& g, int rows, int t) {
    int64_t s = 0;
    for (int u = 0; u < t; ++u) s += (int64_t)rows * tap_elems(g, u);
    return s;
}

// ------------------------------------------------------------------ weight pack
// fwd weights [K][Cout] per layer, input-gradient weights [Cout*k*k][Cin] (taps flipped) of layers 1..4, conv0's weight as is,
// biases, mean, std, lin
struct PackLayout {
    int64_t wf[kLayers], wd[kLayers], w0, bias[kLayers], mean, std_, lin[kLayers], total;
};
static int64_t align64(int64_t v) { return (v + 63) & ~(int64_t)63; }
static PackLayout pack_layout() {
    PackLayout p;
    int64_t o = 0;
    for (int l = 0; l < kLayers; ++l) {
        p.wf[l] = o;
        o = align64(o + (int64_t)kCin[l] * kKs[l] * kKs[l] * kCout[l]);
    }
    p.wd[0] = -1;
    for (int l = 1; l < kLayers; ++l) {
        p.wd[l] = o;
        o = align64(o + (int64_t)kCin[l] * kKs[l] * kKs[l] * kCout[l]);
    }
    p.w0 = o;
    o = align64(o + (int64_t)kCin[0] * kKs[0] * kKs[0] * kCout[0]);
    for (int l = 0; l < kLayers; ++l) {
        p.bias[l] = o;
        o = align64(o + kCout[l]);
    }
    p.mean = o, o = align64(o + 3);
    p.std_ = o, o = align64(o + 3);
    for (int l = 0; l < kLayers; ++l) {
        p.lin[l] = o;
        o += kCout[l];
    }
    p.total = align64(o);
    return p;
}

enum { SEG_COPY = 0, SEG_FWD = 1, SEG_DGRAD = 2 };
constexpr int kSegs = 22;
struct PackSeg {
    const float* src;
    int64_t dst, count;
    int kind, cin, cout, ks;
};
struct PackArgs {
    PackSeg s[kSegs];
    float* pack;
    int64_t total;
};
static_assert(sizeof(PackArgs) < 4096, "prepack kernel arguments must stay below 4 KB");

__global__ __launch_bounds__(kThreads) void lpips_pack_kernel(PackArgs a) {
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.total; e += (int64_t)gridDim.x * kThreads) {
        int si = -1;
        for (int i = 0; i < kSegs; ++i)
            if (e >= a.s[i].dst && e < a.s[i].dst + a.s[i].count) si = i;
        if (si < 0) {
            a.pack[e] = 0.f;        // alignment padding
            continue;
        }
        const PackSeg& s = a.s[si];
        const int64_t j = e - s.dst;
        float v;
        if (s.kind == SEG_COPY) {
            v = s.src[j];
        } else if (s.kind == SEG_FWD) {   // [k = (ci*ks + kh)*ks + kw][co] <- W[co][ci][kh][kw]
            const int64_t K = (int64_t)s.cin * s.ks * s.ks;
            const int64_t k = j / s.cout, co = j % s.cout;
            v = s.src[co * K + k];
        } else {                            // [(co*ks + kh)*ks + kw][ci] <- W[co][ci][ks-1-kh][ks-1-kw]
            const int kk = s.ks * s.ks;
            const int64_t row = j / s.cin, ci = j % s.cin;
            const int64_t co = row / kk;
            const int r = (int)(row % kk), kh = r / s.ks, kw = r % s.ks;
            v = s.src[((co * s.cin + ci) * s.ks + (s.ks - 1 - kh)) * s.ks + (s.ks - 1 - kw)];
        }
        a.pack[e] = v;
    }
}

// ------------------------------------------------------------------ implicit-GEMM conv
struct ConvArgs {
    const float* src;    // [rows, Cin, Hs, Ws]; rows >= r_split come from src2 (the live target of a two-input forward)
    const float* src2;
    const float* wp;     // [K][N]
    const float* bias;   // EPI_BIAS_RELU
    const float* mask;   // EPI_GRAD: forward activation [R, N, Ho, Wo] (ReLU mask: > 0)
    const float* gadd;   // EPI_GRAD: masked tap gradient, same layout
    const float* mean;   // LOAD_ZSCORE
    const float* stdv;
    float* out;          // S == 1 and epi != RAW: [R,N,Ho,Wo]; else partials [S][R,N,Ho,Wo]
    int64_t out_elems;
    int R, r_split, Cin, Hs, Ws, Hin, Win, N, Ho, Wo, K, stride, pad, cps, epi;
};
static_assert(sizeof(ConvArgs) < 4096, "conv kernel arguments must stay below 4 KB");

// first maximum in row-major window order, strict '>' (NaN wins), as PyTorch's max_pool2d kernels pick it
__device__ __forceinline__ float pool_max(const float* plane, int Ws, int y0, int x0, int* arg) {
    float best = -INFINITY;
    int bi = y0 * Ws + x0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int idx = (y0 + i) * Ws + x0 + j;
            const float v = plane[idx];
            if (v > best || __builtin_isnan(v)) best = v, bi = idx;
        }
    if (arg) *arg = bi;
    return best;
}

template <int KS, int LOAD>
__global__ __launch_bounds__(kThreads) void lpips_conv_kernel(ConvArgs a) {
    __shared__ float xs[BK][BM + 4];    // pixels (MFMA B operand / columns)
    __shared__ float ws[BK][BN + 4];    // output channels (MFMA A operand / rows)
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN, split = blockIdx.z;
    const int HWo = a.Ho * a.Wo, M = a.R * HWo;
    const int64_t plane = (int64_t)a.Hs * a.Ws;

    // the pixel this thread gathers (fixed over K)
    const int lm = t & (BM - 1), gm = m0 + lm;
    const bool mvalid = gm < M;
    int b = 0, oh = 0, ow = 0;
    if (mvalid) {
        b = gm / HWo;
        const int p = gm - b * HWo;
        oh = p / a.Wo;
        ow = p - oh * a.Wo;
    }
    const int ih0 = oh * a.stride - a.pad, iw0 = ow * a.stride - a.pad;
    const float* srcb = b < a.r_split ? a.src + (int64_t)b * a.Cin * plane : a.src2 + (int64_t)(b - a.r_split) * a.Cin * plane;

    const int nchunks = (a.K + BK - 1) / BK;
    const int c0 = split * a.cps, c1 = min(nchunks, c0 + a.cps);
    const int wm = wv & 1, wn = wv >> 1;
    floatx4 acc[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    for (int c = c0; c < c1; ++c) {
        const int k0 = c * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = (t >> 6) + 4 * i, k = k0 + kk;
            float v = 0.f;
            if (mvalid && k < a.K) {
                const int ci = k / (KS * KS), r = k - ci * (KS * KS), kh = r / KS, kw = r - kh * KS;
                const int ih = ih0 + kh, iw = iw0 + kw;
                if (ih >= 0 && ih < a.Hin && iw >= 0 && iw < a.Win) {
                    const float* pl = srcb + ci * plane;
                    if (LOAD == LOAD_POOL) {
                        v = pool_max(pl, a.Ws, 2 * ih, 2 * iw, nullptr);
                    } else if (LOAD == LOAD_ZSCORE) {
                        v = (pl[ih * a.Ws + iw] - a.mean[ci]) / a.stdv[ci];
                    } else {
                        v = pl[ih * a.Ws + iw];
                    }
                }
            }
            xs[kk][lm] = v;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = t + kThreads * i, n = e & (BN - 1), kk = e >> 6;
            const int k = k0 + kk, gn = n0 + n;
            ws[kk][n] = (k < a.K && gn < a.N) ? a.wp[(int64_t)k * a.N + gn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < BK; ks += 4) {
            const int kr = ks + (lane >> 4);
            float wa[2], xa[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) wa[i] = ws[kr][wn * 32 + i * 16 + (lane & 15)];
            for (int j = 0; j < 2; ++j) xa[j] = xs[kr][wm * 32 + j * 16 + (lane & 15)];
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[i], xa[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // D[row = channel][col = pixel]: lane holds channel (lane>>4)*4 + r of a 16-row block, pixel lane&15
    const bool raw = gridDim.z > 1 || a.epi == EPI_RAW;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int gp = m0 + wm * 32 + j * 16 + (lane & 15);
        if (gp >= M) continue;
        const int bb = gp / HWo, p = gp - bb * HWo;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gn = n0 + wn * 32 + i * 16 + (lane >> 4) * 4 + r;
                if (gn >= a.N) continue;
                const int64_t idx = ((int64_t)bb * a.N + gn) * HWo + p;
                const float v = acc[i][j][r];
                if (raw)
                    a.out[(int64_t)split * a.out_elems + idx] = v;
                else if (a.epi == EPI_BIAS_RELU)
                    a.out[idx] = fmaxf(v + a.bias[gn], 0.f);
                else
                    a.out[idx] = (a.mask[idx] > 0.f ? v : 0.f) + a.gadd[idx];
            }
    }
}

// sum of the K slices in fixed order + the conv's epilogue
__global__ __launch_bounds__(kThreads) void lpips_finish_kernel(const float* __restrict__ part, int S, int64_t n, int N, int HW, int epi,
                                                                 const float* __restrict__ bias, const float* __restrict__ mask,
                                                                 const float* __restrict__ gadd, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        float v = part[i];
        for (int s = 1; s < S; ++s) v += part[(int64_t)s * n + i];
        if (epi == EPI_BIAS_RELU)
            out[i] = fmaxf(v + bias[(i / HW) % N], 0.f);
        else
            out[i] = (mask[i] > 0.f ? v : 0.f) + gadd[i];
    }
}

// max-pool 3/2 backward as a gather: each element of the pooled conv's input [B,C,Hs,Ws] collects the pooled gradient (S slices,
// summed in order) of every window (up to four) whose first maximum it is; then the ReLU mask of f and the tap's own gradient
__global__ __launch_bounds__(kThreads) void lpips_pool_bwd_kernel(const float* __restrict__ dpool, int S, const float* __restrict__ f,
                                                                  const float* __restrict__ gadd, float* __restrict__ out, int B, int C,
                                                                  int Hs, int Ws, int P, int Q) {
    const int64_t n = (int64_t)B * C * Hs * Ws, np = (int64_t)B * C * P * Q;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const int w = (int)(i % Ws), h = (int)((i / Ws) % Hs);
        const int64_t bc = i / ((int64_t)Hs * Ws);
        const float* pl = f + bc * Hs * Ws;
        const int me = h * Ws + w;
        float g = 0.f;
        const int py0 = h >= 2 ? (h - 1) / 2 : 0, py1 = min(P - 1, h / 2);
        const int px0 = w >= 2 ? (w - 1) / 2 : 0, px1 = min(Q - 1, w / 2);
        for (int py = py0; py <= py1; ++py)
            for (int px = px0; px <= px1; ++px) {
                int arg;
                pool_max(pl, Ws, 2 * py, 2 * px, &arg);
                if (arg != me) continue;
                const int64_t j = (bc * P + py) * Q + px;
                float d = dpool[j];
                for (int s = 1; s < S; ++s) d += dpool[(int64_t)s * np + j];
                g += d;
            }
        out[i] = (pl[me] > 0.f ? g : 0.f) + gadd[i];
    }
}

// dL/dx of conv0 (3 output channels, stride 4, 11x11) as a gather per input pixel, then the z-score adjoint (/ std)
__global__ __launch_bounds__(kThreads) void lpips_dgrad0_kernel(const float* __restrict__ g1, const float* __restrict__ w0,
                                                                const float* __restrict__ stdv, float* __restrict__ dx, int B, int H,
                                                                int W, int H1, int W1) {
    const int64_t n = (int64_t)B * H * W;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const int iw = (int)(i % W), ih = (int)((i / W) % H), b = (int)(i / ((int64_t)H * W));
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int kh = (ih + 2) & 3; kh < 11; kh += 4) {
            const int dy = ih + 2 - kh;
            if (dy < 0) break;
            const int oh = dy >> 2;
            if (oh >= H1) continue;
            for (int kw = (iw + 2) & 3; kw < 11; kw += 4) {
                const int dxw = iw + 2 - kw;
                if (dxw < 0) break;
                const int ow = dxw >> 2;
                if (ow >= W1) continue;
                const float* gp = g1 + ((int64_t)b * 64 * H1 + oh) * W1 + ow;
                const float* wp = w0 + kh * 11 + kw;
                for (int co = 0; co < 64; ++co) {
                    const float g = gp[(int64_t)co * H1 * W1];
                    s0 = fmaf(wp[(co * 3 + 0) * 121], g, s0);
                    s1 = fmaf(wp[(co * 3 + 1) * 121], g, s1);
                    s2 = fmaf(wp[(co * 3 + 2) * 121], g, s2);
                }
            }
        }
        const int64_t o = (int64_t)b * 3 * H * W + (int64_t)ih * W + iw;
        dx[o] = s0 / stdv[0];
        dx[o + (int64_t)H * W] = s1 / stdv[1];
        dx[o + 2 * (int64_t)H * W] = s2 / stdv[2];
    }
}

// ------------------------------------------------------------------ taps
struct TapArgs {
    const float* fx[kLayers];    // tap t of x, image 0
    const float* fy[kLayers];    // tap t of y, image y_row0
    float* gtap[kLayers];        // backward: masked dL/df of x's taps [B, C, h, w]
    const float* lin;            // pack: lin heads of all taps
    const float* gl;             // backward: dL/dloss (device scalar)
    float* part;                 // forward: one partial sum per block
    int C[kLayers], HW[kLayers], lin_off[kLayers], blk0[kLayers + 1];
    float wgt[kLayers];          // 1 / (B * h_t * w_t)
    int B, ybcast;
};
static_assert(sizeof(TapArgs) < 4096, "tap kernel arguments must stay below 4 KB");

__device__ __forceinline__ int tap_of_block(const TapArgs& a, int blk) {
    int t = 0;
    for (int u = 1; u < kLayers; ++u)
        if (blk >= a.blk0[u]) t = u;
    return t;
}

// per pixel: n = f / (sqrt(sum_c f^2 + 1e-9) + 1e-10); d = sum_c lin[c] (n_x - n_y)^2, weighted by 1/(B*h*w); block partial sums
__global__ __launch_bounds__(kThreads) void lpips_tap_fwd_kernel(TapArgs a) {
    __shared__ float red[kThreads / kWave];
    const int t = tap_of_block(a, blockIdx.x);
    const int C = a.C[t], HW = a.HW[t];
    const int j = (blockIdx.x - a.blk0[t]) * kThreads + threadIdx.x;
    float val = 0.f;
    if (j < a.B * HW) {
        const int b = j / HW, p = j - b * HW;
        const float* x = a.fx[t] + (int64_t)b * C * HW + p;
        const float* y = a.fy[t] + (int64_t)(a.ybcast ? 0 : b) * C * HW + p;
        const float* lin = a.lin + a.lin_off[t];
        float sx = 0.f, sy = 0.f;
        for (int c = 0; c < C; ++c) {
            const float u = x[(int64_t)c * HW], v = y[(int64_t)c * HW];
            sx = fmaf(u, u, sx);
            sy = fmaf(v, v, sy);
        }
        const float dx = sqrtf(sx + 1e-9f) + 1e-10f, dy = sqrtf(sy + 1e-9f) + 1e-10f;
        float d = 0.f;
        for (int c = 0; c < C; ++c) {
            const float e = x[(int64_t)c * HW] / dx - y[(int64_t)c * HW] / dy;
            d = fmaf(lin[c], e * e, d);
        }
        val = d * a.wgt[t];
    }
    val = wave_sum(val);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = val;
    __syncthreads();
    if (threadIdx.x == 0) a.part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(kThreads) void lpips_sum_kernel(const float* __restrict__ part, int n, float* __restrict__ loss) {
    __shared__ float red[kThreads / kWave];
    float v = 0.f;
    for (int i = threadIdx.x; i < n; i += kThreads) v += part[i];
    v = wave_sum(v);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

// adjoint of the tap head per pixel of x: g_n = gl * wgt * 2 lin (n_x - n_y); g_f = g_n/den - f (f.g_n) / (den^2 r); ReLU mask
__global__ __launch_bounds__(kThreads) void lpips_tap_bwd_kernel(TapArgs a) {
    const int t = tap_of_block(a, blockIdx.x);
    const int C = a.C[t], HW = a.HW[t];
    const int j = (blockIdx.x - a.blk0[t]) * kThreads + threadIdx.x;
    if (j >= a.B * HW) return;
    const int b = j / HW, p = j - b * HW;
    const int64_t xo = (int64_t)b * C * HW + p;
    const float* x = a.fx[t] + xo;
    const float* y = a.fy[t] + (int64_t)(a.ybcast ? 0 : b) * C * HW + p;
    const float* lin = a.lin + a.lin_off[t];
    float* g = a.gtap[t] + xo;
    const float scale = 2.f * a.gl[0] * a.wgt[t];
    float sx = 0.f, sy = 0.f;
    for (int c = 0; c < C; ++c) {
        const float u = x[(int64_t)c * HW], v = y[(int64_t)c * HW];
        sx = fmaf(u, u, sx);
        sy = fmaf(v, v, sy);
    }
    const float rx = sqrtf(sx + 1e-9f), dx = rx + 1e-10f, dy = sqrtf(sy + 1e-9f) + 1e-10f;
    float dot = 0.f;
    for (int c = 0; c < C; ++c) {
        const float u = x[(int64_t)c * HW];
        const float gn = scale * lin[c] * (u / dx - y[(int64_t)c * HW] / dy);
        dot = fmaf(u, gn, dot);
    }
    const float k2 = dot / (dx * dx * rx);
    for (int c = 0; c < C; ++c) {
        const float u = x[(int64_t)c * HW];
        const float gn = scale * lin[c] * (u / dx - y[(int64_t)c * HW] / dy);
        g[(int64_t)c * HW] = u > 0.f ? gn / dx - u * k2 : 0.f;
    }
}

// ------------------------------------------------------------------ host side
int grid_1d(int64_t n) { return (int)std::min<int64_t>((n + kThreads - 1) / kThreads, 4096); }

struct ConvPlan {
    int S, cps, mt, nt;
    int64_t out_elems;
};
static ConvPlan plan_conv(int R, int N, int Ho, int Wo, int K, bool allow_split) {
    ConvPlan p;
    const int M = R * Ho * Wo;
    p.mt = (M + BM - 1) / BM, p.nt = (N + BN - 1) / BN;
    const int nchunks = (K + BK - 1) / BK, tiles = p.mt * p.nt;
    int S = allow_split ? std::min(512 / std::max(tiles, 1), nchunks / 6) : 1;
    S = std::max(1, std::min(S, 16));
    p.cps = (nchunks + S - 1) / S;
    p.S = (nchunks + p.cps - 1) / p.cps;
    p.out_elems = (int64_t)M * N;
    return p;
}

// the convs of one call: layer l forward (dgrad = false) on R rows, or its input-gradient conv (l >= 1) on R rows
static ConvPlan layer_plan(const Geom& g, int l, int R, bool dgrad) {
    const int N = dgrad ? kCin[l] : kCout[l];
    const int K = (dgrad ? kCout[l] : kCin[l]) * kKs[l] * kKs[l];
    const int Ho = dgrad ? (l == 1 ? g.ph1 : g.ph2) : g.h[l], Wo = dgrad ? (l == 1 ? g.pw1 : g.pw2) : g.w[l];
    return plan_conv(R, N, Ho, Wo, K, dgrad || l > 0);
}

struct WsLayout {
    int64_t part, gtap, bufa, bufb, tpart, total;   // float offsets
    int tap_blocks;
};
static int tap_blocks(const Geom& g, int B, int* blk0) {
    int s = 0;
    for (int t = 0; t < kLayers; ++t) {
        if (blk0) blk0[t] = s;
        s += (int)(((int64_t)B * g.h[t] * g.w[t] + kThreads - 1) / kThreads);
    }
    if (blk0) blk0[kLayers] = s;
    return s;
}
static WsLayout ws_layout(const Geom& g, int B) {
    WsLayout w;
    int64_t part = 0, maxchw = 0;
    for (int l = 0; l < kLayers; ++l) {
        for (int R = B; R <= 2 * B; R += B) {
            const ConvPlan f = layer_plan(g, l, R, false);
            part = std::max(part, f.S * f.out_elems);
        }
        if (l >= 1) {
            const ConvPlan d = layer_plan(g, l, B, true);
            part = std::max(part, d.S * d.out_elems);
        }
        maxchw = std::max(maxchw, tap_elems(g, l));
    }
    w.tap_blocks = tap_blocks(g, B, nullptr);
    int64_t o = 0;
    w.part = o, o = align64(o + part);
    w.gtap = o, o = align64(o + (int64_t)B * feat_elems_per_row(g));
    w.bufa = o, o = align64(o + (int64_t)B * maxchw);
    w.bufb = o, o = align64(o + (int64_t)B * maxchw);
    w.tpart = o, o = align64(o + w.tap_blocks);
    w.total = o;
    return w;
}

static int launch_conv(const ConvArgs& a0, const ConvPlan& p, int ks, int load, hipStream_t st) {
    ConvArgs a = a0;
    a.cps = p.cps;
    a.out_elems = p.out_elems;
    const dim3 grid(p.mt, p.nt, p.S);
#define SGDFR_LPIPS_CONV(KS_, LD_)                                                           \
    if (ks == KS_ && load == LD_) {                                                           \
        hipLaunchKernelGGL((lpips_conv_kernel<KS_, LD_>), grid, dim3(kThreads), 0, st, a);    \
        return check_launch("lpips conv");                                                    \
    }
    SGDFR_LPIPS_CONV(11, LOAD_ZSCORE)
    SGDFR_LPIPS_CONV(5, LOAD_POOL)
    SGDFR_LPIPS_CONV(3, LOAD_POOL)
    SGDFR_LPIPS_CONV(3, LOAD_PLAIN)
    SGDFR_LPIPS_CONV(5, LOAD_PLAIN)
#undef SGDFR_LPIPS_CONV
    set_error("lpips: no conv instance for k=%d load=%d", ks, load);
    return 1;
}

static int launch_finish(const float* part, const ConvPlan& p, int N, int HW, int epi, const float* bias, const float* mask,
                         const float* gadd, float* out, hipStream_t st) {
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(grid_1d(p.out_elems)), dim3(kThreads), 0, st, part, p.S, p.out_elems, N, HW, epi,
                       bias, mask, gadd, out);
    return check_launch("lpips finish");
}

static void fill_taps(TapArgs& ta, const Geom& g, const PackLayout& pl, const float* pack, const float* fx, int rows_x, const float* fy,
                      int rows_y, int y_row0, int B, int y_bcast) {
    memset(&ta, 0, sizeof(ta));
    tap_blocks(g, B, ta.blk0);
    for (int t = 0; t < kLayers; ++t) {
        ta.fx[t] = fx + tap_offset(g, rows_x, t);
        ta.fy[t] = fy + tap_offset(g, rows_y, t) + (int64_t)y_row0 * tap_elems(g, t);
        ta.C[t] = kCout[t];
        ta.HW[t] = g.h[t] * g.w[t];
        ta.lin_off[t] = (int)(pl.lin[t] - pl.lin[0]);
        ta.wgt[t] = (float)(1.0 / ((double)B * g.h[t] * g.w[t]));
    }
    ta.lin = pack + pl.lin[0];
    ta.B = B;
    ta.ybcast = y_bcast;
}

static int check_pair(const Geom& g, const float* fx, int rows_x, const float* fy, int rows_y, int y_row0, int B, int y_bcast) {
    (void)g;
    SGDFR_REQUIRE(fx && fy, "lpips: null feature buffer");
    SGDFR_REQUIRE(B >= 1 && rows_x >= B, "lpips: B=%d with %d x rows", B, rows_x);
    SGDFR_REQUIRE(y_bcast == 0 || y_bcast == 1, "lpips: y_bcast must be 0 or 1");
    SGDFR_REQUIRE(y_row0 >= 0 && y_row0 + (y_bcast ? 1 : B) <= rows_y, "lpips: y rows %d..%d outside the %d rows of the y features",
                  y_row0, y_row0 + (y_bcast ? 1 : B), rows_y);
    return 0;
}

}  // namespace
}  // namespace sgdfr

using namespace sgdfr;

extern "C" int64_t sgdfr_lpips_pack_elems(void) { return pack_layout().total; }

extern "C" int64_t sgdfr_lpips_feature_elems(int rows, int H, int W) {
    Geom g;
    if (rows < 1 || !make_geom(H, W, g)) return -1;
    return (int64_t)rows * feat_elems_per_row(g);
}

extern "C" int64_t sgdfr_lpips_workspace_bytes(int B, int H, int W) {
    Geom g;
    if (B < 1 || !make_geom(H, W, g)) return -1;
    return ws_layout(g, B).total * (int64_t)sizeof(float);
}

extern "C" int sgdfr_lpips_prepack_f32(const float* const* params, float* pack, void* stream) {
    SGDFR_REQUIRE(params && pack, "lpips_prepack: null pointer");
    for (int i = 0; i < 17; ++i) SGDFR_REQUIRE(params[i], "lpips_prepack: parameter %d is null", i);
    const PackLayout pl = pack_layout();
    PackArgs a;
    memset(&a, 0, sizeof(a));
    int s = 0;
    for (int l = 0; l < kLayers; ++l) {
        const int64_t n = (int64_t)kCin[l] * kKs[l] * kKs[l] * kCout[l];
        a.s[s++] = PackSeg{params[2 * l], pl.wf[l], n, SEG_FWD, kCin[l], kCout[l], kKs[l]};
        if (l >= 1) a.s[s++] = PackSeg{params[2 * l], pl.wd[l], n, SEG_DGRAD, kCin[l], kCout[l], kKs[l]};
        else a.s[s++] = PackSeg{params[0], pl.w0, n, SEG_COPY, 0, 0, 0};
        a.s[s++] = PackSeg{params[2 * l + 1], pl.bias[l], kCout[l], SEG_COPY, 0, 0, 0};
    }
    a.s[s++] = PackSeg{params[10], pl.mean, 3, SEG_COPY, 0, 0, 0};
    a.s[s++] = PackSeg{params[11], pl.std_, 3, SEG_COPY, 0, 0, 0};
    for (int l = 0; l < kLayers; ++l) a.s[s++] = PackSeg{params[12 + l], pl.lin[l], kCout[l], SEG_COPY, 0, 0, 0};
    SGDFR_REQUIRE(s == kSegs, "lpips_prepack: %d segments", s);
    a.pack = pack;
    a.total = pl.total;
    hipLaunchKernelGGL(lpips_pack_kernel, dim3(grid_1d(pl.total)), dim3(kThreads), 0, as_stream(stream), a);
    return check_launch("lpips prepack");
}

extern "C" int sgdfr_lpips_features_f32(const float* x, int rows_x, const float* y, int rows_y, int H, int W, const float* pack,
                                        float* feats, void* workspace, int64_t workspace_bytes, void* stream) {
    Geom g;
    SGDFR_REQUIRE(make_geom(H, W, g), "lpips: unsupported image size %dx%d (31..4096 per side)", H, W);
    SGDFR_REQUIRE(x && rows_x >= 1 && rows_y >= 0 && (rows_y == 0 || y), "lpips_features: bad inputs (rows %d + %d)", rows_x, rows_y);
    SGDFR_REQUIRE(pack && feats && workspace, "lpips_features: null pointer");
    const int R = rows_x + rows_y;
    const PackLayout pl = pack_layout();
    int64_t need = 0;
    for (int l = 0; l < kLayers; ++l) {
        const ConvPlan p = layer_plan(g, l, R, false);
        if (p.S > 1) need = std::max(need, p.S * p.out_elems);
    }
    SGDFR_REQUIRE(need * (int64_t)sizeof(float) <= workspace_bytes, "lpips_features: workspace of %lld bytes, %d rows need %lld",
                  (long long)workspace_bytes, R, (long long)(need * (int64_t)sizeof(float)));
    float* part = reinterpret_cast<float*>(workspace);     // the partial region sits at offset 0 of every layout
    hipStream_t st = as_stream(stream);
    const float* src = x;
    for (int l = 0; l < kLayers; ++l) {
        const ConvPlan p = layer_plan(g, l, R, false);
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        float* out = feats + tap_offset(g, R, l);
        a.src = src;
        a.src2 = src;
        a.r_split = R;
        a.wp = pack + pl.wf[l];
        a.bias = pack + pl.bias[l];
        a.R = R, a.Cin = kCin[l], a.N = kCout[l], a.Ho = g.h[l], a.Wo = g.w[l];
        a.K = kCin[l] * kKs[l] * kKs[l], a.stride = l == 0 ? 4 : 1, a.pad = kPad[l];
        a.epi = EPI_BIAS_RELU;
        a.out = p.S > 1 ? part : out;
        int load = LOAD_PLAIN;
        if (l == 0) {
            load = LOAD_ZSCORE;
            a.src2 = y, a.r_split = rows_x;
            a.mean = pack + pl.mean, a.stdv = pack + pl.std_;
            a.Hs = a.Hin = H, a.Ws = a.Win = W;
        } else if (l <= 2) {
            load = LOAD_POOL;
            a.Hs = g.h[l - 1], a.Ws = g.w[l - 1];
            a.Hin = l == 1 ? g.ph1 : g.ph2, a.Win = l == 1 ? g.pw1 : g.pw2;
        } else {
            a.Hs = a.Hin = g.h[l - 1], a.Ws = a.Win = g.w[l - 1];
        }
        if (launch_conv(a, p, kKs[l], load, st)) return 2;
        if (p.S > 1 && launch_finish(part, p, kCout[l], g.h[l] * g.w[l], EPI_BIAS_RELU, a.bias, nullptr, nullptr, out, st)) return 2;
        src = out;
    }
    return 0;
}

extern "C" int sgdfr_lpips_distance_f32(const float* fx, int rows_x, const float* fy, int rows_y, int y_row0, int y_bcast, int B, int H,
                                        int W, const float* pack, float* loss, void* workspace, int64_t workspace_bytes, void* stream) {
    Geom g;
    SGDFR_REQUIRE(make_geom(H, W, g), "lpips: unsupported image size %dx%d (31..4096 per side)", H, W);
    if (check_pair(g, fx, rows_x, fy, rows_y, y_row0, B, y_bcast)) return 1;
    SGDFR_REQUIRE(pack && loss && workspace, "lpips_distance: null pointer");
    const PackLayout pl = pack_layout();
    const WsLayout wl = ws_layout(g, B);
    SGDFR_REQUIRE(wl.total * (int64_t)sizeof(float) <= workspace_bytes, "lpips: workspace of %lld bytes, B=%d needs %lld",
                  (long long)workspace_bytes, B, (long long)(wl.total * (int64_t)sizeof(float)));
    TapArgs ta;
    fill_taps(ta, g, pl, pack, fx, rows_x, fy, rows_y, y_row0, B, y_bcast);
    ta.part = reinterpret_cast<float*>(workspace) + wl.tpart;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(lpips_tap_fwd_kernel, dim3(wl.tap_blocks), dim3(kThreads), 0, st, ta);
    if (check_launch("lpips taps")) return 2;
    hipLaunchKernelGGL(lpips_sum_kernel, dim3(1), dim3(kThreads), 0, st, ta.part, wl.tap_blocks, loss);
    return check_launch("lpips sum");
}

extern "C" int sgdfr_lpips_backward_f32(const float* grad_loss, const float* fx, int rows_x, const float* fy, int rows_y, int y_row0,
                                        int y_bcast, int B, int H, int W, const float* pack, float* dx, void* workspace, int64_t workspace_bytes, void* stream) {
    Geom g;
    SGDFR_REQUIRE(make_geom(H, W, g), "lpips: unsupported image size %dx%d (31..4096 per side)", H, W);
    if (check_pair(g, fx, rows_x, fy, rows_y, y_row0, B, y_bcast)) return 1;
    SGDFR_REQUIRE(grad_loss && pack && dx && workspace, "lpips_backward: null pointer");
    const PackLayout pl = pack_layout();
    const WsLayout wl = ws_layout(g, B);
    SGDFR_REQUIRE(wl.total * (int64_t)sizeof(float) <= workspace_bytes, "lpips: workspace of %lld bytes, B=%d needs %lld",
                  (long long)workspace_bytes, B, (long long)(wl.total * (int64_t)sizeof(float)));
    float* wsf = reinterpret_cast<float*>(workspace);
    float* part = wsf + wl.part;
    float* gtap = wsf + wl.gtap;
    float* bufs[2] = {wsf + wl.bufa, wsf + wl.bufb};
    hipStream_t st = as_stream(stream);

    TapArgs ta;
    fill_taps(ta, g, pl, pack, fx, rows_x, fy, rows_y, y_row0, B, y_bcast);
    for (int t = 0; t < kLayers; ++t) ta.gtap[t] = gtap + tap_offset(g, B, t);
    ta.gl = grad_loss;
    hipLaunchKernelGGL(lpips_tap_bwd_kernel, dim3(wl.tap_blocks), dim3(kThreads), 0, st, ta);
    if (check_launch("lpips tap backward")) return 2;

    // the gradient at tap l+1 (full: own head + everything above, masked) -> at tap l through conv l+1's input-gradient conv
    const float* gin = ta.gtap[4];
    for (int l = 4; l >= 1; --l) {
        const ConvPlan p = layer_plan(g, l, B, true);
        const int Hi = l == 1 ? g.ph1 : g.ph2, Wi = l == 1 ? g.pw1 : g.pw2;
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.src = a.src2 = gin;
        a.r_split = B;
        a.wp = pack + pl.wd[l];
        a.R = B, a.Cin = kCout[l], a.N = kCin[l], a.Ho = Hi, a.Wo = Wi;
        a.Hs = a.Hin = Hi, a.Ws = a.Win = Wi;
        a.K = kCout[l] * kKs[l] * kKs[l], a.stride = 1, a.pad = kPad[l];
        float* gout = bufs[l & 1];
        const bool pooled = l <= 2;     // conv3 / conv6 read a max-pooled tap: their input gradient goes through the pool adjoint
        a.epi = pooled ? EPI_RAW : EPI_GRAD;
        a.mask = ta.fx[l - 1], a.gadd = ta.gtap[l - 1];
        a.out = (pooled || p.S > 1) ? part : gout;
        if (launch_conv(a, p, kKs[l], LOAD_PLAIN, st)) return 2;
        if (pooled) {
            const int Hs = g.h[l - 1], Ws = g.w[l - 1];
            hipLaunchKernelGGL(lpips_pool_bwd_kernel, dim3(grid_1d((int64_t)B * kCin[l] * Hs * Ws)), dim3(kThreads), 0, st, part, p.S,
                               ta.fx[l - 1], ta.gtap[l - 1], gout, B, kCin[l], Hs, Ws, Hi, Wi);
            if (check_launch("lpips pool backward")) return 2;
        } else if (p.S > 1) {
            if (launch_finish(part, p, kCin[l], Hi * Wi, EPI_GRAD, nullptr, a.mask, a.gadd, gout, st)) return 2;
        }
        gin = gout;
    }
    hipLaunchKernelGGL(lpips_dgrad0_kernel, dim3(grid_1d((int64_t)B * H * W)), dim3(kThreads), 0, st, gin, pack + pl.w0,
                       pack + pl.std_, dx, B, H, W, g.h[0], g.w[0]);
    return check_launch("lpips conv0 input gradient");
}
