// ArcFace identity loss backbone, IR-SE-50 at 112x112 in eval mode (libs/criteria/id_loss.py:20-25, model_irse.py:9-48,
// helpers.py:57-121): crop [35:223, 32:220] (PyTorch slice clamping) -> AdaptiveAvgPool2d(112) -> stem conv3x3 + BN + PReLU ->
// 24 bottleneck_IR_SE units -> BN2d / Dropout (eval: identity) / Linear 25088->512 / BN1d -> l2_norm; and dL/dx of that
// embedding for a given dL/de (the weights are frozen: no weight gradients).
//
// Every conv, every input-gradient conv and the two head GEMMs are one implicit-GEMM kernel on exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32): rows = output channels, columns = pixels, K gathered from the activation with the unit's operand
// transform fused into the load (BN1 before conv1 -- zero padding after BN, so it is not folded --, PReLU before conv2, the SE
// adjoint before conv2's input gradient).  The K loop is double-buffered: the next slice is fetched into registers while the MFMAs
// run on the current one from LDS.  Layers with few output tiles split K; the slices are summed in fixed order by the finish
// kernel, which applies the same epilogue.  BN2, the shortcut BN, the stem BN and the head's BN2d/BN1d are folded on the host
// (id_loss.py, once per weight version).  No float atomics, no host synchronisation, everything on the given stream.
#include <limits.h>
#include <string.h>

#include <algorithm>

#include "conv_tile.h"

namespace sgdfr {
namespace {

constexpr int kUnits = 24;
constexpr int kRes = 112;                       // pooled face size
constexpr int kPlane = kRes * kRes;
constexpr int kEmb = 512, kHeadK = 512 * 7 * 7;
constexpr int kParams = 3 + 10 * kUnits + 2;    // pointers sgdfr_idloss_prepack_f32 takes
constexpr int BN = 64;
// split K only below 256 output tiles, at most 512 / tiles slices of the planned rows; the forward's rows are at most twice the
// planned ones (rows_y <= rows_x), so S * (output tiles) <= 1024
constexpr int64_t kPartElems = 1024LL * BM * BN;

enum { TAP_FWD = 0, TAP_DGRAD = 1 };
enum { LD_PLAIN = 0, LD_AFFINE = 1, LD_PRELU = 2 };
enum { EP_RAW = 0, EP_BIAS = 1, EP_BIAS_PRELU = 2, EP_BIAS_SE = 3, EP_PRELU_GRAD = 4, EP_ADD = 5, EP_ADD_SUB = 6 };

// ------------------------------------------------------------------ network geometry
struct Unit {
    int cin, d, stride, h, w, ho, wo;   // input [cin, h, w] -> output [d, ho, wo]
    bool sc_conv;                       // shortcut conv1x1/2 + BN (in != depth); else MaxPool2d(1, stride)
};
static void make_units(Unit* u) {
    const int depth[4] = {64, 128, 256, 512}, count[4] = {3, 4, 14, 3};
    int c = 64, h = kRes, i = 0;
    for (int s = 0; s < 4; ++s)
        for (int k = 0; k < count[s]; ++k, ++i) {
            Unit& x = u[i];
            x.cin = c, x.d = depth[s], x.stride = k == 0 ? 2 : 1, x.h = x.w = h;
            x.ho = x.wo = (h - 1) / x.stride + 1;
            x.sc_conv = c != depth[s];
            c = depth[s], h = x.ho;
        }
}
static int64_t gate_elems(const Unit& u) { return u.d + u.d / 16; }   // per row: g [d], h [d/16]

// ------------------------------------------------------------------ weight pack
struct UnitPack {
    int64_t wf1, wd1, wf2, wd2, wfsc, s1, t1, a1, b2, bsc, f1, f2;
};
struct PackLayout {
    int64_t wf0, w0, b0, a0;
    UnitPack u[kUnits];
    int64_t wfh, wdh, bh, total;
};
static PackLayout pack_layout() {
    Unit us[kUnits];
    make_units(us);
    PackLayout p;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    p.wf0 = take(27 * 64), p.w0 = take(27 * 64), p.b0 = take(64), p.a0 = take(64);
    for (int i = 0; i < kUnits; ++i) {
        const Unit& u = us[i];
        UnitPack& q = p.u[i];
        q.wf1 = take((int64_t)u.cin * 9 * u.d);
        q.wd1 = take(((int64_t)u.d * 9 + (u.sc_conv ? u.d : 0)) * u.cin);
        q.wf2 = take((int64_t)u.d * 9 * u.d);
        q.wd2 = take((int64_t)u.d * 9 * u.d);
        q.wfsc = u.sc_conv ? take((int64_t)u.cin * u.d) : -1;
        q.s1 = take(u.cin), q.t1 = take(u.cin), q.a1 = take(u.d), q.b2 = take(u.d);
        q.bsc = u.sc_conv ? take(u.d) : -1;
        q.f1 = take((int64_t)u.d / 16 * u.d), q.f2 = take((int64_t)u.d * (u.d / 16));
    }
    p.wfh = take((int64_t)kHeadK * kEmb), p.wdh = take((int64_t)kHeadK * kEmb), p.bh = take(kEmb);
    p.total = o;
    return p;
}

enum { SEG_COPY = 0, SEG_FWD = 1, SEG_DGRAD = 2 };
// COPY: dst[j] = src[j].  FWD: [k = ci*kk + r][co] <- W[co][ci][r].  DGRAD: [co*kk + r][ci] <- W[co][ci][r] * scale[ci] (scale may
// be null): the input-gradient conv gathers dO at (o + pad - kh) / stride, so its weights are transposed, not flipped.
__global__ __launch_bounds__(kThreads) void idl_pack_kernel(const float* __restrict__ src, const float* __restrict__ scale,
                                                            float* __restrict__ dst, int64_t count, int kind, int cin, int cout, int kk) {
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
            if (scale) v *= scale[ci];
        }
        dst[j] = v;
    }
}

// ------------------------------------------------------------------ activations
// rows < rsplit live at p + b * rs, the others at p2 + (b - rsplit) * rs: x's rows in the saved buffer and a live y's rows in the
// workspace, or x and y as the two inputs of the front
struct Act {
    float* p;
    float* p2;
    int rsplit;
    int64_t rs;
};
__host__ __device__ __forceinline__ float* rowp(const Act& a, int b) {
    return b < a.rsplit ? a.p + (int64_t)b * a.rs : a.p2 + (int64_t)(b - a.rsplit) * a.rs;
}
static Act act(const float* p, int64_t rs) { return Act{const_cast<float*>(p), const_cast<float*>(p), INT_MAX, rs}; }
static Act act2(const float* p, int rsplit, const float* p2, int64_t rs) {
    return Act{const_cast<float*>(p), const_cast<float*>(p2), rsplit, rs};
}

// ------------------------------------------------------------------ implicit-GEMM conv
struct ConvArgs {
    Act src;             // [R, Cs, Hs, Ws]
    Act ext;             // EXT, k >= K1: the shortcut conv's dO [R, K - K1, He, We] at (oh/2, ow/2) for even oh, ow (else 0)
    const float* wp;     // [K][N]
    const float* lsc;    // LD_AFFINE: v * lsc[row*lrs + ci] + lsh[row*lrs + ci]; LD_PRELU: slope lsc[ci]
    const float* lsh;
    const float* bias;   // EP_BIAS*
    const float* slope;  // EP_BIAS_PRELU, EP_PRELU_GRAD
    Act aux;             // EP_BIAS_SE: c2; EP_PRELU_GRAD: the pre-activation; EP_ADD: addend (all [R,N,Ho,Wo]); EP_ADD_SUB: [R,N,auxH,auxW]
    Act gate;            // EP_BIAS_SE: g at rowp(gate, b)[n]
    Act out;             // [R, N, Ho, Wo]
    Act out2;            // EP_BIAS_PRELU: the pre-activation of rows < out2.rsplit
    float* part;         // split K: [S][R*N*Ho*Wo]
    int64_t part_elems;
    int R, Hs, Ws, N, Ho, Wo, K, K1, stride, pad, cps, epi, lrs, auxH, auxW, He, We;
    int plan_rows;       // host: the rows the split-K plan is made for (x's rows; 0: R)
};
static_assert(sizeof(ConvArgs) < 4096, "conv kernel arguments must stay below 4 KB");

__device__ __forceinline__ void epilogue(const ConvArgs& a, int b, int n, int p, float v) {
    const int64_t o = (int64_t)n * (a.Ho * a.Wo) + p;
    float r;
    switch (a.epi) {
        case EP_RAW: r = v; break;
        case EP_BIAS: r = v + a.bias[n]; break;
        case EP_BIAS_PRELU: {
            const float pre = v + a.bias[n];
            if (b < a.out2.rsplit) rowp(a.out2, b)[o] = pre;
            r = pre > 0.f ? pre : a.slope[n] * pre;
            break;
        }
        case EP_BIAS_SE: r = (rowp(a.aux, b)[o] * rowp(a.gate, b)[n]) + (v + a.bias[n]); break;
        case EP_PRELU_GRAD: r = rowp(a.aux, b)[o] > 0.f ? v : a.slope[n] * v; break;
        case EP_ADD: r = v + rowp(a.aux, b)[o]; break;
        default: {   // EP_ADD_SUB: the adjoint of MaxPool2d(1, 2)
            const int oh = p / a.Wo, ow = p - oh * a.Wo;
            r = v;
            if (!((oh | ow) & 1)) r += rowp(a.aux, b)[((int64_t)n * a.auxH + (oh >> 1)) * a.auxW + (ow >> 1)];
        }
    }
    rowp(a.out, b)[o] = r;
}

template <int TAP, int KS, int LOAD, bool EXT>
__global__ __launch_bounds__(kThreads) void idl_conv_kernel(ConvArgs a) {
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
    const float* srcb = rowp(a.src, b);
    const float* extb = EXT ? rowp(a.ext, b) : nullptr;
    const float* lsc = LOAD == LD_AFFINE ? a.lsc + (int64_t)b * a.lrs : a.lsc;
    const float* lsh = LOAD == LD_AFFINE ? a.lsh + (int64_t)b * a.lrs : nullptr;

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
                    if (mvalid && !((oh | ow) & 1)) v = extb[((int64_t)(k - a.K1) * a.He + (oh >> 1)) * a.We + (ow >> 1)];
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
                    if (mvalid && ok) {
                        const float s = srcb[ci * plane + ih * a.Ws + iw];
                        if (LOAD == LD_AFFINE) v = fmaf(s, lsc[ci], lsh[ci]);
                        else if (LOAD == LD_PRELU) v = s > 0.f ? s : lsc[ci] * s;
                        else v = s;
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
__global__ __launch_bounds__(kThreads) void idl_finish_kernel(ConvArgs a, int S) {
    finish_slices(a.part, a.part_elems, S, a.N, a.Ho * a.Wo, [=](int b, int n, int p, float v) { epilogue(a, b, n, p, v); });
}

// ------------------------------------------------------------------ front: crop + AdaptiveAvgPool2d(112) and its adjoint
struct Window {
    int h0, ch, w0, cw;
};
__device__ __forceinline__ int bin_lo(int i, int in) { return (i * in) / kRes; }
__device__ __forceinline__ int bin_hi(int i, int in) { return ((i + 1) * in + kRes - 1) / kRes; }

__global__ __launch_bounds__(kThreads) void idl_front_kernel(Act src, int H, int W, Window win, float* __restrict__ out, int R) {
    const int64_t n = (int64_t)R * 3 * kPlane;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(idx % kRes), i = (int)((idx / kRes) % kRes);
        const int rc = (int)(idx / kPlane), r = rc / 3, c = rc - 3 * r;
        const float* pl = rowp(src, r) + (int64_t)c * H * W + (int64_t)win.h0 * W + win.w0;
        const int hs = bin_lo(i, win.ch), he = bin_hi(i, win.ch), ws = bin_lo(j, win.cw), we = bin_hi(j, win.cw);
        float s = 0.f;
        for (int y = hs; y < he; ++y)
            for (int x = ws; x < we; ++x) s += pl[(int64_t)y * W + x];
        out[idx] = s / (float)((he - hs) * (we - ws));
    }
}

// dL/dx of the whole [B,3,H,W]: zero outside the window, else the gather of every pooling bin that covers the pixel
__global__ __launch_bounds__(kThreads) void idl_front_bwd_kernel(const float* __restrict__ dpool, int B, int H, int W, Window win,
                                                                 float* __restrict__ dx) {
    const int64_t n = (int64_t)B * 3 * H * W;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int w = (int)(idx % W), h = (int)((idx / W) % H);
        const int64_t bc = idx / ((int64_t)H * W);
        const int y = h - win.h0, x = w - win.w0;
        float g = 0.f;
        if (y >= 0 && y < win.ch && x >= 0 && x < win.cw) {
            const int i0 = max(0, (y * kRes) / win.ch - 1), i1 = min(kRes - 1, ((y + 1) * kRes) / win.ch);
            const int j0 = max(0, (x * kRes) / win.cw - 1), j1 = min(kRes - 1, ((x + 1) * kRes) / win.cw);
            const float* dp = dpool + bc * kPlane;
            for (int i = i0; i <= i1; ++i) {
                const int hs = bin_lo(i, win.ch), he = bin_hi(i, win.ch);
                if (y < hs || y >= he) continue;
                for (int j = j0; j <= j1; ++j) {
                    const int ws = bin_lo(j, win.cw), we = bin_hi(j, win.cw);
                    if (x < ws || x >= we) continue;
                    g += dp[i * kRes + j] / (float)((he - hs) * (we - ws));
                }
            }
        }
        dx[idx] = g;
    }
}

// stem adjoint: PReLU (slope where the pre-activation p0 <= 0), then conv3x3 3<-64 as a gather per pooled pixel
__global__ __launch_bounds__(kThreads) void idl_stem_bwd_kernel(const float* __restrict__ da0, const float* __restrict__ p0,
                                                                const float* __restrict__ slope, const float* __restrict__ w0,
                                                                float* __restrict__ dxp, int B) {
    const int64_t n = (int64_t)B * kPlane;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int x = (int)(idx % kRes), y = (int)((idx / kRes) % kRes), b = (int)(idx / kPlane);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        const int64_t base = (int64_t)b * 64 * kPlane;
        for (int co = 0; co < 64; ++co) {
            const float al = slope[co];
            for (int kh = 0; kh < 3; ++kh) {
                const int yy = y + 1 - kh;
                if (yy < 0 || yy >= kRes) continue;
                for (int kw = 0; kw < 3; ++kw) {
                    const int xx = x + 1 - kw;
                    if (xx < 0 || xx >= kRes) continue;
                    const int64_t o = base + (int64_t)co * kPlane + yy * kRes + xx;
                    float d = da0[o];
                    d = p0[o] > 0.f ? d : al * d;
                    const float* wp = w0 + co * 27 + kh * 3 + kw;
                    s0 = fmaf(wp[0], d, s0);
                    s1 = fmaf(wp[9], d, s1);
                    s2 = fmaf(wp[18], d, s2);
                }
            }
        }
        const int64_t o = (int64_t)b * 3 * kPlane + y * kRes + x;
        dxp[o] = s0;
        dxp[o + kPlane] = s1;
        dxp[o + 2 * kPlane] = s2;
    }
}

// ------------------------------------------------------------------ SE gate and its adjoint (one block per row)
// m = mean_hw c2; h = relu(fc1 m); g = sigmoid(fc2 h) -> gate row: g [D], h [D/16].  Sums in fixed order (lanes, then wave_sum).
__global__ __launch_bounds__(kThreads) void idl_gate_kernel(Act c2, int D, int HW, const float* __restrict__ f1,
                                                            const float* __restrict__ f2, Act gate) {
    __shared__ float sm[512], sh[32];
    const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6, Dr = D / 16;
    const float* x = rowp(c2, r);
    float* g = rowp(gate, r);
    for (int c = wv; c < D; c += kThreads / kWave) {
        float s = 0.f;
        for (int p = lane; p < HW; p += kWave) s += x[(int64_t)c * HW + p];
        s = wave_sum(s);
        if (lane == 0) sm[c] = s / (float)HW;
    }
    __syncthreads();
    for (int j = wv; j < Dr; j += kThreads / kWave) {
        float s = 0.f;
        for (int c = lane; c < D; c += kWave) s = fmaf(f1[j * D + c], sm[c], s);
        s = wave_sum(s);
        if (lane == 0) sh[j] = fmaxf(s, 0.f);
    }
    __syncthreads();
    for (int c = t; c < D; c += kThreads) {
        float z = 0.f;
        for (int j = 0; j < Dr; ++j) z = fmaf(f2[c * Dr + j], sh[j], z);
        g[c] = 1.f / (1.f + expf(-z));
    }
    for (int j = t; j < Dr; j += kThreads) g[D + j] = sh[j];
}

// dg = sum_hw dout c2; dz = dg g (1 - g); dh = fc2^T dz [h > 0]; dm = fc1^T dh -> coef row: g [D], dm / HW [D]
// (conv2's input gradient then loads dc2 = dout g + dm / HW)
__global__ __launch_bounds__(kThreads) void idl_gate_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ c2,
                                                                const float* __restrict__ gate, int D, int HW, const float* __restrict__ f1,
                                                                const float* __restrict__ f2, float* __restrict__ coef) {
    __shared__ float sdz[512], sdh[32];
    const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6, Dr = D / 16;
    const float* dO = dout + (int64_t)r * D * HW;
    const float* x = c2 + (int64_t)r * D * HW;
    const float* g = gate + (int64_t)r * (D + Dr);
    float* cf = coef + (int64_t)r * 2 * D;
    for (int c = wv; c < D; c += kThreads / kWave) {
        float s = 0.f;
        for (int p = lane; p < HW; p += kWave) s = fmaf(dO[(int64_t)c * HW + p], x[(int64_t)c * HW + p], s);
        s = wave_sum(s);
        if (lane == 0) sdz[c] = s * g[c] * (1.f - g[c]);
    }
    __syncthreads();
    for (int j = wv; j < Dr; j += kThreads / kWave) {
        float s = 0.f;
        for (int c = lane; c < D; c += kWave) s = fmaf(f2[c * Dr + j], sdz[c], s);
        s = wave_sum(s);
        if (lane == 0) sdh[j] = g[D + j] > 0.f ? s : 0.f;
    }
    __syncthreads();
    for (int c = t; c < D; c += kThreads) {
        float dm = 0.f;
        for (int j = 0; j < Dr; ++j) dm = fmaf(f1[j * D + c], sdh[j], dm);
        cf[c] = g[c];
        cf[D + c] = dm / (float)HW;
    }
}

// out = c2 g + shortcut, the shortcut being x itself or x[:, :, ::2, ::2] (MaxPool2d(1, stride))
__global__ __launch_bounds__(kThreads) void idl_combine_kernel(Act c2, Act gate, Act a, Act out, int R, int D, int Ho, int Wo, int Hi,
                                                               int Wi, int stride) {
    const int HWo = Ho * Wo;
    const int64_t n = (int64_t)R * D * HWo;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int p = (int)(idx % HWo);
        const int rc = (int)(idx / HWo), r = rc / D, c = rc - r * D;
        const int oh = p / Wo, ow = p - oh * Wo;
        const float sc = rowp(a, r)[((int64_t)c * Hi + oh * stride) * Wi + ow * stride];
        const int64_t o = (int64_t)c * HWo + p;
        rowp(out, r)[o] = (rowp(c2, r)[o] * rowp(gate, r)[c]) + sc;
    }
}

// ------------------------------------------------------------------ head: folded Linear slices summed in order, l2_norm
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// v = sum_s part[s] + bias; e = v / |v| -> emb and the saved (e, |v|) row
__global__ __launch_bounds__(kThreads) void idl_head_kernel(const float* __restrict__ part, int S, int R, const float* __restrict__ bias,
                                                            Act hv, float* __restrict__ emb) {
    __shared__ float red[kThreads / kWave];
    const int r = blockIdx.x, t = threadIdx.x;
    const int64_t n = (int64_t)R * kEmb;
    float v[2];
    for (int q = 0; q < 2; ++q) {
        const int64_t i = (int64_t)r * kEmb + t + q * kThreads;
        float s = part[i];
        for (int sl = 1; sl < S; ++sl) s += part[sl * n + i];
        v[q] = s + bias[t + q * kThreads];
    }
    const float nrm = sqrtf(block_sum(fmaf(v[0], v[0], v[1] * v[1]), red));
    float* h = rowp(hv, r);
    for (int q = 0; q < 2; ++q) {
        const float e = v[q] / nrm;
        emb[(int64_t)r * kEmb + t + q * kThreads] = e;
        h[t + q * kThreads] = e;
    }
    if (t == 0) h[kEmb] = nrm;
}

// l2_norm adjoint: dv = (de - e (e . de)) / |v|
__global__ __launch_bounds__(kThreads) void idl_head_bwd_kernel(const float* __restrict__ ge, const float* __restrict__ hv,
                                                                float* __restrict__ dv) {
    __shared__ float red[kThreads / kWave];
    const int r = blockIdx.x, t = threadIdx.x;
    const float* e = hv + (int64_t)r * (kEmb + 1);
    const float* g = ge + (int64_t)r * kEmb;
    const float dot = block_sum(fmaf(e[t], g[t], e[t + kThreads] * g[t + kThreads]), red);
    const float nrm = e[kEmb];
    for (int q = 0; q < 2; ++q) {
        const int i = t + q * kThreads;
        dv[(int64_t)r * kEmb + i] = (g[i] - e[i] * dot) / nrm;
    }
}

// ------------------------------------------------------------------ host side
// The number of K slices follows the output tiles of `plan_rows` rows (x's rows): a live y in the same launches, or a broadcast
// one, changes no summation order, so x's embedding and dL/dx do not depend on how y is passed.
static ConvPlan plan_for_rows(int R, int plan_rows, int N, int Ho, int Wo, int K) {
    const int HWo = Ho * Wo;
    return plan_conv(R * HWo, N, K, BN, conv_tiles(std::min(R, std::max(plan_rows, 1)) * HWo, N, BN));
}

static int launch_conv(const ConvArgs& a0, int tap, int ks, int load, bool ext, float* part, hipStream_t st) {
    ConvArgs a = a0;
    const ConvPlan p = plan_for_rows(a.R, a.plan_rows ? a.plan_rows : a.R, a.N, a.Ho, a.Wo, a.K);
    SGDFR_REQUIRE(p.S == 1 || p.S * p.out_elems <= kPartElems, "idloss: split-K partials of %lld floats exceed the workspace",
                  (long long)(p.S * p.out_elems));
    a.cps = p.cps;
    a.part = part;
    a.part_elems = p.out_elems;
    const dim3 grid(p.mt, p.nt, p.S);
    bool done = false;
#define SGDFR_IDL_CONV(T_, KS_, LD_, EXT_)                                                    \
    if (!done && tap == T_ && ks == KS_ && load == LD_ && ext == EXT_) {                       \
        hipLaunchKernelGGL((idl_conv_kernel<T_, KS_, LD_, EXT_>), grid, dim3(kThreads), 0, st, a); \
        done = true;                                                                           \
    }
    SGDFR_IDL_CONV(TAP_FWD, 3, LD_PLAIN, false)     // stem
    SGDFR_IDL_CONV(TAP_FWD, 3, LD_AFFINE, false)    // conv1 (BN1 in the load)
    SGDFR_IDL_CONV(TAP_FWD, 3, LD_PRELU, false)     // conv2 (PReLU in the load)
    SGDFR_IDL_CONV(TAP_FWD, 1, LD_PLAIN, false)     // shortcut conv, head GEMMs
    SGDFR_IDL_CONV(TAP_DGRAD, 3, LD_AFFINE, false)  // conv2 input gradient (SE adjoint in the load)
    SGDFR_IDL_CONV(TAP_DGRAD, 3, LD_PLAIN, false)   // conv1 input gradient
    SGDFR_IDL_CONV(TAP_DGRAD, 3, LD_PLAIN, true)    // conv1 + shortcut-conv input gradient
#undef SGDFR_IDL_CONV
    SGDFR_REQUIRE(done, "idloss: no conv instance for tap=%d k=%d load=%d ext=%d", tap, ks, load, (int)ext);
    if (check_launch("idloss conv")) return 2;
    if (p.S > 1) {
        hipLaunchKernelGGL(idl_finish_kernel, dim3(grid_1d(p.out_elems)), dim3(kThreads), 0, st, a, p.S);
        if (check_launch("idloss finish")) return 2;
    }
    return 0;
}

static bool make_window(int H, int W, int crop, Window& w) {
    if (H < 1 || W < 1 || H > 8192 || W > 8192 || (crop != 0 && crop != 1)) return false;
    if (crop) {
        w.h0 = std::min(35, H), w.w0 = std::min(32, W);
        w.ch = std::min(223, H) - w.h0, w.cw = std::min(220, W) - w.w0;
    } else {
        w.h0 = w.w0 = 0, w.ch = H, w.cw = W;
    }
    return w.ch >= 1 && w.cw >= 1;
}

// saved rows (x only): stem pre-activation, per unit conv1's pre-activation p1, c2 and the gate row, the head's (e, |v|)
struct SavedLayout {
    int64_t p0, p1[kUnits], c2[kUnits], gate[kUnits], hv, total;
};
static SavedLayout saved_layout(int rows) {
    Unit us[kUnits];
    make_units(us);
    SavedLayout s;
    int64_t o = 0;
    s.p0 = o, o += (int64_t)rows * 64 * kPlane;
    for (int i = 0; i < kUnits; ++i) {
        const Unit& u = us[i];
        s.p1[i] = o, o += (int64_t)rows * u.d * u.h * u.w;
        s.c2[i] = o, o += (int64_t)rows * u.d * u.ho * u.wo;
        s.gate[i] = o, o += (int64_t)rows * gate_elems(u);
    }
    s.hv = o, o += (int64_t)rows * (kEmb + 1);
    s.total = o;
    return s;
}

constexpr int64_t kMaxIo = 64LL * kPlane;           // largest activation per row (stem output, unit 0's p1)
constexpr int64_t kMaxC2 = 64LL * 56 * 56;
struct WsLayout {
    int64_t part, pooled, act[2], p1, c2, gate, coef, hv, dv, total;   // float offsets
};
static WsLayout ws_layout(int rows) {
    WsLayout w;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    w.part = take(kPartElems);
    w.pooled = take((int64_t)rows * 3 * kPlane);
    w.act[0] = take((int64_t)rows * kMaxIo);
    w.act[1] = take((int64_t)rows * kMaxIo);
    w.p1 = take((int64_t)rows * kMaxIo);
    w.c2 = take((int64_t)rows * kMaxC2);
    w.gate = take((int64_t)rows * (512 + 32));
    w.coef = take((int64_t)rows * 2 * 512);
    w.hv = take((int64_t)rows * (kEmb + 1));
    w.dv = take((int64_t)rows * kEmb);
    w.total = o;
    return w;
}

}  // namespace
}  // namespace sgdfr

using namespace sgdfr;

extern "C" int64_t sgdfr_idloss_pack_elems(void) { return pack_layout().total; }

extern "C" int64_t sgdfr_idloss_saved_elems(int rows) {
    if (rows < 1 || rows > 4096) return -1;
    return saved_layout(rows).total;
}

extern "C" int64_t sgdfr_idloss_workspace_bytes(int rows, int H, int W) {
    // the size does not depend on the window; forward / backward refuse an empty crop window themselves (crop=1 only)
    Window w;
    if (rows < 1 || rows > 4096 || !make_window(H, W, 0, w)) return -1;
    return ws_layout(rows).total * (int64_t)sizeof(float);
}

extern "C" int sgdfr_idloss_prepack_f32(const float* const* params, float* pack, void* stream) {
    SGDFR_REQUIRE(params && pack, "idloss_prepack: null pointer");
    Unit us[kUnits];
    make_units(us);
    for (int i = 0; i < kParams; ++i) {
        const int u = (i - 3) / 10, j = (i - 3) % 10;
        const bool optional = i >= 3 && i < 3 + 10 * kUnits && j >= 8 && !us[u].sc_conv;   // shortcut conv of an identity unit
        SGDFR_REQUIRE(optional || params[i], "idloss_prepack: parameter %d is null", i);
    }
    const PackLayout pl = pack_layout();
    hipStream_t st = as_stream(stream);
    auto seg = [&](const float* src, const float* scale, int64_t dst, int64_t count, int kind, int cin, int cout, int kk) {
        hipLaunchKernelGGL(idl_pack_kernel, dim3(grid_1d(count)), dim3(kThreads), 0, st, src, scale, pack + dst, count, kind, cin, cout, kk);
        return check_launch("idloss prepack");
    };
    int rc = 0;
    rc |= seg(params[0], nullptr, pl.wf0, 27 * 64, SEG_FWD, 3, 64, 9);
    rc |= seg(params[0], nullptr, pl.w0, 27 * 64, SEG_COPY, 0, 0, 0);
    rc |= seg(params[1], nullptr, pl.b0, 64, SEG_COPY, 0, 0, 0);
    rc |= seg(params[2], nullptr, pl.a0, 64, SEG_COPY, 0, 0, 0);
    for (int i = 0; i < kUnits && !rc; ++i) {
        const Unit& u = us[i];
        const UnitPack& q = pl.u[i];
        const float* const* P = params + 3 + 10 * i;   // s1, t1, w1, a1, w2, b2, f1, f2, wsc, bsc
        const int64_t n1 = (int64_t)u.cin * 9 * u.d, n2 = (int64_t)u.d * 9 * u.d;
        rc |= seg(P[0], nullptr, q.s1, u.cin, SEG_COPY, 0, 0, 0);
        rc |= seg(P[1], nullptr, q.t1, u.cin, SEG_COPY, 0, 0, 0);
        rc |= seg(P[2], nullptr, q.wf1, n1, SEG_FWD, u.cin, u.d, 9);
        rc |= seg(P[2], P[0], q.wd1, n1, SEG_DGRAD, u.cin, u.d, 9);     // BN1's scale folded into conv1's input gradient
        rc |= seg(P[3], nullptr, q.a1, u.d, SEG_COPY, 0, 0, 0);
        rc |= seg(P[4], nullptr, q.wf2, n2, SEG_FWD, u.d, u.d, 9);
        rc |= seg(P[4], nullptr, q.wd2, n2, SEG_DGRAD, u.d, u.d, 9);
        rc |= seg(P[5], nullptr, q.b2, u.d, SEG_COPY, 0, 0, 0);
        rc |= seg(P[6], nullptr, q.f1, (int64_t)u.d / 16 * u.d, SEG_COPY, 0, 0, 0);
        rc |= seg(P[7], nullptr, q.f2, (int64_t)u.d * (u.d / 16), SEG_COPY, 0, 0, 0);
        if (u.sc_conv) {
            rc |= seg(P[8], nullptr, q.wfsc, (int64_t)u.cin * u.d, SEG_FWD, u.cin, u.d, 1);
            rc |= seg(P[8], nullptr, q.wd1 + n1, (int64_t)u.cin * u.d, SEG_COPY, 0, 0, 0);   // extra K rows of conv1's dgrad
            rc |= seg(P[9], nullptr, q.bsc, u.d, SEG_COPY, 0, 0, 0);
        }
    }
    const float* const* H = params + 3 + 10 * kUnits;
    if (!rc) rc |= seg(H[0], nullptr, pl.wfh, (int64_t)kHeadK * kEmb, SEG_FWD, kHeadK, kEmb, 1);
    if (!rc) rc |= seg(H[0], nullptr, pl.wdh, (int64_t)kHeadK * kEmb, SEG_COPY, 0, 0, 0);
    if (!rc) rc |= seg(H[1], nullptr, pl.bh, kEmb, SEG_COPY, 0, 0, 0);
    return rc ? 2 : 0;
}

extern "C" int sgdfr_idloss_forward_f32(const float* x, int rows_x, const float* y, int rows_y, int H, int W, int crop, const float* pack,
                                        float* emb, float* saved, void* workspace, int64_t workspace_bytes, void* stream) {
    Window win;
    SGDFR_REQUIRE(make_window(H, W, crop, win), "idloss: unsupported image size %dx%d (crop=%d)", H, W, crop);
    SGDFR_REQUIRE(x && rows_x >= 1 && rows_y >= 0 && rows_y <= rows_x && (rows_y == 0 || y) && rows_x + rows_y <= 4096,
                  "idloss_forward: bad inputs (rows %d + %d)", rows_x, rows_y);
    SGDFR_REQUIRE(pack && emb && workspace, "idloss_forward: null pointer");
    const int R = rows_x + rows_y;
    const WsLayout wl = ws_layout(R);
    SGDFR_REQUIRE(wl.total * (int64_t)sizeof(float) <= workspace_bytes, "idloss_forward: workspace of %lld bytes, %d rows need %lld",
                  (long long)workspace_bytes, R, (long long)(wl.total * (int64_t)sizeof(float)));
    Unit us[kUnits];
    make_units(us);
    const PackLayout pl = pack_layout();
    const SavedLayout sl = saved_layout(rows_x);
    const int Bs = saved ? rows_x : 0;             // rows whose activations go to `saved`
    float* wsf = reinterpret_cast<float*>(workspace);
    float* part = wsf + wl.part;
    hipStream_t st = as_stream(stream);
    // rows < Bs in the saved buffer, the rest in workspace scratch (indexed from row Bs)
    auto split_act = [&](int64_t saved_off, int64_t scratch_off, int64_t rs) {
        return Bs ? act2(saved + saved_off, Bs, wsf + scratch_off, rs) : act(wsf + scratch_off, rs);
    };

    float* pooled = wsf + wl.pooled;
    hipLaunchKernelGGL(idl_front_kernel, dim3(grid_1d((int64_t)R * 3 * kPlane)), dim3(kThreads), 0, st,
                       act2(x, rows_x, y ? y : x, (int64_t)3 * H * W), H, W, win, pooled, R);
    if (check_launch("idloss front")) return 2;

    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.src = act(pooled, 3LL * kPlane);
    a.wp = pack + pl.wf0, a.bias = pack + pl.b0, a.slope = pack + pl.a0;
    a.R = R, a.plan_rows = rows_x, a.Hs = a.Ws = kRes, a.N = 64, a.Ho = a.Wo = kRes, a.K = 27, a.K1 = 27, a.stride = 1, a.pad = 1, a.epi = EP_BIAS_PRELU;
    a.out = act(wsf + wl.act[0], kMaxIo);
    a.out2 = Act{saved ? saved + sl.p0 : nullptr, nullptr, Bs, 64LL * kPlane};
    if (launch_conv(a, TAP_FWD, 3, LD_PLAIN, false, part, st)) return 2;

    int cur = 0;
    for (int i = 0; i < kUnits; ++i) {
        const Unit& u = us[i];
        const UnitPack& q = pl.u[i];
        const Act ain = act(wsf + wl.act[cur], (int64_t)u.cin * u.h * u.w);
        const Act aout = act(wsf + wl.act[cur ^ 1], (int64_t)u.d * u.ho * u.wo);
        const Act p1 = split_act(sl.p1[i], wl.p1, (int64_t)u.d * u.h * u.w);
        const Act c2 = split_act(sl.c2[i], wl.c2, (int64_t)u.d * u.ho * u.wo);
        const Act gt = split_act(sl.gate[i], wl.gate, gate_elems(u));
        // conv1: BN1 in the load, raw pre-activation out
        memset(&a, 0, sizeof(a));
        a.src = ain, a.wp = pack + q.wf1, a.lsc = pack + q.s1, a.lsh = pack + q.t1, a.lrs = 0;
        a.R = R, a.plan_rows = rows_x, a.Hs = u.h, a.Ws = u.w, a.N = u.d, a.Ho = u.h, a.Wo = u.w, a.K = a.K1 = u.cin * 9, a.stride = 1, a.pad = 1;
        a.epi = EP_RAW, a.out = p1;
        if (launch_conv(a, TAP_FWD, 3, LD_AFFINE, false, part, st)) return 2;
        // conv2 at the unit's stride: PReLU in the load, folded BN2 bias out
        memset(&a, 0, sizeof(a));
        a.src = p1, a.wp = pack + q.wf2, a.lsc = pack + q.a1;
        a.R = R, a.plan_rows = rows_x, a.Hs = u.h, a.Ws = u.w, a.N = u.d, a.Ho = u.ho, a.Wo = u.wo, a.K = a.K1 = u.d * 9, a.stride = u.stride, a.pad = 1;
        a.epi = EP_BIAS, a.bias = pack + q.b2, a.out = c2;
        if (launch_conv(a, TAP_FWD, 3, LD_PRELU, false, part, st)) return 2;
        hipLaunchKernelGGL(idl_gate_kernel, dim3(R), dim3(kThreads), 0, st, c2, u.d, u.ho * u.wo, pack + q.f1, pack + q.f2, gt);
        if (check_launch("idloss gate")) return 2;
        if (u.sc_conv) {       // out = shortcut conv (folded BN) + c2 g in the conv's epilogue
            memset(&a, 0, sizeof(a));
            a.src = ain, a.wp = pack + q.wfsc;
            a.R = R, a.plan_rows = rows_x, a.Hs = u.h, a.Ws = u.w, a.N = u.d, a.Ho = u.ho, a.Wo = u.wo, a.K = a.K1 = u.cin, a.stride = 2, a.pad = 0;
            a.epi = EP_BIAS_SE, a.bias = pack + q.bsc, a.aux = c2, a.gate = gt, a.out = aout;
            if (launch_conv(a, TAP_FWD, 1, LD_PLAIN, false, part, st)) return 2;
        } else {
            hipLaunchKernelGGL(idl_combine_kernel, dim3(grid_1d((int64_t)R * u.d * u.ho * u.wo)), dim3(kThreads), 0, st, c2, gt, ain, aout,
                               R, u.d, u.ho, u.wo, u.h, u.w, u.stride);
            if (check_launch("idloss combine")) return 2;
        }
        cur ^= 1;
    }

    // head: [R, 25088] x [25088, 512] (K split), then bias, l2_norm
    memset(&a, 0, sizeof(a));
    a.src = act(wsf + wl.act[cur], kHeadK), a.wp = pack + pl.wfh;
    a.R = R, a.plan_rows = rows_x, a.Hs = a.Ws = 1, a.N = kEmb, a.Ho = a.Wo = 1, a.K = a.K1 = kHeadK, a.stride = 1, a.pad = 0;
    a.epi = EP_RAW, a.out = act(part, kEmb);
    const ConvPlan hp = plan_for_rows(R, rows_x, kEmb, 1, 1, kHeadK);
    if (hp.S > 1) {      // the raw slices stay in `part`: launch the kernel alone (no finish)
        ConvArgs b = a;
        b.cps = hp.cps, b.part = part, b.part_elems = hp.out_elems;
        SGDFR_REQUIRE(hp.S * hp.out_elems <= kPartElems, "idloss: head partials exceed the workspace");
        hipLaunchKernelGGL((idl_conv_kernel<TAP_FWD, 1, LD_PLAIN, false>), dim3(hp.mt, hp.nt, hp.S), dim3(kThreads), 0, st, b);
        if (check_launch("idloss head")) return 2;
    } else if (launch_conv(a, TAP_FWD, 1, LD_PLAIN, false, part, st)) {
        return 2;
    }
    const Act hv = Bs ? act2(saved + sl.hv, Bs, wsf + wl.hv, kEmb + 1) : act(wsf + wl.hv, kEmb + 1);
    hipLaunchKernelGGL(idl_head_kernel, dim3(R), dim3(kThreads), 0, st, part, hp.S, R, pack + pl.bh, hv, emb);
    return check_launch("idloss head norm");
}

extern "C" int sgdfr_idloss_backward_f32(const float* grad_emb, const float* saved, int rows, int H, int W, int crop, const float* pack,
                                         float* dx, void* workspace, int64_t workspace_bytes, void* stream) {
    Window win;
    SGDFR_REQUIRE(make_window(H, W, crop, win), "idloss: unsupported image size %dx%d (crop=%d)", H, W, crop);
    SGDFR_REQUIRE(rows >= 1 && rows <= 4096, "idloss_backward: %d rows", rows);
    SGDFR_REQUIRE(grad_emb && saved && pack && dx && workspace, "idloss_backward: null pointer");
    const WsLayout wl = ws_layout(rows);
    SGDFR_REQUIRE(wl.total * (int64_t)sizeof(float) <= workspace_bytes, "idloss_backward: workspace of %lld bytes, %d rows need %lld",
                  (long long)workspace_bytes, rows, (long long)(wl.total * (int64_t)sizeof(float)));
    Unit us[kUnits];
    make_units(us);
    const PackLayout pl = pack_layout();
    const SavedLayout sl = saved_layout(rows);
    const int B = rows;
    float* wsf = reinterpret_cast<float*>(workspace);
    float* part = wsf + wl.part;
    hipStream_t st = as_stream(stream);

    hipLaunchKernelGGL(idl_head_bwd_kernel, dim3(B), dim3(kThreads), 0, st, grad_emb, saved + sl.hv, wsf + wl.dv);
    if (check_launch("idloss head backward")) return 2;
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.src = act(wsf + wl.dv, kEmb), a.wp = pack + pl.wdh;
    a.R = B, a.Hs = a.Ws = 1, a.N = kHeadK, a.Ho = a.Wo = 1, a.K = a.K1 = kEmb, a.stride = 1, a.pad = 0;
    int cur = 0;
    a.epi = EP_RAW, a.out = act(wsf + wl.act[cur], kHeadK);
    if (launch_conv(a, TAP_FWD, 1, LD_PLAIN, false, part, st)) return 2;

    for (int i = kUnits - 1; i >= 0; --i) {
        const Unit& u = us[i];
        const UnitPack& q = pl.u[i];
        const float* dout = wsf + wl.act[cur];
        const int64_t rs_out = (int64_t)u.d * u.ho * u.wo, rs_in = (int64_t)u.cin * u.h * u.w, rs_p1 = (int64_t)u.d * u.h * u.w;
        hipLaunchKernelGGL(idl_gate_bwd_kernel, dim3(B), dim3(kThreads), 0, st, dout, saved + sl.c2[i], saved + sl.gate[i], u.d,
                           u.ho * u.wo, pack + q.f1, pack + q.f2, wsf + wl.coef);
        if (check_launch("idloss gate backward")) return 2;
        // dc1 = conv2^T (dout g + dm/HW), then the PReLU adjoint (slope where p1 <= 0)
        memset(&a, 0, sizeof(a));
        a.src = act(dout, rs_out), a.wp = pack + q.wd2, a.lsc = wsf + wl.coef, a.lsh = wsf + wl.coef + u.d, a.lrs = 2 * u.d;
        a.R = B, a.Hs = u.ho, a.Ws = u.wo, a.N = u.d, a.Ho = u.h, a.Wo = u.w, a.K = a.K1 = u.d * 9, a.stride = u.stride, a.pad = 1;
        a.epi = EP_PRELU_GRAD, a.aux = act(saved + sl.p1[i], rs_p1), a.slope = pack + q.a1, a.out = act(wsf + wl.p1, rs_p1);
        if (launch_conv(a, TAP_DGRAD, 3, LD_AFFINE, false, part, st)) return 2;
        // dx_unit = conv1^T dp1 (BN1's scale in the weights) + the shortcut's adjoint
        memset(&a, 0, sizeof(a));
        a.src = act(wsf + wl.p1, rs_p1), a.wp = pack + q.wd1;
        a.R = B, a.Hs = u.h, a.Ws = u.w, a.N = u.cin, a.Ho = u.h, a.Wo = u.w, a.K1 = u.d * 9, a.stride = 1, a.pad = 1;
        a.K = a.K1 + (u.sc_conv ? u.d : 0);
        a.out = act(wsf + wl.act[cur ^ 1], rs_in);
        if (u.sc_conv) {
            a.ext = act(dout, rs_out), a.He = u.ho, a.We = u.wo, a.epi = EP_RAW;
        } else if (u.stride == 1) {
            a.epi = EP_ADD, a.aux = act(dout, rs_out);
        } else {
            a.epi = EP_ADD_SUB, a.aux = act(dout, rs_out), a.auxH = u.ho, a.auxW = u.wo;
        }
        if (launch_conv(a, TAP_DGRAD, 3, LD_PLAIN, u.sc_conv, part, st)) return 2;
        cur ^= 1;
    }
    float* dpool = wsf + wl.pooled;
    hipLaunchKernelGGL(idl_stem_bwd_kernel, dim3(grid_1d((int64_t)B * kPlane)), dim3(kThreads), 0, st, wsf + wl.act[cur], saved + sl.p0,
                       pack + pl.a0, pack + pl.w0, dpool, B);
    if (check_launch("idloss stem backward")) return 2;
    hipLaunchKernelGGL(idl_front_bwd_kernel, dim3(grid_1d((int64_t)B * 3 * H * W)), dim3(kThreads), 0, st, dpool, B, H, W, win, dx);
    return check_launch("idloss front backward");
}
