// The e4e W+ encoder in eval mode (libs/gan/encoder4editing/psp_encoders.py:33-53 GradualStyleBlock and :122-199 Encoder4Editing(50,
// 'ir_se', R), helpers.py:57-140): stem conv3x3 + BN + PReLU at R x R -> 24 bottleneck_IR_SE units (3 x 64, 4 x 128, 14 x 256, 3 x 512
// channels, the first of a stage at stride 2) with taps c1, c2, c3 behind units 6, 20, 23 -> p2 = bilinear(c3) + latlayer1(c2),
// p1 = bilinear(p2) + latlayer2(c1) (align_corners=True) -> `styles` style heads (heads 0-2 on c3 with 4 convs, 3-6 on p2 with 5,
// 7.. on p1 with 6; conv3x3 stride 2 + bias + LeakyReLU(0.01) down to 1 x 1, then EqualLinear) -> w[:, 0] = w0, w[:, i] = w0 + delta_i.
// Forward only: every call of the reference is under no_grad.
// The head count is the reference's style_count = 2 log2(image_resolution) - 2 (psp_encoders.py:143-156), 8..18 for 32..1024, and is
// independent of the input side R: the 512 and 1024 generators are fed from the same 256 x 256 crop, with 16 and 18 heads.  The
// entries without `_n` take styles = 2 floor(log2 R) - 2, the encoder whose image_resolution is its input side.
//
// Every conv and the head GEMMs are one implicit-GEMM kernel on exact-f32 MFMA (v_mfma_f32_16x16x4_f32), the 64 x 64 x 16 tile with
// the double-buffered K loop, the split over K and the fixed-order finish of idloss.hip.  BN1 sits in front of a zero-padded conv and
// is applied in the loader, PReLU in conv2's loader; BN2, the shortcut BN and the stem BN are folded on the host.  What this network
// adds:
//   * groups: one launch runs the same conv shape for several heads, blockIdx.y = (head, channel tile), each head with its own input
//     channels, filters, bias and output channels.  The first conv of a head group shares its input map and is one conv with
//     N = heads x 512; the deeper convs (8 x 8 down to 1 x 1 maps) and the EqualLinears are one grouped launch per depth;
//   * tap skipping: a head conv enumerates K over the taps that meet the map for at least one output pixel (4 of 9 for 2 x 2 -> 1 x 1,
//     the centre alone for 1 x 1 -> 1 x 1), so the filter slices of the other taps are never read.  Exact: those products are zeros;
//   * the lateral convs add the bilinear resample of the coarser map in their epilogue;
//   * the SE mean is one wave per (row, channel), lanes then wave_sum: a fixed order.
// No float atomics, no host synchronisation, everything on the given stream.
#include <string.h>

#include <algorithm>

#include "conv_tile.h"

namespace sgdfr {
namespace {

constexpr int kUnits = 24, kMinHeads = 8, kMaxHeads = 18, kMaxDepth = 6, kGroups = 3, kStyle = 512;
constexpr int kParkedHeads = 14;                   // the head vectors' two buffers hold at least this many heads per row
constexpr int kMinRes = 32, kMaxRes = 256, kMaxRows = 256;
constexpr int64_t kMaxPixels = 1LL << 24;           // rows * R * R: every element index of a 64-channel map stays below 2^31
constexpr int kTrunkParams = 3 + 10 * kUnits + 4;   // stem, units, the two lateral convs
constexpr int BN = 64;
// split K only below 192 output tiles, at most 512 / tiles slices: S * (output elements) <= 512 tiles of 64 x 64
constexpr int kSplitBelow = 192;
constexpr int64_t kPartElems = 512LL * BM * BN;

enum { LD_PLAIN = 0, LD_AFFINE = 1, LD_PRELU = 2 };
enum { EP_RAW = 0, EP_BIAS = 1, EP_BIAS_PRELU = 2, EP_BIAS_SE = 3, EP_BIAS_LRELU = 4, EP_BIAS_UP = 5 };

// ------------------------------------------------------------------ network geometry
struct Unit {
    int cin, d, stride, h, ho;          // input [cin, h, h] -> output [d, ho, ho]
    bool sc_conv;                       // shortcut conv1x1/2 + BN (in != depth); else MaxPool2d(1, stride)
};
static void make_units(Unit* u, int R) {
    const int depth[4] = {64, 128, 256, 512}, count[4] = {3, 4, 14, 3};
    int c = 64, h = R, i = 0;
    for (int s = 0; s < 4; ++s)
        for (int k = 0; k < count[s]; ++k, ++i) {
            Unit& x = u[i];
            x.cin = c, x.d = depth[s], x.stride = k == 0 ? 2 : 1, x.h = h;
            x.ho = (h - 1) / x.stride + 1;
            x.sc_conv = c != depth[s];
            c = depth[s], h = x.ho;
        }
}
static bool res_ok(int R) { return R >= kMinRes && R <= kMaxRes && R % 16 == 0; }
static bool styles_ok(int n) { return n >= kMinHeads && n <= kMaxHeads; }
// rows * R * R <= 2^24 also keeps the widest parked head map, 11 heads x 512 channels at R/8 = 88 R^2 floats per row, below 2^31
static bool size_ok(int rows, int R) { return res_ok(R) && rows >= 1 && rows <= kMaxRows && (int64_t)rows * R * R <= kMaxPixels; }
static int style_count(int R) {
    int l = 0;
    while ((2 << l) <= R) ++l;          // floor(log2 R)
    return 2 * l - 2;
}
struct Group {
    int lo, hi, depth, side;            // heads lo..hi-1 read a [512, side, side] map with `depth` convs
};
static void make_groups(Group* g, int R, int n) {
    g[0] = Group{0, 3, 4, R / 16}, g[1] = Group{3, 7, 5, R / 8}, g[2] = Group{7, n, 6, R / 4};
}
static int group_of(int head) { return head < 3 ? 0 : head < 7 ? 1 : 2; }
static int param_count(int R, int styles) {
    Group g[kGroups];
    make_groups(g, R, styles);
    int n = kTrunkParams;
    for (int i = 0; i < kGroups; ++i) n += (g[i].hi - g[i].lo) * (2 * g[i].depth + 2);
    return n;
}

// ------------------------------------------------------------------ weight pack
struct UnitPack {
    int64_t wf1, wf2, wfsc, s1, t1, a1, b2, bsc, f1, f2;
};
struct PackLayout {
    int64_t wf0, b0, a0;
    UnitPack u[kUnits];
    int64_t wl1, bl1, wl2, bl2;
    int64_t hw[kGroups][kMaxDepth], hb[kGroups][kMaxDepth];   // depth 0: [4608][G*512]; deeper: per head [4608][512]
    int64_t lw, lb, total;                                    // EqualLinear: per head [512][512] (scaled on the host), [512]
};
static PackLayout pack_layout(int R, int styles) {
    Unit us[kUnits];
    make_units(us, R);
    Group gs[kGroups];
    make_groups(gs, R, styles);
    PackLayout p;
    memset(&p, 0, sizeof(p));
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    p.wf0 = take(27 * 64), p.b0 = take(64), p.a0 = take(64);
    for (int i = 0; i < kUnits; ++i) {
        const Unit& u = us[i];
        UnitPack& q = p.u[i];
        q.wf1 = take((int64_t)u.cin * 9 * u.d);
        q.wf2 = take((int64_t)u.d * 9 * u.d);
        q.wfsc = u.sc_conv ? take((int64_t)u.cin * u.d) : -1;
        q.s1 = take(u.cin), q.t1 = take(u.cin), q.a1 = take(u.d), q.b2 = take(u.d);
        q.bsc = u.sc_conv ? take(u.d) : -1;
        q.f1 = take((int64_t)u.d / 16 * u.d), q.f2 = take((int64_t)u.d * (u.d / 16));
    }
    p.wl1 = take(256LL * kStyle), p.bl1 = take(kStyle), p.wl2 = take(128LL * kStyle), p.bl2 = take(kStyle);
    for (int g = 0; g < kGroups; ++g) {
        const int G = gs[g].hi - gs[g].lo;
        for (int k = 0; k < gs[g].depth; ++k) p.hw[g][k] = take(9LL * kStyle * kStyle * G), p.hb[g][k] = take((int64_t)kStyle * G);
    }
    const int n = styles;
    p.lw = take((int64_t)n * kStyle * kStyle), p.lb = take((int64_t)n * kStyle);
    p.total = o;
    return p;
}

// copy: dst[j] = src[j].  Else [k = ci*kk + r][col0 + co] of a matrix with ldn columns <- W[co][ci][r]
__global__ __launch_bounds__(kThreads) void e4e_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t count, int copy,
                                                            int cin, int cout, int kk, int ldn, int col0) {
    for (int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x; j < count; j += (int64_t)gridDim.x * kThreads) {
        if (copy) {
            dst[j] = src[j];
        } else {
            const int64_t K = (int64_t)cin * kk, k = j / cout, co = j - k * cout;
            dst[k * ldn + col0 + co] = src[co * K + k];
        }
    }
}

// ------------------------------------------------------------------ implicit-GEMM conv
// group g of row b: input channels at src + b*src_rs + g*src_gs, filters at wp + g*w_gs, bias at bias + g*N, output channels at
// out + b*out_rs + g*out_gs.  N, K are per group.
struct ConvArgs {
    const float* src;        // [Cin, Hs, Ws] per (row, group)
    const float* wp;         // [Cin * KS*KS][N] per group
    const float* lsc;        // LD_AFFINE: v * lsc[ci] + lsh[ci]; LD_PRELU: slope lsc[ci]
    const float* lsh;
    const float* bias;
    const float* slope;      // EP_BIAS_PRELU
    const float* aux;        // EP_BIAS_SE: c2 [N, Ho, Wo]; EP_BIAS_UP: the coarser map [N, auxH, auxW]; per row at aux_rs
    const float* gate;       // EP_BIAS_SE: g [N] per row at gate_rs
    float* out;              // [N, Ho, Wo] per (row, group)
    float* part;             // split K: [S][R * G * N * Ho * Wo]
    int64_t src_rs, src_gs, w_gs, out_rs, out_gs, aux_rs, gate_rs, part_elems;
    unsigned long long taps; // SKIP: tap t of the K enumeration is filter position (taps >> 4t) & 15
    float up_sy, up_sx;      // EP_BIAS_UP: (auxH - 1) / (Ho - 1), (auxW - 1) / (Wo - 1)
    int R, G, ntg, Hs, Ws, N, Ho, Wo, K, stride, pad, cps, epi, auxH, auxW, ntaps;
};

__device__ __forceinline__ void epilogue(const ConvArgs& a, int b, int g, int n, int p, float v) {
    const int64_t o = (int64_t)n * (a.Ho * a.Wo) + p;
    float r;
    switch (a.epi) {
        case EP_RAW: r = v; break;
        case EP_BIAS: r = v + a.bias[g * a.N + n]; break;
        case EP_BIAS_PRELU: {
            const float pre = v + a.bias[n];
            r = pre > 0.f ? pre : a.slope[n] * pre;
            break;
        }
        case EP_BIAS_SE: r = (a.aux[b * a.aux_rs + o] * a.gate[b * a.gate_rs + n]) + (v + a.bias[n]); break;
        case EP_BIAS_LRELU: {
            const float pre = v + a.bias[g * a.N + n];
            r = pre > 0.f ? pre : 0.01f * pre;
            break;
        }
        default: {   // EP_BIAS_UP: bilinear, align_corners=True, of aux at this pixel + (conv + bias)
            const int oh = p / a.Wo, ow = p - oh * a.Wo;
            const float fy = a.up_sy * (float)oh, fx = a.up_sx * (float)ow;
            const int y0 = min((int)fy, a.auxH - 1), x0 = min((int)fx, a.auxW - 1);
            const int y1 = min(y0 + 1, a.auxH - 1), x1 = min(x0 + 1, a.auxW - 1);
            const float ly = fminf(fmaxf(fy - (float)y0, 0.f), 1.f), lx = fminf(fmaxf(fx - (float)x0, 0.f), 1.f);
            const float* q = a.aux + b * a.aux_rs + (int64_t)n * (a.auxH * a.auxW);
            const float top = (1.f - lx) * q[y0 * a.auxW + x0] + lx * q[y0 * a.auxW + x1];
            const float bot = (1.f - lx) * q[y1 * a.auxW + x0] + lx * q[y1 * a.auxW + x1];
            r = ((1.f - ly) * top + ly * bot) + (v + a.bias[n]);
        }
    }
    a.out[b * a.out_rs + g * a.out_gs + o] = r;
}

template <int KS, int LOAD, bool SKIP>
__global__ __launch_bounds__(kThreads) void e4e_conv_kernel(ConvArgs a) {
    __shared__ ConvLds<BN> lds;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int g = blockIdx.y / a.ntg;
    const int m0 = blockIdx.x * BM, n0 = (blockIdx.y - g * a.ntg) * BN;
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
    const float* srcb = a.src + b * a.src_rs + g * a.src_gs;
    const float* wg = a.wp + g * a.w_gs;

    const int nchunks = (a.K + BK - 1) / BK;
    const int c0 = blockIdx.z * a.cps, c1 = min(nchunks, c0 + a.cps);
    float xr[4], wr[4];
    auto gload = [&](int c) {
        const int k0 = c * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + wv + 4 * i;      // uniform over the wave: one K row of both operands
            float v = 0.f, w = 0.f;
            if (k < a.K) {
                int ci, r;
                if (SKIP) {
                    ci = k / a.ntaps;
                    r = (int)((a.taps >> (4 * (k - ci * a.ntaps))) & 15);
                } else {
                    ci = k / (KS * KS), r = k - ci * (KS * KS);
                }
                const int kh = r / KS, kw = r - kh * KS;
                const int ih = oh * a.stride - a.pad + kh, iw = ow * a.stride - a.pad + kw;
                if (mvalid && ih >= 0 && ih < a.Hs && iw >= 0 && iw < a.Ws) {
                    const float s = srcb[(int64_t)ci * plane + ih * a.Ws + iw];
                    if (LOAD == LD_AFFINE) v = fmaf(s, a.lsc[ci], a.lsh[ci]);
                    else if (LOAD == LD_PRELU) v = s > 0.f ? s : a.lsc[ci] * s;
                    else v = s;
                }
                const int gn = n0 + lane;
                if (gn < a.N) w = wg[(int64_t)(ci * (KS * KS) + r) * a.N + gn];
            }
            xr[i] = v, wr[i] = w;
        }
    };
    auto sstore = [&](int buf) {
        store_x(lds.xs[buf], xr);
#pragma unroll
        for (int i = 0; i < 4; ++i) lds.ws[buf][wv + 4 * i][lane] = wr[i];
    };

    floatx4 acc[2][2];
    k_loop<BN>(lds, c0, c1, gload, sstore, acc);

    // the partials are [R * G, N, HWo]: (row, group) is the walk's row
    float* const slice = slice_of(a.part, a.part_elems);
    for_each_output<BN>(acc, m0, n0, M, a.N, HWo, [=](int bb, int gn, int p, float v) {
        if (slice)
            slice[(((int64_t)bb * a.G + g) * a.N + gn) * HWo + p] = v;
        else
            epilogue(a, bb, g, gn, p, v);
    });
}

// sum of the K slices in fixed order + the conv's epilogue
__global__ __launch_bounds__(kThreads) void e4e_finish_kernel(ConvArgs a, int S) {
    finish_slices(a.part, a.part_elems, S, a.N, a.Ho * a.Wo, [=](int bg, int n, int p, float v) {
        const int b = bg / a.G;
        epilogue(a, b, bg - b * a.G, n, p, v);
    });
}

// ------------------------------------------------------------------ SE gate
// mean[r, c] = mean_hw x[r, c]: one wave per (row, channel), lanes in fixed stride order, then wave_sum
__global__ __launch_bounds__(kThreads) void e4e_mean_kernel(const float* __restrict__ x, float* __restrict__ mean, int planes, int HW) {
    const int lane = threadIdx.x & 63, w = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6);
    if (w >= planes) return;            // uniform over the wave
    const float* q = x + (int64_t)w * HW;
    float s = 0.f;
    for (int p = lane; p < HW; p += kWave) s += q[p];
    s = wave_sum(s);
    if (lane == 0) mean[w] = s / (float)HW;
}

// h = relu(fc1 m); g = sigmoid(fc2 h): one block per row
__global__ __launch_bounds__(kThreads) void e4e_gate_kernel(const float* __restrict__ mean, int D, const float* __restrict__ f1,
                                                            const float* __restrict__ f2, float* __restrict__ gate) {
    __shared__ float sm[512], sh[32];
    const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6, Dr = D / 16;
    for (int c = t; c < D; c += kThreads) sm[c] = mean[(int64_t)r * D + c];
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
        gate[(int64_t)r * D + c] = 1.f / (1.f + expf(-z));
    }
}

// out = c2 g + shortcut, the shortcut being x itself or x[:, :, ::2, ::2] (MaxPool2d(1, stride))
__global__ __launch_bounds__(kThreads) void e4e_combine_kernel(const float* __restrict__ c2, const float* __restrict__ gate,
                                                               const float* __restrict__ x, float* __restrict__ out, int R, int D, int Ho,
                                                               int Hi, int stride) {
    const int HWo = Ho * Ho;
    const int64_t n = (int64_t)R * D * HWo;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int p = (int)(idx % HWo);
        const int64_t rc = idx / HWo;
        const int oh = p / Ho, ow = p - oh * Ho;
        const float sc = x[(rc * Hi + oh * stride) * Hi + ow * stride];
        out[idx] = (c2[idx] * gate[rc]) + sc;
    }
}

// w[:, 0] = w0; w[:, i] = w0 + delta_i
__global__ __launch_bounds__(kThreads) void e4e_wplus_kernel(const float* __restrict__ delta, float* __restrict__ w, int R, int n) {
    const int64_t total = (int64_t)R * n * kStyle;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int c = (int)(idx % kStyle), i = (int)((idx / kStyle) % n);
        const int64_t r = idx / ((int64_t)kStyle * n);
        const float w0 = delta[r * n * kStyle + c];
        w[idx] = i == 0 ? w0 : w0 + delta[idx];
    }
}

// ------------------------------------------------------------------ host side
static int launch_conv(const ConvArgs& a0, int ks, int load, bool skip, float* part, hipStream_t st) {
    ConvArgs a = a0;
    // the plan looks at the tiles of all groups.  A grid that already puts a block on three quarters of the 256 CUs runs whole: a
    // second block per CU does not pay for the pass over the partials.  Below that, up to 512 / tiles slices of at least 8 chunks.
    const int M = a.R * a.Ho * a.Wo, tiles = conv_tiles(M, a.N, BN) * a.G;
    const ConvPlan p = plan_conv(M, a.N, a.K, BN, tiles, tiles >= kSplitBelow);
    const int64_t out_elems = p.out_elems * a.G;
    SGDFR_REQUIRE(p.S == 1 || p.S * out_elems <= kPartElems, "e4e: split-K partials of %lld floats exceed the workspace",
                  (long long)(p.S * out_elems));
    a.cps = p.cps, a.ntg = p.nt;
    a.part = part;
    a.part_elems = out_elems;
    const dim3 grid(p.mt, p.nt * a.G, p.S);
    bool done = false;
#define SGDFR_E4E_CONV(KS_, LD_, SKIP_)                                                        \
    if (!done && ks == KS_ && load == LD_ && skip == SKIP_) {                                   \
        hipLaunchKernelGGL((e4e_conv_kernel<KS_, LD_, SKIP_>), grid, dim3(kThreads), 0, st, a); \
        done = true;                                                                            \
    }
    SGDFR_E4E_CONV(3, LD_PLAIN, false)     // stem
    SGDFR_E4E_CONV(3, LD_AFFINE, false)    // conv1 (BN1 in the load)
    SGDFR_E4E_CONV(3, LD_PRELU, false)     // conv2 (PReLU in the load)
    SGDFR_E4E_CONV(1, LD_PLAIN, false)     // shortcut and lateral convs, EqualLinears
    SGDFR_E4E_CONV(3, LD_PLAIN, true)      // head convs (live taps only)
#undef SGDFR_E4E_CONV
    SGDFR_REQUIRE(done, "e4e: no conv instance for k=%d load=%d skip=%d", ks, load, (int)skip);
    if (check_launch("e4e conv")) return 2;
    if (p.S > 1) {
        hipLaunchKernelGGL(e4e_finish_kernel, dim3(grid_1d(out_elems)), dim3(kThreads), 0, st, a, p.S);
        if (check_launch("e4e finish")) return 2;
    }
    return 0;
}

// the taps of a 3x3 / stride 2 / pad 1 conv on a side x side map that meet the map for at least one output pixel
static int live_taps(int side, unsigned long long& taps) {
    const int so = (side - 1) / 2 + 1;
    bool live[3];
    for (int k = 0; k < 3; ++k) {
        live[k] = false;
        for (int o = 0; o < so; ++o) live[k] = live[k] || (2 * o - 1 + k >= 0 && 2 * o - 1 + k < side);
    }
    int n = 0;
    taps = 0;
    for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw)
            if (live[kh] && live[kw]) taps |= (unsigned long long)(kh * 3 + kw) << (4 * n++);
    return n;
}

struct DebugLayout {
    int64_t stem, u0, u3, c1, c2, c3, p2, p1, h, total;
};
static DebugLayout debug_layout(int rows, int R, int styles) {
    DebugLayout d;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o += n; return r; };
    const int64_t r2 = (int64_t)rows * R * R;
    d.stem = take(64 * r2), d.u0 = take(64 * r2 / 4), d.u3 = take(128 * r2 / 16);
    d.c1 = take(128 * r2 / 16), d.c2 = take(256 * r2 / 64), d.c3 = take(512 * r2 / 256);
    d.p2 = take(512 * r2 / 64), d.p1 = take(512 * r2 / 16);
    d.h = take((int64_t)rows * styles * kStyle);
    d.total = o;
    return d;
}

struct WsLayout {
    int64_t part, act[2], p1, c2, mean, gate, t1, t2, t3, f2, f1, h, delta, total;   // float offsets
};
static WsLayout ws_layout(int rows, int R, int styles) {
    WsLayout w;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    const int64_t r2 = (int64_t)rows * R * R;
    w.part = take(kPartElems);
    // the two unit buffers and conv1's output hold [64, R, R] per row; behind the trunk the first two hold the head maps, the
    // widest of them the fine group's first conv: G heads x 512 channels at R/8 = 8 G R^2 per row.  7 heads (56 R^2) fit the unit
    // buffer; 9 and 11 heads (72 and 88 R^2) size it
    Group gs[kGroups];
    make_groups(gs, R, styles);
    const int64_t parked = std::max<int64_t>(64 * r2, (int64_t)(gs[2].hi - gs[2].lo) * kStyle * r2 / 64);
    w.act[0] = take(parked), w.act[1] = take(parked), w.p1 = take(64 * r2);
    w.c2 = take(64 * r2 / 4);
    w.mean = take((int64_t)rows * 512), w.gate = take((int64_t)rows * 512);
    w.t1 = take(128 * r2 / 16), w.t2 = take(256 * r2 / 64), w.t3 = take(512 * r2 / 256);
    w.f2 = take(512 * r2 / 64), w.f1 = take(512 * r2 / 16);
    const int held = std::max(styles, kParkedHeads);
    w.h = take((int64_t)rows * held * kStyle), w.delta = take((int64_t)rows * held * kStyle);
    w.total = o;
    return w;
}

}  // namespace
}  // namespace sgdfr

using namespace sgdfr;

extern "C" int sgdfr_e4e_style_count(int R) { return res_ok(R) ? style_count(R) : -1; }

extern "C" int sgdfr_e4e_param_count_n(int R, int styles) { return res_ok(R) && styles_ok(styles) ? param_count(R, styles) : -1; }

extern "C" int64_t sgdfr_e4e_pack_elems_n(int R, int styles) { return res_ok(R) && styles_ok(styles) ? pack_layout(R, styles).total : -1; }

extern "C" int64_t sgdfr_e4e_debug_elems_n(int rows, int R, int styles) {
    return size_ok(rows, R) && styles_ok(styles) ? debug_layout(rows, R, styles).total : -1;
}

extern "C" int64_t sgdfr_e4e_workspace_bytes_n(int rows, int R, int styles) {
    return size_ok(rows, R) && styles_ok(styles) ? ws_layout(rows, R, styles).total * (int64_t)sizeof(float) : -1;
}

// the entries without `_n`: the head count that follows the input side.  A bad R gets a count in range: the `_n` form refuses the R
static int own_styles(int R) { return res_ok(R) ? style_count(R) : kMinHeads; }
extern "C" int sgdfr_e4e_param_count(int R) { return sgdfr_e4e_param_count_n(R, own_styles(R)); }

extern "C" int64_t sgdfr_e4e_pack_elems(int R) { return sgdfr_e4e_pack_elems_n(R, own_styles(R)); }

extern "C" int64_t sgdfr_e4e_debug_elems(int rows, int R) { return sgdfr_e4e_debug_elems_n(rows, R, own_styles(R)); }

extern "C" int64_t sgdfr_e4e_workspace_bytes(int rows, int R) { return sgdfr_e4e_workspace_bytes_n(rows, R, own_styles(R)); }

extern "C" int sgdfr_e4e_prepack_n_f32(const float* const* params, int R, int styles, float* pack, void* stream) {
    SGDFR_REQUIRE(res_ok(R), "e4e_prepack: resolution %d (a multiple of 16 in %d..%d)", R, kMinRes, kMaxRes);
    SGDFR_REQUIRE(styles_ok(styles), "e4e_prepack: %d style heads (%d..%d)", styles, kMinHeads, kMaxHeads);
    SGDFR_REQUIRE(params && pack, "e4e_prepack: null pointer");
    Unit us[kUnits];
    make_units(us, R);
    Group gs[kGroups];
    make_groups(gs, R, styles);
    const int count = param_count(R, styles);
    for (int i = 0; i < count; ++i) {
        const int u = (i - 3) / 10, j = (i - 3) % 10;
        const bool optional = i >= 3 && i < 3 + 10 * kUnits && j >= 8 && !us[u].sc_conv;   // shortcut conv of an identity unit
        SGDFR_REQUIRE(optional || params[i], "e4e_prepack: parameter %d is null", i);
    }
    const PackLayout pl = pack_layout(R, styles);
    hipStream_t st = as_stream(stream);
    auto copy = [&](const float* src, int64_t dst, int64_t n) {
        hipLaunchKernelGGL(e4e_pack_kernel, dim3(grid_1d(n)), dim3(kThreads), 0, st, src, pack + dst, n, 1, 0, 0, 0, 0, 0);
        return check_launch("e4e prepack");
    };
    auto gemm = [&](const float* src, int64_t dst, int cin, int cout, int kk, int ldn, int col0) {
        const int64_t n = (int64_t)cin * kk * cout;
        hipLaunchKernelGGL(e4e_pack_kernel, dim3(grid_1d(n)), dim3(kThreads), 0, st, src, pack + dst, n, 0, cin, cout, kk, ldn, col0);
        return check_launch("e4e prepack");
    };
    int rc = 0;
    rc |= gemm(params[0], pl.wf0, 3, 64, 9, 64, 0);
    rc |= copy(params[1], pl.b0, 64);
    rc |= copy(params[2], pl.a0, 64);
    for (int i = 0; i < kUnits && !rc; ++i) {
        const Unit& u = us[i];
        const UnitPack& q = pl.u[i];
        const float* const* P = params + 3 + 10 * i;   // s1, t1, w1, a1, w2, b2, f1, f2, wsc, bsc
        rc |= copy(P[0], q.s1, u.cin);
        rc |= copy(P[1], q.t1, u.cin);
        rc |= gemm(P[2], q.wf1, u.cin, u.d, 9, u.d, 0);
        rc |= copy(P[3], q.a1, u.d);
        rc |= gemm(P[4], q.wf2, u.d, u.d, 9, u.d, 0);
        rc |= copy(P[5], q.b2, u.d);
        rc |= copy(P[6], q.f1, (int64_t)u.d / 16 * u.d);
        rc |= copy(P[7], q.f2, (int64_t)u.d * (u.d / 16));
        if (u.sc_conv) {
            rc |= gemm(P[8], q.wfsc, u.cin, u.d, 1, u.d, 0);
            rc |= copy(P[9], q.bsc, u.d);
        }
    }
    const float* const* P = params + 3 + 10 * kUnits;
    if (!rc) {
        rc |= gemm(P[0], pl.wl1, 256, kStyle, 1, kStyle, 0);
        rc |= copy(P[1], pl.bl1, kStyle);
        rc |= gemm(P[2], pl.wl2, 128, kStyle, 1, kStyle, 0);
        rc |= copy(P[3], pl.bl2, kStyle);
    }
    P += 4;
    const int n = styles;
    for (int h = 0; h < n && !rc; ++h) {
        const int g = group_of(h), j = h - gs[g].lo, G = gs[g].hi - gs[g].lo;
        // the first conv: this head's 512 columns of the group's [4608][G*512] matrix
        rc |= gemm(P[0], pl.hw[g][0], kStyle, kStyle, 9, G * kStyle, j * kStyle);
        rc |= copy(P[1], pl.hb[g][0] + (int64_t)j * kStyle, kStyle);
        for (int k = 1; k < gs[g].depth; ++k) {
            rc |= gemm(P[2 * k], pl.hw[g][k] + (int64_t)j * 9 * kStyle * kStyle, kStyle, kStyle, 9, kStyle, 0);
            rc |= copy(P[2 * k + 1], pl.hb[g][k] + (int64_t)j * kStyle, kStyle);
        }
        P += 2 * gs[g].depth;
        rc |= gemm(P[0], pl.lw + (int64_t)h * kStyle * kStyle, kStyle, kStyle, 1, kStyle, 0);
        rc |= copy(P[1], pl.lb + (int64_t)h * kStyle, kStyle);
        P += 2;
    }
    return rc ? 2 : 0;
}

extern "C" int sgdfr_e4e_prepack_f32(const float* const* params, int R, float* pack, void* stream) {
    return sgdfr_e4e_prepack_n_f32(params, R, own_styles(R), pack, stream);
}

extern "C" int sgdfr_e4e_forward_n_f32(const float* x, int rows, int R, int styles, const float* pack, float* w, float* debug,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(res_ok(R), "e4e_forward: resolution %d (a multiple of 16 in %d..%d, so that every head ends at 1x1)", R, kMinRes, kMaxRes);
    SGDFR_REQUIRE(styles_ok(styles), "e4e_forward: %d style heads (%d..%d)", styles, kMinHeads, kMaxHeads);
    SGDFR_REQUIRE(size_ok(rows, R), "e4e_forward: %d rows at resolution %d (1..%d rows, rows*R*R <= 2^24)", rows, R, kMaxRows);
    SGDFR_REQUIRE(x && pack && w && workspace, "e4e_forward: null pointer");
    const WsLayout wl = ws_layout(rows, R, styles);
    SGDFR_REQUIRE(wl.total * (int64_t)sizeof(float) <= workspace_bytes, "e4e_forward: workspace of %lld bytes, %d rows at %d need %lld",
                  (long long)workspace_bytes, rows, R, (long long)(wl.total * (int64_t)sizeof(float)));
    Unit us[kUnits];
    make_units(us, R);
    Group gs[kGroups];
    make_groups(gs, R, styles);
    const PackLayout pl = pack_layout(R, styles);
    const DebugLayout dl = debug_layout(rows, R, styles);
    const int n_styles = styles;
    float* wsf = reinterpret_cast<float*>(workspace);
    float* part = wsf + wl.part;
    hipStream_t st = as_stream(stream);
    auto tap = [&](int64_t dst, const float* src, int64_t n) {
        if (!debug) return 0;
        if (hipMemcpyAsync(debug + dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
            set_error("e4e_forward: debug copy failed");
            return 2;
        }
        return 0;
    };
    auto conv_args = [&](const float* src, int cin, int hs, const float* wp, int N, int ho, int ksq, int stride, int pad) {
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.src = src, a.src_rs = (int64_t)cin * hs * hs, a.wp = wp;
        a.R = rows, a.G = 1, a.Hs = a.Ws = hs, a.N = N, a.Ho = a.Wo = ho, a.K = cin * ksq, a.stride = stride, a.pad = pad;
        a.out_rs = (int64_t)N * ho * ho;
        return a;
    };

    // stem
    ConvArgs a = conv_args(x, 3, R, pack + pl.wf0, 64, R, 9, 1, 1);
    a.bias = pack + pl.b0, a.slope = pack + pl.a0, a.epi = EP_BIAS_PRELU, a.out = wsf + wl.act[0];
    if (launch_conv(a, 3, LD_PLAIN, false, part, st)) return 2;
    if (tap(dl.stem, wsf + wl.act[0], (int64_t)rows * 64 * R * R)) return 2;

    const float* cur = wsf + wl.act[0];
    int flip = 1;
    for (int i = 0; i < kUnits; ++i) {
        const Unit& u = us[i];
        const UnitPack& q = pl.u[i];
        const int64_t out_elems = (int64_t)rows * u.d * u.ho * u.ho;
        // the taps behind units 6, 20 and 23 live in buffers of their own: the lateral convs and the heads read them later
        float* aout = i == 6 ? wsf + wl.t1 : i == 20 ? wsf + wl.t2 : i == 23 ? wsf + wl.t3 : wsf + wl.act[flip];
        float* p1 = wsf + wl.p1;
        float* c2 = wsf + wl.c2;
        // conv1: BN1 in the load, raw pre-activation out
        a = conv_args(cur, u.cin, u.h, pack + q.wf1, u.d, u.h, 9, 1, 1);
        a.lsc = pack + q.s1, a.lsh = pack + q.t1, a.epi = EP_RAW, a.out = p1;
        if (launch_conv(a, 3, LD_AFFINE, false, part, st)) return 2;
        // conv2 at the unit's stride: PReLU in the load, folded BN2 bias out
        a = conv_args(p1, u.d, u.h, pack + q.wf2, u.d, u.ho, 9, u.stride, 1);
        a.lsc = pack + q.a1, a.epi = EP_BIAS, a.bias = pack + q.b2, a.out = c2;
        if (launch_conv(a, 3, LD_PRELU, false, part, st)) return 2;
        const int planes = rows * u.d;
        hipLaunchKernelGGL(e4e_mean_kernel, dim3((planes + 3) / 4), dim3(kThreads), 0, st, c2, wsf + wl.mean, planes, u.ho * u.ho);
        if (check_launch("e4e mean")) return 2;
        hipLaunchKernelGGL(e4e_gate_kernel, dim3(rows), dim3(kThreads), 0, st, wsf + wl.mean, u.d, pack + q.f1, pack + q.f2, wsf + wl.gate);
        if (check_launch("e4e gate")) return 2;
        if (u.sc_conv) {       // out = shortcut conv (folded BN) + c2 g in the conv's epilogue
            a = conv_args(cur, u.cin, u.h, pack + q.wfsc, u.d, u.ho, 1, 2, 0);
            a.epi = EP_BIAS_SE, a.bias = pack + q.bsc, a.aux = c2, a.aux_rs = a.out_rs, a.gate = wsf + wl.gate, a.gate_rs = u.d, a.out = aout;
            if (launch_conv(a, 1, LD_PLAIN, false, part, st)) return 2;
        } else {
            hipLaunchKernelGGL(e4e_combine_kernel, dim3(grid_1d(out_elems)), dim3(kThreads), 0, st, c2, wsf + wl.gate, cur, aout, rows, u.d,
                               u.ho, u.h, u.stride);
            if (check_launch("e4e combine")) return 2;
        }
        if (i == 0 && tap(dl.u0, aout, out_elems)) return 2;
        if (i == 3 && tap(dl.u3, aout, out_elems)) return 2;
        if (i == 6 && tap(dl.c1, aout, out_elems)) return 2;
        if (i == 20 && tap(dl.c2, aout, out_elems)) return 2;
        if (i == 23 && tap(dl.c3, aout, out_elems)) return 2;
        if (aout == wsf + wl.act[flip]) flip ^= 1;
        cur = aout;
    }

    // FPN merge: the lateral conv1x1 + bias with the bilinear resample of the coarser map added in its epilogue
    const int s1 = R / 4, s2 = R / 8, s3 = R / 16;
    a = conv_args(wsf + wl.t2, 256, s2, pack + pl.wl1, kStyle, s2, 1, 1, 0);
    a.epi = EP_BIAS_UP, a.bias = pack + pl.bl1, a.aux = wsf + wl.t3, a.aux_rs = (int64_t)kStyle * s3 * s3, a.auxH = a.auxW = s3;
    a.up_sy = a.up_sx = (float)(s3 - 1) / (float)(s2 - 1), a.out = wsf + wl.f2;
    if (launch_conv(a, 1, LD_PLAIN, false, part, st)) return 2;
    if (tap(dl.p2, wsf + wl.f2, (int64_t)rows * kStyle * s2 * s2)) return 2;
    a = conv_args(wsf + wl.t1, 128, s1, pack + pl.wl2, kStyle, s1, 1, 1, 0);
    a.epi = EP_BIAS_UP, a.bias = pack + pl.bl2, a.aux = wsf + wl.f2, a.aux_rs = (int64_t)kStyle * s2 * s2, a.auxH = a.auxW = s2;
    a.up_sy = a.up_sx = (float)(s2 - 1) / (float)(s1 - 1), a.out = wsf + wl.f1;
    if (launch_conv(a, 1, LD_PLAIN, false, part, st)) return 2;
    if (tap(dl.p1, wsf + wl.f1, (int64_t)rows * kStyle * s1 * s1)) return 2;

    // style heads, one group per feature map: the trunk's two unit buffers hold the head maps now
    float* hvec = wsf + wl.h;               // [rows, n_styles, 512]: every head's vector in front of its EqualLinear
    const float* feat[kGroups] = {wsf + wl.t3, wsf + wl.f2, wsf + wl.f1};
    for (int g = 0; g < kGroups; ++g) {
        const Group& grp = gs[g];
        const int G = grp.hi - grp.lo;
        const float* src = feat[g];
        int side = grp.side, hb = 0;
        for (int k = 0; k < grp.depth; ++k) {
            const int so = (side - 1) / 2 + 1;
            const bool last = k == grp.depth - 1;
            SGDFR_REQUIRE(!last || so == 1, "e4e_forward: a head of group %d ends at %dx%d, not 1x1", g, so, so);
            float* dst = last ? hvec + (int64_t)grp.lo * kStyle : wsf + wl.act[hb];
            a = conv_args(src, kStyle, side, pack + pl.hw[g][k], k == 0 ? G * kStyle : kStyle, so, 9, 2, 1);
            a.ntaps = live_taps(side, a.taps);
            a.K = kStyle * a.ntaps;
            a.bias = pack + pl.hb[g][k], a.epi = EP_BIAS_LRELU, a.out = dst;
            a.out_rs = last ? (int64_t)n_styles * kStyle : (int64_t)G * kStyle * so * so;
            if (k > 0) {
                a.G = G;
                a.src_rs = (int64_t)G * kStyle * side * side, a.src_gs = (int64_t)kStyle * side * side;
                a.w_gs = 9LL * kStyle * kStyle, a.out_gs = (int64_t)kStyle * so * so;
            }
            if (launch_conv(a, 3, LD_PLAIN, true, part, st)) return 2;
            src = dst, side = so, hb ^= 1;
        }
    }
    if (tap(dl.h, hvec, (int64_t)rows * n_styles * kStyle)) return 2;

    // the EqualLinears of every head in one grouped launch, then w0 + delta
    a = conv_args(hvec, kStyle, 1, pack + pl.lw, kStyle, 1, 1, 1, 0);
    a.G = n_styles, a.src_rs = (int64_t)n_styles * kStyle, a.src_gs = kStyle, a.w_gs = (int64_t)kStyle * kStyle;
    a.bias = pack + pl.lb, a.epi = EP_BIAS, a.out = wsf + wl.delta, a.out_rs = (int64_t)n_styles * kStyle, a.out_gs = kStyle;
    if (launch_conv(a, 1, LD_PLAIN, false, part, st)) return 2;
    hipLaunchKernelGGL(e4e_wplus_kernel, dim3(grid_1d((int64_t)rows * n_styles * kStyle)), dim3(kThreads), 0, st, wsf + wl.delta, w, rows,
                       n_styles);
    return check_launch("e4e w plus");
}

extern "C" int sgdfr_e4e_forward_f32(const float* x, int rows, int R, const float* pack, float* w, float* debug, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    return sgdfr_e4e_forward_n_f32(x, rows, R, own_styles(R), pack, w, debug, workspace, workspace_bytes, stream);
}
