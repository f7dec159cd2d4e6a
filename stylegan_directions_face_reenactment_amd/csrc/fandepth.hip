// The depth head of the 3D landmark type in eval mode (libs/face_models/fan_model/models.py:58-95 Bottleneck and :205-265
// ResNetDepth, layers [3, 8, 36, 3]): crop [B,3,256,256] in [0,1] and the 68 drawn maps [B,68,256,256] -> conv7x7/2 71->64 + BN +
// ReLU -> max-pool 3x3/2 -> 50 bottlenecks (1x1 -> 3x3 at the stride -> 1x1, + shortcut, ReLU) -> AvgPool2d(7) on the 8x8 map
// (rows and columns 0..6 only) -> Linear 2048->68: one depth per landmark.  Forward only: nothing is kept for a backward.
//
// Every one of the 155 convs and the linear layer is one implicit-GEMM kernel on exact-f32 MFMA (v_mfma_f32_16x16x4_f32), the
// 64 x 64 x 16 tile of conv_tile.h with its split over K and fixed-order finish; deca.hip runs a ResNet-50 of the same block
// shape.  All 155 BatchNorms are folded into filters + bias on the host (landmarks.ResNetDepth.folded).  What this network adds:
// the stem gathers its 71 input channels from two tensors (channels 0..2 from the crop, 3..70 from the maps), so the reference's
// torch.cat never exists in memory; K = 71 * 49 = 3479 leaves 7 valid rows in the last chunk, and the linear layer's N = 68 leaves
// 4 valid columns in the second channel tile.  No float atomics, no host synchronisation, everything on the given stream.
#include <string.h>

#include <algorithm>

#include "conv_tile.h"

namespace sgdfr {
namespace {

constexpr int kBlocks = 3 + 8 + 36 + 3;
constexpr int kIn = 256, kInPlane = kIn * kIn;
constexpr int kCropC = 3, kMapC = 68, kInC = kCropC + kMapC;
constexpr int kStem = 128, kPool = 64, kLast = 8;
constexpr int kFeat = 2048, kOut = 68;
constexpr int kParams = 2 + 6 * kBlocks + 2 * 4 + 2;     // pointers sgdfr_fandepth_prepack_f32 takes
constexpr int kMaxRows = 256;
constexpr int BN = 64;
// split K only below 512 output tiles, at most 512 / tiles slices: S * (output elements) <= 512 tiles
constexpr int64_t kPartElems = 512LL * BM * BN;

// ------------------------------------------------------------------ network geometry
struct Block {
    int cin, p, stride, h, ho;   // input [cin, h, h] -> conv1 [p, h, h] -> conv2 [p, ho, ho] -> conv3 [4p, ho, ho]
    bool ds;                     // projection shortcut conv1x1 at the stride + BN; else identity
};
static void make_blocks(Block* b) {
    const int planes[4] = {64, 128, 256, 512}, count[4] = {3, 8, 36, 3};
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
    int64_t w1, b1, w2, b2, w3, b3, wd, bd;
};
struct PackLayout {
    int64_t w0, b0;
    BlockPack u[kBlocks];
    int64_t w_fc, b_fc, total;
};
static PackLayout pack_layout() {
    Block bs[kBlocks];
    make_blocks(bs);
    PackLayout p;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    p.w0 = take((int64_t)kInC * 49 * 64), p.b0 = take(64);
    for (int i = 0; i < kBlocks; ++i) {
        const Block& u = bs[i];
        BlockPack& q = p.u[i];
        const int64_t c4 = 4LL * u.p;
        q.w1 = take((int64_t)u.cin * u.p), q.b1 = take(u.p);
        q.w2 = take(9LL * u.p * u.p), q.b2 = take(u.p);
        q.w3 = take(u.p * c4), q.b3 = take(c4);
        q.wd = u.ds ? take(u.cin * c4) : -1;
        q.bd = u.ds ? take(c4) : -1;
    }
    p.w_fc = take((int64_t)kFeat * kOut), p.b_fc = take(kOut);
    p.total = o;
    return p;
}

// copy: dst[j] = src[j].  Else [k = ci*kk + r][co] <- W[co][ci][r]
__global__ __launch_bounds__(kThreads) void fandepth_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int64_t count,
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
    const float* src;        // [R, C1, Hs, Ws]: input channels 0 .. C1-1
    const float* src2;       // TWO: [R, C - C1, Hs, Ws]: input channels C1 .. C-1, C = K / (KS*KS)
    const float* wp;         // [K][N]
    const float* bias;       // + bias[n]
    const float* aux;        // + aux at the output's own index (NULL: none)
    float* out;              // [R, N, Ho, Wo]
    float* part;             // split K: [S][R*N*Ho*Wo]
    int64_t part_elems;
    int R, Hs, Ws, N, Ho, Wo, K, C1, stride, pad, cps, relu;
};

__device__ __forceinline__ void epilogue(const ConvArgs& a, int b, int n, int p, float v) {
    const int64_t o = ((int64_t)b * a.N + n) * (a.Ho * a.Wo) + p;
    v += a.bias[n];
    if (a.aux) v += a.aux[o];
    a.out[o] = a.relu ? fmaxf(v, 0.f) : v;
}

template <int KS, bool TWO>
__global__ __launch_bounds__(kThreads) void fandepth_conv_kernel(ConvArgs a) {
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
    const float* srcb = a.src + (int64_t)b * a.C1 * plane;
    const float* src2b = TWO ? a.src2 + (int64_t)b * (a.K / (KS * KS) - a.C1) * plane : nullptr;

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
                const int ci = k / (KS * KS), r = k - ci * (KS * KS), kh = r / KS, kw = r - kh * KS;
                const int ih = oh * a.stride - a.pad + kh, iw = ow * a.stride - a.pad + kw;
                if (mvalid && ih >= 0 && ih < a.Hs && iw >= 0 && iw < a.Ws) {
                    const float* pl = (TWO && ci >= a.C1) ? src2b + (ci - a.C1) * plane : srcb + ci * plane;   // ci is uniform over the wave
                    v = pl[ih * a.Ws + iw];
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
__global__ __launch_bounds__(kThreads) void fandepth_finish_kernel(ConvArgs a, int S) {
    finish_slices(a.part, a.part_elems, S, a.N, a.Ho * a.Wo, [=](int b, int n, int p, float v) { epilogue(a, b, n, p, v); });
}

// ------------------------------------------------------------------ max-pool 3x3 / 2, pad 1 (128 -> 64)
// the padding never wins: only taps inside the map are compared (the centre tap always is)
__global__ __launch_bounds__(kThreads) void fandepth_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t planes) {
    const int64_t n = planes * kPool * kPool;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const int j = (int)(idx % kPool), i = (int)((idx / kPool) % kPool);
        const float* pl = in + (idx / (kPool * kPool)) * (kStem * kStem);
        float best = pl[(2 * i) * kStem + 2 * j];
        for (int kh = 0; kh < 3; ++kh) {
            const int y = 2 * i - 1 + kh;
            if (y < 0 || y >= kStem) continue;
            for (int kw = 0; kw < 3; ++kw) {
                const int xx = 2 * j - 1 + kw;
                if (xx < 0 || xx >= kStem) continue;
                best = fmaxf(best, pl[y * kStem + xx]);
            }
        }
        out[idx] = best;
    }
}

// ------------------------------------------------------------------ AvgPool2d(7) on the 8x8 map: rows and columns 0..6
__global__ __launch_bounds__(kThreads) void fandepth_avg_kernel(const float* __restrict__ in, float* __restrict__ feat, int64_t n) {
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * kThreads) {
        const float* p = in + idx * (kLast * kLast);
        float s = 0.f;
        for (int i = 0; i < 7; ++i)
            for (int j = 0; j < 7; ++j) s += p[i * kLast + j];
        feat[idx] = s / 49.f;
    }
}

// ------------------------------------------------------------------ host side
static int launch_conv(const ConvArgs& a0, int ks, bool two, float* part, hipStream_t st) {
    ConvArgs a = a0;
    // The number of K slices follows the output tiles, i.e. the layer and the row count, nothing else.
    const int M = a.R * a.Ho * a.Wo;
    const ConvPlan p = plan_conv(M, a.N, a.K, BN, conv_tiles(M, a.N, BN));
    SGDFR_REQUIRE(p.S == 1 || p.S * p.out_elems <= kPartElems, "fandepth: split-K partials of %lld floats exceed the workspace",
                  (long long)(p.S * p.out_elems));
    a.cps = p.cps;
    a.part = part;
    a.part_elems = p.out_elems;
    const dim3 grid(p.mt, p.nt, p.S);
    if (ks == 7 && two)
        hipLaunchKernelGGL((fandepth_conv_kernel<7, true>), grid, dim3(kThreads), 0, st, a);      // stem
    else if (ks == 3 && !two)
        hipLaunchKernelGGL((fandepth_conv_kernel<3, false>), grid, dim3(kThreads), 0, st, a);     // conv2
    else if (ks == 1 && !two)
        hipLaunchKernelGGL((fandepth_conv_kernel<1, false>), grid, dim3(kThreads), 0, st, a);     // conv1, conv3, projection, fc
    else
        SGDFR_REQUIRE(false, "fandepth: no conv instance for k=%d two=%d", ks, (int)two);
    if (check_launch("fandepth conv")) return 2;
    if (p.S > 1) {
        hipLaunchKernelGGL(fandepth_finish_kernel, dim3(grid_1d(p.out_elems)), dim3(kThreads), 0, st, a, p.S);
        if (check_launch("fandepth finish")) return 2;
    }
    return 0;
}

constexpr int64_t kMaxAct = 64LL * kStem * kStem;   // largest activation per row (stem output = layer1's outputs)
struct WsLayout {
    int64_t part, act[5], feat, total;   // float offsets
};
static WsLayout ws_layout(int rows) {
    WsLayout w;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t r = o; o = align64(o + n); return r; };
    w.part = take(kPartElems);
    for (int i = 0; i < 5; ++i) w.act[i] = take((int64_t)rows * kMaxAct);
    w.feat = take((int64_t)rows * kFeat);
    w.total = o;
    return w;
}

// debug stage outputs, each [rows, ...]: stem, pool, the output of each layer, pooled features
struct DebugLayout {
    int64_t stem, pool, layer[4], feat, total;
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
        d.layer[s] = take((int64_t)rows * (256 << s) * h * h);
    }
    d.feat = take((int64_t)rows * kFeat);
    d.total = o;
    return d;
}

static bool rows_ok(int rows) { return rows >= 1 && rows <= kMaxRows; }

static ConvArgs conv_args(const float* src, int Hs, const float* wp, const float* bias, int K, int N, int Ho, int stride, int pad, int relu,
                          float* out, int R) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.src = src, a.wp = wp, a.bias = bias, a.out = out;
    a.R = R, a.Hs = a.Ws = Hs, a.N = N, a.Ho = a.Wo = Ho, a.K = K, a.stride = stride, a.pad = pad, a.relu = relu;
    a.C1 = K / ((pad * 2 + 1) * (pad * 2 + 1));      // one source: all channels (pad = (k - 1) / 2 for every conv here)
    return a;
}

}  // namespace
}  // namespace sgdfr

using namespace sgdfr;

extern "C" int64_t sgdfr_fandepth_pack_elems(void) { return pack_layout().total; }

extern "C" int64_t sgdfr_fandepth_debug_elems(int rows) {
    if (!rows_ok(rows)) return -1;
    return debug_layout(rows).total;
}

extern "C" int64_t sgdfr_fandepth_workspace_bytes(int rows) {
    if (!rows_ok(rows)) return -1;
    return ws_layout(rows).total * (int64_t)sizeof(float);
}

extern "C" int sgdfr_fandepth_prepack_f32(const float* const* params, float* pack, void* stream) {
    SGDFR_REQUIRE(params && pack, "fandepth_prepack: null pointer");
    for (int i = 0; i < kParams; ++i) SGDFR_REQUIRE(params[i], "fandepth_prepack: parameter %d is null", i);
    Block bs[kBlocks];
    make_blocks(bs);
    const PackLayout pl = pack_layout();
    hipStream_t st = as_stream(stream);
    auto seg = [&](const float* src, int64_t dst, int64_t count, int copy, int cin, int cout, int kk) {
        hipLaunchKernelGGL(fandepth_pack_kernel, dim3(grid_1d(count)), dim3(kThreads), 0, st, src, pack + dst, count, copy, cin, cout, kk);
        return check_launch("fandepth prepack");
    };
    int rc = 0;
    rc |= seg(params[0], pl.w0, (int64_t)kInC * 49 * 64, 0, kInC, 64, 49);
    rc |= seg(params[1], pl.b0, 64, 1, 0, 0, 0);
    const float* const* P = params + 2;      // per block w1, b1, w2, b2, w3, b3 and, with a projection, wd, bd
    for (int i = 0; i < kBlocks && !rc; ++i) {
        const Block& u = bs[i];
        const BlockPack& q = pl.u[i];
        const int c4 = 4 * u.p;
        rc |= seg(P[0], q.w1, (int64_t)u.cin * u.p, 0, u.cin, u.p, 1);
        rc |= seg(P[1], q.b1, u.p, 1, 0, 0, 0);
        rc |= seg(P[2], q.w2, 9LL * u.p * u.p, 0, u.p, u.p, 9);
        rc |= seg(P[3], q.b2, u.p, 1, 0, 0, 0);
        rc |= seg(P[4], q.w3, (int64_t)u.p * c4, 0, u.p, c4, 1);
        rc |= seg(P[5], q.b3, c4, 1, 0, 0, 0);
        P += 6;
        if (u.ds) {
            rc |= seg(P[0], q.wd, (int64_t)u.cin * c4, 0, u.cin, c4, 1);
            rc |= seg(P[1], q.bd, c4, 1, 0, 0, 0);
            P += 2;
        }
    }
    if (!rc) rc |= seg(P[0], pl.w_fc, (int64_t)kFeat * kOut, 0, kFeat, kOut, 1);
    if (!rc) rc |= seg(P[1], pl.b_fc, kOut, 1, 0, 0, 0);
    return rc ? 2 : 0;
}

extern "C" int sgdfr_fandepth_network_f32(const float* crop, const float* maps, int rows, const float* pack, float* depth, float* debug,
                                          void* workspace, int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(rows_ok(rows), "fandepth_network: unsupported size (%d rows)", rows);
    SGDFR_REQUIRE(crop && maps && pack && depth && workspace, "fandepth_network: null pointer");
    const int R = rows;
    const WsLayout wl = ws_layout(R);
    SGDFR_REQUIRE(wl.total * (int64_t)sizeof(float) <= workspace_bytes, "fandepth_network: workspace of %lld bytes, %d rows need %lld",
                  (long long)workspace_bytes, R, (long long)(wl.total * (int64_t)sizeof(float)));
    Block bs[kBlocks];
    make_blocks(bs);
    const PackLayout pl = pack_layout();
    const DebugLayout dl = debug_layout(R);
    float* wsf = reinterpret_cast<float*>(workspace);
    float* part = wsf + wl.part;
    hipStream_t st = as_stream(stream);
    auto dump = [&](int64_t off, const float* src, int64_t n) {
        if (!debug) return 0;
        if (hipMemcpyAsync(debug + off, src, n * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
            set_error("fandepth_network: debug copy failed");
            return 2;
        }
        return 0;
    };

    float* A[5];
    for (int i = 0; i < 5; ++i) A[i] = wsf + wl.act[i];
    ConvArgs a = conv_args(crop, kIn, pack + pl.w0, pack + pl.b0, kInC * 49, 64, kStem, 2, 3, 1, A[0], R);
    a.C1 = kCropC, a.src2 = maps;
    if (launch_conv(a, 7, true, part, st)) return 2;
    if (dump(dl.stem, A[0], (int64_t)R * 64 * kStem * kStem)) return 2;
    hipLaunchKernelGGL(fandepth_pool_kernel, dim3(grid_1d((int64_t)R * 64 * kPool * kPool)), dim3(kThreads), 0, st, A[0], A[1],
                       (int64_t)R * 64);
    if (check_launch("fandepth pool")) return 2;
    if (dump(dl.pool, A[1], (int64_t)R * 64 * kPool * kPool)) return 2;

    int cur = 1, stage = -1;
    for (int i = 0; i < kBlocks; ++i) {
        const Block& u = bs[i];
        const BlockPack& q = pl.u[i];
        const int c4 = 4 * u.p;
        float* in = A[cur];
        float* out = A[cur ^ 1];
        float *t1 = A[2], *t2 = A[3], *res = A[4];
        a = conv_args(in, u.h, pack + q.w1, pack + q.b1, u.cin, u.p, u.h, 1, 0, 1, t1, R);
        if (launch_conv(a, 1, false, part, st)) return 2;
        a = conv_args(t1, u.h, pack + q.w2, pack + q.b2, 9 * u.p, u.p, u.ho, u.stride, 1, 1, t2, R);
        if (launch_conv(a, 3, false, part, st)) return 2;
        if (u.ds) {
            ++stage;
            a = conv_args(in, u.h, pack + q.wd, pack + q.bd, u.cin, c4, u.ho, u.stride, 0, 0, res, R);
            if (launch_conv(a, 1, false, part, st)) return 2;
        }
        a = conv_args(t2, u.ho, pack + q.w3, pack + q.b3, u.p, c4, u.ho, 1, 0, 1, out, R);
        a.aux = u.ds ? res : in;
        if (launch_conv(a, 1, false, part, st)) return 2;
        cur ^= 1;
        if (i + 1 == kBlocks || bs[i + 1].ds)
            if (dump(dl.layer[stage], out, (int64_t)R * c4 * u.ho * u.ho)) return 2;
    }

    float* feat = wsf + wl.feat;
    hipLaunchKernelGGL(fandepth_avg_kernel, dim3(grid_1d((int64_t)R * kFeat)), dim3(kThreads), 0, st, A[cur], feat, (int64_t)R * kFeat);
    if (check_launch("fandepth average pool")) return 2;
    if (dump(dl.feat, feat, (int64_t)R * kFeat)) return 2;
    a = conv_args(feat, 1, pack + pl.w_fc, pack + pl.b_fc, kFeat, kOut, 1, 1, 0, 0, depth, R);
    return launch_conv(a, 1, false, part, st);
}
