// The implicit-GEMM conv tile of the fp32 network heads (idloss.hip, deca.hip, fan.hip, s3fd.hip, e4e.hip): what is the same in all
// of them.  64 pixels x BN output channels per block of 256 threads, K in chunks of 16 on exact-f32 MFMA (v_mfma_f32_16x16x4_f32),
// double-buffered through registers; layers with few tiles split K, and a finish kernel sums the slices in fixed order.
//
// A head supplies its ConvArgs, what a thread gathers for its pixel at a K index (and so its pre-op, second operand, skipped taps),
// its epilogue, its dispatch table and its __global__ kernels.  A conv kernel reads
//     __shared__ ConvLds<BN> lds;
//     auto gload = [&](int c) { ...gather xr[i] for k = c*BK + wv + 4*i...;  load_w<BN>(wr, wp, K, N, c * BK, n0); };
//     auto sstore = [&](int buf) { store_x(lds.xs[buf], xr);  store_w<BN>(lds.ws[buf], wr); };
//     k_loop<BN>(lds, c0, c1, gload, sstore, acc);
//     float* const slice = slice_of(a.part, a.part_elems);
//     for_each_output<BN>(acc, m0, n0, M, N, HWo, [=](int b, int n, int p, float v) { ...slice ? partial : epilogue(a, ...)... });
// and its finish kernel is finish_slices(..., [=](int b, int n, int p, float v) { epilogue(a, ...); }).  These two sinks capture BY
// VALUE: with a reference to the kernel's argument struct in the closure the compiler no longer commons the epilogue's null tests
// and 64-bit address arithmetic across the lane's elements (+ 20 % static instructions behind the K loop, measured on fan.hip).
// Index types, in every gather: one map's pixel count (`plane`) and an offset inside one row's [C, H, W] block are int (every head
// bounds a row's block below 2^31 elements by its fixed geometry or its size check); the offset of a row, and s3fd.hip's and
// e4e.hip's channel offset (up to 1024 channels of a caller-sized map), are int64_t.  `mvalid` is tested with the tap's own bounds,
// inside `k < K`: k is uniform over the wave, so the outer test is a scalar branch and the inner one the lane's predicate.
#pragma once
#include <algorithm>

#include "common.h"

namespace sgdfr {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int BM = 64, BK = 16, kThreads = 256;

// The four waves of a block as WM (pixels) x WN (channels), each wave TM x TN MFMA blocks of 16 x 16.
// BN = 64: 2 x 2 waves of 2 x 2 blocks.  BN = 16 (S3FD's heads): 4 x 1 waves of one block.
template <int BN>
struct Tile {
    static_assert(BN == 64 || BN == 16, "two tiles");
    static constexpr int WN = BN == 64 ? 2 : 1, WM = 4 / WN;
    static constexpr int TM = BM / (16 * WM), TN = BN / (16 * WN);
    static constexpr int WL = BK * BN / kThreads;   // filter values a thread stages per chunk
};

template <int BN>
struct ConvLds {
    float xs[2][BK][BM + 4];    // pixels (MFMA B operand / columns)
    float ws[2][BK][BN + 4];    // output channels (MFMA A operand / rows)
};

// ------------------------------------------------------------------ staging
// the gathered values of this thread's pixel t & 63 at K rows wv, wv + 4, wv + 8, wv + 12 of the chunk
__device__ __forceinline__ void store_x(float (&xs)[BK][BM + 4], const float (&xr)[4]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) xs[(t >> 6) + 4 * i][t & (BM - 1)] = xr[i];
}

// the [BK][BN] filter block of wp [K][N] at (k0, n0), zeros outside, element e = t + 256 i of it per thread
template <int BN>
__device__ __forceinline__ void load_w(float (&wr)[Tile<BN>::WL], const float* wp, int K, int N, int k0, int n0) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < Tile<BN>::WL; ++i) {
        const int e = t + kThreads * i, n = e & (BN - 1), k = k0 + e / BN, gn = n0 + n;
        wr[i] = (k < K && gn < N) ? wp[(int64_t)k * N + gn] : 0.f;
    }
}
template <int BN>
__device__ __forceinline__ void store_w(float (&ws)[BK][BN + 4], const float (&wr)[Tile<BN>::WL]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < Tile<BN>::WL; ++i) {
        const int e = t + kThreads * i;
        ws[e / BN][e & (BN - 1)] = wr[i];
    }
}

// ------------------------------------------------------------------ K loop
// acc = sum over chunks c0 <= c < c1.  gload(c) fetches chunk c into the caller's registers, sstore(buf) puts them into lds buffer
// `buf`: the next chunk is fetched while the MFMAs run on the current one.  Products are added in ascending k into a fixed
// accumulator element, whatever the slicing: the bits of a slice depend on (c0, c1) alone.
template <int BN, class GLoad, class SStore>
__device__ __forceinline__ void k_loop(const ConvLds<BN>& lds, int c0, int c1, GLoad gload, SStore sstore,
                                       floatx4 (&acc)[Tile<BN>::TN][Tile<BN>::TM]) {
    constexpr int TM = Tile<BN>::TM, TN = Tile<BN>::TN, WM = Tile<BN>::WM;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wm = wv % WM, wn = wv / WM;
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    if (c0 < c1) {
        gload(c0);
        sstore(0);
    }
    __syncthreads();
    for (int c = c0; c < c1; ++c) {
        const int buf = (c - c0) & 1;
        const bool more = c + 1 < c1;
        if (more) gload(c + 1);
#pragma unroll
        for (int ks = 0; ks < BK; ks += 4) {
            const int kr = ks + (lane >> 4);
            float wa[TN], xa[TM];
#pragma unroll
            for (int i = 0; i < TN; ++i) wa[i] = lds.ws[buf][kr][wn * (16 * TN) + i * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < TM; ++j) xa[j] = lds.xs[buf][kr][wm * (16 * TM) + j * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[i], xa[j], acc[i][j], 0, 0, 0);
        }
        if (more) sstore(buf ^ 1);   // the other buffer: every wave finished reading it before the previous barrier
        __syncthreads();
    }
}

// ------------------------------------------------------------------ output walk
// where this block's partial sums go: slice blockIdx.z of part [S][part_elems]; NULL when K is not split and the block runs the epilogue
__device__ __forceinline__ float* slice_of(float* part, int64_t part_elems) {
    return gridDim.z > 1 ? part + (int64_t)blockIdx.z * part_elems : nullptr;
}

// D[row = channel][col = pixel]: lane holds channel (lane>>4)*4 + r of a 16-row block, pixel lane&15.
// sink(b, n, p, v): value v of row b, channel n, pixel p of the [R, N, HWo] output, for the elements inside M x N.
template <int BN, class Sink>
__device__ __forceinline__ void for_each_output(const floatx4 (&acc)[Tile<BN>::TN][Tile<BN>::TM], int m0, int n0, int M, int N, int HWo,
                                                Sink sink) {
    constexpr int TM = Tile<BN>::TM, TN = Tile<BN>::TN, WM = Tile<BN>::WM;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, wm = wv % WM, wn = wv / WM;
#pragma unroll
    for (int j = 0; j < TM; ++j) {
        const int gp = m0 + wm * (16 * TM) + j * 16 + (lane & 15);
        if (gp >= M) continue;
        const int bb = gp / HWo, p = gp - bb * HWo;
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gn = n0 + wn * (16 * TN) + i * 16 + (lane >> 4) * 4 + r;
                if (gn >= N) continue;
                sink(bb, gn, p, acc[i][j][r]);
            }
    }
}

// ------------------------------------------------------------------ finish
// The body of a head's finish kernel: element i of the [rows, N, HWo] output = sum of its S partials in slice order, handed to
// sink(row, n, p, v), which runs the conv's epilogue.
template <class Sink>
__device__ __forceinline__ void finish_slices(const float* part, int64_t n, int S, int N, int HWo, Sink sink) {
    const int64_t per_row = (int64_t)N * HWo;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        float v = part[i];
        for (int s = 1; s < S; ++s) v += part[(int64_t)s * n + i];
        const int b = (int)(i / per_row);
        const int64_t rem = i - b * per_row;
        const int gn = (int)(rem / HWo), p = (int)(rem - (int64_t)gn * HWo);
        sink(b, gn, p, v);
    }
}

// ------------------------------------------------------------------ host side
static inline int64_t align64(int64_t v) { return (v + 63) & ~(int64_t)63; }
// at least one block: n = 0 is an idle launch, not a launch error (s3fd.hip's form; the other four heads had no lower bound)
static inline int grid_1d(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>((n + kThreads - 1) / kThreads, 1), 8192); }

struct ConvPlan {
    int S, cps, mt, nt;      // K slices, chunks per slice, pixel and channel tiles
    int64_t out_elems;       // M * N: of one group (e4e.hip multiplies by its G for the partials and the finish grid)
};
static inline int conv_tiles(int M, int N, int bn) { return ((M + BM - 1) / BM) * ((N + bn - 1) / bn); }
// M x N outputs over K in tiles of 64 x bn.  The number of K slices follows `tiles`, the tile count the head plans for (its own
// conv_tiles(M, N, bn), or that of other rows or of all groups of the launch): at most 512 / tiles slices of at least 8 chunks, at
// most 32; `whole`: one slice whatever the tiles.
static inline ConvPlan plan_conv(int M, int N, int K, int bn, int tiles, bool whole = false) {
    ConvPlan p;
    p.mt = (M + BM - 1) / BM, p.nt = (N + bn - 1) / bn;
    const int nchunks = (K + BK - 1) / BK;
    int S = whole ? 1 : std::min(512 / std::max(tiles, 1), nchunks / 8);
    S = std::max(1, std::min(S, 32));
    p.cps = (nchunks + S - 1) / S;
    p.S = (nchunks + p.cps - 1) / p.cps;
    p.out_elems = (int64_t)M * N;
    return p;
}

}  // namespace sgdfr
