// The FFHQ alignment crop in front of the e4e encoder (libs/face_models/ffhq_cropping.py crop_using_landmarks): box from the 68
// landmarks, reflected border, feathered Gaussian and median blends where the box leaves the frame (pad_img_to_fit_bbox), truncation
// to uint8 and Pillow's 8-bit bicubic resampler, all on the caller's stream with no host round trip.  Contract: include/sgdfr.h.
//
// Every decision is per row and stays on the device: launches cover the largest geometry the workspace allows and the blocks of a
// row that is invalid, unpadded or smaller leave at once.
//   box        1 block / row      min / max of the landmarks, the box in the reference's integer semantics, borders, validity, ranks
//   blur_v     32 x 256 tiles     axis 0 of the Gaussian: the frame's bytes through the border reflection into LDS, double accumulate
//   blur_h     1 thread / value   axis 1, then the first blend -> the blended padded frame (float32)
//   hist       4 passes           8-bit radix select of the per-channel median: LDS histogram, one global atomic per non-empty bin
//   select     4 passes           the bin that holds each rank; after the last pass the median
//   crop       1 thread / value   second blend on the crop region, truncation to uint8 (unpadded rows: the frame's bytes)
//   coef       1 thread / index   Pillow's bicubic coefficients for this row's crop side, in double, as 22-bit integers
//   resize_h   1 wave / 64 outputs of one row;  resize_v  1 thread / value, writes the crop and the optional e4e tensor
//
// Floating-point contraction is OFF for the whole file: the reference's libraries do not fuse, and every float here is compared
// with them bit for bit or within one rounding (the truncation to uint8 and the (int) of a coefficient turn one ulp into one level).
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace sgdfr {
namespace {

constexpr int kRadius = 20;                  // scipy: int(4.0 * 5.0 + 0.5)
constexpr int kTileY = 32, kTileX = 256;     // blur_v tile: kTileY output rows x kTileX interleaved (x, channel) values
constexpr int kMaxOut = 1024;                // out_size bound behind the workspace's coefficient and row-pass areas
constexpr int kPrecisionBits = 32 - 8 - 2;   // Pillow's Resample.c PRECISION_BITS

struct Row {
    int x1, y1, size;            // box origin in frame coordinates, half side
    int pl, pt, pr, pb;          // border widths
    int ph, pw;                  // padded frame
    int valid, padded;
    float med[3];
    unsigned prefix[2][3];       // radix select: the bits fixed so far, per rank (lower / upper middle) and channel
    unsigned rank[2][3];         // rank left inside the prefix
};

struct GaussW {
    double w[kRadius + 1];       // weight at distance j
};

struct Geometry {
    int B, H, W, M, S;           // M = max_size, S = out_size
    int PH, PW;                  // largest padded frame a valid row can have
    int ksz;                     // coefficient stride per output index
};

struct Workspace {
    Row* rows;
    unsigned* hist;              // [B][4][2][3][256]
    int* coef;                   // [B][coef_cap]
    int* bounds;                 // [B][2][kMaxOut]  xmin, count
    float* t0;                   // [B][PH*PW*3]  axis-0 blur
    float* t1;                   // [B][PH*PW*3]  blended padded frame
    uint8_t* crop;               // [B][2M*2M*3]
    uint8_t* rowpass;            // [B][2M*kMaxOut*3]
    size_t state_bytes;          // rows + hist: cleared per call
};

inline int max_padded(int n, int M) {
    const int one_side = n + (n < 2 * M ? n : 2 * M);
    return one_side > 2 * M ? one_side : 2 * M;
}
__host__ __device__ inline int64_t coef_cap(int M) { return 8ll * M + 5ll * kMaxOut; }
inline int64_t align256(int64_t v) { return (v + 255) & ~255ll; }
constexpr int kHistPerRow = 4 * 2 * 3 * 256;

bool geometry_ok(int B, int H, int W, int M) { return B >= 1 && B <= 1024 && H >= 1 && H <= 4096 && W >= 1 && W <= 4096 && M >= 1 && M <= 4096; }

int64_t layout(int B, int H, int W, int M, char* base, Workspace* ws) {
    const int PH = max_padded(H, M), PW = max_padded(W, M);
    int64_t o = 0;
    auto take = [&](int64_t bytes) { const int64_t at = o; o += align256(bytes); return at; };
    const int64_t o_rows = take((int64_t)B * sizeof(Row));
    const int64_t o_hist = take((int64_t)B * kHistPerRow * 4);
    const int64_t state = o;
    const int64_t o_coef = take((int64_t)B * coef_cap(M) * 4);
    const int64_t o_bounds = take((int64_t)B * 2 * kMaxOut * 4);
    const int64_t o_t0 = take((int64_t)B * PH * PW * 3 * 4);
    const int64_t o_t1 = take((int64_t)B * PH * PW * 3 * 4);
    const int64_t o_crop = take((int64_t)B * 2 * M * 2 * M * 3);
    const int64_t o_rowpass = take((int64_t)B * 2 * M * kMaxOut * 3);
    if (ws) {
        ws->rows = (Row*)(base + o_rows);
        ws->hist = (unsigned*)(base + o_hist);
        ws->coef = (int*)(base + o_coef);
        ws->bounds = (int*)(base + o_bounds);
        ws->t0 = (float*)(base + o_t0);
        ws->t1 = (float*)(base + o_t1);
        ws->crop = (uint8_t*)(base + o_crop);
        ws->rowpass = (uint8_t*)(base + o_rowpass);
        ws->state_bytes = (size_t)state;
    }
    return o;
}

// ---------------------------------------------------------------------------------------------------------------- index helpers
// cv2.BORDER_REFLECT / np.pad 'symmetric' with a border no wider than the frame: cba|abc|cba
__device__ __forceinline__ int border_src(int v, int n) { return v < 0 ? -v - 1 : (v >= n ? 2 * n - 1 - v : v); }

// scipy's 'reflect' (the same symmetric rule) for any distance beyond the edge
__device__ __forceinline__ int reflect_any(int i, int n) {
    if (i >= 0 && i < n) return i;
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// the reference's feather mask at padded-frame pixel (px, py), float32 step by step
__device__ __forceinline__ float pad_width(int p) { return p == 0 ? 1e-10f : (float)p; }
__device__ __forceinline__ float feather(const Row& r, int px, int py) {
    const float fx = fminf(__fdiv_rn((float)px, pad_width(r.pl)), __fdiv_rn((float)(r.pw - 1 - px), pad_width(r.pr)));
    const float fy = fminf(__fdiv_rn((float)py, pad_width(r.pt)), __fdiv_rn((float)(r.ph - 1 - py), pad_width(r.pb)));
    return fmaxf(1.0f - fx, 1.0f - fy);
}
// element c of a three-element register array without a scratch copy
template <typename T>
__device__ __forceinline__ T pick3(const T (&a)[3], int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : a[2]); }
__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// ---------------------------------------------------------------------------------------------------------------- box
__global__ __launch_bounds__(64) void box_kernel(const float* __restrict__ lm, Geometry g, Row* rows, int* boxes, int* sizes, int* valid) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* p = lm + (size_t)b * 68 * 2;
    float x0 = p[lane * 2], y0 = p[lane * 2 + 1];
    float mnx = x0, mxx = x0, mny = y0, mxy = y0;
    bool finite = isfinite(x0) && isfinite(y0);
    if (lane + 64 < 68) {
        const float x1 = p[(lane + 64) * 2], y1 = p[(lane + 64) * 2 + 1];
        finite = finite && isfinite(x1) && isfinite(y1);
        mnx = fminf(mnx, x1), mxx = fmaxf(mxx, x1), mny = fminf(mny, y1), mxy = fmaxf(mxy, y1);
    }
    for (int o = 32; o > 0; o >>= 1) {
        mnx = fminf(mnx, __shfl_xor(mnx, o)), mxx = fmaxf(mxx, __shfl_xor(mxx, o));
        mny = fminf(mny, __shfl_xor(mny, o)), mxy = fmaxf(mxy, __shfl_xor(mxy, o));
    }
    finite = __all(finite);
    if (lane != 0) return;
    // centre = round((min + max) / 2) half to even, size = (int) max extent, centre_y -= size // 6 (ffhq_cropping.py:51-54)
    const float cxf = rintf((mnx + mxx) / 2.0f), cyf = rintf((mny + mxy) / 2.0f);
    const float ext = fmaxf(mxx - mnx, mxy - mny);
    const bool sane = finite && fabsf(cxf) < 1e6f && fabsf(cyf) < 1e6f && ext < 1e6f;
    int cx = 0, cy = 0, size = 0;
    if (sane) {
        cx = (int)cxf, cy = (int)cyf, size = (int)ext;
        cy -= size / 6;
    }
    const int x1 = cx - size, y1 = cy - size, x2 = cx + size, y2 = cy + size;
    if (boxes) boxes[b * 4 + 0] = x1, boxes[b * 4 + 1] = y1, boxes[b * 4 + 2] = x2, boxes[b * 4 + 3] = y2;
    if (sizes) sizes[b] = size;
    if (!rows) return;
    Row r;
    r.x1 = x1, r.y1 = y1, r.size = size;
    r.pl = max(-x1, 0), r.pt = max(-y1, 0), r.pr = max(x2 - g.W, 0), r.pb = max(y2 - g.H, 0);
    r.ph = g.H + r.pt + r.pb, r.pw = g.W + r.pl + r.pr;
    r.padded = (r.pl | r.pt | r.pr | r.pb) != 0;
    r.valid = sane && size >= 1 && size <= g.M && r.pl <= g.W && r.pr <= g.W && r.pt <= g.H && r.pb <= g.H && r.ph <= g.PH && r.pw <= g.PW;
    const unsigned n = (unsigned)r.ph * (unsigned)r.pw;
    for (int c = 0; c < 3; ++c) {
        r.med[c] = 0.f;
        r.prefix[0][c] = r.prefix[1][c] = 0u;
        r.rank[0][c] = (n - 1) / 2, r.rank[1][c] = n / 2;       // np.median: the middle value, or the two middle values
    }
    rows[b] = r;
    if (valid) valid[b] = r.valid;
}

// ---------------------------------------------------------------------------------------------------------------- Gaussian
// axis 0 (scipy filters the axes in order).  correlate1d's symmetric branch: centre tap, then the pairs from the outermost inwards,
// in double; the result is rounded to float32 because the image is float32.
__global__ __launch_bounds__(kTileX) void blur_v_kernel(const uint8_t* __restrict__ frames, Geometry g, const Row* __restrict__ rows,
                                                        GaussW gw, float* __restrict__ t0) {
    __shared__ uint8_t tile[kTileY + 2 * kRadius][kTileX];
    const int b = blockIdx.z;
    const Row r = rows[b];
    if (!r.valid || !r.padded) return;
    const int pw3 = r.pw * 3, xc0 = blockIdx.x * kTileX, py0 = blockIdx.y * kTileY;
    if (xc0 >= pw3 || py0 >= r.ph) return;
    const int tx = threadIdx.x, xc = xc0 + tx;
    const bool live = xc < pw3;
    if (live) {
        const int px = xc / 3, c = xc - px * 3;
        const int sx = border_src(px - r.pl, g.W);
        const uint8_t* col = frames + (size_t)b * g.H * g.W * 3 + (size_t)sx * 3 + c;
        for (int ty = 0; ty < kTileY + 2 * kRadius; ++ty) {
            const int py = reflect_any(py0 - kRadius + ty, r.ph);
            const int sy = border_src(py - r.pt, g.H);
            tile[ty][tx] = col[(size_t)sy * g.W * 3];
        }
    }
    __syncthreads();
    if (!live) return;
    float* out = t0 + (size_t)b * g.PH * g.PW * 3;
    const int rows_here = min(kTileY, r.ph - py0);
    for (int ty = 0; ty < rows_here; ++ty) {
        const int l = ty + kRadius;
        double acc = (double)tile[l][tx] * gw.w[0];
#pragma unroll
        for (int j = kRadius; j >= 1; --j) acc += ((double)tile[l - j][tx] + (double)tile[l + j][tx]) * gw.w[j];
        out[(size_t)(py0 + ty) * pw3 + xc] = (float)acc;
    }
}

// axis 1 and the first blend: img += (blur - img) * clip(3 mask + 1, 0, 1), in exactly this form (weight 0 keeps the integer)
__global__ __launch_bounds__(256) void blur_h_blend_kernel(const uint8_t* __restrict__ frames, Geometry g, const Row* __restrict__ rows,
                                                           GaussW gw, const float* __restrict__ t0, float* __restrict__ t1) {
    const int b = blockIdx.z;
    const Row r = rows[b];
    if (!r.valid || !r.padded) return;
    const int pw3 = r.pw * 3, xc = blockIdx.x * 256 + threadIdx.x, py = blockIdx.y;
    if (xc >= pw3 || py >= r.ph) return;
    const int px = xc / 3, c = xc - px * 3;
    const float* line = t0 + (size_t)b * g.PH * g.PW * 3 + (size_t)py * pw3 + c;
    double acc = (double)line[px * 3] * gw.w[0];
    if (px >= kRadius && px + kRadius < r.pw) {
#pragma unroll
        for (int j = kRadius; j >= 1; --j) acc += ((double)line[(px - j) * 3] + (double)line[(px + j) * 3]) * gw.w[j];
    } else {
#pragma unroll
        for (int j = kRadius; j >= 1; --j)
            acc += ((double)line[reflect_any(px - j, r.pw) * 3] + (double)line[reflect_any(px + j, r.pw) * 3]) * gw.w[j];
    }
    const float blur = (float)acc;
    const int sx = border_src(px - r.pl, g.W), sy = border_src(py - r.pt, g.H);
    float img = (float)frames[(((size_t)b * g.H + sy) * g.W + sx) * 3 + c];
    const float w = clip01(feather(r, px, py) * 3.0f + 1.0f);
    img = img + (blur - img) * w;
    t1[(size_t)b * g.PH * g.PW * 3 + (size_t)py * pw3 + xc] = img;
}

// ---------------------------------------------------------------------------------------------------------------- median
// The blended values are non-negative floats, so their bit patterns order as unsigned integers: four passes of an 8-bit radix select
// per channel and rank.  Integer atomics only, so the result does not depend on arrival order.
__global__ __launch_bounds__(256) void hist_kernel(Geometry g, const Row* __restrict__ rows, const float* __restrict__ t1,
                                                   unsigned* __restrict__ hist, int pass) {
    __shared__ unsigned h[2][3][256];
    const int b = blockIdx.z;
    const Row r = rows[b];
    if (!r.valid || !r.padded) return;
    const int n3 = r.ph * r.pw * 3;
    const int per_block = (n3 + gridDim.x - 1) / gridDim.x;
    const int per3 = (per_block + 2) / 3 * 3;                  // a multiple of 3: a thread's channel follows its index
    const int begin = blockIdx.x * per3;
    if (begin >= n3) return;
    const int end = min(begin + per3, n3);
    for (int i = threadIdx.x; i < 2 * 3 * 256; i += 256) (&h[0][0][0])[i] = 0u;
    __syncthreads();
    const int shift_prefix = 32 - 8 * pass, shift_bin = 24 - 8 * pass;
    const float* src = t1 + (size_t)b * g.PH * g.PW * 3;
    for (int i = begin + threadIdx.x; i < end; i += 256) {
        const int c = i % 3;
        const unsigned bits = __float_as_uint(src[i]);
        const unsigned top = pass == 0 ? 0u : bits >> shift_prefix;
        const unsigned bin = (bits >> shift_bin) & 255u;
        const unsigned p0 = pick3(r.prefix[0], c), p1 = pick3(r.prefix[1], c);
        if (top == p0) atomicAdd(&h[0][c][bin], 1u);
        if (p1 != p0 && top == p1) atomicAdd(&h[1][c][bin], 1u);
    }
    __syncthreads();
    unsigned* out = hist + ((size_t)b * 4 + pass) * (2 * 3 * 256);
    for (int i = threadIdx.x; i < 2 * 3 * 256; i += 256) {
        const unsigned v = (&h[0][0][0])[i];
        if (v) atomicAdd(out + i, v);
    }
}

__global__ __launch_bounds__(256) void select_kernel(Row* rows, const unsigned* __restrict__ hist, int pass) {
    __shared__ unsigned h[2][256];
    const int b = blockIdx.y, c = blockIdx.x;
    Row* r = rows + b;
    if (!r->valid || !r->padded) return;
    const unsigned* src = hist + ((size_t)b * 4 + pass) * (2 * 3 * 256);
    const bool same = r->prefix[0][c] == r->prefix[1][c];
    h[0][threadIdx.x] = src[(0 * 3 + c) * 256 + threadIdx.x];
    h[1][threadIdx.x] = src[((same ? 0 : 1) * 3 + c) * 256 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned value[2];
    for (int k = 0; k < 2; ++k) {
        unsigned left = r->rank[k][c], bin = 0;
        for (; bin < 255u; ++bin) {
            if (left < h[k][bin]) break;
            left -= h[k][bin];
        }
        r->rank[k][c] = left;
        value[k] = r->prefix[k][c] = (r->prefix[k][c] << 8) | bin;
    }
    if (pass == 3) r->med[c] = (__uint_as_float(value[0]) + __uint_as_float(value[1])) / 2.0f;      // float32 mean, as np.mean
}

// ---------------------------------------------------------------------------------------------------------------- crop
// second blend on the crop region, img += (median - img) * clip(mask, 0, 1), then astype(uint8): truncation
__global__ __launch_bounds__(256) void crop_kernel(const uint8_t* __restrict__ frames, Geometry g, const Row* __restrict__ rows,
                                                   const float* __restrict__ t1, uint8_t* __restrict__ crop, float* __restrict__ crop_f) {
    const int b = blockIdx.z;
    const Row r = rows[b];
    if (!r.valid) return;
    const int side = 2 * r.size, xc = blockIdx.x * 256 + threadIdx.x, cy = blockIdx.y;
    if (xc >= side * 3 || cy >= side) return;
    const int cx = xc / 3, c = xc - cx * 3;
    const size_t at = (size_t)b * (2 * g.M) * (2 * g.M) * 3 + (size_t)cy * side * 3 + xc;
    if (!r.padded) {
        const uint8_t v = frames[(((size_t)b * g.H + (r.y1 + cy)) * g.W + (r.x1 + cx)) * 3 + c];
        crop[at] = v;
        if (crop_f) crop_f[at] = (float)v;
        return;
    }
    const int px = r.x1 + r.pl + cx, py = r.y1 + r.pt + cy;
    float img = t1[(size_t)b * g.PH * g.PW * 3 + ((size_t)py * r.pw + px) * 3 + c];
    img = img + (pick3(r.med, c) - img) * clip01(feather(r, px, py));
    crop[at] = (uint8_t)(int)fminf(fmaxf(img, 0.0f), 255.0f);
    if (crop_f) crop_f[at] = img;
}

// ---------------------------------------------------------------------------------------------------------------- Pillow's resampler
__device__ __forceinline__ double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Resample.c precompute_coeffs + normalize_coeffs_8bpc for in = 2 size, out = S: the crop is square, so both passes share them
__global__ __launch_bounds__(64) void coef_kernel(Geometry g, const Row* __restrict__ rows, int* __restrict__ coef, int* __restrict__ bounds) {
    const int b = blockIdx.y, xx = blockIdx.x * 64 + threadIdx.x;
    const Row r = rows[b];
    if (!r.valid || xx >= g.S) return;
    const int in = 2 * r.size;
    const double scale = (double)in / g.S;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    if (xmax > g.ksz) xmax = g.ksz;          // cannot happen (ksz = (int) ceil(support) * 2 + 1 at the largest side): a guard, not a path
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += bicubic((x + xmin - center + 0.5) * ss);
    int* k = coef + (size_t)b * coef_cap(g.M) + (size_t)xx * g.ksz;
    for (int x = 0; x < xmax; ++x) {
        double w = bicubic((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        k[x] = w < 0 ? (int)(-0.5 + w * (double)(1 << kPrecisionBits)) : (int)(0.5 + w * (double)(1 << kPrecisionBits));
    }
    bounds[((size_t)b * 2 + 0) * kMaxOut + xx] = xmin;
    bounds[((size_t)b * 2 + 1) * kMaxOut + xx] = xmax;
}

__device__ __forceinline__ uint8_t clip8(int v) {
    v >>= kPrecisionBits;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// horizontal pass: one wave per 64 outputs of one crop row -> uint8 [side, S, 3]
__global__ __launch_bounds__(256) void resize_h_kernel(Geometry g, const Row* __restrict__ rows, const int* __restrict__ coef,
                                                       const int* __restrict__ bounds, const uint8_t* __restrict__ crop,
                                                       uint8_t* __restrict__ rowpass) {
    const int b = blockIdx.z;
    const Row r = rows[b];
    if (!r.valid) return;
    const int side = 2 * r.size, y = blockIdx.y * 4 + (threadIdx.x >> 6), xx = blockIdx.x * 64 + (threadIdx.x & 63);
    if (y >= side || xx >= g.S) return;
    const int xmin = bounds[((size_t)b * 2 + 0) * kMaxOut + xx], cnt = bounds[((size_t)b * 2 + 1) * kMaxOut + xx];
    const int* k = coef + (size_t)b * coef_cap(g.M) + (size_t)xx * g.ksz;
    const uint8_t* src = crop + (size_t)b * (2 * g.M) * (2 * g.M) * 3 + ((size_t)y * side + xmin) * 3;
    int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < cnt; ++x) {
        const int kk = k[x];
        s0 += src[x * 3 + 0] * kk, s1 += src[x * 3 + 1] * kk, s2 += src[x * 3 + 2] * kk;
    }
    uint8_t* dst = rowpass + (size_t)b * (2 * g.M) * kMaxOut * 3 + ((size_t)y * g.S + xx) * 3;
    dst[0] = clip8(s0), dst[1] = clip8(s1), dst[2] = clip8(s2);
}

// vertical pass -> crops [B,S,S,3] and the optional e4e tensor [B,3,S,S] = u8 / 255 * 2 - 1 in that float32 order; an invalid row
// is written as zeros here, so no other kernel has to touch it
__global__ __launch_bounds__(256) void resize_v_kernel(Geometry g, const Row* __restrict__ rows, const int* __restrict__ coef,
                                                       const int* __restrict__ bounds, const uint8_t* __restrict__ rowpass,
                                                       uint8_t* __restrict__ crops, float* __restrict__ e4e) {
    const int b = blockIdx.z, yy = blockIdx.y, xc = blockIdx.x * 256 + threadIdx.x;
    if (xc >= g.S * 3) return;
    const int xx = xc / 3, c = xc - xx * 3;
    const Row r = rows[b];
    uint8_t v = 0;
    if (r.valid) {
        const int ymin = bounds[((size_t)b * 2 + 0) * kMaxOut + yy], cnt = bounds[((size_t)b * 2 + 1) * kMaxOut + yy];
        const int* k = coef + (size_t)b * coef_cap(g.M) + (size_t)yy * g.ksz;
        const uint8_t* src = rowpass + (size_t)b * (2 * g.M) * kMaxOut * 3 + (size_t)ymin * g.S * 3 + xc;
        int s = 1 << (kPrecisionBits - 1);
        for (int y = 0; y < cnt; ++y) s += src[(size_t)y * g.S * 3] * k[y];
        v = clip8(s);
    }
    crops[((size_t)b * g.S + yy) * g.S * 3 + xc] = v;
    if (e4e) e4e[(((size_t)b * 3 + c) * g.S + yy) * g.S + xx] = r.valid ? __fdiv_rn((float)v, 255.0f) * 2.0f - 1.0f : 0.0f;
}

GaussW gauss_weights() {
    // scipy _gaussian_kernel1d(5.0, 0, 20): exp(-0.5 / sigma^2 * x^2) / sum, the 41 terms summed as numpy's add.reduce does (eight
    // running sums over the first 40, joined pairwise, then the last term)
    GaussW g;
    double phi[2 * kRadius + 1], part[8];
    for (int i = 0; i <= 2 * kRadius; ++i) {
        const double x = (double)(i - kRadius);
        phi[i] = exp(-0.5 / 25.0 * (x * x));
    }
    for (int k = 0; k < 8; ++k) part[k] = phi[k];
    for (int i = 8; i < 2 * kRadius; i += 8)
        for (int k = 0; k < 8; ++k) part[k] += phi[i + k];
    double sum = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
    sum += phi[2 * kRadius];
    for (int j = 0; j <= kRadius; ++j) g.w[j] = phi[kRadius + j] / sum;
    return g;
}

int resample_stride(int M, int S) {
    double fs = 2.0 * M / S;
    if (fs < 1.0) fs = 1.0;
    return (int)ceil(2.0 * fs) * 2 + 1;
}

}  // namespace
}  // namespace sgdfr

using namespace sgdfr;

extern "C" int64_t sgdfr_facecrop_workspace_bytes(int rows, int H, int W, int max_size) {
    if (!geometry_ok(rows, H, W, max_size)) return -1;
    return layout(rows, H, W, max_size, nullptr, nullptr);
}

extern "C" int sgdfr_facecrop_boxes_f32(const float* landmarks, int rows, int* boxes, int* sizes, void* stream) {
    SGDFR_REQUIRE(landmarks && boxes && sizes, "facecrop_boxes: null pointer");
    SGDFR_REQUIRE(rows >= 1 && rows <= 1024, "facecrop_boxes: rows=%d (1..1024)", rows);
    Geometry g{};
    g.B = rows;
    box_kernel<<<rows, 64, 0, as_stream(stream)>>>(landmarks, g, nullptr, boxes, sizes, nullptr);
    return check_launch("facecrop box_kernel");
}

extern "C" int sgdfr_facecrop_forward_u8(const uint8_t* frames, const float* landmarks, int rows, int H, int W, int out_size, int max_size,
                                         uint8_t* crops, int* valid, float* e4e, int* boxes, int* sizes, float* crop_float,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(frames && landmarks && crops && valid, "facecrop_forward: null pointer");
    SGDFR_REQUIRE(geometry_ok(rows, H, W, max_size), "facecrop_forward: rows=%d H=%d W=%d max_size=%d (rows 1..1024, the others 1..4096)",
                  rows, H, W, max_size);
    SGDFR_REQUIRE(out_size >= 1 && out_size <= kMaxOut, "facecrop_forward: out_size=%d (1..%d)", out_size, kMaxOut);
    Workspace ws;
    const int64_t need = layout(rows, H, W, max_size, (char*)workspace, &ws);
    SGDFR_REQUIRE(workspace && workspace_bytes >= need, "facecrop_forward: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)need);
    Geometry g;
    g.B = rows, g.H = H, g.W = W, g.M = max_size, g.S = out_size;
    g.PH = max_padded(H, max_size), g.PW = max_padded(W, max_size);
    g.ksz = resample_stride(max_size, out_size);
    SGDFR_REQUIRE((int64_t)g.ksz * out_size <= coef_cap(max_size), "facecrop_forward: coefficient area too small (%d x %d)", g.ksz, out_size);
    hipStream_t st = as_stream(stream);
    const GaussW gw = gauss_weights();
    if (hipMemsetAsync(workspace, 0, ws.state_bytes, st) != hipSuccess) {
        set_error("facecrop_forward: hipMemsetAsync failed");
        return 1;
    }
    box_kernel<<<rows, 64, 0, st>>>(landmarks, g, ws.rows, boxes, sizes, valid);
    if (check_launch("facecrop box_kernel")) return 1;
    const int pw3 = g.PW * 3;
    blur_v_kernel<<<dim3((pw3 + kTileX - 1) / kTileX, (g.PH + kTileY - 1) / kTileY, rows), kTileX, 0, st>>>(frames, g, ws.rows, gw, ws.t0);
    if (check_launch("facecrop blur_v_kernel")) return 1;
    blur_h_blend_kernel<<<dim3((pw3 + 255) / 256, g.PH, rows), 256, 0, st>>>(frames, g, ws.rows, gw, ws.t0, ws.t1);
    if (check_launch("facecrop blur_h_blend_kernel")) return 1;
    const int64_t n3 = (int64_t)g.PH * pw3;
    int hist_blocks = (int)((n3 + 256 * 16 - 1) / (256 * 16));
    hist_blocks = hist_blocks < 1 ? 1 : (hist_blocks > 256 ? 256 : hist_blocks);
    for (int pass = 0; pass < 4; ++pass) {
        hist_kernel<<<dim3(hist_blocks, 1, rows), 256, 0, st>>>(g, ws.rows, ws.t1, ws.hist, pass);
        if (check_launch("facecrop hist_kernel")) return 1;
        select_kernel<<<dim3(3, rows), 256, 0, st>>>(ws.rows, ws.hist, pass);
        if (check_launch("facecrop select_kernel")) return 1;
    }
    crop_kernel<<<dim3((2 * max_size * 3 + 255) / 256, 2 * max_size, rows), 256, 0, st>>>(frames, g, ws.rows, ws.t1, ws.crop, crop_float);
    if (check_launch("facecrop crop_kernel")) return 1;
    coef_kernel<<<dim3((out_size + 63) / 64, rows), 64, 0, st>>>(g, ws.rows, ws.coef, ws.bounds);
    if (check_launch("facecrop coef_kernel")) return 1;
    resize_h_kernel<<<dim3((out_size + 63) / 64, (2 * max_size + 3) / 4, rows), 256, 0, st>>>(g, ws.rows, ws.coef, ws.bounds, ws.crop,
                                                                                              ws.rowpass);
    if (check_launch("facecrop resize_h_kernel")) return 1;
    resize_v_kernel<<<dim3((out_size * 3 + 255) / 256, out_size, rows), 256, 0, st>>>(g, ws.rows, ws.coef, ws.bounds, ws.rowpass, crops, e4e);
    return check_launch("facecrop resize_v_kernel");
}
