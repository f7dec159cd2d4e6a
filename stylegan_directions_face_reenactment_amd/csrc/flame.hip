// FLAME decode (DECA.decode = FLAME.forward + batch_orth_proj), its backward to the 3DMM coefficients, and the shape / mouth / eye
// L1 terms with their cotangents (include/sgdfr.h, "FLAME").  fp32, deterministic (no float atomics: block partials -> slab -> one
// fixed-order sum), no host synchronisation, everything on the caller's stream.
//
// Tables live in one device pack built by sgdfr_flame_prepack_f32:
//   SDF [47][3V] float4  shape/expression basis (quads 0..37: 150 components + 2 zeros) and pose correctives (quads 38..46), laid out
//                        so that a thread per vertex coordinate reads consecutive 16-byte words (forward)
//   SDB [3V][47] float4  the same numbers with the quad index fastest (backward: a thread per quad sweeps the block's coordinates)
//   v_template, skinning weights, the folded joint regressor (J = JT + JD . betas), landmark corner vertices + barycentric weights
//   (static 51, full 68, dynamic 79 x 17) and the inverse landmark index (per vertex: the landmark corners that reference it).
// The vertex kernels tile over 64 vertices (192 coordinates) per block and loop over the rows in chunks of 16 inside the block, so a
// basis element is fetched from memory once per launch.
#include <math.h>

#include "common.h"

namespace {

using namespace sgdfr;

constexpr int V = 5023, C3 = 3 * V, NSHAPE = 100, NEXP = 50, NB = 150, NQS = 38, NQP = 9, NQ = NQS + NQP, NJ = 5, NF = 36;
constexpr int LSTAT = 51, LFULL = 68, LDYN = 17, DYNROWS = 79, NLM = 68;
constexpr int NCSR = (LSTAT + LFULL + DYNROWS * LDYN) * 3;
constexpr int FLAME_PARAMS = 15;
constexpr float HALF = 112.f;                    // image_size / 2 of DECA.decode

constexpr int align4(int n) { return (n + 3) & ~3; }
// pack offsets (floats)
constexpr int64_t OFF_SDF = 0;
constexpr int64_t OFF_SDB = OFF_SDF + (int64_t)NQ * C3 * 4;
constexpr int64_t OFF_VT = OFF_SDB + (int64_t)NQ * C3 * 4;
constexpr int64_t OFF_W = OFF_VT + align4(C3);
constexpr int64_t OFF_JT = OFF_W + align4(V * NJ);
constexpr int64_t OFF_JD = OFF_JT + 16;
constexpr int64_t OFF_LSV = OFF_JD + align4(15 * NB);
constexpr int64_t OFF_LSB = OFF_LSV + align4(LSTAT * 3);
constexpr int64_t OFF_LFV = OFF_LSB + align4(LSTAT * 3);
constexpr int64_t OFF_LFB = OFF_LFV + align4(LFULL * 3);
constexpr int64_t OFF_LDV = OFF_LFB + align4(LFULL * 3);
constexpr int64_t OFF_LDB = OFF_LDV + align4(DYNROWS * LDYN * 3);
constexpr int64_t OFF_CO = OFF_LDB + align4(DYNROWS * LDYN * 3);
constexpr int64_t OFF_CS = OFF_CO + align4(V + 1);
constexpr int64_t OFF_CW = OFF_CS + align4(NCSR);
constexpr int64_t PACK_ELEMS = OFF_CW + align4(NCSR);

// per-row saved block: SMALL floats of pose state, then v_posed [3V], then the un-projected vertices [3V]
constexpr int SMALL = 256, SROW = SMALL + 2 * C3;
constexpr int S_R = 0, S_J = 45, S_F = 60, S_A = 96, S_G = 156, S_DYN = 201, S_POSE = 202, S_CAM = 208;

constexpr int VB = 64, TB = 3 * VB, RC = 16, NBLK = (V + VB - 1) / VB;
constexpr int P_DA = 188, P_CAM = 248, PCOLS = 252;       // partial columns: 0..149 betas, 152..187 pose feature, dA [5][12], dcam
constexpr int LOSS_BLOCKS = 64;

__device__ __forceinline__ float sgn(float x) { return (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f); }
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ void flame_prepack_kernel(const float* __restrict__ sd, const float* __restrict__ pd, float4* __restrict__ sdf,
                                     float4* __restrict__ sdb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NQ * C3) return;
    const int q = i / C3, c = i - q * C3;
    float v[4];
    for (int e = 0; e < 4; ++e) {
        if (q < NQS) {
            const int l = 4 * q + e;
            v[e] = l < NB ? sd[(int64_t)c * NB + l] : 0.f;
        } else {
            v[e] = pd[(int64_t)(4 * (q - NQS) + e) * C3 + c];
        }
    }
    const float4 o = make_float4(v[0], v[1], v[2], v[3]);
    sdf[i] = o;
    sdb[(int64_t)c * NQ + q] = o;
}

// batch_rodrigues as written: angle = |r + 1e-8|, direction r / angle, R = I + sin K + (1 - cos) K K
__device__ void rodrigues(const float* r, float* R) {
    const float a0 = r[0] + 1e-8f, a1 = r[1] + 1e-8f, a2 = r[2] + 1e-8f;
    const float th = sqrtf(a0 * a0 + a1 * a1 + a2 * a2);
    const float dx = r[0] / th, dy = r[1] / th, dz = r[2] / th;
    const float s = sinf(th), c1 = 1.f - cosf(th);
    const float K[9] = {0.f, -dz, dy, dz, 0.f, -dx, -dy, dx, 0.f};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float kk = 0.f;
            for (int m = 0; m < 3; ++m) kk += K[i * 3 + m] * K[m * 3 + j];
            R[i * 3 + j] = (i == j ? 1.f : 0.f) + s * K[i * 3 + j] + c1 * kk;
        }
}

// dL/dr of the above for dL/dR = M
__device__ void rodrigues_bwd(const float* r, const float* M, float* dr) {
    const float a[3] = {r[0] + 1e-8f, r[1] + 1e-8f, r[2] + 1e-8f};
    const float th = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const float dx = r[0] / th, dy = r[1] / th, dz = r[2] / th;
    const float s = sinf(th), c = cosf(th);
    const float K[9] = {0.f, -dz, dy, dz, 0.f, -dx, -dy, dx, 0.f};
    float mk = 0.f, mkk = 0.f, dK[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            float kk = 0.f, a1 = 0.f, a2 = 0.f;
            for (int m = 0; m < 3; ++m) {
                kk += K[i * 3 + m] * K[m * 3 + j];
                a1 += M[i * 3 + m] * K[j * 3 + m];       // (M K^T)[i][j]
                a2 += K[m * 3 + i] * M[m * 3 + j];       // (K^T M)[i][j]
            }
            mk += M[i * 3 + j] * K[i * 3 + j];
            mkk += M[i * 3 + j] * kk;
            dK[i * 3 + j] = s * M[i * 3 + j] + (1.f - c) * (a1 + a2);
        }
    const float dd[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
    float dth = c * mk + s * mkk;
    dth -= (dd[0] * r[0] + dd[1] * r[1] + dd[2] * r[2]) / (th * th);
    for (int i = 0; i < 3; ++i) dr[i] = dd[i] / th + dth * a[i] / th;
}

__device__ __forceinline__ int parent_of(int j) { return j == 0 ? -1 : (j == 1 ? 0 : 1); }

// one block per row: joints from the folded regressor, rotations, pose feature, rigid-transform chain, dynamic contour row
__global__ void __launch_bounds__(64) flame_pose_kernel(const float* __restrict__ shape_a, const float* __restrict__ exp_a,
                                                        const float* __restrict__ pose_a, int rows_a,
                                                        const float* __restrict__ shape_b, const float* __restrict__ exp_b,
                                                        const float* __restrict__ pose_b, const float* __restrict__ cam,
                                                        const float* __restrict__ pack, float* __restrict__ saved) {
    __shared__ float Js[15];
    const int r = blockIdx.x, t = threadIdx.x;
    const bool first = r < rows_a;
    const int rr = first ? r : r - rows_a;
    const float* sh = (first ? shape_a : shape_b) + (int64_t)rr * NSHAPE;
    const float* ex = (first ? exp_a : exp_b) + (int64_t)rr * NEXP;
    const float* po = (first ? pose_a : pose_b) + (int64_t)rr * 6;
    if (t < 15) {
        const float* jd = pack + OFF_JD + t * NB;
        float acc = pack[OFF_JT + t];
        for (int l = 0; l < NSHAPE; ++l) acc = fmaf(jd[l], sh[l], acc);
        for (int l = 0; l < NEXP; ++l) acc = fmaf(jd[NSHAPE + l], ex[l], acc);
        Js[t] = acc;
    }
    __syncthreads();
    if (t != 0) return;
    float* S = saved + (int64_t)r * SROW;
    float R[NJ][9], G[NJ][9], Gt[NJ][3];
    for (int j = 0; j < NJ; ++j)
        for (int i = 0; i < 9; ++i) R[j][i] = (i % 4 == 0) ? 1.f : 0.f;      // neck and eyes: zero vectors give the identity exactly
    float p6[6];
    for (int i = 0; i < 6; ++i) p6[i] = po[i];
    rodrigues(p6, R[0]);
    rodrigues(p6 + 3, R[2]);
    for (int i = 0; i < 9; ++i) G[0][i] = R[0][i];
    for (int i = 0; i < 3; ++i) Gt[0][i] = Js[i];
    for (int j = 1; j < NJ; ++j) {
        const int p = parent_of(j);
        float rel[3];
        for (int i = 0; i < 3; ++i) rel[i] = Js[j * 3 + i] - Js[p * 3 + i];
        for (int i = 0; i < 3; ++i) {
            for (int k = 0; k < 3; ++k) {
                float a = 0.f;
                for (int m = 0; m < 3; ++m) a += G[p][i * 3 + m] * R[j][m * 3 + k];
                G[j][i * 3 + k] = a;
            }
            float a = 0.f;
            for (int m = 0; m < 3; ++m) a += G[p][i * 3 + m] * rel[m];
            Gt[j][i] = a + Gt[p][i];
        }
    }
    for (int j = 0; j < NJ; ++j) {
        for (int i = 0; i < 9; ++i) {
            S[S_R + j * 9 + i] = R[j][i];
            S[S_G + j * 9 + i] = G[j][i];
        }
        for (int i = 0; i < 3; ++i) {
            S[S_J + j * 3 + i] = Js[j * 3 + i];
            float a = 0.f;
            for (int m = 0; m < 3; ++m) a += G[j][i * 3 + m] * Js[j * 3 + m];
            for (int k = 0; k < 3; ++k) S[S_A + j * 12 + i * 4 + k] = G[j][i * 3 + k];
            S[S_A + j * 12 + i * 4 + 3] = Gt[j][i] - a;
        }
        if (j > 0)
            for (int i = 0; i < 9; ++i) S[S_F + (j - 1) * 9 + i] = R[j][i] - ((i % 4 == 0) ? 1.f : 0.f);
    }
    // FLAME._find_dynamic_lmk_idx_and_bcoords: the neck chain [1, 0] with a zero neck pose is the global rotation
    const float sy = sqrtf(R[0][0] * R[0][0] + R[0][3] * R[0][3]);
    float ang = atan2f(-R[0][6], sy) * 180.0f / 3.14159265358979323846f;
    ang = rintf(fminf(ang, 39.f));                                           // torch.round: half to even
    int y = (ang == ang) ? (int)ang : 0;
    if (y < 0) y = (y < -39) ? 78 : 39 - y;
    y = clampi(y, 0, DYNROWS - 1);
    S[S_DYN] = __int_as_float(y);
    for (int i = 0; i < 6; ++i) S[S_POSE + i] = p6[i];
    for (int i = 0; i < 3; ++i) S[S_CAM + i] = cam ? cam[(int64_t)r * 3 + i] : (i == 0 ? 1.f : 0.f);
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}

// blend shapes + pose correctives + skinning (+ projection): a thread per vertex coordinate, rows in chunks of RC
__global__ void __launch_bounds__(TB) flame_verts_kernel(const float* __restrict__ shape_a, const float* __restrict__ exp_a, int rows_a,
                                                         const float* __restrict__ shape_b, const float* __restrict__ exp_b, int rows,
                                                         const float* __restrict__ pack, int project, float* __restrict__ saved,
                                                         float* __restrict__ tv) {
    __shared__ float4 beta4[RC][NQS];
    __shared__ float4 feat4[RC][NQP];
    __shared__ float As[RC][60];
    __shared__ float cams[RC][4];
    __shared__ float vps[RC][TB];
    const int t = threadIdx.x, c = blockIdx.x * TB + t;
    const bool valid = c < C3;
    const int cc = valid ? c : C3 - 1;
    const int vl = t / 3, k = t - 3 * vl, v = cc / 3;
    const float4* sdf = reinterpret_cast<const float4*>(pack + OFF_SDF);
    float w[NJ];
    for (int j = 0; j < NJ; ++j) w[j] = pack[OFF_W + v * NJ + j];
    const float vt = pack[OFF_VT + cc];
    for (int r0 = 0; r0 < rows; r0 += RC) {
        const int nr = min(RC, rows - r0);
        __syncthreads();
        for (int i = t; i < RC * 4 * NQS; i += TB) {
            const int rr = i / (4 * NQS), l = i - rr * (4 * NQS), row = r0 + rr;
            float val = 0.f;
            if (rr < nr && l < NB) {
                const bool first = row < rows_a;
                const int64_t ra = first ? row : row - rows_a;
                val = l < NSHAPE ? (first ? shape_a : shape_b)[ra * NSHAPE + l] : (first ? exp_a : exp_b)[ra * NEXP + l - NSHAPE];
            }
            reinterpret_cast<float*>(beta4)[i] = val;
        }
        for (int i = t; i < RC * NF; i += TB) {
            const int rr = i / NF, l = i - rr * NF;
            reinterpret_cast<float*>(feat4)[i] = rr < nr ? saved[(int64_t)(r0 + rr) * SROW + S_F + l] : 0.f;
        }
        for (int i = t; i < RC * 60; i += TB) {
            const int rr = i / 60, l = i - rr * 60;
            As[rr][l] = rr < nr ? saved[(int64_t)(r0 + rr) * SROW + S_A + l] : 0.f;
        }
        if (t < RC * 3) {
            const int rr = t / 3, l = t - rr * 3;
            cams[rr][l] = rr < nr ? saved[(int64_t)(r0 + rr) * SROW + S_CAM + l] : 0.f;
        }
        __syncthreads();
        float acc[RC];
#pragma unroll
        for (int r = 0; r < RC; ++r) acc[r] = 0.f;
#pragma unroll 2
        for (int q = 0; q < NQS; ++q) {
            const float4 s = sdf[(int64_t)q * C3 + cc];
#pragma unroll
            for (int r = 0; r < RC; ++r) acc[r] = dot4(s, beta4[r][q], acc[r]);
        }
        float pacc[RC];
#pragma unroll
        for (int r = 0; r < RC; ++r) pacc[r] = 0.f;
#pragma unroll 1
        for (int q = 0; q < NQP; ++q) {
            const float4 s = sdf[(int64_t)(NQS + q) * C3 + cc];
#pragma unroll
            for (int r = 0; r < RC; ++r) pacc[r] = dot4(s, feat4[r][q], pacc[r]);
        }
#pragma unroll
        for (int r = 0; r < RC; ++r) {
            const float vp = pacc[r] + (vt + acc[r]);             // pose_offsets + (v_template + blend_shapes)
            vps[r][t] = vp;
            if (valid && r < nr) saved[(int64_t)(r0 + r) * SROW + SMALL + c] = vp;
        }
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < nr; ++r) {
            float T[4];
            for (int i = 0; i < 4; ++i) {
                float a = 0.f;
                for (int j = 0; j < NJ; ++j) a = fmaf(w[j], As[r][j * 12 + k * 4 + i], a);
                T[i] = a;
            }
            const float o = T[0] * vps[r][vl * 3] + T[1] * vps[r][vl * 3 + 1] + T[2] * vps[r][vl * 3 + 2] + T[3];
            if (!valid) continue;
            saved[(int64_t)(r0 + r) * SROW + SMALL + C3 + c] = o;
            if (project) {
                float p = cams[r][0] * (k < 2 ? o + cams[r][1 + k] : o);
                if (k >= 1) p = -p;
                tv[(int64_t)(r0 + r) * C3 + c] = p * HALF + HALF;
            }
        }
    }
}

// corner vertices and weights of landmark slot s (0..67: landmarks2d, 68..135: landmarks3d) of a row with dynamic row `dyn`
__device__ __forceinline__ void lmk_corners(const float* pack, int s, int dyn, int* idx, float* b) {
    int64_t ov, ob;
    if (s < LDYN) {
        ov = OFF_LDV + (dyn * LDYN + s) * 3;
        ob = OFF_LDB + (dyn * LDYN + s) * 3;
    } else if (s < NLM) {
        ov = OFF_LSV + (s - LDYN) * 3;
        ob = OFF_LSB + (s - LDYN) * 3;
    } else {
        ov = OFF_LFV + (s - NLM) * 3;
        ob = OFF_LFB + (s - NLM) * 3;
    }
    for (int e = 0; e < 3; ++e) {
        idx[e] = clampi(__float_as_int(pack[ov + e]), 0, V - 1);
        b[e] = pack[ob + e];
    }
}

__global__ void flame_lmk_kernel(int rows, const float* __restrict__ pack, int project, const float* __restrict__ saved,
                                 float* __restrict__ lm2d, float* __restrict__ lm3d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * 2 * NLM) return;
    const int r = i / (2 * NLM), s = i - r * 2 * NLM;
    const float* S = saved + (int64_t)r * SROW;
    const float* verts = S + SMALL + C3;
    int idx[3];
    float b[3], p[3];
    lmk_corners(pack, s, __float_as_int(S[S_DYN]), idx, b);
    for (int k = 0; k < 3; ++k) p[k] = verts[idx[0] * 3 + k] * b[0] + verts[idx[1] * 3 + k] * b[1] + verts[idx[2] * 3 + k] * b[2];
    if (project) {
        const float sc = S[S_CAM];
        p[0] = (sc * (p[0] + S[S_CAM + 1])) * HALF + HALF;
        p[1] = (-(sc * (p[1] + S[S_CAM + 2]))) * HALF + HALF;
        p[2] = (-(sc * p[2])) * HALF + HALF;
    }
    if (s < NLM) {
        const int n = project ? 2 : 3;
        for (int k = 0; k < n; ++k) lm2d[((int64_t)r * NLM + s) * n + k] = p[k];
    } else {
        for (int k = 0; k < 3; ++k) lm3d[((int64_t)r * NLM + s - NLM) * 3 + k] = p[k];
    }
}

// ---- loss
__constant__ int kPairs[16][2] = {{48, 54}, {49, 59}, {50, 58}, {51, 57}, {52, 56}, {53, 55}, {60, 64}, {61, 67}, {62, 66}, {63, 65},
                                  {36, 39}, {37, 41}, {38, 40}, {42, 45}, {43, 47}, {44, 46}};

__device__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// blocks 0..LOSS_BLOCKS-1: sum |gt - reen| over [B,V,3] and its cotangent; block LOSS_BLOCKS: the 10 mouth / 6 eye pairs
__global__ void __launch_bounds__(256) flame_loss_kernel(const float* __restrict__ lm2d, const float* __restrict__ tv, int B, float ls,
                                                         float lm, float le, float* __restrict__ part, float* __restrict__ g_lm,
                                                         float* __restrict__ g_tv) {
    __shared__ float red[4];
    const int t = threadIdx.x;
    if (blockIdx.x < LOSS_BLOCKS) {
        const int64_t n = (int64_t)B * C3;
        const float gs = ls / (float)n;
        float acc = 0.f;
        for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < n; i += (int64_t)LOSS_BLOCKS * 256) {
            const float d = tv[n + i] - tv[i];
            acc += fabsf(d);
            g_tv[i] = gs * sgn(d);
        }
        const float s = block_sum_256(acc, red);
        if (t == 0) part[blockIdx.x] = s;
        return;
    }
    const int64_t half = (int64_t)B * NLM * 2;
    for (int i = t; i < B * 36 * 2; i += 256) {                 // landmarks 0..35 are in no pair
        const int r = i / 72, l = i - r * 72;
        g_lm[(int64_t)r * NLM * 2 + l] = 0.f;
    }
    float am = 0.f, ae = 0.f;
    const float gm = lm / (10.f * (float)(B * 2)), ge = le / (6.f * (float)(B * 2));
    for (int i = t; i < B * 32; i += 256) {
        const int r = i / 32, pc = i - r * 32, p = pc >> 1, c = pc & 1;
        const int a = kPairs[p][0], b = kPairs[p][1];
        const int64_t ia = ((int64_t)r * NLM + a) * 2 + c, ib = ((int64_t)r * NLM + b) * 2 + c;
        const float dg = fabsf(lm2d[ia] - lm2d[ib]);
        const float de = lm2d[half + ia] - lm2d[half + ib];
        const float u = fabsf(de);
        const float term = fabsf(dg - u);
        const float coef = sgn(u - dg) * sgn(de) * (p < 10 ? gm : ge);
        if (p < 10) am += term; else ae += term;
        g_lm[ia] = coef;
        g_lm[ib] = -coef;
    }
    const float sm = block_sum_256(am, red);
    const float se = block_sum_256(ae, red);
    if (t == 0) {
        part[LOSS_BLOCKS] = sm;
        part[LOSS_BLOCKS + 1] = se;
    }
}

// loss[0]: total; terms: [0..2] lambda-weighted shape / mouth / eye, [3..5] the plain terms
__global__ void __launch_bounds__(64) flame_loss_sum_kernel(const float* __restrict__ part, int B, float ls, float lm, float le,
                                                            float* __restrict__ loss, float* __restrict__ out) {
    const float s = wave_sum(part[threadIdx.x]);
    if (threadIdx.x != 0) return;
    const float t0 = s / (float)((int64_t)B * C3);
    const float t1 = part[LOSS_BLOCKS] / (float)(B * 2) / 10.f;
    const float t2 = part[LOSS_BLOCKS + 1] / (float)(B * 2) / 6.f;
    out[3] = t0; out[4] = t1; out[5] = t2;
    out[0] = ls * t0; out[1] = lm * t1; out[2] = le * t2;
    out[6] = 0.f; out[7] = 0.f;
    loss[0] = (lm * t1 + ls * t0) + le * t2;
}

// ---- backward
// cotangent of landmark slot `l` of landmarks2d (which = 0) / landmarks3d (1), coordinate k, taken back through the projection
__device__ __forceinline__ float lmk_cot(const float* g2, const float* g3, int which, int64_t row, int l, int k, int project, float ps) {
    if (which == 0) {
        if (!g2) return 0.f;
        if (project) return k < 2 ? ps * g2[(row * NLM + l) * 2 + k] : 0.f;
        return g2[(row * NLM + l) * 3 + k];
    }
    if (!g3) return 0.f;
    const float g = g3[(row * NLM + l) * 3 + k];
    return project ? ps * g : g;
}

__global__ void __launch_bounds__(TB) flame_verts_bwd_kernel(const float* __restrict__ g_lm2d, const float* __restrict__ g_lm3d,
                                                             const float* __restrict__ g_tv, int rows, const float* __restrict__ pack,
                                                             int project, const float* __restrict__ saved, float* __restrict__ part) {
    __shared__ float gl[RC][TB], dv[RC][TB], vp[RC][TB];
    __shared__ float As[RC][60];
    __shared__ float cams[RC][4];
    __shared__ int dyns[RC];
    __shared__ float Ws[VB * NJ];
    __shared__ float wred[3][RC][3];
    const int t = threadIdx.x, blk = blockIdx.x, c = blk * TB + t;
    const bool valid = c < C3;
    const int cc = valid ? c : C3 - 1;
    const int vl = t / 3, k = t - 3 * vl, v = cc / 3;
    const float4* sdb = reinterpret_cast<const float4*>(pack + OFF_SDB);
    const int* coff = reinterpret_cast<const int*>(pack + OFF_CO);
    const int* cslot = reinterpret_cast<const int*>(pack + OFF_CS);
    const float* cw = pack + OFF_CW;
    float w[NJ];
    for (int j = 0; j < NJ; ++j) w[j] = valid ? pack[OFF_W + v * NJ + j] : 0.f;
    if (k == 0)
        for (int j = 0; j < NJ; ++j) Ws[vl * NJ + j] = w[j];
    const int e0 = clampi(coff[v], 0, NCSR), e1 = valid ? clampi(coff[v + 1], e0, NCSR) : e0;
    const int nvalid = min(TB, C3 - blk * TB);
    const float sk = (k >= 1) ? -1.f : 1.f;
    for (int r0 = 0; r0 < rows; r0 += RC) {
        const int nr = min(RC, rows - r0);
        __syncthreads();
        for (int i = t; i < RC * 60; i += TB) {
            const int rr = i / 60, l = i - rr * 60;
            As[rr][l] = rr < nr ? saved[(int64_t)(r0 + rr) * SROW + S_A + l] : 0.f;
        }
        if (t < RC * 3) {
            const int rr = t / 3, l = t - rr * 3;
            cams[rr][l] = rr < nr ? saved[(int64_t)(r0 + rr) * SROW + S_CAM + l] : 0.f;
        }
        if (t < RC) dyns[t] = t < nr ? __float_as_int(saved[(int64_t)(r0 + t) * SROW + S_DYN]) : 0;
        __syncthreads();
        // 1. cotangent of the un-projected vertex coordinate: trans_verts through the projection + the landmarks that use the vertex
        for (int r = 0; r < RC; ++r) {
            const int64_t row = r0 + r;
            float g = 0.f, x = 0.f, ds = 0.f, dt = 0.f;
            if (valid && r < nr) {
                const float* S = saved + row * SROW;
                x = S[SMALL + c];
                const float ps = project ? HALF * sk * cams[r][0] : 1.f;
                if (g_tv) {
                    const float gt = g_tv[row * C3 + c];
                    g = project ? ps * gt : gt;
                    if (project) {
                        const float o = S[SMALL + C3 + c];
                        ds = HALF * sk * gt * (k < 2 ? o + cams[r][1 + k] : o);
                        dt = g;
                    }
                }
                for (int e = e0; e < e1; ++e) {
                    const int slot = clampi(cslot[e], 0, NCSR / 3 - 1);
                    float gg = 0.f;
                    if (slot < LSTAT) {
                        gg = lmk_cot(g_lm2d, g_lm3d, 0, row, LDYN + slot, k, project, ps);
                    } else if (slot < LSTAT + LFULL) {
                        gg = lmk_cot(g_lm2d, g_lm3d, 1, row, slot - LSTAT, k, project, ps);
                    } else {
                        const int d = (slot - LSTAT - LFULL) / LDYN, j = (slot - LSTAT - LFULL) - d * LDYN;
                        if (d == dyns[r]) gg = lmk_cot(g_lm2d, g_lm3d, 0, row, j, k, project, ps);
                    }
                    g = fmaf(cw[e], gg, g);
                }
            }
            gl[r][t] = g;
            vp[r][t] = x;
            // dcam of trans_verts: all 64 lanes of every wave are here (wave_sum's precondition)
            const float s0 = wave_sum(ds), s1 = wave_sum(k == 0 ? dt : 0.f), s2 = wave_sum(k == 1 ? dt : 0.f);
            if ((t & 63) == 0) {
                wred[t >> 6][r][0] = s0;
                wred[t >> 6][r][1] = s1;
                wred[t >> 6][r][2] = s2;
            }
        }
        __syncthreads();
        // 2. through the skinning: dL/dv_posed[k] = sum_k' T[k'][k] g[k']
        for (int r = 0; r < RC; ++r) {
            float a = 0.f;
            for (int kp = 0; kp < 3; ++kp) {
                float T = 0.f;
                for (int j = 0; j < NJ; ++j) T = fmaf(w[j], As[r][j * 12 + kp * 4 + k], T);
                a = fmaf(T, gl[r][vl * 3 + kp], a);
            }
            dv[r][t] = a;
        }
        __syncthreads();
        // 3a. dL/dA[j][k'][i] = sum_v W[v][j] g[v][k'] [v_posed, 1][i]
        for (int o = t; o < RC * 60; o += TB) {
            const int r = o / 60, rem = o - r * 60, j = rem / 12, kp = (rem - j * 12) >> 2, i = rem & 3;
            if (r >= nr) continue;
            float a = 0.f;
            for (int u = 0; u < VB; ++u) a = fmaf(Ws[u * NJ + j] * gl[r][u * 3 + kp], i < 3 ? vp[r][u * 3 + i] : 1.f, a);
            part[((int64_t)blk * rows + r0 + r) * PCOLS + P_DA + rem] = a;
        }
        if (t < RC * 3) {
            const int r = t / 3, i = t - r * 3;
            if (r < nr) part[((int64_t)blk * rows + r0 + r) * PCOLS + P_CAM + i] = (wred[0][r][i] + wred[1][r][i]) + wred[2][r][i];
        }
        // 3b. dL/dbetas and dL/dfeature: a thread per (quad of components, group of 4 rows) sweeps the block's coordinates
        if (t < 4 * NQ) {
            const int rg = t / NQ, q = t - rg * NQ;
            float4 acc[4];
            for (int i = 0; i < 4; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int u = 0; u < nvalid; ++u) {
                const float4 s = sdb[(int64_t)(blk * TB + u) * NQ + q];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float d = dv[rg * 4 + i][u];
                    acc[i].x = fmaf(s.x, d, acc[i].x);
                    acc[i].y = fmaf(s.y, d, acc[i].y);
                    acc[i].z = fmaf(s.z, d, acc[i].z);
                    acc[i].w = fmaf(s.w, d, acc[i].w);
                }
            }
            for (int i = 0; i < 4; ++i) {
                const int r = rg * 4 + i;
                if (r < nr) *reinterpret_cast<float4*>(part + ((int64_t)blk * rows + r0 + r) * PCOLS + q * 4) = acc[i];
            }
        }
    }
}

// one block per row: sums the slab in block order, takes dA / dfeature back through the kinematic chain and Rodrigues
__global__ void __launch_bounds__(256) flame_pose_bwd_kernel(const float* __restrict__ part, const float* __restrict__ g_lm2d,
                                                             const float* __restrict__ g_lm3d, const float* __restrict__ gscale,
                                                             int rows, const float* __restrict__ pack, int project,
                                                             const float* __restrict__ saved, float* __restrict__ dshape,
                                                             float* __restrict__ dexp, float* __restrict__ dpose,
                                                             float* __restrict__ dcam) {
    __shared__ float Sm[PCOLS];
    __shared__ float lmc[2 * NLM][3];
    __shared__ float dJs[15];
    const int r = blockIdx.x, t = threadIdx.x;
    const float* S = saved + (int64_t)r * SROW;
    const float scale = gscale ? gscale[0] : 1.f;
    if (t < PCOLS) {
        float a = 0.f;
        for (int b = 0; b < NBLK; ++b) a += part[((int64_t)b * rows + r) * PCOLS + t];
        Sm[t] = a;
    }
    if (t < 2 * NLM) {
        float ds = 0.f, dx = 0.f, dy = 0.f;
        if (project && dcam) {
            const float* verts = S + SMALL + C3;
            int idx[3];
            float b[3];
            lmk_corners(pack, t, __float_as_int(S[S_DYN]), idx, b);
            const float sc = S[S_CAM];
            for (int k = 0; k < 3; ++k) {
                const float sk = (k >= 1) ? -1.f : 1.f;
                const float g = lmk_cot(g_lm2d, g_lm3d, t < NLM ? 0 : 1, r, t < NLM ? t : t - NLM, k, 1, 1.f);
                const float p = verts[idx[0] * 3 + k] * b[0] + verts[idx[1] * 3 + k] * b[1] + verts[idx[2] * 3 + k] * b[2];
                ds += HALF * sk * g * (k < 2 ? p + S[S_CAM + 1 + k] : p);
                if (k == 0) dx = HALF * sc * g;
                if (k == 1) dy = -HALF * sc * g;
            }
        }
        lmc[t][0] = ds; lmc[t][1] = dx; lmc[t][2] = dy;
    }
    __syncthreads();
    if (t == 0) {
        float R[NJ][9], G[NJ][9], J[NJ][3], dG[NJ][9], dGt[NJ][3], dJ[NJ][3], dR0[9], dR2[9];
        for (int j = 0; j < NJ; ++j) {
            for (int i = 0; i < 9; ++i) { R[j][i] = S[S_R + j * 9 + i]; G[j][i] = S[S_G + j * 9 + i]; }
            for (int i = 0; i < 3; ++i) J[j][i] = S[S_J + j * 3 + i];
        }
        for (int j = 0; j < NJ; ++j)
            for (int kk = 0; kk < 3; ++kk) {
                const float at = Sm[P_DA + j * 12 + kk * 4 + 3];
                dGt[j][kk] = at;
                for (int i = 0; i < 3; ++i) dG[j][kk * 3 + i] = Sm[P_DA + j * 12 + kk * 4 + i] - at * J[j][i];
            }
        for (int j = 0; j < NJ; ++j)
            for (int i = 0; i < 3; ++i) {
                float a = 0.f;
                for (int kk = 0; kk < 3; ++kk) a += G[j][kk * 3 + i] * dGt[j][kk];
                dJ[j][i] = -a;
            }
        for (int j = NJ - 1; j >= 1; --j) {
            const int p = parent_of(j);
            float rel[3], drel[3];
            for (int i = 0; i < 3; ++i) rel[i] = J[j][i] - J[p][i];
            if (j == 2)
                for (int kk = 0; kk < 3; ++kk)
                    for (int i = 0; i < 3; ++i) {
                        float a = 0.f;
                        for (int m = 0; m < 3; ++m) a += G[p][m * 3 + kk] * dG[j][m * 3 + i];
                        dR2[kk * 3 + i] = a + Sm[152 + (j - 1) * 9 + kk * 3 + i];
                    }
            for (int kk = 0; kk < 3; ++kk) {
                float a = 0.f;
                for (int m = 0; m < 3; ++m) a += G[p][m * 3 + kk] * dGt[j][m];
                drel[kk] = a;
            }
            for (int kk = 0; kk < 3; ++kk)
                for (int i = 0; i < 3; ++i) {
                    float a = dGt[j][kk] * rel[i];
                    for (int m = 0; m < 3; ++m) a += dG[j][kk * 3 + m] * R[j][i * 3 + m];
                    dG[p][kk * 3 + i] += a;
                }
            for (int i = 0; i < 3; ++i) {
                dGt[p][i] += dGt[j][i];
                dJ[j][i] += drel[i];
                dJ[p][i] -= drel[i];
            }
        }
        for (int i = 0; i < 9; ++i) dR0[i] = dG[0][i];
        for (int i = 0; i < 3; ++i) dJ[0][i] += dGt[0][i];
        for (int j = 0; j < NJ; ++j)
            for (int i = 0; i < 3; ++i) dJs[j * 3 + i] = dJ[j][i];
        float p6[6], dr[3];
        for (int i = 0; i < 6; ++i) p6[i] = S[S_POSE + i];
        rodrigues_bwd(p6, dR0, dr);
        for (int i = 0; i < 3; ++i) dpose[(int64_t)r * 6 + i] = scale * dr[i];
        rodrigues_bwd(p6 + 3, dR2, dr);
        for (int i = 0; i < 3; ++i) dpose[(int64_t)r * 6 + 3 + i] = scale * dr[i];
        if (dcam) {
            float a[3] = {Sm[P_CAM], Sm[P_CAM + 1], Sm[P_CAM + 2]};
            for (int l = 0; l < 2 * NLM; ++l)
                for (int i = 0; i < 3; ++i) a[i] += lmc[l][i];
            for (int i = 0; i < 3; ++i) dcam[(int64_t)r * 3 + i] = project ? scale * a[i] : 0.f;
        }
    }
    __syncthreads();
    if (t < NB) {
        float a = Sm[t];
        for (int kk = 0; kk < 15; ++kk) a = fmaf(pack[OFF_JD + kk * NB + t], dJs[kk], a);
        a *= scale;
        if (t < NSHAPE) dshape[(int64_t)r * NSHAPE + t] = a;
        else dexp[(int64_t)r * NEXP + t - NSHAPE] = a;
    }
}

constexpr int MAX_ROWS = 4096;

// DECA.visofp (deca.py:143-148): the barycentric gather of any per-vertex values at n landmarks (seletec_3d68 of the normals), and
// z < threshold as 0 / 1.  The landmark launch above reads the decode's saved block, so arbitrary [rows,V,3] values get this one.
__global__ void __launch_bounds__(256) flame_visofp_kernel(const float* __restrict__ values, int rows, int nv, const int* __restrict__ corners,
                                                           const float* __restrict__ bary, int n, float threshold, float* __restrict__ vis,
                                                           float* __restrict__ gathered) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * n) return;
    const int r = i / n, s = i - r * n;
    const float* v = values + (int64_t)r * nv * 3;
    const unsigned i0 = (unsigned)corners[s * 3], i1 = (unsigned)corners[s * 3 + 1], i2 = (unsigned)corners[s * 3 + 2];
    float p[3] = {0.f, 0.f, 0.f};
    if (i0 < (unsigned)nv && i1 < (unsigned)nv && i2 < (unsigned)nv)
        for (int k = 0; k < 3; ++k) p[k] = v[i0 * 3 + k] * bary[s * 3] + v[i1 * 3 + k] * bary[s * 3 + 1] + v[i2 * 3 + k] * bary[s * 3 + 2];
    vis[i] = p[2] < threshold ? 1.f : 0.f;
    if (gathered)
        for (int k = 0; k < 3; ++k) gathered[(int64_t)i * 3 + k] = p[k];
}

}  // namespace

extern "C" {

int64_t sgdfr_flame_pack_elems(void) { return PACK_ELEMS; }

int64_t sgdfr_flame_saved_elems(int rows) { return rows <= 0 || rows > MAX_ROWS ? -1 : (int64_t)rows * SROW; }

int64_t sgdfr_flame_workspace_bytes(int rows) {
    if (rows <= 0 || rows > MAX_ROWS) return -1;
    return ((int64_t)NBLK * rows * PCOLS + 128) * (int64_t)sizeof(float);
}

int sgdfr_flame_prepack_f32(const void* const* params, int n_vertices, int n_betas, int n_pose_feature, int n_joints, int n_dynamic_rows,
                            int n_csr, float* pack, void* stream) {
    SGDFR_REQUIRE(n_vertices == V && n_betas == NB && n_pose_feature == NF && n_joints == NJ && n_dynamic_rows == DYNROWS && n_csr == NCSR,
                  "flame: sizes V=%d betas=%d pose feature=%d joints=%d dynamic rows=%d csr=%d, the kernels are built for %d / %d / %d / %d / %d / %d",
                  n_vertices, n_betas, n_pose_feature, n_joints, n_dynamic_rows, n_csr, V, NB, NF, NJ, DYNROWS, NCSR);
    SGDFR_REQUIRE(params && pack, "flame: NULL params or pack");
    for (int i = 0; i < FLAME_PARAMS; ++i) SGDFR_REQUIRE(params[i], "flame: NULL table %d", i);
    hipStream_t st = as_stream(stream);
    const int n = NQ * C3;
    hipLaunchKernelGGL(flame_prepack_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)params[1], (const float*)params[2],
                       reinterpret_cast<float4*>(pack + OFF_SDF), reinterpret_cast<float4*>(pack + OFF_SDB));
    if (check_launch("flame_prepack")) return 1;
    const struct { int p; int64_t off; int n; } copies[] = {
        {0, OFF_VT, C3}, {3, OFF_W, V * NJ}, {4, OFF_JT, 15}, {5, OFF_JD, 15 * NB}, {6, OFF_LSV, LSTAT * 3}, {7, OFF_LSB, LSTAT * 3},
        {8, OFF_LFV, LFULL * 3}, {9, OFF_LFB, LFULL * 3}, {10, OFF_LDV, DYNROWS * LDYN * 3}, {11, OFF_LDB, DYNROWS * LDYN * 3},
        {12, OFF_CO, V + 1}, {13, OFF_CS, NCSR}, {14, OFF_CW, NCSR}};
    for (const auto& cp : copies) {
        const hipError_t e = hipMemcpyAsync(pack + cp.off, params[cp.p], (size_t)cp.n * sizeof(float), hipMemcpyDeviceToDevice, st);
        SGDFR_REQUIRE(e == hipSuccess, "flame: table copy %d failed: %s", cp.p, hipGetErrorString(e));
    }
    return 0;
}

int sgdfr_flame_decode_f32(const float* shape, const float* exp, const float* pose, int rows, const float* shape_b, const float* exp_b,
                           const float* pose_b, int rows_b, const float* cam, const float* pack, int project, float* landmarks2d,
                           float* landmarks3d, float* trans_verts, float* saved, void* stream) {
    SGDFR_REQUIRE(rows > 0 && rows_b >= 0 && rows + rows_b <= MAX_ROWS, "flame: rows=%d rows_b=%d (1..%d in all)", rows, rows_b, MAX_ROWS);
    SGDFR_REQUIRE(shape && exp && pose, "flame: NULL shape / exp / pose");
    SGDFR_REQUIRE(rows_b == 0 || (shape_b && exp_b && pose_b), "flame: NULL second coefficient set with rows_b=%d", rows_b);
    SGDFR_REQUIRE(pack && saved && landmarks2d && landmarks3d, "flame: NULL pack, saved or landmark output");
    SGDFR_REQUIRE(project == 0 || project == 1, "flame: project=%d", project);
    SGDFR_REQUIRE(!project || (cam && trans_verts), "flame: the projection needs cam and trans_verts");
    hipStream_t st = as_stream(stream);
    const int R = rows + rows_b;
    hipLaunchKernelGGL(flame_pose_kernel, dim3(R), dim3(64), 0, st, shape, exp, pose, rows, shape_b, exp_b, pose_b, project ? cam : nullptr,
                       pack, saved);
    if (check_launch("flame_pose")) return 1;
    hipLaunchKernelGGL(flame_verts_kernel, dim3(NBLK), dim3(TB), 0, st, shape, exp, rows, shape_b, exp_b, R, pack, project, saved,
                       trans_verts);
    if (check_launch("flame_verts")) return 1;
    hipLaunchKernelGGL(flame_lmk_kernel, dim3((R * 2 * NLM + 127) / 128), dim3(128), 0, st, R, pack, project, saved, landmarks2d,
                       landmarks3d);
    return check_launch("flame_lmk");
}

int sgdfr_flame_decode_backward_f32(const float* g_landmarks2d, const float* g_landmarks3d, const float* g_trans_verts,
                                    const float* gscale, int rows, const float* pack, int project, const float* saved, float* dshape,
                                    float* dexp, float* dpose, float* dcam, void* workspace, int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(rows > 0 && rows <= MAX_ROWS, "flame: rows=%d (1..%d)", rows, MAX_ROWS);
    SGDFR_REQUIRE(pack && saved && dshape && dexp && dpose, "flame: NULL pack, saved or gradient output");
    SGDFR_REQUIRE(project == 0 || project == 1, "flame: project=%d", project);
    SGDFR_REQUIRE(workspace && workspace_bytes >= sgdfr_flame_workspace_bytes(rows), "flame: workspace of %lld bytes, %lld needed",
                  (long long)workspace_bytes, (long long)sgdfr_flame_workspace_bytes(rows));
    hipStream_t st = as_stream(stream);
    float* part = reinterpret_cast<float*>(workspace) + 128;
    hipLaunchKernelGGL(flame_verts_bwd_kernel, dim3(NBLK), dim3(TB), 0, st, g_landmarks2d, g_landmarks3d, g_trans_verts, rows, pack,
                       project, saved, part);
    if (check_launch("flame_verts_bwd")) return 1;
    hipLaunchKernelGGL(flame_pose_bwd_kernel, dim3(rows), dim3(256), 0, st, (const float*)part, g_landmarks2d, g_landmarks3d, gscale, rows,
                       pack, project, saved, dshape, dexp, dpose, dcam);
    return check_launch("flame_pose_bwd");
}

int sgdfr_shape_loss_f32(const float* landmarks2d, const float* trans_verts, int rows, float lambda_shape, float lambda_mouth,
                         float lambda_eye, float* loss, float* terms, float* g_landmarks2d, float* g_trans_verts, void* workspace,
                         int64_t workspace_bytes, void* stream) {
    SGDFR_REQUIRE(rows > 0 && 2 * rows <= MAX_ROWS, "shape_loss: rows=%d (1..%d)", rows, MAX_ROWS / 2);
    SGDFR_REQUIRE(landmarks2d && trans_verts && loss && terms && g_landmarks2d && g_trans_verts, "shape_loss: NULL input or output");
    SGDFR_REQUIRE(workspace && workspace_bytes >= (int64_t)128 * (int64_t)sizeof(float), "shape_loss: workspace of %lld bytes, %lld needed",
                  (long long)workspace_bytes, (long long)(128 * sizeof(float)));
    hipStream_t st = as_stream(stream);
    float* part = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(flame_loss_kernel, dim3(LOSS_BLOCKS + 1), dim3(256), 0, st, landmarks2d, trans_verts, rows, lambda_shape,
                       lambda_mouth, lambda_eye, part, g_landmarks2d, g_trans_verts);
    if (check_launch("flame_loss")) return 1;
    hipLaunchKernelGGL(flame_loss_sum_kernel, dim3(1), dim3(64), 0, st, (const float*)part, rows, lambda_shape, lambda_mouth, lambda_eye,
                       loss, terms);
    return check_launch("flame_loss_sum");
}

int sgdfr_flame_visofp_f32(const float* values, int rows, int n_vertices, const int* corners, const float* bary, int n, float threshold,
                           float* vis, float* gathered, void* stream) {
    SGDFR_REQUIRE(values && corners && bary && vis, "flame_visofp: NULL input or output");
    SGDFR_REQUIRE(rows > 0 && rows <= MAX_ROWS && n_vertices >= 1 && n_vertices <= (1 << 24) && n >= 1 && n <= 4096,
                  "flame_visofp: rows=%d vertices=%d landmarks=%d (rows 1..%d, vertices 1..2^24, landmarks 1..4096)", rows, n_vertices, n, MAX_ROWS);
    hipLaunchKernelGGL(flame_visofp_kernel, dim3((rows * n + 255) / 256), dim3(256), 0, as_stream(stream), values, rows, n_vertices, corners,
                       bary, n, threshold, vis, gathered);
    return check_launch("flame_visofp");
}

}  // extern "C"
