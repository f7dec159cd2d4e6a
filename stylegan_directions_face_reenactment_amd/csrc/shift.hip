// Shift-vector construction on the device: (3DMM parameters of source and target) -> rows of the DirectionMatrix input.
//
// The reference builds this vector on the host, one frame at a time, with ~10 `.detach().cpu().numpy()` round trips
// (run_inference.py:201-254 Inference.make_shift), and in the trainer with one small torch op per direction
// (libs/utilities/utils_train.py:127-175 make_shift_vector, :177-288 make_shift_vector_50).  Here a whole batch is one
// launch, one thread per (frame, direction); the per-direction recipe is a small table passed by value.
//
// The two reference call sites do NOT use the same arithmetic, and both are mirrored operation by operation so the
// result is bit-identical to the one the caller would have computed:
//   arith 0 (run_inference.py): 0-d float32 numpy values against float64 numpy scalars ->  the angle is scaled in
//           float32 (`yaw * shift_scale`), divided in float64 (`/ angle_scales[i]`), differences are taken in float64 and
//           rounded once when stored into the float32 tensor; `a*x + b` is float64 throughout.
//   arith 1 (utils_train.py): float32 torch tensors against Python/numpy scalars -> every operation rounds to float32
//           (scalar operands are cast to float32 first), multiply and add are separate roundings (no fma).
#include "common.h"

namespace sgdfr {

struct DirTable {
    sgdfr_direction d[SGDFR_MAX_DIRECTIONS];
};

// the three parameter arrays of one face set, indexed by (kind - 1): angles [*,3] (yaw, pitch, roll), pose [*,pose_dim],
// alpha_exp [*,exp_dim]; bs = batch stride in floats (0 = one source for every frame)
struct ShiftSrc {
    const float* base[3];
    int64_t bs[3];
};

// (An if-chain over three (pointer, stride) members was miscompiled by hipcc 7.2 for gfx950: the expression branch kept
// the pose stride -- caught by the golden test.  Both selections are therefore written as explicit, separate selects.)
__device__ __forceinline__ float pick(const ShiftSrc& p, const sgdfr_direction& e, int n) {
    const int k = e.kind;
    const float* b = k == SGDFR_DIR_ANGLE ? p.base[0] : (k == SGDFR_DIR_JAW ? p.base[1] : p.base[2]);
    const int64_t st = k == SGDFR_DIR_ANGLE ? p.bs[0] : (k == SGDFR_DIR_JAW ? p.bs[1] : p.bs[2]);
    return b[n * st + e.col];
}

// position of a value on the direction's shift axis, float64 flavour (run_inference.py:217-252)
__device__ __forceinline__ double place64(const sgdfr_direction& e, float x) {
    if (e.kind == SGDFR_DIR_ANGLE) return __ddiv_rn((double)__fmul_rn(x, (float)e.a), e.b);
    return __dadd_rn(__dmul_rn(e.a, (double)x), e.b);
}

// float32 flavour (utils_train.py:132-172)
__device__ __forceinline__ float place32(const sgdfr_direction& e, float x) {
    if (e.kind == SGDFR_DIR_ANGLE) return __fdiv_rn(__fmul_rn(x, (float)e.a), (float)e.b);
    return __fadd_rn(__fmul_rn((float)e.a, x), (float)e.b);
}

__global__ __launch_bounds__(256) void make_shift_kernel(ShiftSrc src, ShiftSrc tgt, DirTable tab, int D, float* __restrict__ out,
                                                        int N, int arith) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * D) return;
    const int n = i / D, k = i - n * D;
    const sgdfr_direction e = tab.d[k];
    float v = 0.f;
    if (e.kind != SGDFR_DIR_ZERO) {
        const float xs = pick(src, e, n), xt = pick(tgt, e, n);
        if (arith == 0) v = (float)__dsub_rn(place64(e, xt), place64(e, xs));
        else v = __fsub_rn(place32(e, xt), place32(e, xs));
    }
    out[i] = v;
}

// second half of make_shift_vector_50 (utils_train.py:227-286): one randomly chosen direction per sample gets a uniform
// draw from [-shift_scale - start, shift_scale - start]; `u` in [0,1) and the direction indices come from the caller
__global__ __launch_bounds__(256) void make_shift_random_kernel(ShiftSrc src, DirTable tab, int D, const int* __restrict__ which,
                                                               const float* __restrict__ u, float shift_scale,
                                                               float* __restrict__ out, int N) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * D) return;
    const int n = i / D, k = i - n * D;
    float v = 0.f;
    const sgdfr_direction e = tab.d[k];
    if (which[n] == k && e.kind != SGDFR_DIR_ZERO) {
        const float start = place32(e, pick(src, e, n));
        const float lo = __fsub_rn(-shift_scale, start), hi = __fsub_rn(shift_scale, start);
        v = __fadd_rn(__fmul_rn(__fsub_rn(lo, hi), u[n]), hi);
    }
    out[i] = v;
}

// batch_euler2axis(deg2rad(angles)) (decalib/utils/rotation_converter.py:48-90, 256-307) for one row, every float32 operation
// of the tensor code rounded on its own and in its order: x*pi/180, the half angles, euler_to_quaternion's products,
// quaternion_to_angle_axis with both of its `where`s (cos_theta < 0; sin^2 > 0, else k = 2).  sinf / cosf / atan2f are the device
// library's: an ulp or two from the host's, which is all that separates this from the reference's own fp32 result.
__device__ __forceinline__ void euler_deg_to_axis(const float ang[3], float aa[3]) {
    const float pi = 3.14159265358979323846f;
    float c[3], s[3];
    for (int i = 0; i < 3; ++i) {
        const float h = __fdiv_rn(__fdiv_rn(__fmul_rn(ang[i], pi), 180.f), 2.f);
        c[i] = cosf(h);
        s[i] = sinf(h);
    }
    const float cx = c[0], cy = c[1], cz = c[2], sx = s[0], sy = s[1], sz = s[2];
    const float q0 = __fsub_rn(__fmul_rn(__fmul_rn(cx, cy), cz), __fmul_rn(__fmul_rn(sx, sy), sz));
    const float q1 = __fadd_rn(__fmul_rn(__fmul_rn(cx, sy), sz), __fmul_rn(__fmul_rn(cy, cz), sx));
    const float q2 = __fsub_rn(__fmul_rn(__fmul_rn(cx, cz), sy), __fmul_rn(__fmul_rn(sx, cy), sz));
    const float q3 = __fadd_rn(__fmul_rn(__fmul_rn(cx, cy), sz), __fmul_rn(__fmul_rn(sx, cz), sy));
    const float sin2 = __fadd_rn(__fadd_rn(__fmul_rn(q1, q1), __fmul_rn(q2, q2)), __fmul_rn(q3, q3));
    const float sin_t = __fsqrt_rn(sin2);
    const float two_t = __fmul_rn(2.f, q0 < 0.f ? atan2f(-sin_t, -q0) : atan2f(sin_t, q0));
    const float k = sin2 > 0.f ? __fdiv_rn(two_t, sin_t) : 2.f;
    aa[0] = __fmul_rn(q1, k);
    aa[1] = __fmul_rn(q2, k);
    aa[2] = __fmul_rn(q3, k);
}

// get_params_gt_reenacted (utils_train.py:291-374), one thread per row: the first half of the batch copies the target's pose and
// expression, a row of the second half copies the source's and moves the ONE coefficient its drawn direction which[row - B/2]
// drives by the drawn shift.  An index outside the table, or one the table does not drive, leaves the source copy (the
// reference's chain of ifs falls through in the same way).
__global__ __launch_bounds__(64) void gt_reenacted_kernel(ShiftSrc src, const float* __restrict__ pose_t, const float* __restrict__ exp_t,
                                                          const float* __restrict__ shift, const int* __restrict__ which, DirTable tab,
                                                          int D, float shift_scale, float* __restrict__ pose_gt,
                                                          float* __restrict__ exp_gt, int B, int pose_dim, int exp_dim) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= B) return;
    const int half = B / 2;
    const bool first = n < half;
    const float* pose = (first ? pose_t : src.base[1]) + (int64_t)n * pose_dim;
    const float* expr = (first ? exp_t : src.base[2]) + (int64_t)n * exp_dim;
    float* po = pose_gt + (int64_t)n * pose_dim;
    float* eo = exp_gt + (int64_t)n * exp_dim;
    for (int j = 0; j < pose_dim; ++j) po[j] = pose[j];
    for (int j = 0; j < exp_dim; ++j) eo[j] = expr[j];
    if (first) return;
    const int ind = which[n - half];
    if (ind < 0 || ind >= D) return;
    const sgdfr_direction e = tab.d[ind];
    const float sh = shift[(int64_t)n * D + ind];
    if (e.kind == SGDFR_DIR_ANGLE) {
        const float* a = src.base[0] + (int64_t)n * 3;
        float ang[3] = {a[0], a[1], a[2]}, aa[3];
        const float start = __fdiv_rn(__fmul_rn(e.col == 0 ? ang[0] : (e.col == 1 ? ang[1] : ang[2]), shift_scale), (float)e.b);
        const float moved = __fdiv_rn(__fmul_rn(__fadd_rn(start, sh), (float)e.b), shift_scale);
        for (int j = 0; j < 3; ++j) ang[j] = j == e.col ? moved : ang[j];     // (a select: no dynamically indexed private array)
        euler_deg_to_axis(ang, aa);
        po[0] = aa[1];                                                          // utils_train.py:311-314: the reference's swap
        po[1] = -aa[0];
        po[2] = aa[2];
    } else if (e.kind == SGDFR_DIR_JAW || e.kind == SGDFR_DIR_EXP) {
        const float fa = (float)e.a, fb = (float)e.b;
        const float x = e.kind == SGDFR_DIR_JAW ? pose[e.col] : expr[e.col];
        const float moved = __fdiv_rn(__fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(fa, x), fb), sh), fb), fa);
        if (e.kind == SGDFR_DIR_JAW) po[e.col] = moved;
        else eo[e.col] = moved;
    }
}

static int check_table(const sgdfr_direction* table, int D, int pose_dim, int exp_dim, DirTable* out) {
    SGDFR_REQUIRE(table && D >= 1 && D <= SGDFR_MAX_DIRECTIONS, "make_shift: 1..%d directions, got %d", SGDFR_MAX_DIRECTIONS, D);
    for (int k = 0; k < D; ++k) {
        const sgdfr_direction& e = table[k];
        const int lim = e.kind == SGDFR_DIR_ANGLE ? 3 : e.kind == SGDFR_DIR_JAW ? pose_dim : e.kind == SGDFR_DIR_EXP ? exp_dim : 1;
        SGDFR_REQUIRE(e.kind >= SGDFR_DIR_ZERO && e.kind <= SGDFR_DIR_EXP, "make_shift: direction %d has unknown kind %d", k, e.kind);
        SGDFR_REQUIRE(e.col >= 0 && e.col < lim, "make_shift: direction %d reads column %d of %d", k, e.col, lim);
        SGDFR_REQUIRE(e.kind != SGDFR_DIR_ANGLE || e.b != 0.0, "make_shift: direction %d has a zero angle scale", k);
        out->d[k] = e;
    }
    return 0;
}

}  // namespace sgdfr

using namespace sgdfr;

extern "C" int sgdfr_make_shift_f32(const float* ang_s, int64_t ang_s_bs, const float* pose_s, int64_t pose_s_bs, const float* exp_s,
                                    int64_t exp_s_bs, const float* ang_t, const float* pose_t, const float* exp_t, int pose_dim,
                                    int exp_dim, const struct sgdfr_direction* table, int D, float* shift, int N, int arith,
                                    void* stream) {
    SGDFR_REQUIRE(N >= 0 && pose_dim >= 1 && exp_dim >= 1, "make_shift: bad sizes N=%d pose_dim=%d exp_dim=%d", N, pose_dim, exp_dim);
    SGDFR_REQUIRE(arith == 0 || arith == 1, "make_shift: arith must be 0 (float64 scalars) or 1 (float32 tensors), got %d", arith);
    DirTable tab;
    if (int rc = check_table(table, D, pose_dim, exp_dim, &tab)) return rc;
    if (N == 0) return 0;                  // empty batch: empty tensors carry null pointers
    SGDFR_REQUIRE(ang_s && pose_s && exp_s && ang_t && pose_t && exp_t && shift, "make_shift: null pointer");
    ShiftSrc src{{ang_s, pose_s, exp_s}, {ang_s_bs, pose_s_bs, exp_s_bs}};
    ShiftSrc tgt{{ang_t, pose_t, exp_t}, {3, pose_dim, exp_dim}};
    const int total = N * D;
    hipLaunchKernelGGL(make_shift_kernel, dim3((total + 255) / 256), dim3(256), 0, as_stream(stream), src, tgt, tab, D, shift, N, arith);
    return check_launch("make_shift");
}

extern "C" int sgdfr_make_shift_random_f32(const float* ang_s, const float* pose_s, const float* exp_s, int pose_dim, int exp_dim,
                                           const int* which, const float* u, float shift_scale,
                                           const struct sgdfr_direction* table, int D, float* shift, int N, void* stream) {
    SGDFR_REQUIRE(N >= 0 && pose_dim >= 1 && exp_dim >= 1, "make_shift_random: bad sizes N=%d pose_dim=%d exp_dim=%d", N, pose_dim,
                  exp_dim);
    DirTable tab;
    if (int rc = check_table(table, D, pose_dim, exp_dim, &tab)) return rc;
    if (N == 0) return 0;
    SGDFR_REQUIRE(ang_s && pose_s && exp_s && which && u && shift, "make_shift_random: null pointer");
    ShiftSrc src{{ang_s, pose_s, exp_s}, {3, pose_dim, exp_dim}};
    const int total = N * D;
    hipLaunchKernelGGL(make_shift_random_kernel, dim3((total + 255) / 256), dim3(256), 0, as_stream(stream), src, tab, D, which, u,
                       shift_scale, shift, N);
    return check_launch("make_shift_random");
}

extern "C" int sgdfr_gt_reenacted_f32(const float* pose_s, const float* exp_s, const float* ang_s, const float* pose_t, const float* exp_t,
                                      int pose_dim, int exp_dim, const float* shift, const int* which, float shift_scale,
                                      const struct sgdfr_direction* table, int D, float* pose_gt, float* exp_gt, int B, void* stream) {
    SGDFR_REQUIRE(B >= 0 && B % 2 == 0, "gt_reenacted: the batch must be even (two halves), got %d", B);
    SGDFR_REQUIRE(pose_dim >= 3 && exp_dim >= 1, "gt_reenacted: bad sizes pose_dim=%d exp_dim=%d", pose_dim, exp_dim);
    SGDFR_REQUIRE(shift_scale != 0.f, "gt_reenacted: shift_scale is zero");
    DirTable tab;
    if (int rc = check_table(table, D, pose_dim, exp_dim, &tab)) return rc;
    for (int k = 0; k < D; ++k)
        SGDFR_REQUIRE((tab.d[k].kind != SGDFR_DIR_JAW && tab.d[k].kind != SGDFR_DIR_EXP) || tab.d[k].a != 0.0,
                      "gt_reenacted: direction %d has a zero slope", k);
    if (B == 0) return 0;
    SGDFR_REQUIRE(pose_s && exp_s && ang_s && pose_t && exp_t && shift && which && pose_gt && exp_gt, "gt_reenacted: null pointer");
    ShiftSrc src{{ang_s, pose_s, exp_s}, {3, pose_dim, exp_dim}};
    hipLaunchKernelGGL(gt_reenacted_kernel, dim3((B + 63) / 64), dim3(64), 0, as_stream(stream), src, pose_t, exp_t, shift, which, tab, D,
                       shift_scale, pose_gt, exp_gt, B, pose_dim, exp_dim);
    return check_launch("gt_reenacted");
}
