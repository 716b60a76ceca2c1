// yavo_se3.h -- device restatements of the Sophus SE3d operations the geometry kernels share (pose = SE3d::data()
// = {qx, qy, qz, qw, tx, ty, tz}): Eigen quaternion product / rotation / toRotationMatrix, SE3 act / mul (with
// Sophus' renormalisation) / inverse and SE3::exp with fdlibm's sin / cos kernels (oracle/yavo_oracle_geom.c: or_se3_*).
// Every expression in the oracle's order; files are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace yavo {
namespace se3 {

// 3 x 3 product, sequential dot products (OpenCV small-matrix gemm)
__device__ __forceinline__ void mm3(const double* A, const double* B, double* C) {
    double R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = A[i * 3 + 0] * B[0 * 3 + j] + A[i * 3 + 1] * B[1 * 3 + j] + A[i * 3 + 2] * B[2 * 3 + j];
#pragma unroll
    for (int i = 0; i < 9; ++i) C[i] = R[i];
}

// sin / cos past pi/4, operation for operation the oracle's (k_rem_pio2 / k_sin_tail / k_cos_tail in
// oracle/yavo_oracle_geom.c): below 2^20 fdlibm's medium-range reduction (Cody-Waite with pi/2 in three 33-bit pieces,
// always with the cancellation check) and its kernels on the reduced argument with its tail; the device library's and
// the host's own sin / cos differ by an ulp there.  Larger or non-finite arguments go to the library (Payne-Hanek
// reduction and all).  Rare and register-hungry, so kept out of line -- inlined into the pose LM's lane-0 step they
// set the whole kernel's register peak.
__device__ __forceinline__ int dbl_exponent(double x) { return (__double2hiint(x) >> 20) & 0x7ff; }

// x = n pi/2 + (y0 + y1), |y0| <= pi/4 (+ an ulp); returns n mod 4
__device__ __forceinline__ int k_rem_pio2(double x, double& y0o, double& y1o) {
    const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00,
                 pio2_1t = 6.07710050650619224932e-11, pio2_2 = 6.07710050630396597660e-11,
                 pio2_2t = 2.02226624879595063154e-21, pio2_3 = 2.02226624871116645580e-21,
                 pio2_3t = 8.47842766036889956997e-32;
    const double t0 = fabs(x);
    const int n = (int)(t0 * invpio2 + 0.5);
    const double fn = (double)n;
    double r = t0 - fn * pio2_1, w = fn * pio2_1t;
    const int j = dbl_exponent(t0);
    double y0 = r - w;
    if (j - dbl_exponent(y0) > 16) {  // 2nd iteration, good to 118 bits
        double t = r;
        w = fn * pio2_2;
        r = t - w;
        w = fn * pio2_2t - ((t - r) - w);
        y0 = r - w;
        if (j - dbl_exponent(y0) > 49) {  // 3rd iteration, 151 bits
            t = r;
            w = fn * pio2_3;
            r = t - w;
            w = fn * pio2_3t - ((t - r) - w);
            y0 = r - w;
        }
    }
    const double y1 = (r - y0) - w;
    const bool neg = x < 0;
    y0o = neg ? -y0 : y0;
    y1o = neg ? -y1 : y1;
    return (neg ? -n : n) & 3;
}

__device__ __forceinline__ double k_sin_tail(double x, double y) {  // __kernel_sin(x, y, 1)
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    double z = x * x, v = z * x;
    double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}

__device__ __forceinline__ double k_cos_tail(double x, double y) {  // __kernel_cos(x, y)
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    double z = x * x;
    double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    double hz = 0.5 * z, w = 1.0 - hz;
    return w + (((1.0 - w) - hz) + (z * r - x * y));
}

// q = 0: sin(x), q = 1: cos(x) = sin(x + pi/2)
__device__ __noinline__ double k_trig_full(double x, int q) {
    if (!(fabs(x) < 1048576.0)) return q ? cos(x) : sin(x);
    double y0, y1;
    const int n = (k_rem_pio2(x, y0, y1) + q) & 3;
    const double v = (n & 1) ? k_cos_tail(y0, y1) : k_sin_tail(y0, y1);
    return (n & 2) ? -v : v;
}
__device__ __forceinline__ double k_sin_full(double x) { return k_trig_full(x, 0); }
__device__ __forceinline__ double k_cos_full(double x) { return k_trig_full(x, 1); }

__device__ __forceinline__ double k_sin(double x) {
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    if (!(fabs(x) <= 0.78539816339744827900)) return k_sin_full(x);
    double z = x * x, v = z * x;
    double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    return x + v * (S1 + z * r);
}

__device__ __forceinline__ double k_cos(double x) {
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    if (!(fabs(x) <= 0.78539816339744827900)) return k_cos_full(x);
    double z = x * x;
    double r = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    double hz = 0.5 * z, w = 1.0 - hz;
    return w + (((1.0 - w) - hz) + (z * r - x * 0.0));
}

__device__ __forceinline__ void quat_mul(const double* a, const double* b, double* r) {
    double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    r[3] = aw * bw - ax * bx - ay * by - az * bz;
    r[0] = aw * bx + ax * bw + ay * bz - az * by;
    r[1] = aw * by + ay * bw + az * bx - ax * bz;
    r[2] = aw * bz + az * bw + ax * by - ay * bx;
}

__device__ __forceinline__ void quat_rotate(const double* q, const double* v, double* out) {
    double uv0 = q[1] * v[2] - q[2] * v[1];
    double uv1 = q[2] * v[0] - q[0] * v[2];
    double uv2 = q[0] * v[1] - q[1] * v[0];
    uv0 += uv0; uv1 += uv1; uv2 += uv2;
    double c0 = q[1] * uv2 - q[2] * uv1;
    double c1 = q[2] * uv0 - q[0] * uv2;
    double c2 = q[0] * uv1 - q[1] * uv0;
    out[0] = v[0] + q[3] * uv0 + c0;
    out[1] = v[1] + q[3] * uv1 + c1;
    out[2] = v[2] + q[3] * uv2 + c2;
}

__device__ __forceinline__ void quat_to_R(const double* q, double* R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

__device__ __forceinline__ void se3_act(const double* T, const double* p, double* out) {
    double r[3];
    quat_rotate(T, p, r);
    out[0] = r[0] + T[4];
    out[1] = r[1] + T[5];
    out[2] = r[2] + T[6];
}

__device__ __forceinline__ void se3_mul(const double* A, const double* B, double* out) {
    double r[3], q[4];
    quat_rotate(A, B + 4, r);
    double t0 = A[4] + r[0], t1 = A[5] + r[1], t2 = A[6] + r[2];
    quat_mul(A, B, q);
    double sn = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (sn != 1.0) {
        double sc = 2.0 / (1.0 + sn);
        for (int i = 0; i < 4; ++i) q[i] *= sc;
    }
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; out[3] = q[3];
    out[4] = t0; out[5] = t1; out[6] = t2;
}

// Sophus SE3d::inverse on data() = {qx, qy, qz, qw, tx, ty, tz}: SO3(q*) renormalised, -t rotated as Eigen's
// Quaternion * Vector3 (uv = 2 (q.vec x v); v + w uv + q.vec x uv): or_se3_inverse / ya_vo_amd/sequence.py
// se3_inverse, operation for operation (no contraction: -ffp-contract=off; sqrt and / correctly rounded)
__device__ void se3_inverse(const double* T, double* o) {
    double x = -T[0], y = -T[1], z = -T[2], w = T[3];
    const double len = sqrt((x * x + z * z) + (y * y + w * w));  // the SO3 constructor's normalisation
    x = x / len;
    y = y / len;
    z = z / len;
    w = w / len;
    const double vx = T[4] * -1.0, vy = T[5] * -1.0, vz = T[6] * -1.0;
    double ux = y * vz - z * vy, uy = z * vx - x * vz, uz = x * vy - y * vx;
    ux += ux;
    uy += uy;
    uz += uz;
    const double cx = y * uz - z * uy, cy = z * ux - x * uz, cz = x * uy - y * ux;
    o[0] = x;
    o[1] = y;
    o[2] = z;
    o[3] = w;
    o[4] = vx + w * ux + cx;
    o[5] = vy + w * uy + cy;
    o[6] = vz + w * uz + cz;
}

__device__ void se3_exp(const double* a, double* out) {
    const double* om = a + 3;
    const double eps = 1e-10;
    double theta_sq = om[0] * om[0] + om[1] * om[1] + om[2] * om[2];
    double theta, imag, real;
    if (theta_sq < eps * eps) {
        theta = 0;
        double theta_po4 = theta_sq * theta_sq;
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * theta_po4;
        real = 1 - (1.0 / 8.0) * theta_sq + (1.0 / 384.0) * theta_po4;
    } else {
        theta = sqrt(theta_sq);
        double half = 0.5 * theta;
        imag = k_sin(half) / theta;
        real = k_cos(half);
    }
    double q[4] = {imag * om[0], imag * om[1], imag * om[2], real};
    double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double O2[9];
    mm3(O, O, O2);
    double V[9];
    if (theta < eps) {
        quat_to_R(q, V);
    } else {
        double theta_sq2 = theta * theta;
        double a1 = (1 - k_cos(theta)) / theta_sq2;
        double a2 = (theta - k_sin(theta)) / (theta_sq2 * theta);
        for (int i = 0; i < 9; ++i) V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + a1 * O[i] + a2 * O2[i];
    }
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; out[3] = q[3];
    for (int i = 0; i < 3; ++i) out[4 + i] = V[3 * i] * a[0] + V[3 * i + 1] * a[1] + V[3 * i + 2] * a[2];
}

}  // namespace se3
}  // namespace yavo
