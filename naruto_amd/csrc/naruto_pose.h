// The pose arithmetic shared by camera tracking (naruto_track.hip) and by the pose refinement inside global_BA (naruto_bapose.hip):
// a pose is (omega [3], the absolute axis-angle of the camera-to-world rotation; t [3]), R(omega) = exp([omega]x) by Rodrigues' formula,
// stepped by torch.optim.Adam (single tensor, no weight decay, amsgrad off).  Host and device: the host-only debug entry points run
// the same code.
#pragma once

#include "naruto_common.h"

namespace naruto {

// A = sin(th)/th, B = (1 - cos(th))/th^2 and a = A'(th)/th, b = B'(th)/th; series below th = 1e-2 (fp64: the closed forms lose
// ~1e-16 / th^2 there; the truncated series' error is below th^8 / 1e6)
__host__ __device__ inline void rodrigues_coeffs(double th2, double& A, double& B, double& a, double& b) {
    if (th2 < 1e-4) {
        A = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0 * (1.0 - th2 / 42.0));
        B = 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0 * (1.0 - th2 / 56.0));
        a = -1.0 / 3.0 + th2 / 30.0 - th2 * th2 / 840.0 + th2 * th2 * th2 / 45360.0;
        b = -1.0 / 12.0 + th2 / 180.0 - th2 * th2 / 6720.0 + th2 * th2 * th2 / 453600.0;
        return;
    }
    const double th = sqrt(th2), s = sin(th), c = cos(th);
    A = s / th;
    B = (1.0 - c) / th2;
    a = (th * c - s) / (th2 * th);
    b = (th * s - 2.0 * (1.0 - c)) / (th2 * th2);
}

// R = I + A K + B K^2, K = [w]x (row-major)
__host__ __device__ inline void rodrigues(const double w[3], double R[9]) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double A, B, a, b;
    rodrigues_coeffs(th2, A, B, a, b);
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double k2 = 0.0;
            for (int m = 0; m < 3; ++m) k2 += K[3 * i + m] * K[3 * m + j];
            R[3 * i + j] = (i == j ? 1.0 : 0.0) + A * K[3 * i + j] + B * k2;
        }
}

// d_w = VJP of rodrigues at w with cotangent G (dL/dR, row-major):
//   dR/dw_k = a w_k K + A K_k + b w_k K^2 + B (K_k K + K K_k),  K_k = [e_k]x
__host__ __device__ inline void rodrigues_vjp(const double w[3], const double G[9], double d_w[3]) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double A, B, a, b;
    rodrigues_coeffs(th2, A, B, a, b);
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double gK = 0.0, gK2 = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double k2 = 0.0;
            for (int m = 0; m < 3; ++m) k2 += K[3 * i + m] * K[3 * m + j];
            gK += G[3 * i + j] * K[3 * i + j];
            gK2 += G[3 * i + j] * k2;
        }
    for (int k = 0; k < 3; ++k) {
        double Kk[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const int p = (k + 1) % 3, q = (k + 2) % 3;        // [e_k]x: +1 at (q, p), -1 at (p, q)
        Kk[3 * q + p] = 1.0;
        Kk[3 * p + q] = -1.0;
        double gKk = 0.0, gS = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double s = 0.0;
                for (int m = 0; m < 3; ++m) s += Kk[3 * i + m] * K[3 * m + j] + K[3 * i + m] * Kk[3 * m + j];
                gKk += G[3 * i + j] * Kk[3 * i + j];
                gS += G[3 * i + j] * s;
            }
        d_w[k] = a * w[k] * gK + A * gKk + b * w[k] * gK2 + B * gS;
    }
}

// the fp32 rotation the rays are formed with: R(omega) in fp64, rounded once
__host__ __device__ inline void track_pose_matrix(const float p[6], float Rf[9]) {
    const double w[3] = {(double)p[0], (double)p[1], (double)p[2]};
    double R[9];
    rodrigues(w, R);
#pragma unroll
    for (int i = 0; i < 9; ++i) Rf[i] = (float)R[i];
}

// [4,4] row-major camera-to-world of the pose p = (omega, t)
__host__ __device__ inline void track_write_c2w(float* c2w, const float p[6]) {
    float Rf[9];
    track_pose_matrix(p, Rf);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c2w[4 * i] = Rf[3 * i]; c2w[4 * i + 1] = Rf[3 * i + 1]; c2w[4 * i + 2] = Rf[3 * i + 2]; c2w[4 * i + 3] = p[3 + i];
    }
    c2w[12] = 0.0f; c2w[13] = 0.0f; c2w[14] = 0.0f; c2w[15] = 1.0f;
}

// ---- the pose chain's arithmetic (naruto_posechain.hip): [4,4] row-major camera-to-world matrices, fp32 in memory, fp64 in registers,
// every result rounded to fp32 once

__host__ __device__ inline void pose_load(const float* m, double M[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) M[i] = (double)m[i];
}

__host__ __device__ inline void pose_store(float* m, const double M[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = (float)M[i];
}

// C = A @ B
__host__ __device__ inline void pose_mul(const double A[16], const double B[16], double C[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += A[4 * i + k] * B[4 * k + j];
            C[4 * i + j] = s;
        }
}

// the inverse of the affine map [A t; 0 0 0 1]: adj(A) / det(A), then -A^-1 t.  General: A need not be a rotation (a tracked or
// refined pose is R(omega) rounded to fp32, and torch.linalg.inv, which this restates, does not assume one either)
__host__ __device__ inline void pose_affine_inverse(const double M[16], double inv[16]) {
    const double a = M[0], b = M[1], c = M[2], d = M[4], e = M[5], f = M[6], g = M[8], h = M[9], k = M[10];
    const double c00 = e * k - f * h, c01 = c * h - b * k, c02 = b * f - c * e;
    const double c10 = f * g - d * k, c11 = a * k - c * g, c12 = c * d - a * f;
    const double c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
    const double r = 1.0 / (a * c00 + b * c10 + c * c20);
    const double A[9] = {c00 * r, c01 * r, c02 * r, c10 * r, c11 * r, c12 * r, c20 * r, c21 * r, c22 * r};
    const double t[3] = {M[3], M[7], M[11]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        inv[4 * i] = A[3 * i]; inv[4 * i + 1] = A[3 * i + 1]; inv[4 * i + 2] = A[3 * i + 2];
        inv[4 * i + 3] = -(A[3 * i] * t[0] + A[3 * i + 1] * t[1] + A[3 * i + 2] * t[2]);
    }
    inv[12] = 0.0; inv[13] = 0.0; inv[14] = 0.0; inv[15] = 1.0;
}

// (omega, t) of a camera-to-world matrix: naruto_amd.tracking.matrices_to_pose6, branch for branch -- the unit quaternion through the
// largest of 4w^2, 4x^2, 4y^2, 4z^2 (the first of equal ones), w >= 0 (angle in [0, pi]), omega = 2 atan2(|v|, w) v / |v|, and
// 2 v / w below |v| = 1e-12
__host__ __device__ inline void pose_log(const float* c2w, float pose6[6]) {
    double M[16];
    pose_load(c2w, M);
    const double d0 = M[0], d1 = M[5], d2 = M[10];
    const double cand[4] = {1.0 + d0 + d1 + d2, 1.0 + d0 - d1 - d2, 1.0 - d0 + d1 - d2, 1.0 - d0 - d1 + d2};
    int br = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (cand[i] > cand[br]) br = i;
    const double cb = cand[br] > 1e-300 ? cand[br] : 1e-300;
    const double s = 2.0 * sqrt(cb), q4 = s / 4.0;
    const double x = M[9] - M[6], y = M[2] - M[8], z = M[4] - M[1];
    const double xy = M[1] + M[4], xz = M[2] + M[8], yz = M[6] + M[9];
    double q[4];
    if (br == 0)      { q[0] = q4;    q[1] = x / s;  q[2] = y / s;  q[3] = z / s;  }
    else if (br == 1) { q[0] = x / s; q[1] = q4;     q[2] = xy / s; q[3] = xz / s; }
    else if (br == 2) { q[0] = y / s; q[1] = xy / s; q[2] = q4;     q[3] = yz / s; }
    else              { q[0] = z / s; q[1] = xz / s; q[2] = yz / s; q[3] = q4;     }
    if (q[0] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double scale = n < 1e-12 ? 2.0 / q[0] : 2.0 * atan2(n, q[0]) / n;
    pose6[0] = (float)(q[1] * scale); pose6[1] = (float)(q[2] * scale); pose6[2] = (float)(q[3] * scale);
    pose6[3] = (float)M[3]; pose6[4] = (float)M[7]; pose6[5] = (float)M[11];
}

// torch.optim.Adam (single tensor, no weight decay, amsgrad off) on the six components of a pose, step number `step` (1-based): moments
// in fp32, bias corrections in fp64; lr_rot for omega, lr_trans for t.  p, m, v are updated in place.
__host__ __device__ inline void pose_adam_step(float p[6], const float g[6], float m[6], float v[6], int32_t step, float lr_rot, float lr_trans, float beta1,
                                               float beta2, float eps) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    const float bc2_sqrt = (float)sqrt(bc2);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float lr = k < 3 ? lr_rot : lr_trans;
        const float step_size = (float)((double)lr / bc1);
        float mk = m[k], vk = v[k];
        mk = fmaf(1.0f - beta1, g[k] - mk, mk);
        vk = fmaf((1.0f - beta2) * g[k], g[k], vk * beta2);
        m[k] = mk; v[k] = vk;
        const float denom = sqrtf(vk) / bc2_sqrt + eps;
        p[k] = p[k] - step_size * (mk / denom);
    }
}

}  // namespace naruto
