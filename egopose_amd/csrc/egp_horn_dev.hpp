// The best proper rotation between two centred point sets, for K10 (egp_pose3d.hip): Horn's closed form (B. K. P. Horn, "Closed-form
// solution of absolute orientation using unit quaternions", JOSA A 4(4), 1987). With the cross-covariance S = sum x y^T the unit
// quaternion q that maximises sum y . R(q) x is the eigenvector of the largest eigenvalue of the symmetric 4x4 matrix N(S) below;
// that eigenvalue IS the maximum, so the least-squares scale is lambda_max / sum |x|^2. A quaternion only ever gives a proper
// rotation: a mirrored set is never matched by a reflection, with no determinant test anywhere.
// The eigenvector comes from cyclic Jacobi sweeps, a FIXED number of them (no data-dependent loop: every wave runs the same
// instructions), every matrix entry addressed at compile-time indices so that both 4x4 arrays live in registers.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

namespace egp_horn {

constexpr int SWEEPS = 8;        // 5 sweeps agree with the determinant-corrected SVD to 1e-15 on humanoid pairs; convergence is quadratic

// One Jacobi rotation in the (P, Q) plane: A <- J^T A J with A[P][Q] -> 0, V <- V J. An entry that is already zero is left alone.
template <int P, int Q>
__host__ __device__ __forceinline__ void rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));      // |theta| = inf gives 0
    t = apq == 0.0 ? 0.0 : t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// S[3 a + b] = sum x_a y_b over the centred sets -> R (row major) with y ~ s R x; returns lambda_max = sum y . R x.
__host__ __device__ __forceinline__ double best_rotation(const double *S, double *R) {
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
#pragma unroll
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        rotate<0, 1>(A, V); rotate<0, 2>(A, V); rotate<0, 3>(A, V);
        rotate<1, 2>(A, V); rotate<1, 3>(A, V); rotate<2, 3>(A, V);
    }
    double lam = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const bool up = A[k][k] > lam;
        lam = up ? A[k][k] : lam;
        w = up ? V[0][k] : w; x = up ? V[1][k] : x; y = up ? V[2][k] : y; z = up ? V[3][k] : z;
    }
    const double inv = 1.0 / sqrt(w * w + x * x + y * y + z * z);      // V is orthogonal to rounding; this takes the rounding out of R
    w *= inv; x *= inv; y *= inv; z *= inv;
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
    return lam;
}

}  // namespace egp_horn
