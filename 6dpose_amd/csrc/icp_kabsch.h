// TransformationEstimationPointToPoint::ComputeTransformation = Eigen::umeyama(source, target, with_scaling = false) from the sums of
// an evaluation: the rotation that minimises sum |R (p - pm) - (q - qm)|^2 and t = qm - R pm.
// The rotation is found as Horn's unit quaternion: the eigenvector of the largest eigenvalue of the symmetric 4x4 matrix built from
// H = sum q p^T - n qm pm^T, by cyclic Jacobi in f64.  It equals U diag(1, 1, det(U) det(V)) V^T of H = U D V^T wherever that is
// unique, and is a proper rotation by construction (no determinant fix).  One thread runs it in the prologue of k_icp_eval<true>; like
// the 6x6 solve of the team kernel it is NOT inlined: inside the prologue its 32 live doubles would be added to the
// register budget of the whole kernel.  Plain C++ (no intrinsics), so that a host program can call the same text.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define LM_KABSCH_FN static __device__ __noinline__
#else
#define LM_KABSCH_FN static inline
#endif

namespace lm {

// One Jacobi rotation of the symmetric A (and of the eigenvector matrix V) that annihilates A[P][Q]; P < Q are compile-time, so every
// index below is a constant and the matrices stay in registers.
template <int P, int Q>
static inline
#ifdef __HIPCC__
__device__ __attribute__((always_inline))
#endif
void jacobi_rotate4(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    // t = tan of the rotation angle, the smaller root: one square root and one division; c = 1 / sqrt(1 + t^2)
    const double diff = A[Q][Q] - A[P][P];
    const double t = 2.0 * apq / (diff + (diff >= 0.0 ? 1.0 : -1.0) * sqrt(diff * diff + 4.0 * apq * apq));
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = 0.0; A[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != P && k != Q) {
            const double akp = A[k][P], akq = A[k][Q];
            A[k][P] = c * akp - s * akq; A[P][k] = A[k][P];
            A[k][Q] = s * akp + c * akq; A[Q][k] = A[k][Q];
        }
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// sums: [0..2] sum p, [3..5] sum q, [6..14] sum q p^T (row-major: 6 + 3 a + b = sum q_a p_b), n correspondences.
// U: the update [R | t] (3 x 4 row-major).  Returns false (U untouched) when n < 3 or an entry of the result is not finite.
LM_KABSCH_FN bool kabsch_update(const double* sums, const int n, double* U) {
    if (n < 3) return false;
    const double inv_n = 1.0 / (double)n;
    double pm[3], qm[3], S[3][3];                                   // S[a][b] = sum (p - pm)_a (q - qm)_b = H[b][a]
#pragma unroll
    for (int a = 0; a < 3; ++a) { pm[a] = sums[a] * inv_n; qm[a] = sums[3 + a] * inv_n; }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) S[a][b] = sums[6 + 3 * b + a] - (double)n * qm[b] * pm[a];
    double A[4][4], V[4][4];
    A[0][0] = S[0][0] + S[1][1] + S[2][2];
    A[1][1] = S[0][0] - S[1][1] - S[2][2];
    A[2][2] = -S[0][0] + S[1][1] - S[2][2];
    A[3][3] = -S[0][0] - S[1][1] + S[2][2];
    A[0][1] = A[1][0] = S[1][2] - S[2][1];
    A[0][2] = A[2][0] = S[2][0] - S[0][2];
    A[0][3] = A[3][0] = S[0][1] - S[1][0];
    A[1][2] = A[2][1] = S[0][1] + S[1][0];
    A[1][3] = A[3][1] = S[2][0] + S[0][2];
    A[2][3] = A[3][2] = S[1][2] + S[2][1];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) V[a][b] = a == b ? 1.0 : 0.0;
    // cyclic sweeps until the off-diagonal part is below rounding (quadratic convergence: four to six sweeps); 16 bounds the loop
    for (int sweep = 0; sweep < 16; ++sweep) {
        const double off = (A[0][1] * A[0][1] + A[0][2] * A[0][2]) + (A[0][3] * A[0][3] + A[1][2] * A[1][2]) + (A[1][3] * A[1][3] + A[2][3] * A[2][3]);
        const double dia = (A[0][0] * A[0][0] + A[1][1] * A[1][1]) + (A[2][2] * A[2][2] + A[3][3] * A[3][3]);
        if (!(off > 1e-34 * dia)) break;                            // (also leaves on NaN)
        jacobi_rotate4<0, 1>(A, V); jacobi_rotate4<0, 2>(A, V); jacobi_rotate4<0, 3>(A, V);
        jacobi_rotate4<1, 2>(A, V); jacobi_rotate4<1, 3>(A, V); jacobi_rotate4<2, 3>(A, V);
    }
    // the column of the largest eigenvalue (the first one on a tie), selected without dynamic indexing
    double best = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > best) { best = A[k][k]; w = V[0][k]; x = V[1][k]; y = V[2][k]; z = V[3][k]; }
    const double nrm = 1.0 / sqrt((w * w + x * x) + (y * y + z * z));
    w *= nrm; x *= nrm; y *= nrm; z *= nrm;
    double R[9];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
    double t[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        t[a] = qm[a] - (R[3 * a] * pm[0] + R[3 * a + 1] * pm[1] + R[3 * a + 2] * pm[2]);
        ok = ok && isfinite(t[a]) && isfinite(R[3 * a]) && isfinite(R[3 * a + 1]) && isfinite(R[3 * a + 2]);
    }
    if (!ok) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) { U[4 * a] = R[3 * a]; U[4 * a + 1] = R[3 * a + 1]; U[4 * a + 2] = R[3 * a + 2]; U[4 * a + 3] = t[a]; }
    return true;
}

}  // namespace lm
