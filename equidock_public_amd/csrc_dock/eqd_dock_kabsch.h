// Device code shared by the batched RMSD meter (eqd_dock_meter.hip) and the docking-quality kernels
// (eqd_dock_quality.hip): the fixed-order workgroup sum of doubles and the Kabsch solve of one weighted row set from its
// moments (3 x 3 one-sided Jacobi SVD, the proper rotation that stays defined for rank-1 and rank-2 sets).
#ifndef EQD_DOCK_KABSCH_H
#define EQD_DOCK_KABSCH_H

#include "../csrc/eqd_common.h"

#include <math.h>

#define DM_NRB 12           // R [9] and b [3] of one (complex, set)

__device__ __forceinline__ double dm_shfl_xor_d(double v, int m) {
    long long b = __builtin_bit_cast(long long, v);
    int lo = (int)(b & 0xffffffffll), hi = (int)(b >> 32);
    lo = __shfl_xor(lo, m);
    hi = __shfl_xor(hi, m);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned long long)(unsigned)lo);
}
// sum over the workgroup in a fixed order (butterfly inside a wave, then the four waves); every thread must call it
__device__ __forceinline__ double dm_block_sum(double v, double* red) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += dm_shfl_xor_d(v, m);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// A = U S V^T by one-sided Jacobi on the columns of A (A V = U S); on return the columns of A are s_k u_k and V is
// orthogonal.  Single thread, fixed pair order.
__device__ __forceinline__ void dm_jacobi(double A[3][3], double V[3][3]) {
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) V[a][b] = a == b ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int k = 0; k < 3; ++k) {
                    al += A[k][p] * A[k][p];
                    be += A[k][q] * A[k][q];
                    ga += A[k][p] * A[k][q];
                }
                if (ga == 0.0 || fabs(ga) <= 2.3e-16 * sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int k = 0; k < 3; ++k) {
                    const double ap = A[k][p], aq = A[k][q];
                    A[k][p] = cs * ap - sn * aq;
                    A[k][q] = sn * ap + cs * aq;
                    const double vp = V[k][p], vq = V[k][q];
                    V[k][p] = cs * vp - sn * vq;
                    V[k][q] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
}

__device__ __forceinline__ void dm_cross(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// One weighted row set from its moments m = (sum w, sum w p [3], sum w t [3], sum w p t^T [9]): R [9] and b [3] of the
// superposition of p onto t into rb; returns whether the reference's reflection branch det(V U^T) < 0 was taken.  An
// empty set gives the identity and b = 0.
__device__ __forceinline__ bool dm_kabsch(const double m[16], double* __restrict__ rb) {
    double R[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    double cp[3] = {0.0, 0.0, 0.0}, ct[3] = {0.0, 0.0, 0.0};
    bool reflect = false;
    const double sw = m[0];
    if (sw > 0.0) {
        double H[3][3], V[3][3];
        for (int a = 0; a < 3; ++a) {
            cp[a] = m[1 + a] / sw;
            ct[a] = m[4 + a] / sw;
        }
        // H = sum w (p - c_P)(t - c_T)^T = sum w p t^T - (sum w p) c_T^T
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) H[a][b] = m[7 + 3 * a + b] - m[1 + a] * ct[b];
        const double det = H[0][0] * (H[1][1] * H[2][2] - H[1][2] * H[2][1]) - H[0][1] * (H[1][0] * H[2][2] - H[1][2] * H[2][0]) +
                           H[0][2] * (H[1][0] * H[2][1] - H[1][1] * H[2][0]);
        // det(V U^T) = sign(det H) for any SVD of a full-rank H: the reference's reflection branch
        reflect = det < 0.0;
        dm_jacobi(H, V);
        double s2[3];
        int ord[3] = {0, 1, 2};
        for (int k = 0; k < 3; ++k) s2[k] = (H[0][k] * H[0][k] + H[1][k] * H[1][k]) + H[2][k] * H[2][k];
        for (int a = 0; a < 2; ++a)                        // descending singular values
            for (int b = 0; b < 2 - a; ++b)
                if (s2[ord[b]] < s2[ord[b + 1]]) {
                    const int tmp = ord[b];
                    ord[b] = ord[b + 1];
                    ord[b + 1] = tmp;
                }
        const double s1 = sqrt(s2[ord[0]]);
        if (s1 > 0.0) {
            double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
            for (int k = 0; k < 3; ++k) {
                u1[k] = H[k][ord[0]] / s1;
                v1[k] = V[k][ord[0]];
                v2[k] = V[k][ord[1]];
            }
            // u2: the second column, orthogonal to u1; without one (rank 1) any unit vector orthogonal to u1 is optimal
            const double dot = (H[0][ord[1]] * u1[0] + H[1][ord[1]] * u1[1]) + H[2][ord[1]] * u1[2];
            for (int k = 0; k < 3; ++k) u2[k] = H[k][ord[1]] - dot * u1[k];
            double n2 = sqrt((u2[0] * u2[0] + u2[1] * u2[1]) + u2[2] * u2[2]);
            if (!(n2 > 1e-14 * s1)) {
                const int small = fabs(u1[0]) <= fabs(u1[1]) ? (fabs(u1[0]) <= fabs(u1[2]) ? 0 : 2) : (fabs(u1[1]) <= fabs(u1[2]) ? 1 : 2);
                double e[3] = {0.0, 0.0, 0.0};
                e[small] = 1.0;
                dm_cross(u1, e, u2);
                n2 = sqrt((u2[0] * u2[0] + u2[1] * u2[1]) + u2[2] * u2[2]);
            }
            for (int k = 0; k < 3; ++k) u2[k] /= n2;
            // the proper rotation with R u1 = v1, R u2 = v2: R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T, which is
            // V U^T when det(V U^T) > 0 and V diag(1, 1, -1) U^T otherwise
            dm_cross(u1, u2, u3);
            dm_cross(v1, v2, v3);
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) R[a][b] = (v1[a] * u1[b] + v2[a] * u2[b]) + v3[a] * u3[b];
        }
    }
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) rb[3 * a + b] = R[a][b];
        rb[9 + a] = ct[a] - ((R[a][0] * cp[0] + R[a][1] * cp[1]) + R[a][2] * cp[2]);
    }
    return reflect;
}

#endif
