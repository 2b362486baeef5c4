// quadric_solve.h -- the fixed 3x3 cyclic Jacobi and the rank-limited quadric minimiser that mesh_simplify.hip (place_kernel) and
// mesh_decimate.hip (candidate_kernel) share: one body, so both round alike (contract in include/tdgp.h, tdgp_mesh_cluster_place).
// Everything is double, sequential, every operation rounded once (-ffp-contract=off), and inlined into its caller.
#pragma once
#include "common.h"

// One rotation of the cyclic Jacobi method on the symmetric a, pair (p, q), r the third index; the eigenvectors accumulate in the columns of u.
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&u)[3][3], int p, int q, int r) {
    const double apq = a[p][q];
    if (apq == 0.0) return;
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    const double den = fabs(theta) + sqrt(theta * theta + 1.0);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / den;          // Rutishauser: the smaller root of t^2 + 2 t theta - 1 = 0
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    a[p][p] = a[p][p] - t * apq;
    a[q][q] = a[q][q] + t * apq;
    a[p][q] = 0.0;
    a[q][p] = 0.0;
    const double arp = a[r][p], arq = a[r][q];
    a[r][p] = c * arp - s * arq;
    a[p][r] = a[r][p];
    a[r][q] = s * arp + c * arq;
    a[q][r] = a[r][q];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double ukp = u[k][p], ukq = u[k][q];
        u[k][p] = c * ukp - s * ukq;
        u[k][q] = s * ukp + c * ukq;
    }
}

// The minimiser of x^T A x + 2 b^T x started from m, restricted to the eigen-directions of the symmetric A whose eigenvalue exceeds
// rank_tol times the largest: r = -b - A m;  8 sweeps over the pairs (0,1), (0,2), (1,2);  x = m + sum_i u_i (u_i . r) / l_i.
__device__ __forceinline__ void quadric_minimise(const double (&A)[3][3], const double (&bv)[3], const double (&m)[3], double rank_tol, double (&x)[3]) {
    double r[3];
#pragma unroll
    for (int c = 0; c < 3; c++) r[c] = -bv[c] - ((A[c][0] * m[0] + A[c][1] * m[1]) + A[c][2] * m[2]);
    double a[3][3], u[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) a[i][j] = A[i][j];
    for (int sweep = 0; sweep < 8; sweep++) {
        jacobi_rotate(a, u, 0, 1, 2);
        jacobi_rotate(a, u, 0, 2, 1);
        jacobi_rotate(a, u, 1, 2, 0);
    }
    double lmax = a[0][0];
    lmax = a[1][1] > lmax ? a[1][1] : lmax;
    lmax = a[2][2] > lmax ? a[2][2] : lmax;
    const double floor_l = rank_tol * lmax;
#pragma unroll
    for (int c = 0; c < 3; c++) x[c] = m[c];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double l = a[i][i];
        if (l > floor_l) {
            const double coef = ((u[0][i] * r[0] + u[1][i] * r[1]) + u[2][i] * r[2]) / l;
#pragma unroll
            for (int c = 0; c < 3; c++) x[c] = x[c] + u[c][i] * coef;
        }
    }
}
