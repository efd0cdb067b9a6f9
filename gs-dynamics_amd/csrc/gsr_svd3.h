// gsr_svd3.h -- the 3x3 one-sided Jacobi sweep in fp64, the ONE definition shared by its callers: fit_one_rotation (gsr_dynamics.hip, the
// bones' rotation fit of the rollout) and rigid_fit_kernel (gsr_rigid_fit.hip, the Umeyama fit of the training loss).  Each caller keeps
// its own decision tree on top of the factors.
#pragma once
#include <hip/hip_runtime.h>

// A V0 = U S: rotate column pairs of A (and of V, which the caller hands in as the identity) until A's columns are orthogonal.  On return
// A's columns are the left singular vectors times their singular values (in no particular order) and V's columns the right singular
// vectors.  The loop has a hard bound of 40 sweeps whatever the data: a NaN cannot keep it going (fmax drops it, `off` stays 0 and the
// first sweep is the last), and if it did the bound would end it -- nothing here can spin.
__device__ __forceinline__ void gsr_svd3_jacobi(double A[3][3], double V[3][3]) {
  for (int sweep = 0; sweep < 40; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
        for (int i = 0; i < 3; ++i) { al += A[i][p] * A[i][p]; be += A[i][q] * A[i][q]; ga += A[i][p] * A[i][q]; }
        if (ga == 0.0 || fabs(ga) <= 1e-17 * sqrt(al * be)) continue;
        off = fmax(off, fabs(ga) / sqrt(al * be));
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < 3; ++i) {
          const double ap = A[i][p], aq = A[i][q];
          A[i][p] = c * ap - s * aq; A[i][q] = s * ap + c * aq;
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq;
        }
      }
    if (off < 1e-15) break;
  }
}
