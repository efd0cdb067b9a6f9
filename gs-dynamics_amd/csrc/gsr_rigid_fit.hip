// gsr_rigid_fit.hip -- the rigid alignment of the training loss (gsdyn.rigid_fit.umeyama_fit; the reference's umeyama_algorithm with
// fixed_scale=True, its src/gnn/utils.py:7-40, and the alignment of rigid_loss, src/train.py:32-40), B samples in ONE launch.
//   rigid_fit_kernel : one WAVE per sample.  Pass 1: each lane walks its rows (lane, lane + 64, ...) in ascending order and sums the count
//                      and the masked X and Y in fp64; a fixed xor butterfly combines the lanes (every lane ends with the same bits).
//                      Pass 2: the nine centred moments (Y - mu_y)(X - mu_x)^T the same way.  Then every lane runs the fp64 Jacobi sweep
//                      (gsr_svd3.h) on C = moments / n, applies the rule set below and, pass 3, writes its rows of aligned and residual
//                      from the fp64 R, t; the squared residuals are summed like the moments.
// Rule set: s1 >= s2 >= s3 the singular values of C;
//   n >= 3 and s2 > 3 * 2^-23 * s1 -> R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T, t = mu_y - R mu_x                       code 0
//   otherwise (rank <= 1, n < 3)   -> R = I, t = mu_y - mu_x                                                                code 1
//   n = 0                          -> R = I, t = 0, sse = 0 (no 0 / 0)                                                      code 1
//   a non-finite masked value      -> R, t, aligned, the masked rows of residual and sse are NaN                            code 1
// No atomics, no LDS, no host read; every output is rounded to fp32 once, from fp64.  Built with -ffp-contract=off: every sum above is
// defined one fp64 operation at a time, so the bits do not hang on which products a compiler fuses.
#include "gsr_common.h"
#include "gsr_svd3.h"

namespace gsr_rigid_fit_k {

__device__ __forceinline__ double wave_sum(double v) {      // xor butterfly, strides 32 .. 1: the same sum, bit for bit, in every lane
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(64) void rigid_fit_kernel(int B, int N, const float* __restrict__ X, const float* __restrict__ Y,
                                                       const unsigned char* __restrict__ mask, float* __restrict__ R, float* __restrict__ t,
                                                       float* __restrict__ aligned, float* __restrict__ residual, float* __restrict__ sse,
                                                       int* __restrict__ count, int* __restrict__ code) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const float *Xb = X + (size_t)b * N * 3, *Yb = Y + (size_t)b * N * 3;
  const unsigned char* mb = mask + (size_t)b * N;
  // ---- pass 1: count and means
  double n = 0.0, sx[3] = {0.0, 0.0, 0.0}, sy[3] = {0.0, 0.0, 0.0};
  for (int r = lane; r < N; r += 64) {
    if (!mb[r]) continue;
    n += 1.0;
    for (int j = 0; j < 3; ++j) { sx[j] += (double)Xb[3 * r + j]; sy[j] += (double)Yb[3 * r + j]; }
  }
  n = wave_sum(n);
  for (int j = 0; j < 3; ++j) { sx[j] = wave_sum(sx[j]); sy[j] = wave_sum(sy[j]); }
  const int cnt = (int)n;
  double mux[3] = {0.0, 0.0, 0.0}, muy[3] = {0.0, 0.0, 0.0};
  if (cnt > 0)
    for (int j = 0; j < 3; ++j) { mux[j] = sx[j] / n; muy[j] = sy[j] / n; }
  // ---- pass 2: centred moments C[i][j] = (1 / n) sum (Y - mu_y)_i (X - mu_x)_j
  double A[3][3], V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) { A[i][j] = 0.0; V[i][j] = i == j ? 1.0 : 0.0; }
  if (cnt > 0) {      // (uniform)
    for (int r = lane; r < N; r += 64) {
      if (!mb[r]) continue;
      double dx[3], dy[3];
      for (int j = 0; j < 3; ++j) { dx[j] = (double)Xb[3 * r + j] - mux[j]; dy[j] = (double)Yb[3 * r + j] - muy[j]; }
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] += dy[i] * dx[j];
    }
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) A[i][j] = wave_sum(A[i][j]) / n;
  }
  bool finite = true;
  for (int i = 0; i < 3; ++i) {
    finite = finite && isfinite(mux[i]) && isfinite(muy[i]);
    for (int j = 0; j < 3; ++j) finite = finite && isfinite(A[i][j]);
  }
  // ---- the rule set
  double Rm[3][3], tv[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rm[i][j] = i == j ? 1.0 : 0.0;
  int cd = 1;
  if (!finite) {
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    for (int i = 0; i < 3; ++i) {
      tv[i] = qnan;
      for (int j = 0; j < 3; ++j) Rm[i][j] = qnan;
    }
  } else if (cnt > 0) {
    if (cnt >= 3) {
      gsr_svd3_jacobi(A, V);
      double sg[3];
      for (int j = 0; j < 3; ++j) sg[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
      int o0 = 0, o1 = 1, o2 = 2;                          // descending order of the singular values
      if (sg[o0] < sg[o1]) { const int s = o0; o0 = o1; o1 = s; }
      if (sg[o1] < sg[o2]) { const int s = o1; o1 = o2; o2 = s; }
      if (sg[o0] < sg[o1]) { const int s = o0; o0 = o1; o1 = s; }
      if (sg[o1] > sg[o0] * 3.0 * 1.1920928955078125e-07) {      // rank >= 2 (then s1 > 0 and s2 > 0)
        double u1[3], u2[3], v1[3], v2[3];
        for (int i = 0; i < 3; ++i) { u1[i] = A[i][o0] / sg[o0]; u2[i] = A[i][o1] / sg[o1]; v1[i] = V[i][o0]; v2[i] = V[i][o1]; }
        const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
        const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) Rm[i][j] = u1[i] * v1[j] + u2[i] * v2[j] + u3[i] * v3[j];
        cd = 0;
      }
    }
    for (int i = 0; i < 3; ++i) tv[i] = muy[i] - ((Rm[i][0] * mux[0] + Rm[i][1] * mux[1]) + Rm[i][2] * mux[2]);
  }
  // ---- pass 3: aligned = X R^T + t, residual = Y - aligned on the masked rows, sse
  double ss = 0.0;
  for (int r = lane; r < N; r += 64) {
    const double x0 = (double)Xb[3 * r], x1 = (double)Xb[3 * r + 1], x2 = (double)Xb[3 * r + 2];
    const bool m = mb[r] != 0;
    for (int j = 0; j < 3; ++j) {
      const double a = ((x0 * Rm[j][0] + x1 * Rm[j][1]) + x2 * Rm[j][2]) + tv[j];
      const double d = m ? (double)Yb[3 * r + j] - a : 0.0;
      aligned[((size_t)b * N + r) * 3 + j] = (float)a;
      residual[((size_t)b * N + r) * 3 + j] = (float)d;
      ss += d * d;
    }
  }
  ss = wave_sum(ss);
  if (lane == 0) {      // (static indices only: Rm and tv stay in registers)
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) R[(size_t)b * 9 + 3 * i + j] = (float)Rm[i][j];
      t[(size_t)b * 3 + i] = (float)tv[i];
    }
    sse[b] = (float)ss; count[b] = cnt; code[b] = cd;
  }
}

}  // namespace gsr_rigid_fit_k
using namespace gsr_rigid_fit_k;

int gsr_rigid_fit(int32_t B, int32_t N, const float* X, const float* Y, const uint8_t* mask, float* R, float* t, float* aligned,
                  float* residual, float* sse, int32_t* count, int32_t* code, void* stream) {
  GsrRange _range("gsr_rigid_fit");
  if (B < 1 || N < 1) {
    gsr_set_error("gsr_rigid_fit: bad argument (B, N >= 1; got B = %d, N = %d)", (int)B, (int)N);
    return -2;
  }
  if (!X || !Y || !mask || !R || !t || !aligned || !residual || !sse || !count || !code) {
    gsr_set_error("gsr_rigid_fit: NULL pointer");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  { GSR_PROF("rigid_fit", st);
    hipLaunchKernelGGL(rigid_fit_kernel, dim3(B), dim3(64), 0, st, (int)B, (int)N, X, Y, (const unsigned char*)mask, R, t, aligned, residual,
                       sse, count, code); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}
