// gsr_sh_views.hip -- the SH pass behind the multi-view per-Gaussian backward.  Built with contraction off, like
// gsr_preprocess_bwd.hip: both take the basis and the view-direction gradient from sh_basis_dmean (gsr_sh.h).
//
// gsr_backward_batch_ex, given dL_dcolors_views after an SH batch forward, leaves every view's dL/d(rgb) [P,3] (zeros where the view
// did not see the Gaussian).  This kernel turns them into dL/dsh [P,M,3] summed over the views and adds the view-direction term to
// dL/dmeans3D: sh_basis_dmean per view in fp32, every view in one pass, the sum in ascending view order in registers.  No atomics.
//
// Layout: a Gaussian's row is 12 M bytes, so one lane per Gaussian straight from HBM is a 192-byte-stride pattern (M = 16).  Here ONE
// WAVE owns 64 consecutive Gaussians, whose rows are one contiguous, 16-byte-aligned run of 768 M bytes:
//   1. the run goes HBM -> LDS with consecutive lanes on consecutive addresses (16-byte loads, a scalar tail);
//   2. each lane works on its own LDS row; the row stride is 3 M made odd (48 -> 49 floats: lanes l and l + k never share a bank),
//      the accumulators (3 M floats) and the dmean sums stay in registers across the wave-uniform view loop;
//   3. the accumulators go back through the same tile and out with coalesced stores.
// The workgroup IS the wave (64 threads): the tile is wave-private, the two barriers are wave-wide waits on LDS and nothing else, and
// at 12.25 KiB of LDS a CU holds 12 such waves -- more than P = 100 k spreads over 256 CUs (6.1 per CU).
// HBM per Gaussian: reads 12 M + 12 + V (12 + 4 + 4) + 12 (the dmeans3D read-modify-write), writes 12 M + 12.

// (the table, GsrShViews: gsr_common.h)
#include "gsr_common.h"
#include "gsr_sh.h"

namespace gsr_sh_views {

#define GSR_SH_TILE 64          // Gaussians per wave
// MC = the coefficient count when it is one of 1 / 4 / 9 / 16 (the coalesced phases then divide by a constant), 0 = any M in 1..16.
template <int MC>
__global__ void __launch_bounds__(GSR_SH_TILE) sh_bwd_views_kernel(const GsrShViews t) {
  constexpr int RS_MAX = MC ? ((3 * MC) | 1) : 49;
  __shared__ float tile[GSR_SH_TILE * RS_MAX];
  const int M = MC ? MC : t.M;
  const int M3 = 3 * M, RS = M3 | 1;            // LDS row stride: 3 M made odd
  const int P = t.P, lane = (int)threadIdx.x;
  const int g0 = (int)blockIdx.x * GSR_SH_TILE;
  const int rows = min(GSR_SH_TILE, P - g0);
  const int n = rows * M3;                      // floats of this tile's run: element e is valid when e < n
  const size_t base = (size_t)g0 * (size_t)M3;
  const float* __restrict__ src = t.shs + base;
  float* __restrict__ dst = t.dL_dsh + base;
  // 1. the coefficient rows: HBM -> LDS, consecutive lanes on consecutive addresses
  if (t.vec4) {
    for (int e = 4 * lane; e < n; e += 4 * GSR_SH_TILE) {
      if (e + 3 < n) {
        const float4 q = *reinterpret_cast<const float4*>(src + e);
        const float qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int r = (e + j) / M3; tile[r * RS + (e + j - r * M3)] = qv[j]; }
      } else {
        for (int j = 0; j < 4; ++j)
          if (e + j < n) { const int r = (e + j) / M3; tile[r * RS + (e + j - r * M3)] = src[e + j]; }
      }
    }
  } else {
    for (int e = lane; e < n; e += GSR_SH_TILE) { const int r = e / M3; tile[r * RS + (e - r * M3)] = src[e]; }
  }
  __syncthreads();
  // 2. one lane per Gaussian, its row in LDS; the view loop is wave-uniform (the table is a kernel argument: scalar loads)
  const int i = g0 + lane;
  const bool live = i < P;
  const int deg = t.deg, ncoef = (deg + 1) * (deg + 1);
  float acc[16][3];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.f;
  float dm[3] = {0.f, 0.f, 0.f};
  const float* row = tile + lane * RS;
  float3 p = make_float3(0.f, 0.f, 0.f);
  if (live) p = make_float3(t.means3D[3 * (size_t)i], t.means3D[3 * (size_t)i + 1], t.means3D[3 * (size_t)i + 2]);
  for (int v = 0; v < t.V; ++v) {
    const GsrShView& w = t.v[v];
    if (!live || w.radii[i] <= 0) continue;       // not seen by this view: no term (and no 1 / |p - campos|)
    const uint32_t cl = w.clamped[i];
    const float g0c = w.dcol[3 * (size_t)i], g1c = w.dcol[3 * (size_t)i + 1], g2c = w.dcol[3 * (size_t)i + 2];
    const float dL[3] = {(cl & 1u) ? 0.f : g0c, (cl & 2u) ? 0.f : g1c, (cl & 4u) ? 0.f : g2c};
    float basis[16], dmean[3];
    sh_basis_dmean(deg, row, p, w.campos, dL, basis, dmean);
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < ncoef) { acc[k][0] += basis[k] * dL[0]; acc[k][1] += basis[k] * dL[1]; acc[k][2] += basis[k] * dL[2]; }
    dm[0] += dmean[0]; dm[1] += dmean[1]; dm[2] += dmean[2];
  }
  if (live) {   // read-modify-write of what the per-Gaussian kernel left (a NaN stays a NaN)
    float* o = t.dL_dmeans3D + 3 * (size_t)i;
    o[0] += dm[0]; o[1] += dm[1]; o[2] += dm[2];
  }
  __syncthreads();      // every lane is through with the coefficients: the tile now takes the sums
  // 3. every coefficient of the row is written (zeros beyond the degree's, zeros for a Gaussian no view saw), then LDS -> HBM coalesced
  {
    float* wrow = tile + lane * RS;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < M) { wrow[3 * k] = acc[k][0]; wrow[3 * k + 1] = acc[k][1]; wrow[3 * k + 2] = acc[k][2]; }
  }
  __syncthreads();
  if (t.vec4) {
    for (int e = 4 * lane; e < n; e += 4 * GSR_SH_TILE) {
      if (e + 3 < n) {
        float qv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int r = (e + j) / M3; qv[j] = tile[r * RS + (e + j - r * M3)]; }
        *reinterpret_cast<float4*>(dst + e) = make_float4(qv[0], qv[1], qv[2], qv[3]);
      } else {
        for (int j = 0; j < 4; ++j)
          if (e + j < n) { const int r = (e + j) / M3; dst[e + j] = tile[r * RS + (e + j - r * M3)]; }
      }
    }
  } else {
    for (int e = lane; e < n; e += GSR_SH_TILE) { const int r = e / M3; dst[e] = tile[r * RS + (e - r * M3)]; }
  }
}

}  // namespace gsr_sh_views
using namespace gsr_sh_views;

int gsr_launch_sh_bwd_views(const GsrShViews& t, hipStream_t st) {
  if (t.P <= 0 || t.V <= 0) return 0;
  {
    GSR_PROF("sh_bwd_views", st);
    const dim3 grid((t.P + GSR_SH_TILE - 1) / GSR_SH_TILE), block(GSR_SH_TILE);
    switch (t.M) {
      case 1: hipLaunchKernelGGL(sh_bwd_views_kernel<1>, grid, block, 0, st, t); break;
      case 4: hipLaunchKernelGGL(sh_bwd_views_kernel<4>, grid, block, 0, st, t); break;
      case 9: hipLaunchKernelGGL(sh_bwd_views_kernel<9>, grid, block, 0, st, t); break;
      case 16: hipLaunchKernelGGL(sh_bwd_views_kernel<16>, grid, block, 0, st, t); break;
      default: hipLaunchKernelGGL(sh_bwd_views_kernel<0>, grid, block, 0, st, t); break;
    }
  }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}
