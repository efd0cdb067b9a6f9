// gsr_camera_bwd.inc -- the camera pass of the backward (DESIGN.md section 3g), included by gsr_preprocess_bwd.hip inside its namespace:
// dL/d(viewmatrix, projmatrix, campos, bg) of every view of a call.  It runs behind the per-Gaussian backward, on the same stream, over the
// same records; the per-Gaussian kernels are not touched (the fp64 chain is theirs: view_chain<..., CAM = true> exports its intermediates).
//
//   camera_bwd_kernel     grid (blocks, V), 256 threads.  Lane = one (Gaussian, view): the record walk and the fp64 chain, then 27 fp64
//                         terms (12 view, 12 projection, 3 campos); the same lanes also sum final_T * dL/dC over a strided pixel range (3 bg
//                         terms).  Wave sums by __shfl_xor, the four waves through LDS in wave order: one fp64 row per block in the slab.
//   camera_reduce_kernel  one workgroup per view: the view's slab rows in a fixed order, then fp32 [16], [16], [3], [3].
// No atomics anywhere: the result is the same bits on every run.

// the slab row: [0, 12) view[4j + r] at 3j + r (r < 3), [12, 24) proj[4j + k] at 12 + 3j + (0, 1, 2 for k = 0, 1, 3), [24, 27) campos,
// [27, 30) bg, two doubles of padding
#define GSR_CAM_TERMS 30

__device__ __forceinline__ double gsr_wave_sum(double x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);   // butterfly: every lane ends with the same bits
  return x;
}

template <bool USE_SH, bool AA>
__global__ __launch_bounds__(GSR_BLOCK) void camera_bwd_kernel(GsrCamViews cv) {
  const GsrCamView& w = cv.v[blockIdx.y];
  const int i = blockIdx.x * GSR_BLOCK + threadIdx.x;
  double acc[GSR_CAM_TERMS];
#pragma unroll
  for (int k = 0; k < GSR_CAM_TERMS; ++k) acc[k] = 0.0;
  // (see gsr_view_used: the records of an unused Gaussian are zeros, and so would be every term below)
  if (i < cv.P && w.radii[i] > 0 && (!w.used || !w.tracked || *w.tracked == 0u || w.used[i] != 0)) {
    const uint32_t e0 = min(w.offsets[i], w.cap), e1 = min(w.offsets[i + 1], w.cap);
    const PartialSum ps = reduce_partials(w.partials, e0, e1, USE_SH);
    const float3 p = make_float3(cv.means3D[3 * i], cv.means3D[3 * i + 1], cv.means3D[3 * i + 2]);
    if (USE_SH) {   // campos enters only through the view direction p - campos: dL/dcampos = -dL/dp of the SH term
      float dmean_sh[3] = {0.f, 0.f, 0.f};
      sh_backward<true>(cv.sh_degree, cv.M, cv.shs + (size_t)i * cv.M * 3, p, w.campos, w.clamped[i], ps.dr, ps.dg, ps.db, nullptr,
                        dmean_sh);
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[24 + k] = -(double)dmean_sh[k];
    }
    Cov3 c3;
    build_cov3(i, cv.mod, cv.scales, cv.rotations, cv.cov3D, c3);
    float c32[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, o_s = 0.f, caa = 1.f;
    if (AA) {
      build_cov3_f32(i, cv.mod, cv.scales, cv.rotations, cv.cov3D, c32);
      o_s = w.rec[GSR_REC_F4 * (size_t)i + 1].y;
    }
    // a view without a depth gradient adds dL/dz = 0 (x + 0 = x: the plain chain's bits)
    const float gz = w.dL_dz ? reduce_partials_dz(w.dL_dz, e0, e1) : 0.f;
    float gcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gm3[3] = {0.f, 0.f, 0.f}, gm2[2] = {0.f, 0.f};
    ChainTerms ct;
    view_chain<true, AA, true>(w.view, w.proj, w.W, w.H, w.tanfovx, w.tanfovy, p, c3.c, ps, gcov, gm3, gm2, 0.f, 0.f, nullptr, gz,
                               c32, o_s, &caa, &ct);
    const real pj[4] = {(real)p.x, (real)p.y, (real)p.z, 1.0};
    // view matrix: t_r = sum_j view[4j + r] p_j, and T0[j] = J00 view[4j] + J02 view[4j + 2], T1[j] = J11 view[4j + 1] + J12 view[4j + 2]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 3; ++r) acc[3 * j + r] = ct.dt[r] * pj[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      acc[3 * j] += ct.dT0[j] * ct.J00;
      acc[3 * j + 1] += ct.dT1[j] * ct.J11;
      acc[3 * j + 2] += ct.dT0[j] * ct.J02 + ct.dT1[j] * ct.J12;
    }
    // projection matrix: ndc = (hx mw, hy mw), mw = 1 / (hw + 1e-7); h_k = sum_j proj[4j + k] p_j, k = 0, 1, 3 (column 2 is never read)
    const real dh0 = ct.m2x * ct.mw, dh1 = ct.m2y * ct.mw, dh3 = -(ct.m2x * ct.hx + ct.m2y * ct.hy) * ct.mw * ct.mw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[12 + 3 * j] = dh0 * pj[j]; acc[12 + 3 * j + 1] = dh1 * pj[j]; acc[12 + 3 * j + 2] = dh3 * pj[j];
    }
  }
  // background: C_c = ... + final_T bg_c per pixel.  final_T == nullptr: nothing was blended (P = 0), T = 1 everywhere
  if (w.dL_dcolor) {
    const int N = w.H * w.W;
    for (int pix = blockIdx.x * GSR_BLOCK + threadIdx.x; pix < N; pix += gridDim.x * GSR_BLOCK) {
      const real T = w.final_T ? (real)w.final_T[pix] : 1.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[27 + c] += T * (real)w.dL_dcolor[(size_t)c * N + pix];
    }
  }
  __shared__ double s_red[GSR_BLOCK / GSR_WAVE][GSR_CAM_TERMS];
  const int lane = threadIdx.x & (GSR_WAVE - 1), wv = threadIdx.x / GSR_WAVE;
#pragma unroll
  for (int k = 0; k < GSR_CAM_TERMS; ++k) {
    const double s = gsr_wave_sum(acc[k]);
    if (lane == 0) s_red[wv][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < GSR_CAM_TERMS) {
    double s = s_red[0][threadIdx.x];
#pragma unroll
    for (int u = 1; u < GSR_BLOCK / GSR_WAVE; ++u) s += s_red[u][threadIdx.x];   // wave order
    w.slab[(size_t)blockIdx.x * GSR_CAM_ROW + threadIdx.x] = s;
  }
}

// One workgroup per view: thread (g, c) sums column c of rows g, g + 8, g + 16, ... in order, then row group 0 adds the eight partials in
// group order.  The outputs are the caller's layouts: view / proj [16] as stored (column-major 4x4), campos / bg [3].
__global__ __launch_bounds__(GSR_BLOCK) void camera_reduce_kernel(GsrCamViews cv) {
  const GsrCamView& w = cv.v[blockIdx.x];
  constexpr int G = GSR_BLOCK / GSR_CAM_ROW;
  const int c = threadIdx.x % GSR_CAM_ROW, g = threadIdx.x / GSR_CAM_ROW;
  double s = 0.0;
  if (c < GSR_CAM_TERMS) {
    int r = g;
    // eight rows per trip, every load issued before the first addition (the walk is a chain of memory round trips); the additions keep
    // their order, so the sum is the one-row-at-a-time sum
    for (; r + 7 * G < cv.nblk; r += 8 * G) {
      double q[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) q[k] = w.slab[(size_t)(r + k * G) * GSR_CAM_ROW + c];
#pragma unroll
      for (int k = 0; k < 8; ++k) s += q[k];
    }
    for (; r < cv.nblk; r += G) s += w.slab[(size_t)r * GSR_CAM_ROW + c];
  }
  __shared__ double s_sum[G][GSR_CAM_ROW];
  s_sum[g][c] = s;
  __syncthreads();
  if (threadIdx.x < GSR_CAM_ROW) {
    double t = s_sum[0][c];
#pragma unroll
    for (int u = 1; u < G; ++u) t += s_sum[u][c];
    s_sum[0][c] = t;
  }
  __syncthreads();
  const double* tot = s_sum[0];
  const bool err = cv.bwd_error && *cv.bwd_error != 0u;   // the blend backward of this call aborted (GSR_QUEUE_BWD_ERROR): NaN, as dL_dmeans3D
  const int t = threadIdx.x;
  float val = 0.f;
  float* dst = nullptr;
  if (t < 16) {            // view[4j + r]: row 3 (r = 3) is never read by the forward
    const int j = t >> 2, r = t & 3;
    val = r < 3 ? (float)tot[3 * j + r] : 0.f;
    dst = w.out_view ? w.out_view + t : nullptr;
  } else if (t < 32) {     // proj[4j + k]: k = 2 is never read by the forward
    const int k4 = t - 16, j = k4 >> 2, k = k4 & 3;
    val = k == 2 ? 0.f : (float)tot[12 + 3 * j + (k == 3 ? 2 : k)];
    dst = w.out_proj ? w.out_proj + k4 : nullptr;
  } else if (t < 35) {
    val = (float)tot[24 + (t - 32)];
    dst = w.out_campos ? w.out_campos + (t - 32) : nullptr;
  } else if (t < 38) {
    val = (float)tot[27 + (t - 35)];
    dst = w.out_bg ? w.out_bg + (t - 35) : nullptr;
  }
  if (dst) *dst = err ? __builtin_nanf("") : val;
}
