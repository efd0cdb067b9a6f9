// gsr_fps_thin.h -- farthest point sampling of a SMALL cloud (N <= 1024) followed by the radius thinning of the picks, as the body of ONE
// workgroup of FT_THREADS threads.  Device code only.  Users: fps_thin_small_kernel (gsr_dynamics.hip: one cloud per launch, the lists go to
// global memory) and dyn_sample_kernel (gsr_dyn_batch.hip: one cloud per workgroup, the lists stay in LDS).  One body, so both take the same
// picks: squared distances (dx*dx + dy*dy) + dz*dz for the sampling, sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) for the thinning (torch.norm's
// evaluation on the host), first maximum on ties.
#pragma once
#ifdef __HIPCC__
#include "gsr_common.h"

// Arg-max with "first maximum" over a workgroup of FT_THREADS threads whose thread t owns the CONSECUTIVE items 4 t .. 4 t + 3
// (so a lower lane holds lower indices).  (best, besti) = the thread's own candidate (best >= 0, or -1 with besti = INT_MAX when
// it has none).  Wave level: the maximum by DPP (values are non-negative: the zeros a masked DPP step reads are neutral), then the
// first lane holding it (ballot + ffs) -- no LDS crossbar trip; workgroup level: one LDS word pair per wave and ONE barrier (two
// buffers, alternated by the caller), every thread reduces the FT_THREADS / 64 candidates itself.
#define FT_THREADS 256
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float ft_dpp_max(float v) {
  return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false)));
}
__device__ __forceinline__ void block_argmax_first(float& best, int& besti, float* s_val, int* s_idx, int tid) {
  const int lane = tid & 63, wv = tid >> 6;
  float m = fmaxf(best, 0.0f);
  m = ft_dpp_max<0xB1>(m); m = ft_dpp_max<0x4E>(m); m = ft_dpp_max<0x141>(m); m = ft_dpp_max<0x140>(m);
  m = ft_dpp_max<0x142, 0xA>(m); m = ft_dpp_max<0x143, 0xC>(m);
  const float wmax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(m), 63));
  const uint64_t who = __ballot(best == wmax && best >= 0.0f);
  float cv = -1.0f;
  int ci = 0x7fffffff;
  if (who) { cv = wmax; ci = __shfl(besti, __ffsll((long long)who) - 1, 64); }
  if (lane == 0) { s_val[wv] = cv; s_idx[wv] = ci; }
  __syncthreads();
  best = s_val[0]; besti = s_idx[0];
#pragma unroll
  for (int w = 1; w < FT_THREADS / 64; ++w) {
    const float v = s_val[w]; const int i = s_idx[w];
    if (v > best || (v == best && i < besti)) { best = v; besti = i; }
  }
}

// The body.  pos [N, 3] (global); sa [3 * 1024] and sp [3 * npoints] floats, s_val / s_idx [2][FT_THREADS / 64]: LDS of the caller.
// out_idx [npoints] = the picks, thin_idx [0 .. kept) = the positions IN out_idx of the kept picks (global or LDS, any integer type);
// returns kept (the same in every thread).  Ends behind a barrier-free tail: the caller synchronises before it reads the lists.
template <typename I>
__device__ __forceinline__ int gsr_fps_thin_block(const float* __restrict__ pos, int N, int npoints, int start, float radius, int thin_start,
                                                  I* out_idx, I* thin_idx, float* sa, float* sp, float (*s_val)[FT_THREADS / 64],
                                                  int (*s_idx)[FT_THREADS / 64], int tid) {
  float px[4], py[4], pz[4], mind[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = 4 * tid + q;
    const bool have = i < N;
    px[q] = have ? pos[3 * i] : 0.f; py[q] = have ? pos[3 * i + 1] : 0.f; pz[q] = have ? pos[3 * i + 2] : 0.f;
    sa[3 * i] = px[q]; sa[3 * i + 1] = py[q]; sa[3 * i + 2] = pz[q];
    mind[q] = __builtin_inff();
  }
  __syncthreads();
  int cur = start;
  for (int k = 0; k < npoints; ++k) {
    const float cx = sa[3 * cur], cy = sa[3 * cur + 1], cz = sa[3 * cur + 2];
    if (tid == 0) { out_idx[k] = cur; sp[3 * k] = cx; sp[3 * k + 1] = cy; sp[3 * k + 2] = cz; }
    float best = -1.0f;
    int besti = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * tid + q;
      if (i < N) {
        const float dx = px[q] - cx, dy = py[q] - cy, dz = pz[q] - cz;
        const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
        mind[q] = fminf(mind[q], d);
        if (mind[q] > best) { best = mind[q]; besti = i; }      // ascending i: the thread's first maximum
      }
    }
    block_argmax_first(best, besti, s_val[k & 1], s_idx[k & 1], tid);     // (two LDS buffers: one barrier per pick)
    cur = besti;
  }
  __syncthreads();                         // sp[] complete
  // ---- thinning over the npoints picks: thread t owns picks 4 t .. 4 t + 3
  float qx[4], qy[4], qz[4], dist[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = 4 * tid + q;
    const bool mine = i < npoints;
    qx[q] = mine ? sp[3 * i] : 0.f; qy[q] = mine ? sp[3 * i + 1] : 0.f; qz[q] = mine ? sp[3 * i + 2] : 0.f;
    dist[q] = __builtin_inff();
  }
  int kept = 0, nxt = thin_start;
  for (int it = 0; it < npoints; ++it) {
    if (tid == 0) thin_idx[kept] = nxt;
    ++kept;
    const float nx = sp[3 * nxt], ny = sp[3 * nxt + 1], nz = sp[3 * nxt + 2];
    float best = -1.0f;
    int besti = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * tid + q;
      if (i < npoints) {
        const float dx = qx[q] - nx, dy = qy[q] - ny, dz = qz[q] - nz;
        dist[q] = fminf(dist[q], __fsqrt_rn(__fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx)))));
        if (dist[q] > best) { best = dist[q]; besti = i; }
      }
    }
    block_argmax_first(best, besti, s_val[it & 1], s_idx[it & 1], tid);
    if (!(best > radius)) break;           // uniform: every thread reduced the same candidates
    nxt = besti;
  }
  return kept;
}

#endif  // __HIPCC__
