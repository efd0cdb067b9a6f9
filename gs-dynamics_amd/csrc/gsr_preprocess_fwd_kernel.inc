// gsr_preprocess_fwd_kernel.inc -- the preprocess kernel, included twice by gsr_preprocess_fwd.hip (inside its namespace):
//   GSR_PFWD_AA 0: preprocess_fwd_kernel      (every forward entry point)
//   GSR_PFWD_AA 1: preprocess_fwd_aa_kernel   (GSR_SETTINGS_ANTIALIASING: the staged opacity is o * c; DESIGN.md section 3f)
// A compile-time switch: the GSR_PFWD_AA 0 kernel is the code it was before the anti-aliasing build existed.
#if GSR_PFWD_AA
#define GSR_PFWD_NAME(k) k##_aa_kernel
#else
#define GSR_PFWD_NAME(k) k##_kernel
#endif

__global__ __launch_bounds__(GSR_BLOCK) void GSR_PFWD_NAME(preprocess_fwd)(
    GsrPreViews tab, int P, int W, int H, int gx, int gy, float mod, int sh_degree, int M,
    const float* __restrict__ means3D, const float* __restrict__ scales, const float* __restrict__ rotations,
    const float* __restrict__ opacities, const float* __restrict__ colors_precomp,
    const float* __restrict__ shs, const float* __restrict__ cov3D_precomp, int tight_lists) {
  // this block's view (blockIdx.y): its pointers come out of the kernarg table with scalar loads
  const GsrPreView& vw = tab.v[blockIdx.y];
  if (vw.skip) return;
  if (vw.colors) colors_precomp = vw.colors;
  uint32_t* __restrict__ block_sums = vw.block_sums;
  __shared__ uint32_t s_wave_sum[GSR_BLOCK / GSR_WAVE];
  const int i = blockIdx.x * GSR_BLOCK + threadIdx.x;
  __shared__ float4 s_rec[GSR_BLOCK / GSR_WAVE][256];      // a wave's 64 records on their way to memory (see preprocess_gaussian)
  const PreOut po = preprocess_gaussian<GSR_PFWD_AA>(tab, vw, i, P, s_rec[threadIdx.x >> 6], blockIdx.y == 0, W, H, gx, gy, mod, sh_degree, M, means3D, scales, rotations,
                                        opacities, colors_precomp, shs, cov3D_precomp, tight_lists);
  const uint32_t tiles = po.tiles;
  // Compare mode (single-view entry points, list reuse): is everything the tile lists and the blend decisions depend on bit-equal to an
  // earlier forward's geometry state?  One word per block for the host (it rides in the copy that brings the entry counts): 0 = equal.
  // (Rounds 3 - 4 compared a 64-bit fingerprint instead -- "identical up to a 2^-64 coincidence"; the bar for integer work is bit-exact.)
  const int any = vw.block_hash ? __syncthreads_or(po.differs ? 1 : 0) : 0;
  // per-block total of tiles_touched: feeds the two-level offsets scan (no full-length scan kernel)
  uint32_t wsum = tiles;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) wsum += __shfl_xor(wsum, m, 64);
  if ((threadIdx.x & 63) == 0) s_wave_sum[threadIdx.x >> 6] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t total = s_wave_sum[0] + s_wave_sum[1] + s_wave_sum[2] + s_wave_sum[3];
    block_sums[blockIdx.x] = total;
    // the verdict word and the block's entry count in one 8-byte store: block_hash may be PINNED HOST memory (gsr_forward_capacity), where
    // the host adds the counts up as soon as this kernel's blocks are through (gsr_wait_block_counts) -- no readback, no later kernel
    if (vw.block_hash) vw.block_hash[blockIdx.x] = make_uint2(any ? 1u : 0u, total);
  }
}

#undef GSR_PFWD_NAME
