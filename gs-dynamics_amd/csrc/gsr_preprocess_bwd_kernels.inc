// gsr_preprocess_bwd_kernels.inc -- the per-Gaussian backward kernels, included four times by gsr_preprocess_bwd.hip (inside its namespace):
//   GSR_PBWD_DEPTH 0: preprocess_bwd_kernel, preprocess_bwd_views_kernel, preprocess_bwd_views_waves_kernel (gsr_backward*)
//   GSR_PBWD_DEPTH 1: preprocess_bwd_depth_kernel, ... _views_depth_kernel, ... _views_waves_depth_kernel (gsr_backward*_depth): one more
//                     argument -- the blend backward's per-entry dL/dz -- whose per-Gaussian sum joins dL/dtz in the fp64 chain (view_chain).
//   GSR_PBWD_AA 1:    the anti-aliasing builds of both (*_aa_kernel, *_aa_depth_kernel; DESIGN.md section 3f): one more argument -- the
//                     forward's records, whose staged opacity o' = o c the chain needs -- the o g dc term in view_chain, and every view's
//                     dL/do' scaled by its own c BEFORE the views are summed.
// The depth and anti-aliasing builds are compile-time switches: the GSR_PBWD_DEPTH 0 / GSR_PBWD_AA 0 kernels are the code they were before.
#if GSR_PBWD_DEPTH && GSR_PBWD_AA
#define GSR_PBWD_NAME(k) k##_aa_depth_kernel
#elif GSR_PBWD_DEPTH
#define GSR_PBWD_NAME(k) k##_depth_kernel
#elif GSR_PBWD_AA
#define GSR_PBWD_NAME(k) k##_aa_kernel
#else
#define GSR_PBWD_NAME(k) k##_kernel
#endif
#if GSR_PBWD_DEPTH
#define GSR_PBWD_DZ_PARAM(...) , __VA_ARGS__
#define GSR_PBWD_DZ(x) (x)
#else
#define GSR_PBWD_DZ_PARAM(...)
#define GSR_PBWD_DZ(x) ((const float*)nullptr)
#endif
#if GSR_PBWD_AA
#define GSR_PBWD_AA_PARAM(...) , __VA_ARGS__
// the trailing view_chain arguments of an anti-aliasing build: the fp32 covariance, the view's staged o' (record part 1, .y), the factor out
#define GSR_PBWD_AA_ARGS(recs) , cv32, (recs)[GSR_REC_F4 * (size_t)i + 1].y, &caa
#else
#define GSR_PBWD_AA_PARAM(...)
#define GSR_PBWD_AA_ARGS(recs)
#endif

// ---- single view ------------------------------------------------------------------------------------
template <bool USE_SH>
__global__ __launch_bounds__(GSR_BLOCK) void GSR_PBWD_NAME(preprocess_bwd)(
    int P, int W, int H, float tanfovx, float tanfovy, float mod, int sh_degree, int M,
    const float* __restrict__ view, const float* __restrict__ proj, const float* __restrict__ campos,
    const float* __restrict__ means3D, const float* __restrict__ scales, const float* __restrict__ rotations,
    const float* __restrict__ colors_precomp, const float* __restrict__ shs, const float* __restrict__ cov3D_precomp,
    const int32_t* __restrict__ radii, const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ clamped,
    const float4* __restrict__ partials, float* __restrict__ dL_dmeans3D, float* __restrict__ dL_dmeans2D,
    float* __restrict__ dL_dcolors, float* __restrict__ dL_dopacity, float* __restrict__ dL_dscales,
    float* __restrict__ dL_drot, float* __restrict__ dL_dcov3D, float* __restrict__ dL_dsh,
    const uint8_t* __restrict__ used, const uint32_t* __restrict__ tracked, const uint32_t* __restrict__ bwd_error GSR_PBWD_DZ_PARAM(const float* __restrict__ dL_dz)
    GSR_PBWD_AA_PARAM(const float4* __restrict__ rec)) {
  const int i = blockIdx.x * GSR_BLOCK + threadIdx.x;
  if (i >= P) return;
  float gm3[3] = {0.f, 0.f, 0.f}, gm2[2] = {0.f, 0.f}, gcol[3] = {0.f, 0.f, 0.f}, gop = 0.f;
  float gs[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f}, gcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool alive = radii[i] > 0 && (!used || !tracked || *tracked == 0u || used[i] != 0);   // (see gsr_view_used)
  if (USE_SH && !alive && dL_dsh) {
    for (int k = 0; k < M * 3; ++k) dL_dsh[(size_t)i * M * 3 + k] = 0.f;
  }
  if (alive) {
    const PartialSum ps = reduce_partials(partials, offsets[i], offsets[i + 1], USE_SH || dL_dcolors != nullptr);
    gop = ps.gop;
    const float3 p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
    if (USE_SH) {
      float dmean_sh[3] = {0.f, 0.f, 0.f};
      sh_backward(sh_degree, M, shs + (size_t)i * M * 3, p, campos, clamped[i], ps.dr, ps.dg, ps.db,
                  dL_dsh + (size_t)i * M * 3, dmean_sh);
      gm3[0] = dmean_sh[0]; gm3[1] = dmean_sh[1]; gm3[2] = dmean_sh[2];
    } else {
      gcol[0] = ps.dr; gcol[1] = ps.dg; gcol[2] = ps.db;
    }
    Cov3 cv;
    build_cov3(i, mod, scales, rotations, cov3D_precomp, cv);
#if GSR_PBWD_AA
    float cv32[6], caa = 1.f;
    build_cov3_f32(i, mod, scales, rotations, cov3D_precomp, cv32);
#endif
    if (GSR_PBWD_DEPTH) view_chain<true, GSR_PBWD_AA>(view, proj, W, H, tanfovx, tanfovy, p, cv.c, ps, gcov, gm3, gm2, 0.f, 0.f, nullptr,
                                                      reduce_partials_dz(GSR_PBWD_DZ(dL_dz), offsets[i], offsets[i + 1]) GSR_PBWD_AA_ARGS(rec));
    else view_chain<false, GSR_PBWD_AA>(view, proj, W, H, tanfovx, tanfovy, p, cv.c, ps, gcov, gm3, gm2, 0.f, 0.f, nullptr, 0.f GSR_PBWD_AA_ARGS(rec));
#if GSR_PBWD_AA
    gop = caa * ps.gop;     // dL/do = c dL/do'
#endif
    if (!cov3D_precomp) cov3_to_scale_rot(cv, mod, gcov, gs, gq);
  }
  if (bwd_error && *bwd_error != 0u) gm3[0] = gm3[1] = gm3[2] = __builtin_nanf("");   // the blend backward of this call aborted: loud, not garbage (GSR_QUEUE_BWD_ERROR)
  dL_dmeans3D[3 * i] = gm3[0]; dL_dmeans3D[3 * i + 1] = gm3[1]; dL_dmeans3D[3 * i + 2] = gm3[2];
  dL_dmeans2D[3 * i] = gm2[0]; dL_dmeans2D[3 * i + 1] = gm2[1]; dL_dmeans2D[3 * i + 2] = 0.f;
  if (dL_dcolors) { dL_dcolors[3 * i] = gcol[0]; dL_dcolors[3 * i + 1] = gcol[1]; dL_dcolors[3 * i + 2] = gcol[2]; }
  dL_dopacity[i] = gop;
  if (dL_dscales) { dL_dscales[3 * i] = gs[0]; dL_dscales[3 * i + 1] = gs[1]; dL_dscales[3 * i + 2] = gs[2]; }
  if (dL_drot) { dL_drot[4 * i] = gq[0]; dL_drot[4 * i + 1] = gq[1]; dL_drot[4 * i + 2] = gq[2]; dL_drot[4 * i + 3] = gq[3]; }
  if (dL_dcov3D) {
#pragma unroll
    for (int k = 0; k < 6; ++k) dL_dcov3D[6 * i + k] = gcov[k];
  }
}

// ---- all views of a step at once (precomputed colours) ----------------------------------------------
// One lane per Gaussian loops over the V views: per view it reduces that view's entry records and runs the
// view-dependent chain; colour / opacity / mean / cov3D gradients are summed in registers and the
// scale/rotation chain (linear in dL/dcov3D) runs once.  Replaces V kernels + the host-side sums over views.
__global__ __launch_bounds__(GSR_BLOCK) void GSR_PBWD_NAME(preprocess_bwd_views)(
    GsrBwdViews vw, int P, float mod, const float* __restrict__ means3D, const float* __restrict__ scales,
    const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp, float* __restrict__ dL_dmeans3D,
    float* __restrict__ dL_dcolors, float* __restrict__ dL_dopacity, float* __restrict__ dL_dscales,
    float* __restrict__ dL_drot, float* __restrict__ dL_dcov3D GSR_PBWD_DZ_PARAM(GsrDepthViews dz) GSR_PBWD_AA_PARAM(GsrAaViews aa)) {
  const int i = blockIdx.x * GSR_BLOCK + threadIdx.x;
  if (i >= P) return;
  float gm3[3] = {0.f, 0.f, 0.f}, gcol[3] = {0.f, 0.f, 0.f}, gop = 0.f;
  float gs[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f}, gcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float3 p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
  Cov3 cv;
  build_cov3(i, mod, scales, rotations, cov3D_precomp, cv);
#if GSR_PBWD_AA
  float cv32[6];
  build_cov3_f32(i, mod, scales, rotations, cov3D_precomp, cv32);
#endif
  bool any = false;
  for (int v = 0; v < vw.V; ++v) {
    const GsrBwdView& w = vw.v[v];
    if (w.fused_alias) continue;      // its owner's records carry it (fused pair): the owner writes its dL_dmeans2D too
    float gm2[2] = {0.f, 0.f}, gm2a[2] = {0.f, 0.f};
    const bool pair = w.partner_dL_dmeans2D != nullptr;
    if (w.radii[i] > 0 && gsr_view_used(w, i)) {
      any = true;
      const PartialSum ps = reduce_partials(w.partials, min(w.offsets[i], w.cap), min(w.offsets[i + 1], w.cap),
                                            pair || w.dL_dcolors != nullptr || dL_dcolors != nullptr);
#if GSR_PBWD_AA
      float caa = 1.f;
#else
      gop += ps.gop;
#endif
      if (pair) {   // record layout of the pair backward: geometry sums of both views, then (sum t dx, sum t dy) of this view alone
        view_chain<false, GSR_PBWD_AA>(w.view, w.proj, w.W, w.H, w.tanfovx, w.tanfovy, p, cv.c, ps, gcov, gm3, gm2, ps.dr, ps.dg, gm2a,
                                       0.f GSR_PBWD_AA_ARGS(aa.rec[v]));
      } else {
        if (w.dL_dcolors) { w.dL_dcolors[3 * i] = ps.dr; w.dL_dcolors[3 * i + 1] = ps.dg; w.dL_dcolors[3 * i + 2] = ps.db; }
        else { gcol[0] += ps.dr; gcol[1] += ps.dg; gcol[2] += ps.db; }
        if (GSR_PBWD_DEPTH && GSR_PBWD_DZ(dz.dL_dz[v]))   // (a view without a depth gradient: nullptr)
          view_chain<true, GSR_PBWD_AA>(w.view, w.proj, w.W, w.H, w.tanfovx, w.tanfovy, p, cv.c, ps, gcov, gm3, gm2, 0.f, 0.f, nullptr,
                                        reduce_partials_dz(GSR_PBWD_DZ(dz.dL_dz[v]), min(w.offsets[i], w.cap), min(w.offsets[i + 1], w.cap))
                                        GSR_PBWD_AA_ARGS(aa.rec[v]));
        else view_chain<false, GSR_PBWD_AA>(w.view, w.proj, w.W, w.H, w.tanfovx, w.tanfovy, p, cv.c, ps, gcov, gm3, gm2, 0.f, 0.f, nullptr,
                                            0.f GSR_PBWD_AA_ARGS(aa.rec[v]));
      }
#if GSR_PBWD_AA
      gop += caa * ps.gop;    // each view's dL/do' scaled by its own c, then summed
#endif
    } else if (w.dL_dcolors) {
      w.dL_dcolors[3 * i] = 0.f; w.dL_dcolors[3 * i + 1] = 0.f; w.dL_dcolors[3 * i + 2] = 0.f;
    }
    if (pair) {
      w.dL_dmeans2D[3 * i] = gm2a[0]; w.dL_dmeans2D[3 * i + 1] = gm2a[1]; w.dL_dmeans2D[3 * i + 2] = 0.f;
      float* m2b = w.partner_dL_dmeans2D;
      m2b[3 * i] = gm2[0] - gm2a[0]; m2b[3 * i + 1] = gm2[1] - gm2a[1]; m2b[3 * i + 2] = 0.f;
    } else {
      w.dL_dmeans2D[3 * i] = gm2[0]; w.dL_dmeans2D[3 * i + 1] = gm2[1]; w.dL_dmeans2D[3 * i + 2] = 0.f;
    }
  }
  if (any && !cov3D_precomp) cov3_to_scale_rot(cv, mod, gcov, gs, gq);
  if (vw.bwd_error && *vw.bwd_error != 0u) gm3[0] = gm3[1] = gm3[2] = __builtin_nanf("");   // the blend backward of this call aborted: loud, not garbage (GSR_QUEUE_BWD_ERROR)
  dL_dmeans3D[3 * i] = gm3[0]; dL_dmeans3D[3 * i + 1] = gm3[1]; dL_dmeans3D[3 * i + 2] = gm3[2];
  if (dL_dcolors) { dL_dcolors[3 * i] = gcol[0]; dL_dcolors[3 * i + 1] = gcol[1]; dL_dcolors[3 * i + 2] = gcol[2]; }
  if (vw.d_raw_rot) {   // raw-parameter mode: the chain through normalize / sigmoid / exp, here instead of in a launch of its own
    reinterpret_cast<float4*>(vw.d_raw_rot)[i] =
        gsr_act_rotation_bwd(reinterpret_cast<const float4*>(vw.raw_rot)[i], make_float4(gq[0], gq[1], gq[2], gq[3]));
    const float o = vw.act_op[i];
    vw.d_raw_op[i] = gop * o * (1.0f - o);
#pragma unroll
    for (int k = 0; k < 3; ++k) vw.d_raw_sc[3 * (size_t)i + k] = gs[k] * vw.act_sc[3 * (size_t)i + k];
  }
  if (dL_dopacity) dL_dopacity[i] = gop;
  if (dL_dscales) { dL_dscales[3 * i] = gs[0]; dL_dscales[3 * i + 1] = gs[1]; dL_dscales[3 * i + 2] = gs[2]; }
  if (dL_drot) { dL_drot[4 * i] = gq[0]; dL_drot[4 * i + 1] = gq[1]; dL_drot[4 * i + 2] = gq[2]; dL_drot[4 * i + 3] = gq[3]; }
  if (dL_dcov3D) {
#pragma unroll
    for (int k = 0; k < 6; ++k) dL_dcov3D[6 * i + k] = gcov[k];
  }
}

// ---- all views of a step at once, ONE WAVE PER VIEW (V >= 2) ------------------------------------------
// The loop above walks the views strictly load -> chain -> load at 1.5 waves per SIMD: 62 us for 8 views of 100 k Gaussians, 22 % of the
// HBM roofline.  Here a workgroup owns 64 Gaussians and has one wave per (non-alias) view: the view is wave-uniform (its matrices and
// pointers stay scalar loads), every wave reduces its view's records and runs that view's chain for the 64 Gaussians, parks its 13
// per-Gaussian sums in LDS ([view][value][lane]: conflict-free), and wave 0 adds the views up in view order -- the same order of
// additions as the loop, hence the same bits -- and finishes with the view-independent part (scale / rotation chain, activations).
// V x more waves in flight, no second pass over HBM.
#ifndef PBW_VALUES
#define PBW_VALUES 13      // gcov[6], gm3[3], gop, gcol[3]
#endif
// (No occupancy bound: with the chain in fp64 the kernel needs 166 VGPRs; bounded to the fp32 build's 80 it spilled and took 70 us at four views.)
template <int MAXW>      // waves per workgroup the instantiation is compiled for (= views it can take): its register budget follows
__global__ __launch_bounds__(64 * MAXW) void GSR_PBWD_NAME(preprocess_bwd_views_waves)(
    GsrBwdViews vw, int P, float mod, const float* __restrict__ means3D, const float* __restrict__ scales,
    const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp, float* __restrict__ dL_dmeans3D,
    float* __restrict__ dL_dcolors, float* __restrict__ dL_dopacity, float* __restrict__ dL_dscales,
    float* __restrict__ dL_drot, float* __restrict__ dL_dcov3D GSR_PBWD_DZ_PARAM(GsrDepthViews dz) GSR_PBWD_AA_PARAM(GsrAaViews aa)) {
  extern __shared__ float s_part[];                  // [waves][PBW_VALUES + 1][64]  (+1: "this view saw the Gaussian")
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = (int)(blockDim.x >> 6);
  const int i = blockIdx.x * 64 + lane;
  const bool live = i < P;
  // wave wv's view: the wv-th view that is not a fused alias (uniform: scalar code)
  int v = -1;
  for (int u = 0, k = 0; u < vw.V; ++u)
    if (!vw.v[u].fused_alias) { if (k == wv) { v = u; break; } ++k; }
  const GsrBwdView& w = vw.v[v < 0 ? 0 : v];
  float3 p = make_float3(0.f, 0.f, 0.f);
  Cov3 cv;
#if GSR_PBWD_AA
  float cv32[6];
#endif
  if (live) {
    p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
    build_cov3(i, mod, scales, rotations, cov3D_precomp, cv);
#if GSR_PBWD_AA
    build_cov3_f32(i, mod, scales, rotations, cov3D_precomp, cv32);
#endif
  }
  float gm3[3] = {0.f, 0.f, 0.f}, gcol[3] = {0.f, 0.f, 0.f}, gop = 0.f, gcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float seen = 0.f;
  if (live && v >= 0) {
    float gm2[2] = {0.f, 0.f}, gm2a[2] = {0.f, 0.f};
    const bool pair = w.partner_dL_dmeans2D != nullptr;
    if (w.radii[i] > 0 && gsr_view_used(w, i)) {
      seen = 1.f;
      const PartialSum ps = reduce_partials(w.partials, min(w.offsets[i], w.cap), min(w.offsets[i + 1], w.cap),
                                            pair || w.dL_dcolors != nullptr || dL_dcolors != nullptr);
      gop = ps.gop;
#if GSR_PBWD_AA
      float caa = 1.f;
#endif
      if (pair) {
        view_chain<false, GSR_PBWD_AA>(w.view, w.proj, w.W, w.H, w.tanfovx, w.tanfovy, p, cv.c, ps, gcov, gm3, gm2, ps.dr, ps.dg, gm2a,
                                       0.f GSR_PBWD_AA_ARGS(aa.rec[v]));
      } else {
        if (w.dL_dcolors) { w.dL_dcolors[3 * i] = ps.dr; w.dL_dcolors[3 * i + 1] = ps.dg; w.dL_dcolors[3 * i + 2] = ps.db; }
        else { gcol[0] = ps.dr; gcol[1] = ps.dg; gcol[2] = ps.db; }
        if (GSR_PBWD_DEPTH && GSR_PBWD_DZ(dz.dL_dz[v]))   // (a view without a depth gradient: nullptr)
          view_chain<true, GSR_PBWD_AA>(w.view, w.proj, w.W, w.H, w.tanfovx, w.tanfovy, p, cv.c, ps, gcov, gm3, gm2, 0.f, 0.f, nullptr,
                                        reduce_partials_dz(GSR_PBWD_DZ(dz.dL_dz[v]), min(w.offsets[i], w.cap), min(w.offsets[i + 1], w.cap))
                                        GSR_PBWD_AA_ARGS(aa.rec[v]));
        else view_chain<false, GSR_PBWD_AA>(w.view, w.proj, w.W, w.H, w.tanfovx, w.tanfovy, p, cv.c, ps, gcov, gm3, gm2, 0.f, 0.f, nullptr,
                                            0.f GSR_PBWD_AA_ARGS(aa.rec[v]));
      }
#if GSR_PBWD_AA
      gop = caa * ps.gop;     // scaled by this view's c before the LDS exchange sums the views
#endif
    } else if (w.dL_dcolors) {
      w.dL_dcolors[3 * i] = 0.f; w.dL_dcolors[3 * i + 1] = 0.f; w.dL_dcolors[3 * i + 2] = 0.f;
    }
    if (pair) {
      w.dL_dmeans2D[3 * i] = gm2a[0]; w.dL_dmeans2D[3 * i + 1] = gm2a[1]; w.dL_dmeans2D[3 * i + 2] = 0.f;
      float* m2b = w.partner_dL_dmeans2D;
      m2b[3 * i] = gm2[0] - gm2a[0]; m2b[3 * i + 1] = gm2[1] - gm2a[1]; m2b[3 * i + 2] = 0.f;
    } else {
      w.dL_dmeans2D[3 * i] = gm2[0]; w.dL_dmeans2D[3 * i + 1] = gm2[1]; w.dL_dmeans2D[3 * i + 2] = 0.f;
    }
  }
  float* mine = s_part + (size_t)wv * (PBW_VALUES + 1) * 64 + lane;
#pragma unroll
  for (int k = 0; k < 6; ++k) mine[k * 64] = gcov[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) { mine[(6 + k) * 64] = gm3[k]; mine[(10 + k) * 64] = gcol[k]; }
  mine[9 * 64] = gop;
  mine[PBW_VALUES * 64] = seen;
  __syncthreads();
  if (wv != 0 || !live) return;
  // view order: the loop kernel adds view 0's terms to zero-initialised sums first -- start from this wave's own values (view order
  // = wave order) and add the others in order
  bool any = seen != 0.f;
  for (int u = 1; u < nw; ++u) {
    const float* q = s_part + (size_t)u * (PBW_VALUES + 1) * 64 + lane;
#pragma unroll
    for (int k = 0; k < 6; ++k) gcov[k] += q[k * 64];
#pragma unroll
    for (int k = 0; k < 3; ++k) { gm3[k] += q[(6 + k) * 64]; gcol[k] += q[(10 + k) * 64]; }
    gop += q[9 * 64];
    any = any || q[PBW_VALUES * 64] != 0.f;
  }
  float gs[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f};
  if (any && !cov3D_precomp) cov3_to_scale_rot(cv, mod, gcov, gs, gq);
  if (vw.bwd_error && *vw.bwd_error != 0u) gm3[0] = gm3[1] = gm3[2] = __builtin_nanf("");   // the blend backward of this call aborted: loud, not garbage (GSR_QUEUE_BWD_ERROR)
  dL_dmeans3D[3 * i] = gm3[0]; dL_dmeans3D[3 * i + 1] = gm3[1]; dL_dmeans3D[3 * i + 2] = gm3[2];
  if (dL_dcolors) { dL_dcolors[3 * i] = gcol[0]; dL_dcolors[3 * i + 1] = gcol[1]; dL_dcolors[3 * i + 2] = gcol[2]; }
  if (vw.d_raw_rot) {
    reinterpret_cast<float4*>(vw.d_raw_rot)[i] =
        gsr_act_rotation_bwd(reinterpret_cast<const float4*>(vw.raw_rot)[i], make_float4(gq[0], gq[1], gq[2], gq[3]));
    const float o = vw.act_op[i];
    vw.d_raw_op[i] = gop * o * (1.0f - o);
#pragma unroll
    for (int k = 0; k < 3; ++k) vw.d_raw_sc[3 * (size_t)i + k] = gs[k] * vw.act_sc[3 * (size_t)i + k];
  }
  if (dL_dopacity) dL_dopacity[i] = gop;
  if (dL_dscales) { dL_dscales[3 * i] = gs[0]; dL_dscales[3 * i + 1] = gs[1]; dL_dscales[3 * i + 2] = gs[2]; }
  if (dL_drot) { dL_drot[4 * i] = gq[0]; dL_drot[4 * i + 1] = gq[1]; dL_drot[4 * i + 2] = gq[2]; dL_drot[4 * i + 3] = gq[3]; }
  if (dL_dcov3D) {
#pragma unroll
    for (int k = 0; k < 6; ++k) dL_dcov3D[6 * i + k] = gcov[k];
  }
}

#undef GSR_PBWD_NAME
#undef GSR_PBWD_DZ_PARAM
#undef GSR_PBWD_DZ
#undef GSR_PBWD_AA_PARAM
#undef GSR_PBWD_AA_ARGS
