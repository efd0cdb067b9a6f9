// gsr_sh.h -- the spherical-harmonics constants and the one statement of the basis and of its view-direction gradient.  Device code only.
// Users: gsr_preprocess_fwd.hip (the constants: sh_to_rgb), gsr_preprocess_bwd.hip (sh_backward) and gsr_sh_views.hip (the multi-view SH
// pass); all three build with -ffp-contract=off, so every operation below is rounded on its own, in the order written.
#pragma once
#ifdef __HIPCC__

// constexpr, not __constant__: a header's namespace-scope __constant__ would define one host-side shadow symbol per translation unit, and
// the compiler folds these values into the instructions.  (Folding changes no bit: the only products of two constants below are by 2
// and 4, which are exact.)
constexpr float SH_C0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.4886025119029199f;
constexpr float kC2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                          -1.0925484305920792f, 0.5462742152960396f};
constexpr float kC3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                          0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                          -0.5900435899266435f};

// For one Gaussian and one view: the basis values (zeros beyond the degree's coefficients) and the gradient w.r.t. the mean through the
// view direction.  `sh` is the Gaussian's coefficient row (global memory or LDS); dL = the colour gradient, masked by the clamp bits.
__device__ __forceinline__ void sh_basis_dmean(int deg, const float* sh, float3 p, const float* __restrict__ campos, const float dL[3],
                                               float basis[16], float dmean[3]) {
  const float ox = p.x - campos[0], oy = p.y - campos[1], oz = p.z - campos[2];
  const float len = sqrtf(ox * ox + oy * oy + oz * oz), inv = 1.0f / len;
  const float x = ox * inv, y = oy * inv, z = oz * inv;
#pragma unroll
  for (int k = 0; k < 16; ++k) basis[k] = 0.f;
  float dRdx[3] = {0.f, 0.f, 0.f}, dRdy[3] = {0.f, 0.f, 0.f}, dRdz[3] = {0.f, 0.f, 0.f};
  basis[0] = SH_C0;
  if (deg > 0) {
    basis[1] = -SH_C1 * y; basis[2] = SH_C1 * z; basis[3] = -SH_C1 * x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      dRdx[ch] = -SH_C1 * sh[3 * 3 + ch]; dRdy[ch] = -SH_C1 * sh[1 * 3 + ch]; dRdz[ch] = SH_C1 * sh[2 * 3 + ch];
    }
    if (deg > 1) {
      const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      basis[4] = kC2[0] * xy; basis[5] = kC2[1] * yz; basis[6] = kC2[2] * (2.0f * zz - xx - yy);
      basis[7] = kC2[3] * xz; basis[8] = kC2[4] * (xx - yy);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
#define S(k) sh[(k)*3 + ch]
        dRdx[ch] += kC2[0] * y * S(4) - 2.0f * kC2[2] * x * S(6) + kC2[3] * z * S(7) + 2.0f * kC2[4] * x * S(8);
        dRdy[ch] += kC2[0] * x * S(4) + kC2[1] * z * S(5) - 2.0f * kC2[2] * y * S(6) - 2.0f * kC2[4] * y * S(8);
        dRdz[ch] += kC2[1] * y * S(5) + 4.0f * kC2[2] * z * S(6) + kC2[3] * x * S(7);
#undef S
      }
      if (deg > 2) {
        basis[9] = kC3[0] * y * (3.0f * xx - yy); basis[10] = kC3[1] * xy * z;
        basis[11] = kC3[2] * y * (4.0f * zz - xx - yy); basis[12] = kC3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
        basis[13] = kC3[4] * x * (4.0f * zz - xx - yy); basis[14] = kC3[5] * z * (xx - yy);
        basis[15] = kC3[6] * x * (xx - 3.0f * yy);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
#define S(k) sh[(k)*3 + ch]
          dRdx[ch] += kC3[0] * S(9) * 6.0f * xy + kC3[1] * S(10) * yz - kC3[2] * S(11) * 2.0f * xy -
                      kC3[3] * S(12) * 6.0f * xz + kC3[4] * S(13) * (-3.0f * xx + 4.0f * zz - yy) +
                      kC3[5] * S(14) * 2.0f * xz + kC3[6] * S(15) * 3.0f * (xx - yy);
          dRdy[ch] += kC3[0] * S(9) * 3.0f * (xx - yy) + kC3[1] * S(10) * xz +
                      kC3[2] * S(11) * (-3.0f * yy + 4.0f * zz - xx) - kC3[3] * S(12) * 6.0f * yz -
                      kC3[4] * S(13) * 2.0f * xy - kC3[5] * S(14) * 2.0f * yz - kC3[6] * S(15) * 6.0f * xy;
          dRdz[ch] += kC3[1] * S(10) * xy + kC3[2] * S(11) * 8.0f * yz +
                      kC3[3] * S(12) * 3.0f * (2.0f * zz - xx - yy) + kC3[4] * S(13) * 8.0f * xz +
                      kC3[5] * S(14) * (xx - yy);
#undef S
        }
      }
    }
  }
  const float ddx = dRdx[0] * dL[0] + dRdx[1] * dL[1] + dRdx[2] * dL[2];
  const float ddy = dRdy[0] * dL[0] + dRdy[1] * dL[1] + dRdy[2] * dL[2];
  const float ddz = dRdz[0] * dL[0] + dRdz[1] * dL[1] + dRdz[2] * dL[2];
  const float sum2 = ox * ox + oy * oy + oz * oz;
  const float invsum32 = 1.0f / sqrtf(sum2 * sum2 * sum2);
  dmean[0] = ((sum2 - ox * ox) * ddx - oy * ox * ddy - oz * ox * ddz) * invsum32;
  dmean[1] = (-ox * oy * ddx + (sum2 - oy * oy) * ddy - oz * oy * ddz) * invsum32;
  dmean[2] = (-ox * oz * ddx - oy * oz * ddy + (sum2 - oz * oz) * ddz) * invsum32;
}

#endif  // __HIPCC__
