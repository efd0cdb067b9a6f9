// gsr_preprocess_bwd.hip -- per-Gaussian backward for gfx950 (replaces the
// reference extension's computeCov2D-backward + preprocess-backward kernels, fused into one).
//
// One lane per Gaussian:
//   1. reduce its entry records (one 36-byte record per touched tile, contiguous, written by
//      render_bwd) in ascending tile order -> dL/d{mean2D_pix, conic(A,B,C), opacity, rgb};
//   2. conic -> cov2D -> (cov3D, view-space mean) -> (scale, rotation, mean3D);  the 3D covariance is
//      recomputed from scale/rotation rather than stored by the forward (saves 24 B/Gaussian each way);
//   3. 2D mean -> 3D mean through the 4x4 projection; SH backward when colours came from SH.
// Every output element is written (zeros for culled Gaussians): callers need no memset.
// HBM per Gaussian: reads 36*tiles + 12 + 12 + 16 + 8 + 4 + 4, writes 12+12+12+4+12+16+24 = 92 B.
#include "gsr_common.h"
#include "gsr_sh.h"

// kernels live in a NAMED namespace: profilers and traces show gsr_preprocess_bwd::<kernel>, not "(anonymous namespace)"
namespace gsr_preprocess_bwd {

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// SH backward for one Gaussian: writes dL_dsh (all M coefficients; inactive ones get 0) and returns
// the gradient w.r.t. the mean through the view direction.
// NO_DSH (the camera pass): only the mean term, dL_dsh is not written (dsh may be nullptr).  dL/dcampos = -dmean.
template <bool NO_DSH = false>
__device__ void sh_backward(int deg, int M, const float* __restrict__ sh, float3 p, const float* __restrict__ campos,
                            uint32_t clamped, float g0, float g1, float g2, float* __restrict__ dsh, float dmean[3]) {
  const float dL[3] = {(clamped & 1u) ? 0.f : g0, (clamped & 2u) ? 0.f : g1, (clamped & 4u) ? 0.f : g2};
  float basis[16];
  sh_basis_dmean(deg, sh, p, campos, dL, basis, dmean);
  const int ncoef = (deg + 1) * (deg + 1);
  for (int k = 0; !NO_DSH && k < M; ++k) {
    const float bk = k < ncoef ? basis[k < 16 ? k : 15] : 0.f;
    dsh[k * 3 + 0] = bk * dL[0]; dsh[k * 3 + 1] = bk * dL[1]; dsh[k * 3 + 2] = bk * dL[2];
  }
}

// ---- shared pieces ---------------------------------------------------------------------------------
struct PartialSum { float gmx, gmy, gA, gB, gC, gop, dr, dg, db; };

// Sum of a Gaussian's entry records (one per touched tile, contiguous, ascending tile order).
// `col` = false: the blend backward wrote the six geometry sums only (24 of the 36 bytes; no colour gradient wanted).
__device__ __forceinline__ PartialSum reduce_partials(const float4* __restrict__ partials, uint32_t e0, uint32_t e1, bool col = true) {
  float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
  float r2x = 0.f;
  // FOUR records per trip, all of their loads issued before the first is used: the walk is a chain of memory round trips (a lane's
  // records are contiguous, the lanes of a wave are ~150 bytes apart), and the trip count -- the longest rect of the wave -- was the
  // kernel's time.  The additions keep their order (record e0 first).
  constexpr int RU = 4;
  // `col` = false: the blend backward wrote the six geometry sums only (24 of the 36 bytes).  The walk reads whole records all the same
  // -- the same cache lines, and the three-load form measured FASTER than a two-load one (52.5 vs 58 us at 8 views) -- the colour sums
  // then hold whatever the scratch held and are zeroed below (garbage must not propagate).
  for (uint32_t e = e0; e < e1; e += RU) {
    float4 q0[RU], q1[RU];
    float q2x[RU];
#pragma unroll
    for (int k = 0; k < RU; ++k) if (e + k < e1) gsr_load_partial(partials, e + k, q0[k], q1[k], q2x[k]);
#pragma unroll
    for (int k = 0; k < RU; ++k)
      if (e + k < e1) {
        r0.x += q0[k].x; r0.y += q0[k].y; r0.z += q0[k].z; r0.w += q0[k].w;
        r1.x += q1[k].x; r1.y += q1[k].y; r1.z += q1[k].z; r1.w += q1[k].w;
        r2x += q2x[k];
      }
  }
  PartialSum ps;
  // the blend backward stores the conic partials without their constant factors (dA: -1/2, dB: -1, dC: -1/2)
  ps.gmx = r0.x; ps.gmy = r0.y; ps.gA = -0.5f * r0.z; ps.gB = -r0.w; ps.gC = -0.5f * r1.x; ps.gop = r1.y;
  // !col: those twelve bytes were never written (possibly NaN patterns): they must not reach any sum or LDS slot
  ps.dr = col ? r1.z : 0.f; ps.dg = col ? r1.w : 0.f; ps.db = col ? r2x : 0.f;
  return ps;
}
// The depth path of the reduce: dL/dz of a Gaussian = the sum of its entries' dL/dz (the blend backward's depth build writes one float per
// entry, indexed like the records), in the same ascending order.
__device__ __forceinline__ float reduce_partials_dz(const float* __restrict__ dL_dz, uint32_t e0, uint32_t e1) {
  float gz = 0.f;
  for (uint32_t e = e0; e < e1; ++e) gz += dL_dz[e];
  return gz;
}

// The per-Gaussian chain (3D covariance, conic -> cov2D -> cov3D / view-space mean, cov3D -> scale / rotation) runs in DOUBLE precision
// (round 6).  It is a chain of differences of nearly equal products -- det = a c - b b, the inverse of the 2D covariance, the congruence
// with T, the quaternion terms -- and for a Gaussian that is elongated on screen (a nearly singular conic) fp32 loses 1e-4 ... 6e-3 of that
// Gaussian's gradient row THERE, in any operation order: the fp32 oracle's rows are as far from its fp64 build as this kernel's were.  Inputs
// (the record sums of the blend backward, the parameters) and outputs stay fp32; in between, fp64 costs this latency-bound kernel 24 -> 29 us
// at four views, +1 us at one (MI355X issues fp64 FMAs at the fp32 rate; the price is registers: 166 instead of 90 VGPRs), and puts the
// parity soak's tail cases 3 - 40 x closer to the fp64 oracle than the fp32 oracle is (profiles/r06_fp64_chain.txt): seed 9 case 895
// scales 1.03e-4 -> 1.2e-5, GSR_SOAK_BIG seed 6 case 156 worst row 6.2e-3 -> 7.4e-5.
typedef double real;
// Rotation matrix, scaled axes and 3D covariance of one Gaussian (view independent).
struct Cov3 { real R[3][3]; real s[3]; real q[4]; real c[6]; };
__device__ __forceinline__ void build_cov3(int i, float mod, const float* __restrict__ scales,
                                           const float* __restrict__ rotations, const float* __restrict__ cov3D_precomp,
                                           Cov3& o) {
  if (cov3D_precomp) {
#pragma unroll
    for (int k = 0; k < 6; ++k) o.c[k] = cov3D_precomp[6 * i + k];
#pragma unroll
    for (int a = 0; a < 3; ++a) { o.s[a] = 0.f; for (int b = 0; b < 3; ++b) o.R[a][b] = 0.f; }
    o.q[0] = o.q[1] = o.q[2] = o.q[3] = 0.f;
    return;
  }
  const real r = rotations[4 * i], x = rotations[4 * i + 1], y = rotations[4 * i + 2], z = rotations[4 * i + 3];
  o.q[0] = r; o.q[1] = x; o.q[2] = y; o.q[3] = z;
  o.R[0][0] = 1.f - 2.f * (y * y + z * z); o.R[0][1] = 2.f * (x * y - r * z); o.R[0][2] = 2.f * (x * z + r * y);
  o.R[1][0] = 2.f * (x * y + r * z); o.R[1][1] = 1.f - 2.f * (x * x + z * z); o.R[1][2] = 2.f * (y * z - r * x);
  o.R[2][0] = 2.f * (x * z - r * y); o.R[2][1] = 2.f * (y * z + r * x); o.R[2][2] = 1.f - 2.f * (x * x + y * y);
  o.s[0] = (real)mod * scales[3 * i]; o.s[1] = (real)mod * scales[3 * i + 1]; o.s[2] = (real)mod * scales[3 * i + 2];
  real Mm[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) Mm[a][b] = o.R[a][b] * o.s[b];
  o.c[0] = Mm[0][0] * Mm[0][0] + Mm[0][1] * Mm[0][1] + Mm[0][2] * Mm[0][2];
  o.c[1] = Mm[0][0] * Mm[1][0] + Mm[0][1] * Mm[1][1] + Mm[0][2] * Mm[1][2];
  o.c[2] = Mm[0][0] * Mm[2][0] + Mm[0][1] * Mm[2][1] + Mm[0][2] * Mm[2][2];
  o.c[3] = Mm[1][0] * Mm[1][0] + Mm[1][1] * Mm[1][1] + Mm[1][2] * Mm[1][2];
  o.c[4] = Mm[1][0] * Mm[2][0] + Mm[1][1] * Mm[2][1] + Mm[1][2] * Mm[2][2];
  o.c[5] = Mm[2][0] * Mm[2][0] + Mm[2][1] * Mm[2][1] + Mm[2][2] * Mm[2][2];
}

// Anti-aliasing builds: the forward's fp32 3D covariance, with its operations in its order (both files build with
// contraction off, so these are its bits; raw-parameter mode: `scales` / `rotations` are the activated values that forward wrote).
__device__ __forceinline__ void build_cov3_f32(int i, float mod, const float* __restrict__ scales, const float* __restrict__ rotations,
                                               const float* __restrict__ cov3D_precomp, float c[6]) {
  if (cov3D_precomp) {
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = cov3D_precomp[6 * i + k];
    return;
  }
  const float r = rotations[4 * i], x = rotations[4 * i + 1], y = rotations[4 * i + 2], z = rotations[4 * i + 3];
  const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
  const float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
  const float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
  const float s0 = mod * scales[3 * i], s1 = mod * scales[3 * i + 1], s2 = mod * scales[3 * i + 2];
  const float M00 = R00 * s0, M01 = R01 * s1, M02 = R02 * s2;
  const float M10 = R10 * s0, M11 = R11 * s1, M12 = R12 * s2;
  const float M20 = R20 * s0, M21 = R21 * s1, M22 = R22 * s2;
  c[0] = M00 * M00 + M01 * M01 + M02 * M02;
  c[1] = M00 * M10 + M01 * M11 + M02 * M12;
  c[2] = M00 * M20 + M01 * M21 + M02 * M22;
  c[3] = M10 * M10 + M11 * M11 + M12 * M12;
  c[4] = M10 * M20 + M11 * M21 + M12 * M22;
  c[5] = M20 * M20 + M21 * M21 + M22 * M22;
}
// ... and the forward's fp32 ratio r = det0 / det1 of one view (gsr_aa_ratio), from the forward's view-space position: the side of the
// floor the forward took.  An fp64 r within rounding of the floor could fall on the other side.
__device__ __forceinline__ float aa_ratio32(const float* __restrict__ view, int W, int H, float tanfovx, float tanfovy, float pvz,
                                            float txtz, float tytz, const float c[6]) {
  const float fx = (float)W / (2.0f * tanfovx), fy = (float)H / (2.0f * tanfovy);
  const float limx = 1.3f * tanfovx, limy = 1.3f * tanfovy;
  const float tz = pvz;
  const float tx = clampf(txtz, -limx, limx) * tz;
  const float ty = clampf(tytz, -limy, limy) * tz;
  const float J00 = fx / tz, J02 = -(fx * tx) / (tz * tz);
  const float J11 = fy / tz, J12 = -(fy * ty) / (tz * tz);
  const float T00 = J00 * view[0] + J02 * view[2], T01 = J00 * view[4] + J02 * view[6], T02 = J00 * view[8] + J02 * view[10];
  const float T10 = J11 * view[1] + J12 * view[2], T11 = J11 * view[5] + J12 * view[6], T12 = J11 * view[9] + J12 * view[10];
  const float U00 = T00 * c[0] + T01 * c[1] + T02 * c[2], U01 = T00 * c[1] + T01 * c[3] + T02 * c[4], U02 = T00 * c[2] + T01 * c[4] + T02 * c[5];
  const float U10 = T10 * c[0] + T11 * c[1] + T12 * c[2], U11 = T10 * c[1] + T11 * c[3] + T12 * c[4], U12 = T10 * c[2] + T11 * c[4] + T12 * c[5];
  float a = U00 * T00 + U01 * T01 + U02 * T02;
  const float b = U00 * T10 + U01 * T11 + U02 * T12;
  float cc = U10 * T10 + U11 * T11 + U12 * T12;
  const float a0 = a, c0 = cc;
  a += 0.3f; cc += 0.3f;
  const float det = a * cc - b * b;
  return gsr_aa_ratio(a0, b, c0, det);
}

// One view's chain: conic -> cov2D -> (cov3D, view-space mean) and 2D mean -> 3D mean.  ACCUMULATES into
// gcov[6] and gm3[3]; returns this view's dL/d(NDC mean) in gm2.
// DEPTH: gz = dL/d(view-space depth) of the Gaussian from the depth image; depth IS tz (no frustum clamp on it), so it joins dL/dtz and
// reaches dL/dmeans3D as gz * (view[2], view[6], view[10]) inside the fp64 sum.
// AA: the staged opacity was o' = o c(A, B, C).  c32 = the forward's fp32 3D covariance (build_cov3_f32), o_s = this
// view's staged o'; the term o g dc/d{A, B, C} (g = ps.gop = dL/do') joins dL/d{a, b, c}, and *c_out receives the factor of dL/do = c g.
// CAM (the camera pass): *ct receives the fp64 intermediates the camera gradients are made of.
struct ChainTerms {
  real dt[3];             // dL/d(view-space position): frustum-clamp mask, depth and anti-aliasing terms included
  real dT0[3], dT1[3];    // dL/dT, T = J W (the two rows)
  real J00, J02, J11, J12;
  real m2x, m2y;          // dL/d(NDC mean)
  real hx, hy, mw;        // the projection: h = proj p, mw = 1 / (h.w + 1e-7)
};
template <bool DEPTH = false, bool AA = false, bool CAM = false>
__device__ __forceinline__ void view_chain(const float* __restrict__ view, const float* __restrict__ proj, int W, int H,
                                           float tanfovx, float tanfovy, float3 p, const real c[6],
                                           const PartialSum& ps, float gcov[6], float gm3[3], float gm2[2],
                                           float sx_first = 0.f, float sy_first = 0.f, float* gm2_first = nullptr, float gz = 0.f,
                                           const float* c32 = nullptr, float o_s = 0.f, float* c_out = nullptr, ChainTerms* ct = nullptr) {
  // The frustum clamp is the forward's decision: the fp32 view-space position, txtz / tytz and limit, with the forward's operations in its
  // order (both files build with contraction off, so these are its bits).  An fp64 txtz within ~1e-7 of the limit can fall on the other
  // side, and then dtx / dty would be dropped or added in full.  A clamped coordinate sits at the forward's fp32 limit, widened.
  const float pvx32 = view[0] * p.x + view[4] * p.y + view[8] * p.z + view[12];
  const float pvy32 = view[1] * p.x + view[5] * p.y + view[9] * p.z + view[13];
  const float pvz32 = view[2] * p.x + view[6] * p.y + view[10] * p.z + view[14];
  const float txtz32 = pvx32 / pvz32, tytz32 = pvy32 / pvz32;
  const float limx32 = 1.3f * tanfovx, limy32 = 1.3f * tanfovy;
  const bool xlo = txtz32 < -limx32, xhi = txtz32 > limx32, ylo = tytz32 < -limy32, yhi = tytz32 > limy32;
  // the rest of the chain in fp64: every operand widened
  const real pvx = (real)view[0] * (real)p.x + (real)view[4] * (real)p.y + (real)view[8] * (real)p.z + (real)view[12];
  const real pvy = (real)view[1] * (real)p.x + (real)view[5] * (real)p.y + (real)view[9] * (real)p.z + (real)view[13];
  const real pvz = (real)view[2] * (real)p.x + (real)view[6] * (real)p.y + (real)view[10] * (real)p.z + (real)view[14];
  const real fx = (real)W / (2.0f * (real)tanfovx), fy = (real)H / (2.0f * (real)tanfovy);
  const real tz = pvz;
  const real txtz = pvx / tz, tytz = pvy / tz;
  const real xm = (xlo || xhi) ? 0.f : 1.f;
  const real ym = (ylo || yhi) ? 0.f : 1.f;
  const real tx = (xlo ? -(real)limx32 : (xhi ? (real)limx32 : txtz)) * tz, ty = (ylo ? -(real)limy32 : (yhi ? (real)limy32 : tytz)) * tz;
  const real J00 = fx / tz, J02 = -(fx * tx) / (tz * tz), J11 = fy / tz, J12 = -(fy * ty) / (tz * tz);
  const real T0[3] = {J00 * view[0] + J02 * view[2], J00 * view[4] + J02 * view[6], J00 * view[8] + J02 * view[10]};
  const real T1[3] = {J11 * view[1] + J12 * view[2], J11 * view[5] + J12 * view[6], J11 * view[9] + J12 * view[10]};
  const real S[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
  real U0[3], U1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    U0[k] = S[k][0] * T0[0] + S[k][1] * T0[1] + S[k][2] * T0[2];
    U1[k] = S[k][0] * T1[0] + S[k][1] * T1[1] + S[k][2] * T1[2];
  }
  const real a = U0[0] * T0[0] + U0[1] * T0[1] + U0[2] * T0[2] + 0.3f;
  const real b = U0[0] * T1[0] + U0[1] * T1[1] + U0[2] * T1[2];
  const real cc = U1[0] * T1[0] + U1[1] * T1[1] + U1[2] * T1[2] + 0.3f;
  const real det = a * cc - b * b;
  const real d2inv = 1.0f / (det * det + 0.0000001f);
  const real gA = ps.gA, gB = ps.gB, gC = ps.gC;
  const real dL_da0 = d2inv * (-cc * cc * gA + b * cc * gB - b * b * gC);
  const real dL_dc0 = d2inv * (-b * b * gA + a * b * gB - a * a * gC);
  const real dL_db0 = d2inv * (2.0f * b * cc * gA - (det + 2.0f * b * b) * gB + 2.0f * a * b * gC);
  real aa_a = 0.0, aa_b = 0.0, aa_c = 0.0;
  if (AA) {
    // The floor decision is the forward's (fp32 r, its operations).  Floored: c is a constant, dL/do = c g and no covariance term.
    // Otherwise, with A, C the undilated diagonal (a = A + h, cc = C + h), D = det and r = (A C - b^2) / D, the cancellation-free
    //   dr/dA = h (C^2 + h C + b^2) / D^2,  dr/dC = h (A^2 + h A + b^2) / D^2,  dr/db = -2 h b (A + C + h) / D^2
    // and o dc = o dr / (2 c); o = o' / c32 (the forward's c: o' = fl(o c32)).
    const float r32 = aa_ratio32(view, W, H, tanfovx, tanfovy, pvz32, txtz32, tytz32, c32);
    const float cf = gsr_aa_comp(r32);
    if (r32 < GSR_AA_FLOOR) {
      *c_out = cf;
    } else {
      const real h = (real)0.3f;
      const real A = U0[0] * T0[0] + U0[1] * T0[1] + U0[2] * T0[2];
      const real C = U1[0] * T1[0] + U1[1] * T1[1] + U1[2] * T1[2];
      const real cr = sqrt(fmax((A * C - b * b) / det, (real)GSR_AA_FLOOR));
      *c_out = (float)cr;
      const real k = (real)o_s / (real)cf * (real)ps.gop / (2.0 * cr * det * det);
      aa_a = k * h * (C * C + h * C + b * b);
      aa_c = k * h * (A * A + h * A + b * b);
      aa_b = -2.0 * k * h * b * (A + C + h);
    }
  }
  const real dL_da = AA ? dL_da0 + aa_a : dL_da0;
  const real dL_dc = AA ? dL_dc0 + aa_c : dL_dc0;
  const real dL_db = AA ? dL_db0 + aa_b : dL_db0;
  gcov[0] += (float)(T0[0] * T0[0] * dL_da + T0[0] * T1[0] * dL_db + T1[0] * T1[0] * dL_dc);
  gcov[3] += (float)(T0[1] * T0[1] * dL_da + T0[1] * T1[1] * dL_db + T1[1] * T1[1] * dL_dc);
  gcov[5] += (float)(T0[2] * T0[2] * dL_da + T0[2] * T1[2] * dL_db + T1[2] * T1[2] * dL_dc);
  gcov[1] += (float)(2.0f * T0[0] * T0[1] * dL_da + (T0[0] * T1[1] + T0[1] * T1[0]) * dL_db + 2.0f * T1[0] * T1[1] * dL_dc);
  gcov[2] += (float)(2.0f * T0[0] * T0[2] * dL_da + (T0[0] * T1[2] + T0[2] * T1[0]) * dL_db + 2.0f * T1[0] * T1[2] * dL_dc);
  gcov[4] += (float)(2.0f * T0[1] * T0[2] * dL_da + (T0[1] * T1[2] + T0[2] * T1[1]) * dL_db + 2.0f * T1[1] * T1[2] * dL_dc);
  real dT0[3], dT1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    dT0[j] = 2.0f * U0[j] * dL_da + U1[j] * dL_db;
    dT1[j] = 2.0f * U1[j] * dL_dc + U0[j] * dL_db;
  }
  const real dJ00 = dT0[0] * view[0] + dT0[1] * view[4] + dT0[2] * view[8];
  const real dJ02 = dT0[0] * view[2] + dT0[1] * view[6] + dT0[2] * view[10];
  const real dJ11 = dT1[0] * view[1] + dT1[1] * view[5] + dT1[2] * view[9];
  const real dJ12 = dT1[0] * view[2] + dT1[1] * view[6] + dT1[2] * view[10];
  const real itz = 1.0f / tz, itz2 = itz * itz, itz3 = itz2 * itz;
  const real dtx = xm * -fx * itz2 * dJ02;
  const real dty = ym * -fy * itz2 * dJ12;
  real dtz = -fx * itz2 * dJ00 - fy * itz2 * dJ11 + (2.0f * fx * tx) * itz3 * dJ02 + (2.0f * fy * ty) * itz3 * dJ12;
  if (DEPTH) dtz += (real)gz;
  // the blend backward hands over the raw sums of t*dx and t*dy (ps.gmx, ps.gmy); with the conic
  // (A, B, C) = (cc, -b, a) / det:  d/d mean2D.x = -(A sx + B sy),  d/d mean2D.y = -(C sy + B sx)
  const real det_inv = 1.0f / det;
  const real cA = cc * det_inv, cB = -b * det_inv, cC = a * det_inv;
  const real m2x = -(cA * ps.gmx + cB * ps.gmy) * 0.5f * (real)W;
  gm2[0] = (float)m2x;
  const real m2y = -(cC * ps.gmy + cB * ps.gmx) * 0.5f * (real)H;
  gm2[1] = (float)m2y;
  if (gm2_first) {   // fused pair: the share of the first view of the pair (ps.gmx / gmy are the sums over both)
    gm2_first[0] = (float)(-(cA * sx_first + cB * sy_first) * 0.5f * (real)W);
    gm2_first[1] = (float)(-(cC * sy_first + cB * sx_first) * 0.5f * (real)H);
  }
  const real hx = (real)proj[0] * (real)p.x + (real)proj[4] * (real)p.y + (real)proj[8] * (real)p.z + (real)proj[12];
  const real hy = (real)proj[1] * (real)p.x + (real)proj[5] * (real)p.y + (real)proj[9] * (real)p.z + (real)proj[13];
  const real hw = (real)proj[3] * (real)p.x + (real)proj[7] * (real)p.y + (real)proj[11] * (real)p.z + (real)proj[15];
  const real mw = 1.0f / (hw + 0.0000001f);
  const real mul1 = hx * mw * mw, mul2 = hy * mw * mw;
  gm3[0] += (float)(view[0] * dtx + view[1] * dty + view[2] * dtz + (proj[0] * mw - proj[3] * mul1) * m2x + (proj[1] * mw - proj[3] * mul2) * m2y);
  gm3[1] += (float)(view[4] * dtx + view[5] * dty + view[6] * dtz + (proj[4] * mw - proj[7] * mul1) * m2x + (proj[5] * mw - proj[7] * mul2) * m2y);
  gm3[2] += (float)(view[8] * dtx + view[9] * dty + view[10] * dtz + (proj[8] * mw - proj[11] * mul1) * m2x + (proj[9] * mw - proj[11] * mul2) * m2y);
  if (CAM) {
    ct->dt[0] = dtx; ct->dt[1] = dty; ct->dt[2] = dtz;
#pragma unroll
    for (int j = 0; j < 3; ++j) { ct->dT0[j] = dT0[j]; ct->dT1[j] = dT1[j]; }
    ct->J00 = J00; ct->J02 = J02; ct->J11 = J11; ct->J12 = J12;
    ct->m2x = m2x; ct->m2y = m2y; ct->hx = hx; ct->hy = hy; ct->mw = mw;
  }
}

// dL/dcov3D -> dL/dscale, dL/drotation (linear in gcov: in the multi-view kernel it runs once on the sum).
__device__ __forceinline__ void cov3_to_scale_rot(const Cov3& cv, float mod, const float gcov[6], float gs[3], float gq[4]) {
  const real dS[3][3] = {{(real)gcov[0], 0.5f * (real)gcov[1], 0.5f * (real)gcov[2]},
                          {0.5f * (real)gcov[1], (real)gcov[3], 0.5f * (real)gcov[4]},
                          {0.5f * (real)gcov[2], 0.5f * (real)gcov[4], (real)gcov[5]}};
  real G[3][3];
#pragma unroll
  for (int jj = 0; jj < 3; ++jj) {
    const real dM0 = 2.0f * (dS[0][0] * cv.R[0][jj] + dS[0][1] * cv.R[1][jj] + dS[0][2] * cv.R[2][jj]) * cv.s[jj];
    const real dM1 = 2.0f * (dS[1][0] * cv.R[0][jj] + dS[1][1] * cv.R[1][jj] + dS[1][2] * cv.R[2][jj]) * cv.s[jj];
    const real dM2 = 2.0f * (dS[2][0] * cv.R[0][jj] + dS[2][1] * cv.R[1][jj] + dS[2][2] * cv.R[2][jj]) * cv.s[jj];
    gs[jj] = (float)((real)mod * (cv.R[0][jj] * dM0 + cv.R[1][jj] * dM1 + cv.R[2][jj] * dM2));
    G[0][jj] = dM0 * cv.s[jj]; G[1][jj] = dM1 * cv.s[jj]; G[2][jj] = dM2 * cv.s[jj];
  }
  const real r = cv.q[0], x = cv.q[1], y = cv.q[2], z = cv.q[3];
  gq[0] = (float)(2.0f * (-z * G[0][1] + y * G[0][2] + z * G[1][0] - x * G[1][2] - y * G[2][0] + x * G[2][1]));
  gq[1] = (float)(2.0f * (y * G[0][1] + z * G[0][2] + y * G[1][0] - 2.0f * x * G[1][1] - r * G[1][2] + z * G[2][0] + r * G[2][1] - 2.0f * x * G[2][2]));
  gq[2] = (float)(2.0f * (-2.0f * y * G[0][0] + x * G[0][1] + r * G[0][2] + x * G[1][0] + z * G[1][2] - r * G[2][0] + z * G[2][1] - 2.0f * y * G[2][2]));
  gq[3] = (float)(2.0f * (-2.0f * z * G[0][0] - r * G[0][1] + x * G[0][2] + r * G[1][0] - 2.0f * z * G[1][1] + y * G[1][2] + x * G[2][0] + y * G[2][1]));
}

// The tracking forward marks the Gaussians some pixel of the view blended (GeomState::used; trusted when the view's `tracked` word is
// set): the records of the others are all zeros -- 45 % of a benchmark view's entries -- and so is everything the chain rule would make
// of them (exact zeros: every term carries a factor from the records): skipped.
__device__ __forceinline__ bool gsr_view_used(const GsrBwdView& w, int i) {
  return !w.used || !w.tracked || *w.tracked == 0u || w.used[i] != 0;
}

// The three kernels are written once (gsr_preprocess_bwd_kernels.inc) and compiled four times: GSR_PBWD_DEPTH 0 gives the kernels of
// gsr_backward / gsr_backward_batch, 1 their differentiable-depth builds (*_depth_kernel: one more argument, the per-entry dL/dz);
// GSR_PBWD_AA 1 the anti-aliasing builds of both (*_aa_kernel, *_aa_depth_kernel: one more argument, the staged records).
#define GSR_PBWD_AA 0
#define GSR_PBWD_DEPTH 0
#include "gsr_preprocess_bwd_kernels.inc"
#undef GSR_PBWD_DEPTH
#define GSR_PBWD_DEPTH 1
#include "gsr_preprocess_bwd_kernels.inc"
#undef GSR_PBWD_DEPTH
#undef GSR_PBWD_AA
#define GSR_PBWD_AA 1
#define GSR_PBWD_DEPTH 0
#include "gsr_preprocess_bwd_kernels.inc"
#undef GSR_PBWD_DEPTH
#define GSR_PBWD_DEPTH 1
#include "gsr_preprocess_bwd_kernels.inc"
#undef GSR_PBWD_DEPTH
#undef GSR_PBWD_AA

// the camera pass: camera_bwd_kernel<USE_SH, AA>, camera_reduce_kernel
#include "gsr_camera_bwd.inc"

}  // namespace gsr_preprocess_bwd
using namespace gsr_preprocess_bwd;

int gsr_launch_preprocess_bwd(const GsrCam& cam, int P, const float* means3D, const float* scales,
                              const float* rotations, const float* colors_precomp, const float* shs,
                              const float* cov3D_precomp, const int32_t* radii, const GeomState& g,
                              const float4* partials, float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dcolors,
                              float* dL_dopacity, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                              float* dL_dsh, const uint32_t* bwd_error, hipStream_t st, const float* dL_dz) {
  if (P <= 0) return 0;
  const dim3 grid((P + GSR_BLOCK - 1) / GSR_BLOCK), block(GSR_BLOCK);
#define GSR_PBWD_ARGS                                                                                              \
  P, cam.W, cam.H, cam.tanfovx, cam.tanfovy, cam.scale_modifier, cam.sh_degree, cam.M, cam.view, cam.proj,       \
      cam.campos, means3D, scales, rotations, colors_precomp, shs, cov3D_precomp, radii, g.offsets, g.clamped,  \
      partials, dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, dL_dsh, g.used, g.counters + 1, bwd_error
  if (shs && !dL_dsh) { gsr_set_error("gsr_backward: shs given but dL_dsh is NULL"); return -2; }
  if (cam.antialiasing) {   // anti-aliasing builds: one more argument, the forward's records (staged o')
    { GSR_PROF(dL_dz ? "preprocess_bwd_aa_depth" : "preprocess_bwd_aa", st);
      if (dL_dz && shs) hipLaunchKernelGGL(preprocess_bwd_aa_depth_kernel<true>, grid, block, 0, st, GSR_PBWD_ARGS, dL_dz, g.rec);
      else if (dL_dz) hipLaunchKernelGGL(preprocess_bwd_aa_depth_kernel<false>, grid, block, 0, st, GSR_PBWD_ARGS, dL_dz, g.rec);
      else if (shs) hipLaunchKernelGGL(preprocess_bwd_aa_kernel<true>, grid, block, 0, st, GSR_PBWD_ARGS, g.rec);
      else hipLaunchKernelGGL(preprocess_bwd_aa_kernel<false>, grid, block, 0, st, GSR_PBWD_ARGS, g.rec); }
  } else if (dL_dz) {   // differentiable depth (gsr_backward_depth)
    { GSR_PROF("preprocess_bwd_depth", st);
      if (shs) hipLaunchKernelGGL(preprocess_bwd_depth_kernel<true>, grid, block, 0, st, GSR_PBWD_ARGS, dL_dz);
      else hipLaunchKernelGGL(preprocess_bwd_depth_kernel<false>, grid, block, 0, st, GSR_PBWD_ARGS, dL_dz); }
  } else if (shs) {
    { GSR_PROF("preprocess_bwd", st);
  hipLaunchKernelGGL(preprocess_bwd_kernel<true>, grid, block, 0, st, GSR_PBWD_ARGS); }
  } else {
    { GSR_PROF("preprocess_bwd", st);
  hipLaunchKernelGGL(preprocess_bwd_kernel<false>, grid, block, 0, st, GSR_PBWD_ARGS); }
  }
#undef GSR_PBWD_ARGS
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

int gsr_launch_preprocess_bwd_views(const GsrBwdViews& vw, int P, float scale_modifier, const float* means3D,
                                    const float* scales, const float* rotations, const float* cov3D_precomp,
                                    float* dL_dmeans3D, float* dL_dcolors, float* dL_dopacity, float* dL_dscales,
                                    float* dL_drotations, float* dL_dcov3D, hipStream_t st, const GsrDepthViews* depth, const GsrAaViews* aa) {
  if (P <= 0) return 0;
  int nact = 0;
  for (int v = 0; v < vw.V; ++v) nact += vw.v[v].fused_alias ? 0 : 1;
  if (aa) {   // anti-aliasing builds: the same launch shapes, one more argument (the views' records)
    GSR_PROF("preprocess_bwd_views_aa", st);
    const GsrAaViews& a = *aa;
    if (nact >= 2) {
#define PBW_AA_LAUNCH(K, MAXW, ...) hipLaunchKernelGGL(K<MAXW>, dim3((P + 63) / 64), dim3(64 * nact),                                     \
                           sizeof(float) * (size_t)nact * (PBW_VALUES + 1) * 64, st, vw, P, scale_modifier, means3D, scales, rotations,       \
                           cov3D_precomp, dL_dmeans3D, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, __VA_ARGS__)
      if (depth) {
        if (nact <= 4) PBW_AA_LAUNCH(preprocess_bwd_views_waves_aa_depth_kernel, 4, *depth, a);
        else if (nact <= 8) PBW_AA_LAUNCH(preprocess_bwd_views_waves_aa_depth_kernel, 8, *depth, a);
        else PBW_AA_LAUNCH(preprocess_bwd_views_waves_aa_depth_kernel, GSR_MAX_BATCH, *depth, a);
      } else if (nact <= 4) PBW_AA_LAUNCH(preprocess_bwd_views_waves_aa_kernel, 4, a);
      else if (nact <= 8) PBW_AA_LAUNCH(preprocess_bwd_views_waves_aa_kernel, 8, a);
      else PBW_AA_LAUNCH(preprocess_bwd_views_waves_aa_kernel, GSR_MAX_BATCH, a);
#undef PBW_AA_LAUNCH
    } else if (depth) {
      hipLaunchKernelGGL(preprocess_bwd_views_aa_depth_kernel, dim3((P + GSR_BLOCK - 1) / GSR_BLOCK), dim3(GSR_BLOCK), 0, st, vw, P,
                         scale_modifier, means3D, scales, rotations, cov3D_precomp, dL_dmeans3D, dL_dcolors, dL_dopacity,
                         dL_dscales, dL_drotations, dL_dcov3D, *depth, a);
    } else {
      hipLaunchKernelGGL(preprocess_bwd_views_aa_kernel, dim3((P + GSR_BLOCK - 1) / GSR_BLOCK), dim3(GSR_BLOCK), 0, st, vw, P,
                         scale_modifier, means3D, scales, rotations, cov3D_precomp, dL_dmeans3D, dL_dcolors, dL_dopacity,
                         dL_dscales, dL_drotations, dL_dcov3D, a);
    }
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
  }
  if (nact >= 2) {      // one wave per view
    { GSR_PROF("preprocess_bwd_views", st);
#define PBW_LAUNCH(MAXW) hipLaunchKernelGGL(preprocess_bwd_views_waves_kernel<MAXW>, dim3((P + 63) / 64), dim3(64 * nact),              \
                           sizeof(float) * (size_t)nact * (PBW_VALUES + 1) * 64, st, vw, P, scale_modifier, means3D, scales, rotations,       \
                           cov3D_precomp, dL_dmeans3D, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D)
#define PBW_LAUNCH_DEPTH(MAXW) hipLaunchKernelGGL(preprocess_bwd_views_waves_depth_kernel<MAXW>, dim3((P + 63) / 64), dim3(64 * nact),  \
                           sizeof(float) * (size_t)nact * (PBW_VALUES + 1) * 64, st, vw, P, scale_modifier, means3D, scales, rotations,       \
                           cov3D_precomp, dL_dmeans3D, dL_dcolors, dL_dopacity, dL_dscales, dL_drotations, dL_dcov3D, *depth)
      if (depth) { if (nact <= 4) PBW_LAUNCH_DEPTH(4); else if (nact <= 8) PBW_LAUNCH_DEPTH(8); else PBW_LAUNCH_DEPTH(GSR_MAX_BATCH); }
      else if (nact <= 4) PBW_LAUNCH(4); else if (nact <= 8) PBW_LAUNCH(8); else PBW_LAUNCH(GSR_MAX_BATCH);
#undef PBW_LAUNCH
#undef PBW_LAUNCH_DEPTH
    }
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
  }
  if (depth) {
    GSR_PROF("preprocess_bwd_views", st);
    hipLaunchKernelGGL(preprocess_bwd_views_depth_kernel, dim3((P + GSR_BLOCK - 1) / GSR_BLOCK), dim3(GSR_BLOCK), 0, st, vw, P,
                       scale_modifier, means3D, scales, rotations, cov3D_precomp, dL_dmeans3D, dL_dcolors, dL_dopacity,
                       dL_dscales, dL_drotations, dL_dcov3D, *depth);
  } else { GSR_PROF("preprocess_bwd_views", st);
    hipLaunchKernelGGL(preprocess_bwd_views_kernel, dim3((P + GSR_BLOCK - 1) / GSR_BLOCK), dim3(GSR_BLOCK), 0, st, vw, P,
                       scale_modifier, means3D, scales, rotations, cov3D_precomp, dL_dmeans3D, dL_dcolors, dL_dopacity,
                       dL_dscales, dL_drotations, dL_dcov3D); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

int gsr_launch_camera_bwd(const GsrCamViews& cv, bool antialiasing, hipStream_t st) {
  if (cv.V <= 0) return 0;
  {
    GSR_PROF("camera_bwd", st);
    const dim3 grid(cv.nblk, cv.V), block(GSR_BLOCK);
    if (cv.shs && antialiasing) hipLaunchKernelGGL((camera_bwd_kernel<true, true>), grid, block, 0, st, cv);
    else if (cv.shs) hipLaunchKernelGGL((camera_bwd_kernel<true, false>), grid, block, 0, st, cv);
    else if (antialiasing) hipLaunchKernelGGL((camera_bwd_kernel<false, true>), grid, block, 0, st, cv);
    else hipLaunchKernelGGL((camera_bwd_kernel<false, false>), grid, block, 0, st, cv);
  }
  GSR_HIP_CHECK(hipGetLastError());
  {
    GSR_PROF("camera_reduce", st);
    hipLaunchKernelGGL(camera_reduce_kernel, dim3(cv.V), dim3(GSR_BLOCK), 0, st, cv);
  }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}
