// gsr_preprocess_fwd.hip -- per-Gaussian forward preprocess for gfx950 (replaces the reference
// extension's preprocess stage).  One lane per Gaussian.
//
// THIS FILE IS COMPILED WITH -ffp-contract=off: every fp32 op is separately rounded, in the same
// order as oracle/gsr_oracle.c::preprocess_one, so radii / tile rects / depth keys are bit-identical
// to the CPU oracle (integer parity is exact, not "within tolerance").
//
// HBM traffic per Gaussian: reads 12 (mean) + 12 (scale) + 16 (rot) + 4 (opacity) + 12 (colour) = 56 B
// (+48 M-coefficient SH when used), writes 48 (record) + 8 (rect) + 4 (tiles) + 4 (clamp) + 4 (radii) = 68 B.
// The 4x4 matrices are read through uniform (scalar) loads: they never occupy VGPRs.
#include "gsr_common.h"
#include "gsr_sh.h"

// kernels live in a NAMED namespace: profilers and traces show gsr_preprocess_fwd::<kernel>, not "(anonymous namespace)"
namespace gsr_preprocess_fwd {

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ void sh_to_rgb(int deg, int M, const float* __restrict__ sh, float3 p,
                                          const float* __restrict__ campos, float out[3], uint32_t& clamped) {
  float dx = p.x - campos[0], dy = p.y - campos[1], dz = p.z - campos[2];
  float len = sqrtf(dx * dx + dy * dy + dz * dz);
  float inv = 1.0f / len;
  float x = dx * inv, y = dy * inv, z = dz * inv;
  clamped = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
#define S(k) sh[(k)*3 + ch]
    float r = SH_C0 * S(0);
    if (deg > 0) {
      r = r - SH_C1 * y * S(1) + SH_C1 * z * S(2) - SH_C1 * x * S(3);
      if (deg > 1) {
        float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        r = r + kC2[0] * xy * S(4) + kC2[1] * yz * S(5) + kC2[2] * (2.0f * zz - xx - yy) * S(6) +
            kC2[3] * xz * S(7) + kC2[4] * (xx - yy) * S(8);
        if (deg > 2) {
          r = r + kC3[0] * y * (3.0f * xx - yy) * S(9) + kC3[1] * xy * z * S(10) +
              kC3[2] * y * (4.0f * zz - xx - yy) * S(11) +
              kC3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * S(12) +
              kC3[4] * x * (4.0f * zz - xx - yy) * S(13) + kC3[5] * z * (xx - yy) * S(14) +
              kC3[6] * x * (xx - 3.0f * yy) * S(15);
        }
      }
    }
#undef S
    r += 0.5f;
    if (r < 0.0f) { clamped |= (1u << ch); r = 0.0f; }
    out[ch] = r;
  }
  (void)M;
}

__device__ __forceinline__ int sext16_(uint32_t v) { return (int)(int16_t)(v & 0xffffu); }

// What the rest of a launch needs to know about one preprocessed Gaussian (everything else went to memory).
struct PreOut { uint32_t tiles; uint2 rc; uint32_t tmask; uint32_t depth_bits;
                bool differs; };          // compare mode (GsrPreView::cmp_rec): something the tile lists or the blend decisions depend on is not
                                          // bit-equal to the compared geometry state's (entry count, tile rect, tile mask, depth bits, 2D mean, conic, opacity)

// One Gaussian of one view: cull, project, covariance, conic, radius, rect / alpha box / tile mask, colour; every per-Gaussian output
// stored.  `i` may be out of range (in_range = false: nothing loaded, nothing stored, an empty result).
// AA (anti-aliasing): the staged opacity -- and with it the alpha box and the tight lists -- is o * c
// (gsr_aa_comp); conic, radius, rect, depth and radii are the dilated covariance's either way.
template <bool AA>
__device__ __forceinline__ PreOut preprocess_gaussian(
    const GsrPreViews& tab, const GsrPreView& vw, const int i, const int P, float4* __restrict__ s_rec, const bool write_act, int W, int H, int gx, int gy,
    float mod, int sh_degree, int M,
    const float* __restrict__ means3D, const float* __restrict__ scales, const float* __restrict__ rotations,
    const float* __restrict__ opacities, const float* __restrict__ colors_precomp,
    const float* __restrict__ shs, const float* __restrict__ cov3D_precomp, int tight_lists) {
  const bool in_range = i < P;
  const float* __restrict__ view = vw.view;
  const float* __restrict__ proj = vw.proj;
  const float* __restrict__ campos = vw.campos;
  const float tanfovx = vw.tanfovx, tanfovy = vw.tanfovy;
  float4* __restrict__ rec = vw.rec;
  uint2* __restrict__ rect = vw.rect;
  uint32_t* __restrict__ tiles_touched = vw.tiles_touched;
  uint32_t* __restrict__ clamped_out = vw.clamped;
  int32_t* __restrict__ radii = vw.radii;
  // defaults for a culled Gaussian
  int32_t radius_i = 0;
  uint32_t tiles = 0;
  uint2 rc = make_uint2(0u, 0u);
  uint2 box = make_uint2(0x00000001u, 0x00000001u);  // empty: min = 1 > max = 0
  uint32_t tmask = 0u;
  float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f), b4 = a4;
  float2 c2 = make_float2(0.f, 0.f);
  uint32_t clamp_bits = 0;

  float3 p = make_float3(0.f, 0.f, 0.f);
  if (in_range) p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
  // raw-parameter mode: this Gaussian's activated rotation / scale / opacity are computed here (every view's block does, view 0's
  // writes them out for the backward and for the caller)
  float4 act_q = make_float4(1.f, 0.f, 0.f, 0.f);
  float act_s[3] = {0.f, 0.f, 0.f}, act_o = 0.f;
  const bool raw = tab.raw_rot != nullptr;
  if (raw && in_range) {
    act_q = gsr_act_rotation(reinterpret_cast<const float4*>(tab.raw_rot)[i]);
    act_o = gsr_act_opacity(tab.raw_op[i]);
#pragma unroll
    for (int k = 0; k < 3; ++k) act_s[k] = gsr_act_scale(tab.raw_sc[3 * (size_t)i + k]);
    if (write_act) {
      reinterpret_cast<float4*>(tab.rot_out)[i] = act_q;
      tab.op_out[i] = act_o;
#pragma unroll
      for (int k = 0; k < 3; ++k) tab.sc_out[3 * (size_t)i + k] = act_s[k];
    }
  }
  float pvx = view[0] * p.x + view[4] * p.y + view[8] * p.z + view[12];
  float pvy = view[1] * p.x + view[5] * p.y + view[9] * p.z + view[13];
  float pvz = view[2] * p.x + view[6] * p.y + view[10] * p.z + view[14];
  if (in_range && pvz > GSR_NEAR_Z) {
    float hx = proj[0] * p.x + proj[4] * p.y + proj[8] * p.z + proj[12];
    float hy = proj[1] * p.x + proj[5] * p.y + proj[9] * p.z + proj[13];
    float hw = proj[3] * p.x + proj[7] * p.y + proj[11] * p.z + proj[15];
    float pw = 1.0f / (hw + 0.0000001f);
    float ndcx = hx * pw, ndcy = hy * pw;
    // 3D covariance
    float c0, c1, c2_, c3, c4, c5;
    if (cov3D_precomp) {
      c0 = cov3D_precomp[6 * i]; c1 = cov3D_precomp[6 * i + 1]; c2_ = cov3D_precomp[6 * i + 2];
      c3 = cov3D_precomp[6 * i + 3]; c4 = cov3D_precomp[6 * i + 4]; c5 = cov3D_precomp[6 * i + 5];
    } else {
      float r, x, y, z;
      if (raw) { r = act_q.x; x = act_q.y; y = act_q.z; z = act_q.w; }
      else { r = rotations[4 * i]; x = rotations[4 * i + 1]; y = rotations[4 * i + 2]; z = rotations[4 * i + 3]; }
      float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
      float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
      float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
      float s0, s1, s2;
      if (raw) { s0 = mod * act_s[0]; s1 = mod * act_s[1]; s2 = mod * act_s[2]; }
      else { s0 = mod * scales[3 * i]; s1 = mod * scales[3 * i + 1]; s2 = mod * scales[3 * i + 2]; }
      float M00 = R00 * s0, M01 = R01 * s1, M02 = R02 * s2;
      float M10 = R10 * s0, M11 = R11 * s1, M12 = R12 * s2;
      float M20 = R20 * s0, M21 = R21 * s1, M22 = R22 * s2;
      c0 = M00 * M00 + M01 * M01 + M02 * M02;
      c1 = M00 * M10 + M01 * M11 + M02 * M12;
      c2_ = M00 * M20 + M01 * M21 + M02 * M22;
      c3 = M10 * M10 + M11 * M11 + M12 * M12;
      c4 = M10 * M20 + M11 * M21 + M12 * M22;
      c5 = M20 * M20 + M21 * M21 + M22 * M22;
    }
    // EWA projection with the frustum clamp
    float fx = (float)W / (2.0f * tanfovx), fy = (float)H / (2.0f * tanfovy);
    float limx = 1.3f * tanfovx, limy = 1.3f * tanfovy;
    float tz = pvz;
    float txtz = pvx / tz, tytz = pvy / tz;
    float tx = clampf(txtz, -limx, limx) * tz;
    float ty = clampf(tytz, -limy, limy) * tz;
    float J00 = fx / tz, J02 = -(fx * tx) / (tz * tz);
    float J11 = fy / tz, J12 = -(fy * ty) / (tz * tz);
    float T00 = J00 * view[0] + J02 * view[2], T01 = J00 * view[4] + J02 * view[6], T02 = J00 * view[8] + J02 * view[10];
    float T10 = J11 * view[1] + J12 * view[2], T11 = J11 * view[5] + J12 * view[6], T12 = J11 * view[9] + J12 * view[10];
    float U00 = T00 * c0 + T01 * c1 + T02 * c2_, U01 = T00 * c1 + T01 * c3 + T02 * c4, U02 = T00 * c2_ + T01 * c4 + T02 * c5;
    float U10 = T10 * c0 + T11 * c1 + T12 * c2_, U11 = T10 * c1 + T11 * c3 + T12 * c4, U12 = T10 * c2_ + T11 * c4 + T12 * c5;
    float a = U00 * T00 + U01 * T01 + U02 * T02;
    float b = U00 * T10 + U01 * T11 + U02 * T12;
    float cc = U10 * T10 + U11 * T11 + U12 * T12;
    const float a0 = a, c0_ = cc;   // before the dilation (AA)
    a += 0.3f; cc += 0.3f;
    float det = a * cc - b * b;
    if (det != 0.0f) {
      float det_inv = 1.0f / det;
      float cA = cc * det_inv, cB = -b * det_inv, cC = a * det_inv;
      float mid = 0.5f * (a + cc);
      float disc = mid * mid - det;
      float sq = sqrtf(disc > 0.1f ? disc : 0.1f);
      float l1 = mid + sq, l2 = mid - sq;
      float radius = ceilf(3.0f * sqrtf(l1 > l2 ? l1 : l2));
      float px = ((ndcx + 1.0f) * (float)W - 1.0f) * 0.5f;
      float py = ((ndcy + 1.0f) * (float)H - 1.0f) * 0.5f;
      int minx = min(gx, max(0, (int)((px - radius) / (float)GSR_TILE)));
      int miny = min(gy, max(0, (int)((py - radius) / (float)GSR_TILE)));
      int maxx = min(gx, max(0, (int)((px + radius + (float)(GSR_TILE - 1)) / (float)GSR_TILE)));
      int maxy = min(gy, max(0, (int)((py + radius + (float)(GSR_TILE - 1)) / (float)GSR_TILE)));
      int area = (maxx - minx) * (maxy - miny);
      if (area != 0) {
        float rgb[3];
        if (colors_precomp) {
          rgb[0] = colors_precomp[3 * i]; rgb[1] = colors_precomp[3 * i + 1]; rgb[2] = colors_precomp[3 * i + 2];
        } else {
          sh_to_rgb(sh_degree, M, shs + (size_t)i * M * 3, p, campos, rgb, clamp_bits);
        }
        radius_i = (int32_t)radius;
        tiles = (uint32_t)area;
        rc = make_uint2((uint32_t)minx | ((uint32_t)miny << 16), (uint32_t)maxx | ((uint32_t)maxy << 16));
        // Conservative pixel box of {alpha >= 1/255}: the ellipse d^T Sigma^-1 d <= 2 ln(255 o) has half-extents
        // sqrt(2 ln(255 o) * Sigma_xx), sqrt(.. * Sigma_yy).  The +0.02 on the log (2 % slack on alpha) and the
        // outward rounding make it safe against any fp32 difference with the per-pixel evaluation; pixels
        // outside the box would be skipped by the alpha test anyway, so using it cannot change a result.
        const float opac = AA ? (raw ? act_o : opacities[i]) * gsr_aa_comp(gsr_aa_ratio(a0, b, c0_, det))
                              : (raw ? act_o : opacities[i]);
        const float tau2 = 2.0f * (__logf(255.0f * opac) + 0.02f);
        if (tau2 > 0.0f) {
          const float hx = sqrtf(tau2 * a) + 0.01f, hy = sqrtf(tau2 * cc) + 0.01f;
          const int xmin = max(-32768, min(32767, (int)floorf(px - hx)));
          const int xmax = max(-32768, min(32767, (int)ceilf(px + hx)));
          const int ymin = max(-32768, min(32767, (int)floorf(py - hy)));
          const int ymax = max(-32768, min(32767, (int)ceilf(py + hy)));
          box = make_uint2(((uint32_t)xmin & 0xffffu) | ((uint32_t)xmax << 16),
                           ((uint32_t)ymin & 0xffffu) | ((uint32_t)ymax << 16));
        }
        // tile mask of the reference's rect: all of its tiles (a rect of more than 32 tiles is taken whole anyway)
        tmask = tiles >= 32u ? 0xffffffffu : ((1u << tiles) - 1u);
        if (tight_lists) {
          // Tile lists from the alpha box instead of the 3-sigma rect: a (Gaussian, tile) pair outside the
          // box fails the alpha test at every pixel of the tile, so dropping it from the lists changes no
          // pixel and no gradient -- it only shortens the sort and the per-tile walks.  radii keep the
          // reference's 3-sigma value.  (GSR_REFERENCE_LISTS=1 restores the reference's duplicates.)
          const int bx0 = sext16_(box.x) >> 4, bx1 = (sext16_(box.x >> 16) >> 4) + 1;
          const int by0 = sext16_(box.y) >> 4, by1 = (sext16_(box.y >> 16) >> 4) + 1;
          const int tx0 = max(minx, bx0), tx1 = min(maxx, bx1), ty0 = max(miny, by0), ty1 = min(maxy, by1);
          if (tau2 > 0.0f && tx0 < tx1 && ty0 < ty1) {
            tiles = (uint32_t)((tx1 - tx0) * (ty1 - ty0));
            rc = make_uint2((uint32_t)tx0 | ((uint32_t)ty0 << 16), (uint32_t)tx1 | ((uint32_t)ty1 << 16));
#ifdef GSR_ABL_NO_TILE_TEST   /* ablation (tools/build_variant.sh): what the exact per-tile loop costs this kernel */
            if (false) {
#else
            if (tiles <= 32u) {
#endif
              // exact per-tile test: the ellipse {alpha >= 1/255} of an elongated diagonal Gaussian misses the corner
              // tiles of its box (16 % of the benchmark's remaining pairs).  One bit per tile of the rect, row-major.
              const float invA = 1.0f / cA, invC = 1.0f / cC;
              tmask = 0u;
              uint32_t bit = 1u;
              for (int Y = ty0 * GSR_TILE; Y < ty1 * GSR_TILE; Y += GSR_TILE)
                for (int X = tx0 * GSR_TILE; X < tx1 * GSR_TILE; X += GSR_TILE, bit <<= 1)
                  if (gsr_rect_reachable(px, py, cA, cB, cC, invA, invC, tau2 + 0.02f, X, Y, X + GSR_TILE - 1, Y + GSR_TILE - 1))
                    tmask |= bit;
              tiles = (uint32_t)__popc(tmask);
              if (tiles == 0u) rc = make_uint2(0u, 0u);
            }
          } else {
            tiles = 0; rc = make_uint2(0u, 0u);
          }
        }
        a4 = make_float4(px, py, cA, cB);
        b4 = make_float4(cC, opac, rgb[0], rgb[1]);
        c2 = make_float2(rgb[2], pvz);
      }
    }
  }
#ifndef GSR_PRE_LDS_STORE
#define GSR_PRE_LDS_STORE 1
#endif
#if GSR_PRE_LDS_STORE
  {
    // The 64 records of a wave are 4 KiB of CONTIGUOUS memory, but a lane holds one whole record: stored straight from the registers,
    // each of the four 16-byte stores touches a quarter of 64 different lines.  Transposed through the wave's LDS block instead, store k
    // writes the wave's k-th KiB -- whole lines.  Part p of lane l sits at float4 index 4 l + (p ^ ((l >> 1) & 3)): the XOR keeps both the
    // 8-lane groups of the 16-byte LDS writes and the 16-lane groups of the reads conflict-free.
    float4* __restrict__ R = s_rec;
    const int l = (int)(threadIdx.x & 63), sw = (l >> 1) & 3;
    R[4 * l + (0 ^ sw)] = a4;
    R[4 * l + (1 ^ sw)] = b4;
    R[4 * l + (2 ^ sw)] = make_float4(c2.x, c2.y, __uint_as_float(box.x), __uint_as_float(box.y));
    R[4 * l + (3 ^ sw)] = make_float4(__uint_as_float(rc.x), __uint_as_float(rc.y), 0.f, __uint_as_float(tmask));  // .z = offset (emit)
    const int i0 = i - l;                       // the wave's first Gaussian (wave-uniform)
    const int r = l >> 2, pp = l & 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int rr = 16 * k + r;                // record (lane of the wave) whose part pp this lane stores
      const float4 v = R[4 * rr + (pp ^ ((rr >> 1) & 3))];
      if (i0 + rr < P) rec[GSR_REC_F4 * (size_t)i0 + 64 * k + l] = v;
    }
  }
#endif
  if (in_range) {
#if !GSR_PRE_LDS_STORE
    rec[GSR_REC_F4 * i + 0] = a4;
    rec[GSR_REC_F4 * i + 1] = b4;
    rec[GSR_REC_F4 * i + 2] = make_float4(c2.x, c2.y, __uint_as_float(box.x), __uint_as_float(box.y));
    rec[GSR_REC_F4 * i + 3] = make_float4(__uint_as_float(rc.x), __uint_as_float(rc.y), 0.f, __uint_as_float(tmask));  // .z = offset (emit)
#endif
    rect[i] = rc;
    vw.ekey[i] = make_uint2(__float_as_uint(c2.y), tmask);
    tiles_touched[i] = tiles;
    clamped_out[i] = clamp_bits;
    radii[i] = radius_i;
    if (vw.used) vw.used[i] = 0;                  // set by the tracking forward when some pixel blends the Gaussian
    if (i == 0 && vw.tracked) *vw.tracked = 0u;   // ... which also says so here (a forward-only call leaves 0: the flags are then ignored)
  }
  PreOut o;
  o.tiles = tiles; o.rc = rc; o.tmask = tmask; o.depth_bits = __float_as_uint(c2.y);
  o.differs = false;
  if (in_range && vw.cmp_rec) {      // exact comparison with an earlier forward's geometry state (same P, same image size: the caller's business)
    bool d = vw.cmp_tiles[i] != tiles;
    if (!d && tiles) {
      const uint2 pr = vw.cmp_rect[i], pk = vw.cmp_ekey[i];
      const float4 pa = vw.cmp_rec[GSR_REC_F4 * (size_t)i], pb = vw.cmp_rec[GSR_REC_F4 * (size_t)i + 1];
      d = pr.x != rc.x || pr.y != rc.y || pk.x != __float_as_uint(c2.y) || pk.y != tmask ||
          __float_as_uint(pa.x) != __float_as_uint(a4.x) || __float_as_uint(pa.y) != __float_as_uint(a4.y) ||
          __float_as_uint(pa.z) != __float_as_uint(a4.z) || __float_as_uint(pa.w) != __float_as_uint(a4.w) ||
          __float_as_uint(pb.x) != __float_as_uint(b4.x) || __float_as_uint(pb.y) != __float_as_uint(b4.y);
    }
    o.differs = d;
  }
  return o;
}

// The preprocess kernel is written once (gsr_preprocess_fwd_kernel.inc) and compiled twice: GSR_PFWD_AA 0 gives preprocess_fwd_kernel,
// 1 its anti-aliasing build preprocess_fwd_aa_kernel (same arguments).
#define GSR_PFWD_AA 0
#include "gsr_preprocess_fwd_kernel.inc"
#undef GSR_PFWD_AA
#define GSR_PFWD_AA 1
#include "gsr_preprocess_fwd_kernel.inc"
#undef GSR_PFWD_AA

__global__ __launch_bounds__(GSR_BLOCK) void mark_visible_kernel(int P, const float* __restrict__ view,
                                                                 const float* __restrict__ means3D,
                                                                 uint8_t* __restrict__ present) {
  int i = blockIdx.x * GSR_BLOCK + threadIdx.x;
  if (i >= P) return;
  float z = view[2] * means3D[3 * i] + view[6] * means3D[3 * i + 1] + view[10] * means3D[3 * i + 2] + view[14];
  present[i] = z > GSR_NEAR_Z ? 1 : 0;
}

}  // namespace gsr_preprocess_fwd
using namespace gsr_preprocess_fwd;

int gsr_launch_preprocess(const GsrPreViews& tab, const GsrCam& cam, int P, const float* means3D, const float* scales,
                          const float* rotations, const float* opacities, const float* colors_precomp,
                          const float* shs, const float* cov3D_precomp, hipStream_t st) {
  if (P <= 0 || tab.V <= 0) return 0;
  int blocks = (P + GSR_BLOCK - 1) / GSR_BLOCK;
  const char* ref_lists = getenv("GSR_REFERENCE_LISTS");
  const int tight = (ref_lists && ref_lists[0] == '1') ? 0 : 1;
  { GSR_PROF("preprocess_fwd", st);
#define PFWD_LAUNCH(K) hipLaunchKernelGGL(K, dim3(blocks, tab.V), dim3(GSR_BLOCK), 0, st, tab, P, cam.W, cam.H, cam.gx, cam.gy,             \
                                          cam.scale_modifier, cam.sh_degree, cam.M, means3D, scales, rotations, opacities, colors_precomp, \
                                          shs, cov3D_precomp, tight)
  if (cam.antialiasing) PFWD_LAUNCH(preprocess_fwd_aa_kernel);
  else PFWD_LAUNCH(preprocess_fwd_kernel);
#undef PFWD_LAUNCH
  }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

int gsr_launch_mark_visible(const float* view, int P, const float* means3D, uint8_t* present, hipStream_t st) {
  if (P <= 0) return 0;
  int blocks = (P + GSR_BLOCK - 1) / GSR_BLOCK;
  { GSR_PROF("mark_visible", st);
  hipLaunchKernelGGL(mark_visible_kernel, dim3(blocks), dim3(GSR_BLOCK), 0, st, P, view, means3D, present); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}
