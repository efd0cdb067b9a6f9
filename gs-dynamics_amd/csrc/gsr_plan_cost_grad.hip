// gsr_plan_cost_grad.hip -- gsr_plan_cost (gsr_plan_cost.hip) and the gradient of its reward in ONE launch: the gradient planner's cost
// (gsdyn/plan.py ``running_cost_grad``; the reference's utils/planner.py ``trajectory_optimization_gd`` differentiates ``running_cost``).
//   reward, chamfer, collision, box_pen : the bits of gsr_plan_cost on the same inputs -- the value expressions and every association
//                                         order below are cost_kernel's, and this file is compiled with the same flags (contraction on);
//   g_state [B, T, n_obj, 3]            : d reward_b / d state_seqs[b];
//   g_actions [B, T, 4]                 : d reward_b / d actions[b], columns 2 and 3 (angle, length) written as zeros.
// The rule set (include/gsr.h states it in full): every minimum / maximum hands its gradient to ONE element, the LOWEST index among equal
// values, decided on the squared distance where the forward decides on it; a zero distance contributes a zero vector (torch.norm's
// subgradient), never a NaN; a sample whose reward is not finite gets NaN in all its gradient rows.
// No atomics of any kind.  Every output element is written by one thread as a fixed-order fp32 sum, so the outputs are bit-identical from
// run to run and a sample's rows depend neither on B nor on the sample's position in the batch.
#include "gsr_common.h"

namespace gsr_pcgrad {

#define PG_THREADS 256
#define PG_WAVES (PG_THREADS / 64)
#define PG_MAXN 1024            // particles of one sample held in LDS
#define PG_TILE 1024            // target points per LDS tile
#define PG_SLOTS (PG_MAXN / PG_THREADS)   // particles a thread owns: tid, tid + 256, ..

__device__ __forceinline__ float pg_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float pg_relu(float v) { return v < 0.0f ? 0.0f : v; }
// the smaller of two (value, index) pairs: a NaN below every number (the NaN-keeping minimum), the LOWER index among equals
__device__ __forceinline__ void pg_take(float& bv, int& bi, float v, int i) {
  const bool vn = v != v, bn = bv != bv;
  const bool below = vn ? !bn : (!bn && v < bv);
  const bool above = bn ? !vn : (!vn && bv < v);
  if (below || (!above && i < bi)) { bv = v; bi = i; }
}

// what thread 0 hands the workgroup after a frame's reductions: the one particle the next push's collision term reaches and the one
// particle the frame's active wall reaches, with their gradients (an index of -1: nobody)
struct FrameRec {
  int c_idx; float c_gx, c_gy;
  int b_idx, b_coord; float b_g;
};

// One workgroup per sample b; the structure is cost_kernel's.
//  (1) frames t = -1 .. T - 1: the five minima travel as (value, index) pairs through the wave butterfly and the four waves (a total
//      order: any tree gives the same pair).  Thread 0 forms collision[b, t + 1] and box_pen[b, t] exactly as cost_kernel does, then
//        collision: gate open iff d - pusher > 0; u = (start - particle) / d (zero at d = 0); g_actions[b, t + 1, 0:2] = (pw / T) s c u,
//                   the particle's xy in frame t receives the opposite (frame -1 is state_cur: no gradient);
//        box:       the active wall is the lowest index among the four that attains the maximum; margin > 0: (pw / T) s e to the x or y
//                   of the lowest-index particle at that wall's extreme, with the margin's sign in that coordinate.
//      The thread that owns particle n (n = tid, tid + 256, ..) writes frame t's row n: (0 + collision part) + box part.  The last
//      frame's box part waits in registers for the chamfer.
//  (2) chamfer of the last frame, tile by tile (1024 targets):
//        target -> particles: thread i owns the tile's points i, i + 256, ..: strict '<' over ascending n keeps the lowest n; the sum of
//                             roots as in cost_kernel.  After a barrier the thread overwrites ITS points in the tile with (unit vector
//                             from the point to its nearest particle, that particle's index); after another barrier the owner of
//                             particle n walks the tile in ascending j (LDS broadcasts) and adds the unit vectors whose index is n:
//                             ascending m across tiles, from +0, no sort, no atomic.  The sum is scaled by -1 / M once, behind it.
//        particle -> targets: cost_kernel's slices; beside the running minimum of a (slice, particle) its index lives in LDS.  Slices of
//                             successive tiles interleave in m, so combining slices compares the INDICES among equal values.
//      Row n of the last frame = (-(1 / n_obj) unit(P_n - q_m*(n)) + (-(1 / M)) sum) + box part.
//  (3) thread 0 forms chamfer and reward as cost_kernel does; a reward that is not finite makes every thread overwrite the rows it wrote
//      with NaN (the same thread, the same addresses: program order).
__global__ __launch_bounds__(PG_THREADS) void cost_grad_kernel(int T, int n_obj, int M, const float* __restrict__ state_seqs,
                                                               const float* __restrict__ actions, const float* __restrict__ state_cur,
                                                               const float* __restrict__ target, const float* __restrict__ box, float pusher,
                                                               float sharp, float pw, float* __restrict__ reward, float* __restrict__ chamfer,
                                                               float* __restrict__ collision, float* __restrict__ box_pen,
                                                               float* __restrict__ g_state, float* __restrict__ g_actions) {
  __shared__ float4 s_p[PG_MAXN];
  __shared__ float4 s_t[PG_TILE];
  __shared__ float s_min[PG_MAXN];
  __shared__ int s_arg[PG_MAXN];
  __shared__ int s_ti[PG_TILE];
  __shared__ float s_red[5][PG_WAVES];
  __shared__ int s_redi[5][PG_WAVES];
  __shared__ FrameRec s_rec;
  __shared__ int s_bad;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
  const float inf = __builtin_inff();
  const float* __restrict__ seq = state_seqs + (size_t)b * T * n_obj * 3;
  const float* __restrict__ act = actions + (size_t)b * T * 4;
  float* __restrict__ gs = g_state + (size_t)b * T * n_obj * 3;
  float* __restrict__ ga = g_actions + (size_t)b * T * 4;
  const float wT = pw / (float)T;
  float csum = 0.0f, bsum = 0.0f;                  // (thread 0) the sums over t of the two penalty terms
  int lb_idx = -1, lb_coord = 0;                   // the last frame's box part
  float lb_g = 0.0f;
  for (int t = -1; t < T; ++t) {
    const float* __restrict__ src = t < 0 ? state_cur : seq + (size_t)t * n_obj * 3;
    const bool coll = t + 1 < T, boxed = t >= 0, last = t == T - 1;
    float ax = 0.0f, ay = 0.0f;
    if (coll) { ax = act[4 * (t + 1)]; ay = act[4 * (t + 1) + 1]; }
    float v[5] = {inf, inf, inf, inf, inf};
    int vi[5] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
    for (int n = tid; n < n_obj; n += PG_THREADS) {
      const float x = src[3 * n], y = src[3 * n + 1], z = src[3 * n + 2];
      if (coll) { const float dx = ax - x, dy = ay - y; pg_take(v[0], vi[0], dx * dx + dy * dy, n); }
      if (boxed) { pg_take(v[1], vi[1], x, n); pg_take(v[2], vi[2], -x, n); pg_take(v[3], vi[3], y, n); pg_take(v[4], vi[4], -y, n); }
      if (last) s_p[n] = make_float4(x, y, z, 0.0f);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      float r = v[k];
      int ri = vi[k];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(r, off, 64);
        const int oi = __shfl_xor(ri, off, 64);
        pg_take(r, ri, ov, oi);
      }
      if (lane == 0) { s_red[k][wv] = r; s_redi[k][wv] = ri; }
    }
    __syncthreads();
    if (tid == 0) {
      float r[5];
      int ri[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        r[k] = s_red[k][0]; ri[k] = s_redi[k][0];
#pragma unroll
        for (int w = 1; w < PG_WAVES; ++w) pg_take(r[k], ri[k], s_red[k][w], s_redi[k][w]);
      }
      FrameRec rec = {-1, 0.0f, 0.0f, -1, 0, 0.0f};
      if (coll) {
        const float d = sqrtf(r[0]);
        const float c = expf(-sharp * pg_relu(d - pusher));
        collision[(size_t)b * T + t + 1] = c;
        csum += c;
        float gx = 0.0f, gy = 0.0f;
        if (d - pusher > 0.0f && d > 0.0f) {                     // (ri[0] is a particle: n_obj >= 1)
          const float k = wT * sharp * c;
          gx = k * ((ax - src[3 * ri[0]]) / d);
          gy = k * ((ay - src[3 * ri[0] + 1]) / d);
          rec.c_idx = ri[0]; rec.c_gx = -gx; rec.c_gy = -gy;
        }
        float* __restrict__ o = ga + 4 * (t + 1);
        o[0] = gx; o[1] = gy; o[2] = 0.0f; o[3] = 0.0f;
      }
      if (boxed) {
        const float m0 = pg_relu(r[1] - box[0]), m1 = pg_relu(box[1] + r[2]), m2 = pg_relu(r[3] - box[2]), m3 = pg_relu(box[3] + r[4]);
        const float e0 = expf(-sharp * m0), e1 = expf(-sharp * m1), e2 = expf(-sharp * m2), e3 = expf(-sharp * m3);
        float e = -e0;                                           // the largest of the four as a NaN-keeping minimum of the negated
        e = gsr_min_nan(e, -e1); e = gsr_min_nan(e, -e2); e = gsr_min_nan(e, -e3);
        box_pen[(size_t)b * T + t] = -e;
        bsum += -e;
        float best = e0, bm = m0;
        int w = 0;
        if (e1 > best) { best = e1; bm = m1; w = 1; }
        if (e2 > best) { best = e2; bm = m2; w = 2; }
        if (e3 > best) { best = e3; bm = m3; w = 3; }
        if (bm > 0.0f) {
          const float g = wT * sharp * best;
          rec.b_idx = ri[1 + w]; rec.b_coord = w >> 1; rec.b_g = (w & 1) ? -g : g;
        }
      }
      s_rec = rec;
    }
    __syncthreads();
    if (boxed) {
      const FrameRec rec = s_rec;
      if (last) {
        lb_idx = rec.b_idx; lb_coord = rec.b_coord; lb_g = rec.b_g;
      } else {
        float* __restrict__ dst = gs + (size_t)t * n_obj * 3;
        for (int n = tid; n < n_obj; n += PG_THREADS) {
          float gx = 0.0f, gy = 0.0f;
          if (n == rec.c_idx) { gx += rec.c_gx; gy += rec.c_gy; }
          if (n == rec.b_idx) { if (rec.b_coord == 0) gx += rec.b_g; else gy += rec.b_g; }
          dst[3 * n] = gx; dst[3 * n + 1] = gy; dst[3 * n + 2] = 0.0f;
        }
      }
    }
  }

  const int G = (n_obj + 63) >> 6;                               // groups of 64 particles
  const int S = G >= 3 ? 1 : (G == 2 ? 2 : 4);                   // slices of a tile; S G <= 4 or S = 1
  const int WS = PG_WAVES / S;                                   // waves per slice
  const int slice = wv / WS, g0 = wv % WS, GN = G * 64;
  for (int i = tid; i < S * GN; i += PG_THREADS) { s_min[i] = inf; s_arg[i] = 0; }   // (S GN <= 1024)
  float sum_a = 0.0f;
  float ux[PG_SLOTS], uy[PG_SLOTS], uz[PG_SLOTS];                // sums of the unit vectors toward the particles this thread owns
#pragma unroll
  for (int k = 0; k < PG_SLOTS; ++k) { ux[k] = 0.0f; uy[k] = 0.0f; uz[k] = 0.0f; }
  const bool walks = tid - lane < n_obj;                         // the wave owns a particle
  for (int base = 0; base < M; base += PG_TILE) {
    const int tc = min(PG_TILE, M - base);
    __syncthreads();                                             // the tile's readers are done (first pass: s_p, s_min and s_arg are written)
    for (int j = tid; j < tc; j += PG_THREADS) {
      const float* q = target + (size_t)(base + j) * 3;
      s_t[j] = make_float4(q[0], q[1], q[2], 0.0f);
    }
    __syncthreads();
    for (int j = tid; j < tc; j += PG_THREADS) {
      const float4 q = s_t[j];
      float m = inf, nan_acc = 0.0f;
      int am = 0;
      for (int n = 0; n < n_obj; ++n) {
        const float4 p = s_p[n];
        const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z, d = dx * dx + dy * dy + dz * dz;
        if (d < m) { m = d; am = n; }
        nan_acc += d;
      }
      sum_a += sqrtf(nan_acc != nan_acc ? nan_acc : m);
      s_ti[j] = am;
    }
    const int lo = (tc * slice) / S, hi = (tc * (slice + 1)) / S;
    for (int g = g0; g < G; g += WS) {
      const int n = g * 64 + lane;
      if (n < n_obj) {
        const float4 p = s_p[n];
        float m = inf, nan_acc = 0.0f;
        int am = 0;
        for (int j = lo; j < hi; ++j) {
          const float4 q = s_t[j];
          const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z, d = dx * dx + dy * dy + dz * dz;
          if (d < m) { m = d; am = base + j; }
          nan_acc += d;
        }
        // a later tile holds higher indices: it takes over only with a smaller value (or a NaN, which stays)
        const float cur = s_min[slice * GN + n], got = nan_acc != nan_acc ? nan_acc : m;
        if (got < cur || got != got) { s_min[slice * GN + n] = got; s_arg[slice * GN + n] = am; }
      }
    }
    __syncthreads();                                             // both pair loops have read the tile's points
    for (int j = tid; j < tc; j += PG_THREADS) {
      const float4 q = s_t[j];
      const int am = s_ti[j];
      const float4 p = s_p[am];
      const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z, dist = sqrtf(dx * dx + dy * dy + dz * dz);
      const bool z = dist > 0.0f || dist != dist;                // a zero distance: a zero vector
      s_t[j] = make_float4(z ? dx / dist : 0.0f, z ? dy / dist : 0.0f, z ? dz / dist : 0.0f, __int_as_float(am));
    }
    __syncthreads();
    if (walks) {
      if (n_obj <= PG_THREADS) {
        for (int j = 0; j < tc; ++j) {
          const float4 e = s_t[j];
          const bool h = __float_as_int(e.w) == tid;
          ux[0] += h ? e.x : 0.0f; uy[0] += h ? e.y : 0.0f; uz[0] += h ? e.z : 0.0f;
        }
      } else {
        for (int j = 0; j < tc; ++j) {
          const float4 e = s_t[j];
          const int id = __float_as_int(e.w);
#pragma unroll
          for (int k = 0; k < PG_SLOTS; ++k) {
            const bool h = id == tid + k * PG_THREADS;
            ux[k] += h ? e.x : 0.0f; uy[k] += h ? e.y : 0.0f; uz[k] += h ? e.z : 0.0f;
          }
        }
      }
    }
  }
  __syncthreads();
  float sum_b = 0.0f;
  const float cn = 1.0f / (float)n_obj, cm = 1.0f / (float)M;
  float* __restrict__ dst = gs + (size_t)(T - 1) * n_obj * 3;
#pragma unroll
  for (int k = 0; k < PG_SLOTS; ++k) {
    const int n = tid + k * PG_THREADS;
    if (n < n_obj) {
      float m = s_min[n];
      int am = s_arg[n];
      for (int s = 1; s < S; ++s) pg_take(m, am, s_min[s * GN + n], s_arg[s * GN + n]);
      const float dist = sqrtf(m);
      sum_b += dist;
      const float4 p = s_p[n];
      const float* q = target + (size_t)am * 3;                  // (0 <= am < M always: 0 at the start, tile indices after)
      const bool z = dist > 0.0f || dist != dist;
      float gx = -(cn * (z ? (p.x - q[0]) / dist : 0.0f)) + -(cm * ux[k]);
      float gy = -(cn * (z ? (p.y - q[1]) / dist : 0.0f)) + -(cm * uy[k]);
      const float gz = -(cn * (z ? (p.z - q[2]) / dist : 0.0f)) + -(cm * uz[k]);
      if (n == lb_idx) { if (lb_coord == 0) gx += lb_g; else gy += lb_g; }
      dst[3 * n] = gx; dst[3 * n + 1] = gy; dst[3 * n + 2] = gz;
    }
  }
  sum_a = pg_wave_sum(sum_a);
  sum_b = pg_wave_sum(sum_b);
  if (lane == 0) { s_red[0][wv] = sum_a; s_red[1][wv] = sum_b; }
  __syncthreads();
  if (tid == 0) {
    float a = s_red[0][0], c = s_red[1][0];
#pragma unroll
    for (int w = 1; w < PG_WAVES; ++w) { a += s_red[0][w]; c += s_red[1][w]; }
    const float ch = a / (float)M + c / (float)n_obj;
    chamfer[b] = ch;
    const float rw = -ch - pw * (csum / (float)T) - pw * (bsum / (float)T);
    reward[b] = rw;
    s_bad = fabsf(rw) < inf ? 0 : 1;
  }
  __syncthreads();
  if (s_bad) {
    const float nan = __builtin_nanf("");
    for (int t = 0; t < T; ++t)
      for (int n = tid; n < n_obj; n += PG_THREADS) {
        float* __restrict__ o = gs + ((size_t)t * n_obj + n) * 3;
        o[0] = nan; o[1] = nan; o[2] = nan;
      }
    if (tid == 0)
      for (int i = 0; i < 4 * T; ++i) ga[i] = nan;
  }
}
}  // namespace gsr_pcgrad

extern "C" {

int gsr_plan_cost_grad(int32_t B, int32_t T, int32_t n_obj, int32_t M, const float* state_seqs, const float* actions, const float* state_cur,
                       const float* target, const float* box, float pusher_size, float sharpness, float penalty_weight, float* reward,
                       float* chamfer, float* collision, float* box_pen, float* g_state, float* g_actions, void* stream) {
  GsrRange _range("gsr_plan_cost_grad");
  if (B < 1 || T < 1 || M < 1 || n_obj < 1 || n_obj > PG_MAXN) {
    gsr_set_error("gsr_plan_cost_grad: bad argument (B, T, M >= 1, 1 <= n_obj <= 1024; got B = %d, T = %d, M = %d, n_obj = %d)", (int)B, (int)T,
                  (int)M, (int)n_obj);
    return -2;
  }
  if (!state_seqs || !actions || !state_cur || !target || !box || !reward || !chamfer || !collision || !box_pen || !g_state || !g_actions) {
    gsr_set_error("gsr_plan_cost_grad: NULL pointer");
    return -2;
  }
  if ((long long)B * T * n_obj * 3 > 0x7fffffffll || (long long)M * 3 > 0x7fffffffll) {
    gsr_set_error("gsr_plan_cost_grad: B T n_obj 3 = %lld or M 3 = %lld exceeds 2^31", (long long)B * T * n_obj * 3, (long long)M * 3);
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  { GSR_PROF("plan_cost_grad", st);
    hipLaunchKernelGGL(gsr_pcgrad::cost_grad_kernel, dim3(B), dim3(PG_THREADS), 0, st, T, n_obj, M, state_seqs, actions, state_cur, target, box,
                       pusher_size, sharpness, penalty_weight, reward, chamfer, collision, box_pen, g_state, g_actions); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
