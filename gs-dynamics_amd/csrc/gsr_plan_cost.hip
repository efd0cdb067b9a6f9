// gsr_plan_cost.hip -- the two reductions of one planner iteration behind the rollout (gsdyn/plan.py; the reference's real_world/plan.py
// `running_cost` and utils/plan_utils.py `optimize_action_mppi`):
//   gsr_plan_cost        : reward, chamfer distance, collision and box terms of B rolled-out samples -- one workgroup per sample, one launch;
//   gsr_plan_mppi_update : the soft-max weighted push, the best sample and its reward -- one workgroup loops over B, one launch.
// No global atomics, no float atomics.  Every float sum runs in a FIXED order (stated at each reduction), so the outputs are bit-identical
// from run to run, and a sample's cost depends neither on B nor on the sample's position in the batch.
// The NaN-keeping minimum and its wave butterfly (gsr_min_nan, gsr_wave_min_nan: gsr_common.h) are the ones gsr_plan.hip's tail uses.
#include "gsr_common.h"

namespace gsr_pcost {

#define PC_THREADS 256
#define PC_WAVES (PC_THREADS / 64)
#define PC_MAXN 1024            // particles of one sample held in LDS
#define PC_TILE 1024            // target points per LDS tile

// sum of the 64 lanes as an xor butterfly, offsets 32, 16, .. 1: a fixed tree (fp addition commutes, so every lane holds the same sum)
__device__ __forceinline__ float pc_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// max(v, 0) that keeps a NaN (torch.maximum)
__device__ __forceinline__ float pc_relu(float v) { return v < 0.0f ? 0.0f : v; }

// One workgroup per sample b.
//  (1) for the frames t = -1 (state_cur) .. T - 1 (state_seqs[b, t]): thread i walks the particles i, i + 256, ..; five NaN-keeping minima
//      (squared distance to the NEXT step's start point, x, -x, y, -y) go through a wave butterfly and then the four waves in wave order.
//      Thread 0 turns them into collision[b, t + 1] and box_pen[b, t] and adds them to the two means in the order t = 0, 1, ..
//  (2) chamfer of the last frame P (in LDS) against the target, which passes through LDS in tiles of 1024 points.  Both directions walk all
//      n_obj x M pairs of a tile:
//        target -> particles: thread i owns the tile's points i, i + 256, ..; the particles come as LDS broadcasts; the root of the minimum
//                             is added to the thread's sum -- thread i thus adds its terms m = i, i + 256, .. in ascending m;
//        particle -> targets: a wave owns 64 particles (lane = particle) and a slice of the tile (the whole tile from 129 particles on,
//                             a half for 65 .. 128, a quarter up to 64, so that no wave idles at the planner's 100 particles); the
//                             tile's points come as LDS broadcasts; the running minimum of a (slice, particle) lives in LDS between
//                             tiles, never as a per-particle array in registers.
//      At the end thread i adds the roots of the particles i, i + 256, .. (slices combined in slice order) in ascending order.
//      The 256 partial sums of either direction are combined by the same fixed tree: xor butterfly over the 64 lanes (offsets 32 .. 1),
//      then the four waves' sums in wave order.
//  The minimum runs on the squared distance, the root comes after it (monotone: the same value).  In the two pair loops the minimum is a
//  plain v_min_f32 and the NaN travels in a sum of the (non-negative) squared distances beside it, which is NaN exactly when one of them
//  is: one instruction instead of the three of gsr_min_nan (gsr_common.h), the same result.
__global__ __launch_bounds__(PC_THREADS) void cost_kernel(int T, int n_obj, int M, const float* __restrict__ state_seqs,
                                                          const float* __restrict__ actions, const float* __restrict__ state_cur,
                                                          const float* __restrict__ target, const float* __restrict__ box, float pusher,
                                                          float sharp, float pw, float* __restrict__ reward, float* __restrict__ chamfer,
                                                          float* __restrict__ collision, float* __restrict__ box_pen) {
  __shared__ float4 s_p[PC_MAXN];
  __shared__ float4 s_t[PC_TILE];
  __shared__ float s_min[PC_MAXN];
  __shared__ float s_red[5][PC_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
  const float inf = __builtin_inff();
  const float* __restrict__ seq = state_seqs + (size_t)b * T * n_obj * 3;
  const float* __restrict__ act = actions + (size_t)b * T * 4;
  float csum = 0.0f, bsum = 0.0f;                  // (thread 0) the sums over t of the two penalty terms
  for (int t = -1; t < T; ++t) {
    const float* __restrict__ src = t < 0 ? state_cur : seq + (size_t)t * n_obj * 3;
    const bool coll = t + 1 < T, boxed = t >= 0, last = t == T - 1;
    float ax = 0.0f, ay = 0.0f;
    if (coll) { ax = act[4 * (t + 1)]; ay = act[4 * (t + 1) + 1]; }
    float v[5] = {inf, inf, inf, inf, inf};
    for (int n = tid; n < n_obj; n += PC_THREADS) {
      const float x = src[3 * n], y = src[3 * n + 1], z = src[3 * n + 2];
      if (coll) { const float dx = ax - x, dy = ay - y; v[0] = gsr_min_nan(v[0], dx * dx + dy * dy); }
      if (boxed) { v[1] = gsr_min_nan(v[1], x); v[2] = gsr_min_nan(v[2], -x); v[3] = gsr_min_nan(v[3], y); v[4] = gsr_min_nan(v[4], -y); }
      if (last) s_p[n] = make_float4(x, y, z, 0.0f);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float r = gsr_wave_min_nan(v[k]);
      if (lane == 0) s_red[k][wv] = r;
    }
    __syncthreads();
    if (tid == 0) {
      float r[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        r[k] = s_red[k][0];
#pragma unroll
        for (int w = 1; w < PC_WAVES; ++w) r[k] = gsr_min_nan(r[k], s_red[k][w]);
      }
      if (coll) {
        const float c = expf(-sharp * pc_relu(sqrtf(r[0]) - pusher));
        collision[(size_t)b * T + t + 1] = c;
        csum += c;
      }
      if (boxed) {
        const float m0 = pc_relu(r[1] - box[0]), m1 = pc_relu(box[1] + r[2]), m2 = pc_relu(r[3] - box[2]), m3 = pc_relu(box[3] + r[4]);
        float e = -expf(-sharp * m0);                            // the largest of the four as a NaN-keeping minimum of the negated
        e = gsr_min_nan(e, -expf(-sharp * m1)); e = gsr_min_nan(e, -expf(-sharp * m2)); e = gsr_min_nan(e, -expf(-sharp * m3));
        box_pen[(size_t)b * T + t] = -e;
        bsum += -e;
      }
    }
    __syncthreads();
  }

  const int G = (n_obj + 63) >> 6;                               // groups of 64 particles
  const int S = G >= 3 ? 1 : (G == 2 ? 2 : 4);                   // slices of a tile; S G <= 4 or S = 1
  const int WS = PC_WAVES / S;                                   // waves per slice
  const int slice = wv / WS, g0 = wv % WS, GN = G * 64;
  for (int i = tid; i < S * GN; i += PC_THREADS) s_min[i] = inf; // (S GN <= 1024)
  float sum_a = 0.0f;
  for (int base = 0; base < M; base += PC_TILE) {
    const int tc = min(PC_TILE, M - base);
    __syncthreads();                                             // the tile's readers are done (first pass: s_p and s_min are written)
    for (int j = tid; j < tc; j += PC_THREADS) {
      const float* q = target + (size_t)(base + j) * 3;
      s_t[j] = make_float4(q[0], q[1], q[2], 0.0f);
    }
    __syncthreads();
    for (int j = tid; j < tc; j += PC_THREADS) {
      const float4 q = s_t[j];
      float m = inf, nan_acc = 0.0f;
      for (int n = 0; n < n_obj; ++n) {
        const float4 p = s_p[n];
        const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z, d = dx * dx + dy * dy + dz * dz;
        m = fminf(m, d);
        nan_acc += d;
      }
      sum_a += sqrtf(nan_acc != nan_acc ? nan_acc : m);
    }
    const int lo = (tc * slice) / S, hi = (tc * (slice + 1)) / S;
    for (int g = g0; g < G; g += WS) {
      const int n = g * 64 + lane;
      if (n < n_obj) {
        const float4 p = s_p[n];
        float m = inf, nan_acc = 0.0f;
        for (int j = lo; j < hi; ++j) {
          const float4 q = s_t[j];
          const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z, d = dx * dx + dy * dy + dz * dz;
          m = fminf(m, d);
          nan_acc += d;
        }
        s_min[slice * GN + n] = gsr_min_nan(s_min[slice * GN + n], nan_acc != nan_acc ? nan_acc : m);
      }
    }
  }
  __syncthreads();
  float sum_b = 0.0f;
  for (int n = tid; n < n_obj; n += PC_THREADS) {
    float m = s_min[n];
    for (int s = 1; s < S; ++s) m = gsr_min_nan(m, s_min[s * GN + n]);
    sum_b += sqrtf(m);
  }
  sum_a = pc_wave_sum(sum_a);
  sum_b = pc_wave_sum(sum_b);
  if (lane == 0) { s_red[0][wv] = sum_a; s_red[1][wv] = sum_b; }
  __syncthreads();
  if (tid == 0) {
    float a = s_red[0][0], c = s_red[1][0];
#pragma unroll
    for (int w = 1; w < PC_WAVES; ++w) { a += s_red[0][w]; c += s_red[1][w]; }
    const float ch = a / (float)M + c / (float)n_obj;
    chamfer[b] = ch;
    reward[b] = -ch - pw * (csum / (float)T) - pw * (bsum / (float)T);
  }
}

// ---------------------------------------------------------------- the MPPI update
#define PU_THREADS 1024
#define PU_WAVES (PU_THREADS / 64)
// a ranks above b in the arg-max: a NaN above every number (torch.argmax), two NaNs equal
__device__ __forceinline__ bool pu_above(float a, float b) {
  const bool an = a != a, bn = b != b;
  return an ? !bn : (!bn && a > b);
}
// the better of two (reward, index) pairs: the higher rank, the LOWER index among equals
__device__ __forceinline__ void pu_take(float& bv, int& bi, float v, int i) {
  if (pu_above(v, bv) || (!pu_above(bv, v) && i < bi)) { bv = v; bi = i; }
}

// One workgroup.  Pass 1: thread i walks the samples i, i + 1024, ..; the (reward, index) pairs go through a wave butterfly and the sixteen
// waves (a total order: any tree gives the same pair).  Pass 2, per look-ahead step: e_b = exp(reward_weight (r_b - rmax)) -- the
// subtraction BEFORE the multiplication -- and five sums over the samples (e, e x, e y, e len push_length cos theta, e len push_length sin
// theta): thread i adds its samples in ascending order, then the xor butterfly over the 64 lanes (offsets 32 .. 1), then the sixteen waves'
// sums in wave order; the division by the sum of e comes once, behind the sums.  The push's displacement is accumulated directly: the
// reference sums the end points and differences the two sums, the same in exact arithmetic and a cancellation in fp32.
__global__ __launch_bounds__(PU_THREADS) void update_kernel(int B, int T, const float* __restrict__ act_seqs, const float* __restrict__ rewards,
                                                            float rw, float pl, const float* __restrict__ lower, const float* __restrict__ upper,
                                                            float* __restrict__ act_seq, long long* __restrict__ best_index,
                                                            float* __restrict__ best_reward) {
  __shared__ float s_v[PU_WAVES];
  __shared__ int s_i[PU_WAVES];
  __shared__ float s_red[5][PU_WAVES];
  __shared__ float s_rmax;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  float bv = -__builtin_inff();
  int bi = 0x7fffffff;
  for (int b = tid; b < B; b += PU_THREADS) pu_take(bv, bi, rewards[b], b);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    pu_take(bv, bi, ov, oi);
  }
  if (lane == 0) { s_v[wv] = bv; s_i[wv] = bi; }
  __syncthreads();
  if (tid == 0) {
    bv = s_v[0]; bi = s_i[0];
    for (int w = 1; w < PU_WAVES; ++w) pu_take(bv, bi, s_v[w], s_i[w]);
    s_rmax = bv;
    *best_index = (long long)bi;
    *best_reward = bv;
  }
  __syncthreads();
  const float rmax = s_rmax;
  for (int t = 0; t < T; ++t) {
    float acc[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int b = tid; b < B; b += PU_THREADS) {
      const float e = expf(rw * (rewards[b] - rmax));
      const float* __restrict__ a = act_seqs + ((size_t)b * T + t) * 4;
      const float l = a[3] * pl;
      acc[0] += e; acc[1] += e * a[0]; acc[2] += e * a[1]; acc[3] += e * (l * cosf(a[2])); acc[4] += e * (l * sinf(a[2]));
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      float r = acc[k];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) r += __shfl_xor(r, off, 64);
      if (lane == 0) s_red[k][wv] = r;
    }
    __syncthreads();
    if (tid == 0) {
      float r[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        r[k] = s_red[k][0];
        for (int w = 1; w < PU_WAVES; ++w) r[k] += s_red[k][w];
      }
      const float dx = r[3] / r[0], dy = r[4] / r[0];
      float o[4] = {r[1] / r[0], r[2] / r[0], atan2f(dy, dx), hypotf(dx, dy) / pl};
      // the reference's clip (utils/plan_utils.py clip_actions): COLUMN 0 -- x, not the angle -- through ((v + pi) mod 2 pi) - pi with the
      // floored modulo of torch.remainder, then every column clamped to its limits (a NaN passes)
      const float pi = 3.14159265358979323846f, two_pi = 6.28318530717958647692f;
      float m = fmodf(o[0] + pi, two_pi);
      if (m < 0.0f) m += two_pi;
      o[0] = m - pi;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float q = o[c];
        q = q < lower[c] ? lower[c] : q;
        q = q > upper[c] ? upper[c] : q;
        act_seq[4 * t + c] = q;
      }
    }
    __syncthreads();
  }
}
}  // namespace gsr_pcost

extern "C" {

int gsr_plan_cost(int32_t B, int32_t T, int32_t n_obj, int32_t M, const float* state_seqs, const float* actions, const float* state_cur,
                  const float* target, const float* box, float pusher_size, float sharpness, float penalty_weight, float* reward, float* chamfer,
                  float* collision, float* box_pen, void* stream) {
  GsrRange _range("gsr_plan_cost");
  if (B < 1 || T < 1 || M < 1 || n_obj < 1 || n_obj > PC_MAXN) {
    gsr_set_error("gsr_plan_cost: bad argument (B, T, M >= 1, 1 <= n_obj <= 1024; got B = %d, T = %d, M = %d, n_obj = %d)", (int)B, (int)T, (int)M,
                  (int)n_obj);
    return -2;
  }
  if (!state_seqs || !actions || !state_cur || !target || !box || !reward || !chamfer || !collision || !box_pen) {
    gsr_set_error("gsr_plan_cost: NULL pointer");
    return -2;
  }
  if ((long long)B * T * n_obj * 3 > 0x7fffffffll || (long long)M * 3 > 0x7fffffffll) {
    gsr_set_error("gsr_plan_cost: B T n_obj 3 = %lld or M 3 = %lld exceeds 2^31", (long long)B * T * n_obj * 3, (long long)M * 3);
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  { GSR_PROF("plan_cost", st);
    hipLaunchKernelGGL(gsr_pcost::cost_kernel, dim3(B), dim3(PC_THREADS), 0, st, T, n_obj, M, state_seqs, actions, state_cur, target, box, pusher_size,
                       sharpness, penalty_weight, reward, chamfer, collision, box_pen); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

int gsr_plan_mppi_update(int32_t B, int32_t T, const float* act_seqs, const float* rewards, float reward_weight, float push_length, const float* lower,
                         const float* upper, float* act_seq, int64_t* best_index, float* best_reward, void* stream) {
  GsrRange _range("gsr_plan_mppi_update");
  if (B < 1 || T < 1 || (long long)B * T * 4 > 0x7fffffffll) {
    gsr_set_error("gsr_plan_mppi_update: bad argument (B, T >= 1, B T 4 < 2^31; got B = %d, T = %d)", (int)B, (int)T);
    return -2;
  }
  if (!act_seqs || !rewards || !lower || !upper || !act_seq || !best_index || !best_reward) {
    gsr_set_error("gsr_plan_mppi_update: NULL pointer");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  { GSR_PROF("plan_mppi_update", st);
    hipLaunchKernelGGL(gsr_pcost::update_kernel, dim3(1), dim3(PU_THREADS), 0, st, B, T, act_seqs, rewards, reward_weight, push_length, lower, upper,
                       act_seq, (long long*)best_index, best_reward); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
