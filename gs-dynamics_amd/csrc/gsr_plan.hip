// gsr_plan.hip -- the planner's rollout (gsdyn/plan.py; the reference's real_world/plan.py:24-154, `dynamics`): B sampled action
// sequences advance B copies of one particle state through the propagation network TOGETHER.  The two kernels of gsr_gnn.hip take flat
// row and relation lists, so B graphs laid out block-diagonally -- sample b owns the rows b R .. b R + R - 1 (R = n_obj + 1: objects, then
// the one tool particle), one dummy row B R behind the last sample collects the padding -- are ONE graph to them.  What is new here:
//   gsr_construct_edges_batch : the relations of all B graphs as one compact list in global row indices, with its segment bounds;
//   gsr_plan_step_head        : the inputs of one model call for all samples from the histories (gsr_rollout_step_head's column layouts);
//   gsr_plan_step_tail        : clamp + add, the tool's new position, both history shifts and the look-ahead step's result.
// No global atomics and no float reduction whose order could vary: every output is bit-identical from run to run.
#include "gsr_common.h"
#include "gsr_relations.h"

namespace gsr_plan {

// ---------------------------------------------------------------- relations of B graphs
// The per-sample rule is construct_edges_kernel's (gsr_dynamics.hip): both kernels take a row's masks, the scan of the row counts and the
// list write from gsr_relations.h.  Own to this file: the totals across samples, the global row indices, the strided padding.
#define PM_THREADS 1024
#define PR_THREADS 256

// Launch 1, one workgroup per sample: the sample's adjacency matrix as R x 2 ballot masks and its relation total -> scratch
// (masks [B][R][2], then totals [B], 64-bit words).
__global__ __launch_bounds__(PM_THREADS) void masks_kernel(const float* __restrict__ pos_all, int n_obj_cap, const int* __restrict__ n_valid_p,
                                                           float thr2, int topk, unsigned long long* __restrict__ masks,
                                                           unsigned long long* __restrict__ totals) {
  __shared__ float sp[3 * 128];
  __shared__ int s_cnt[PM_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
  const int N = n_obj_cap + 1, n_valid = min(*n_valid_p, n_obj_cap);
  const float* __restrict__ pos = pos_all + (size_t)b * N * 3;
  unsigned long long* __restrict__ out = masks + (size_t)b * N * 2;
  if (tid < N) { sp[3 * tid] = pos[3 * tid]; sp[3 * tid + 1] = pos[3 * tid + 1]; sp[3 * tid + 2] = pos[3 * tid + 2]; }
  __syncthreads();
  const int k = min(min(topk, GSR_REL_MAXK), n_valid);
  int cnt = 0;                                   // (wave-uniform: the relations of this wave's rows)
  for (int i = wv; i < N; i += PM_THREADS / 64) {
    unsigned long long m[2];
    gsr_rel_row_masks(sp, i, lane, N, n_obj_cap, n_valid, thr2, k, m);
    if (lane == 0) { out[2 * i] = m[0]; out[2 * i + 1] = m[1]; }
    cnt += __popcll(m[0]) + __popcll(m[1]);
  }
  if (lane == 0) s_cnt[wv] = cnt;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    for (int w = 0; w < PM_THREADS / 64; ++w) t += s_cnt[w];
    totals[b] = (unsigned long long)t;
  }
}

// Launch 2, one workgroup per sample: its base in the list = the totals before it (integers: any order gives the same sum), its rows in
// the adjacency matrix's row-major order as GLOBAL indices b R + i, its share of the padding and its R entries of row_start.
__global__ __launch_bounds__(PR_THREADS) void rows_kernel(int B, int n_obj_cap, int e_cap, const unsigned long long* __restrict__ masks,
                                                          const unsigned long long* __restrict__ totals, long long* __restrict__ recv,
                                                          long long* __restrict__ send, int* __restrict__ count, long long* __restrict__ row_start) {
  __shared__ unsigned long long s_mask[128][2];
  __shared__ int s_base[128];
  __shared__ int s_red[2][PR_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
  const int N = n_obj_cap + 1;
  const long long dummy = (long long)B * N, row0 = (long long)b * N;
  for (int i = tid; i < 2 * N; i += PR_THREADS) (&s_mask[0][0])[i] = masks[(size_t)b * N * 2 + i];
  int before = 0, all = 0;
  for (int j = tid; j < B; j += PR_THREADS) {
    const int t = (int)totals[j];
    all += t;
    if (j < b) before += t;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { before += __shfl_xor(before, off, 64); all += __shfl_xor(all, off, 64); }
  if (lane == 0) { s_red[0][wv] = before; s_red[1][wv] = all; }
  __syncthreads();
  before = 0; all = 0;
#pragma unroll
  for (int w = 0; w < PR_THREADS / 64; ++w) { before += s_red[0][w]; all += s_red[1][w]; }
  if (wv == 0) gsr_rel_scan_rows(s_mask, lane, N, s_base);
  __syncthreads();
  for (int i = wv; i < N; i += PR_THREADS / 64) gsr_rel_write_row(s_mask[i][0], s_mask[i][1], i, lane, before + s_base[i], e_cap, row0, recv, send);
  for (int i = tid; i < N; i += PR_THREADS) row_start[row0 + i] = (long long)min(before + s_base[i], e_cap);
  for (long long e = (long long)all + (long long)b * PR_THREADS + tid; e < e_cap; e += (long long)B * PR_THREADS) { recv[e] = dummy; send[e] = dummy; }
  if (b == 0 && tid == 0) {
    *count = min(all, e_cap);
    row_start[dummy] = (long long)min(all, e_cap);      // the dummy row's segment: the padding
    row_start[dummy + 1] = (long long)e_cap;
  }
}

// ---------------------------------------------------------------- the glue around one model call, all samples
// One thread per global row r = b R + i (and the dummy row B R, all zeros but its attribute / instance entries, which the caller passes
// as zeros): gsr_rollout_step_head's columns -- p_in = (attributes, [state], action), nodes = (attributes, instance, state).
__global__ __launch_bounds__(GSR_BLOCK) void head_kernel(int B, int n_his, int n_obj, int A, int with_state, const float* __restrict__ hist,
                                                         const float* __restrict__ eef_hist, const float* __restrict__ eef_delta,
                                                         const float* __restrict__ attrs, const float* __restrict__ inst,
                                                         float* __restrict__ state_t, float* __restrict__ p_in, float* __restrict__ nodes,
                                                         float* __restrict__ states_last) {
  const int R = n_obj + 1, n_rows = B * R + 1;
  const int r = blockIdx.x * GSR_BLOCK + threadIdx.x;
  if (r >= n_rows) return;
  const int S3 = 3 * n_his, Dp = A + (with_state ? S3 : 0) + 3, Dn = A + 1 + S3;
  const int b = r / R, i = r - b * R;
  const bool pad = r == n_rows - 1, tool = !pad && i == n_obj;
  for (int k = 0; k < A; ++k) { const float v = attrs[(size_t)r * A + k]; p_in[(size_t)r * Dp + k] = v; nodes[(size_t)r * Dn + k] = v; }
  nodes[(size_t)r * Dn + A] = inst[r];
  for (int h = 0; h < n_his; ++h)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = pad ? 0.f : (tool ? eef_hist[((size_t)b * n_his + h) * 3 + c] : hist[(((size_t)b * n_his + h) * n_obj + i) * 3 + c]);
      state_t[(size_t)r * S3 + 3 * h + c] = v;
      nodes[(size_t)r * Dn + A + 1 + 3 * h + c] = v;
      if (with_state) p_in[(size_t)r * Dp + A + 3 * h + c] = v;
      if (h == n_his - 1 && !pad) states_last[(size_t)r * 3 + c] = v;
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) p_in[(size_t)r * Dp + Dp - 3 + c] = tool ? eef_delta[(size_t)b * 3 + c] : 0.f;
}

// One workgroup per sample, thread i = object particle i (n_obj <= 127): predicted = last + clamp(motion), the history window shifted in
// place (a thread touches its own particle only), the look-ahead step's result for the samples whose repeat count is reached, and the
// tool: x, y advanced by the displacement, z = the sample's lowest predicted particle (plan.py:119-122) -- LDS, then one wave's butterfly.
#define PT_THREADS 128
__global__ __launch_bounds__(PT_THREADS) void tail_kernel(int n_his, int n_obj, int T, int ai, int li, float clampv,
                                                          const float* __restrict__ motion, const float* __restrict__ eef_delta,
                                                          const int* __restrict__ repeat, float* __restrict__ hist,
                                                          float* __restrict__ eef_hist, float* __restrict__ out_seq) {
  __shared__ float s_z[PT_THREADS];
  const int b = blockIdx.x, i = threadIdx.x, R = n_obj + 1;
  float pz = __builtin_inff();
  if (i < n_obj) {
    float* hb = hist + ((size_t)b * n_his * n_obj + i) * 3;
    const size_t hs = (size_t)n_obj * 3;
    const bool keep = repeat[(size_t)b * T + li] == ai;
    float pr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float m = motion[((size_t)b * R + i) * 3 + c];
      const float cl = m < -clampv ? -clampv : (m > clampv ? clampv : m);
      pr[c] = hb[(n_his - 1) * hs + c] + cl;
    }
    for (int h = 0; h + 1 < n_his; ++h)
#pragma unroll
      for (int c = 0; c < 3; ++c) hb[h * hs + c] = hb[(h + 1) * hs + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      hb[(n_his - 1) * hs + c] = pr[c];
      if (keep) out_seq[(((size_t)b * T + li) * n_obj + i) * 3 + c] = pr[c];
    }
    pz = pr[2];
  }
  s_z[i] = pz;
  __syncthreads();
  if (i < 64) {
    const float m = gsr_wave_min_nan(gsr_min_nan(s_z[i], s_z[i + 64]));
    if (i == 0) {
      float* eb = eef_hist + (size_t)b * n_his * 3;
      const float nx = eb[3 * (n_his - 1)] + eef_delta[(size_t)b * 3], ny = eb[3 * (n_his - 1) + 1] + eef_delta[(size_t)b * 3 + 1];
      for (int h = 0; h + 1 < n_his; ++h)
        for (int c = 0; c < 3; ++c) eb[3 * h + c] = eb[3 * (h + 1) + c];
      eb[3 * (n_his - 1)] = nx; eb[3 * (n_his - 1) + 1] = ny; eb[3 * (n_his - 1) + 2] = m;
    }
  }
}
}  // namespace gsr_plan

extern "C" {

int gsr_construct_edges_batch(int32_t B, const float* positions, int32_t n_obj_cap, const int32_t* n_valid, float thresh_sq, int32_t topk,
                              int32_t e_cap, int64_t* receivers, int64_t* senders, int32_t* count, int64_t* row_start, uint64_t* scratch,
                              void* stream) {
  GsrRange _range("gsr_construct_edges_batch");
  if (B < 1 || n_obj_cap < 1 || n_obj_cap > 127 || topk < 1 || topk > 16) {
    gsr_set_error("gsr_construct_edges_batch: bad argument (B >= 1, 1 <= n_obj_cap <= 127, 1 <= topk <= 16; got B = %d, n_obj_cap = %d, topk = %d)",
                  (int)B, (int)n_obj_cap, (int)topk);
    return -2;
  }
  if (!positions || !n_valid || !receivers || !senders || !count || !row_start || !scratch) {
    gsr_set_error("gsr_construct_edges_batch: NULL pointer");
    return -2;
  }
  const long long bound = (long long)B * ((long long)n_obj_cap * (topk < n_obj_cap ? topk : n_obj_cap) + 2ll * n_obj_cap);
  if ((long long)e_cap < bound || bound > 0x7fffffffll || (long long)B * (n_obj_cap + 1) + 2 > 0x7fffffffll) {
    gsr_set_error("gsr_construct_edges_batch: e_cap = %d is below the bound B (n_obj_cap min(topk, n_obj_cap) + 2 n_obj_cap) = %lld (or the list "
                  "exceeds 2^31 entries): nothing is ever truncated, so nothing was launched", (int)e_cap, bound);
    return -3;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* masks = (unsigned long long*)scratch;
  unsigned long long* totals = masks + (size_t)B * (n_obj_cap + 1) * 2;
  { GSR_PROF("plan_edge_masks", st);
    hipLaunchKernelGGL(gsr_plan::masks_kernel, dim3(B), dim3(PM_THREADS), 0, st, positions, n_obj_cap, (const int*)n_valid, thresh_sq, topk, masks, totals); }
  GSR_HIP_CHECK(hipGetLastError());
  { GSR_PROF("plan_edge_rows", st);
    hipLaunchKernelGGL(gsr_plan::rows_kernel, dim3(B), dim3(PR_THREADS), 0, st, B, n_obj_cap, e_cap, masks, totals, (long long*)receivers, (long long*)senders,
                       (int*)count, (long long*)row_start); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

int gsr_plan_step_head(int32_t B, int32_t n_his, int32_t n_obj, int32_t attr_dim, int32_t with_state, const float* hist, const float* eef_hist,
                       const float* eef_delta, const float* attrs, const float* instance, float* state_rows, float* particle_inputs, float* rel_nodes,
                       float* states_last, void* stream) {
  GsrRange _range("gsr_plan_step_head");
  if (B < 1 || n_his < 1 || n_obj < 1 || attr_dim < 0 || (long long)B * (n_obj + 1) + 1 > 0x7fffffffll / 64 || !hist || !eef_hist || !eef_delta ||
      (attr_dim > 0 && !attrs) || !instance || !state_rows || !particle_inputs || !rel_nodes || !states_last) {
    gsr_set_error("gsr_plan_step_head: bad argument (B, n_his, n_obj >= 1, B (n_obj + 1) < 2^25, no NULL pointer)");
    return -2;
  }
  const int n_rows = B * (n_obj + 1) + 1;
  hipStream_t st = (hipStream_t)stream;
  { GSR_PROF("plan_head", st);
    hipLaunchKernelGGL(gsr_plan::head_kernel, dim3((n_rows + GSR_BLOCK - 1) / GSR_BLOCK), dim3(GSR_BLOCK), 0, st, B, n_his, n_obj, attr_dim, with_state ? 1 : 0,
                       hist, eef_hist, eef_delta, attrs, instance, state_rows, particle_inputs, rel_nodes, states_last); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

int gsr_plan_step_tail(int32_t B, int32_t n_his, int32_t n_obj, int32_t T, int32_t ai, int32_t li, float motion_clamp, const float* pred_motion,
                       const float* eef_delta, const int32_t* repeat, float* hist, float* eef_hist, float* out_seq, void* stream) {
  GsrRange _range("gsr_plan_step_tail");
  if (B < 1 || n_his < 1 || n_obj < 1 || n_obj > 127 || T < 1 || li < 0 || li >= T || !(motion_clamp >= 0.0f) || !pred_motion || !eef_delta || !repeat ||
      !hist || !eef_hist || !out_seq) {
    gsr_set_error("gsr_plan_step_tail: bad argument (B, n_his >= 1, 1 <= n_obj <= 127, 0 <= li < T, no NULL pointer)");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  { GSR_PROF("plan_tail", st);
    hipLaunchKernelGGL(gsr_plan::tail_kernel, dim3(B), dim3(PT_THREADS), 0, st, n_his, n_obj, T, ai, li, motion_clamp, pred_motion, eef_delta,
                       (const int*)repeat, hist, eef_hist, out_seq); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
