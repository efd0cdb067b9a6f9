// gsr_gnn_bwd.hip -- the backward of the two kernels of gsr_gnn.hip, so that the split propagation (gsdyn/dynamics.py:
// DynamicsPredictor.propagate_split_grad) can be trained on the device.  Both are gathers over two fixed-order lists -- a node's receiver
// segment [row_start[i], row_start[i + 1]) and its reverse list rev_edge[rev_ptr[i] .. rev_ptr[i + 1]), the relations it SENDS, ids
// ascending -- so every output element is one thread's running fp32 sum in a stated order: no atomics, no LDS, bit-identical from run to
// run (what index_add's / scatter_add's backward through the eager path is not).  Built with -ffp-contract=off: only additions and one
// subtraction occur, and the tests compare bit for bit.
#include "gsr_common.h"

namespace gsr_gnn_bwd {
// threshold_backward's rule on the recomputed pre-activation: z <= 0 blocks the gradient (z = +-0 included), a NaN z passes it
__device__ __forceinline__ float gate(float z, float g) { return z <= 0.f ? 0.f : g; }

// One thread per (node i, 4 columns), as the forward.  z[e] = (rew1[e] + a2[recv_e]) + a3[send_e] is recomputed in the forward's
// association order (no mask was stored); m[e] = gate(z[e], d_agg[recv_e]), zero for receivers >= n_sum (rows the forward did not sum).
//   walk 1, the receiver segment of i in list order:  d_rew1[e] = m[e],  d_a23[i, :H]  = sum m[e]
//   walk 2, the reverse list of i in ascending e:                        d_a23[i, H:]  = sum m[e]
// Rows >= n_sum own no segment: d_a23[i, :H] = 0, and the d_rew1 rows of their relations are the caller's to zero.
__global__ __launch_bounds__(256) void aggregate_backward_kernel(int N, int n_sum, int H, const float* __restrict__ rew1, const float* __restrict__ a23,
                                                                 const long long* __restrict__ send, const long long* __restrict__ recv,
                                                                 const long long* __restrict__ row_start, const long long* __restrict__ rev_ptr,
                                                                 const long long* __restrict__ rev_edge, const float* __restrict__ d_agg,
                                                                 float* __restrict__ d_rew1, float* __restrict__ d_a23) {
  const int o = blockIdx.x * 256 + threadIdx.x, q = H >> 2;
  if (o >= N * q) return;
  const int i = o / q, k4 = (o - i * q) << 2;
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n_sum) {
    const float4 a2 = *reinterpret_cast<const float4*>(a23 + (size_t)i * 2 * H + k4);
    const float4 g = *reinterpret_cast<const float4*>(d_agg + (size_t)i * H + k4);
    const int e1 = (int)row_start[i + 1];
    for (int e = (int)row_start[i]; e < e1; ++e) {
      const float4 r1 = *reinterpret_cast<const float4*>(rew1 + (size_t)e * H + k4);
      const float4 a3 = *reinterpret_cast<const float4*>(a23 + (size_t)send[e] * 2 * H + H + k4);
      const float4 m = make_float4(gate((r1.x + a2.x) + a3.x, g.x), gate((r1.y + a2.y) + a3.y, g.y), gate((r1.z + a2.z) + a3.z, g.z),
                                   gate((r1.w + a2.w) + a3.w, g.w));
      *reinterpret_cast<float4*>(d_rew1 + (size_t)e * H + k4) = m;
      sum.x += m.x; sum.y += m.y; sum.z += m.z; sum.w += m.w;
    }
  }
  *reinterpret_cast<float4*>(d_a23 + (size_t)i * 2 * H + k4) = sum;
  sum = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 a3 = *reinterpret_cast<const float4*>(a23 + (size_t)i * 2 * H + H + k4);
  const int j1 = (int)rev_ptr[i + 1];
  for (int j = (int)rev_ptr[i]; j < j1; ++j) {
    const long long e = rev_edge[j], r = recv[e];
    if (r >= n_sum) continue;          // m = +0: adding it would not change the sum (which starts at +0 and never becomes -0)
    const float4 r1 = *reinterpret_cast<const float4*>(rew1 + (size_t)e * H + k4);          // scattered rows, 16 bytes each
    const float4 a2 = *reinterpret_cast<const float4*>(a23 + (size_t)r * 2 * H + k4);
    const float4 g = *reinterpret_cast<const float4*>(d_agg + (size_t)r * H + k4);
    sum.x += gate((r1.x + a2.x) + a3.x, g.x); sum.y += gate((r1.y + a2.y) + a3.y, g.y);
    sum.z += gate((r1.z + a2.z) + a3.z, g.z); sum.w += gate((r1.w + a2.w) + a3.w, g.w);
  }
  *reinterpret_cast<float4*>(d_a23 + (size_t)i * 2 * H + H + k4) = sum;
}

// d_state[i, s] = (sum over the receiver segment of i, list order, of d_out[e, 2A + 1 + s]) - (sum over the reverse list of i, ascending e,
// of the same column): the state columns of gsr_gnn_rel_inputs are state[recv] - state[send].  One thread per (node, state column).
__global__ __launch_bounds__(256) void rel_inputs_backward_kernel(int N, int A, int S, const float* __restrict__ d_out, const long long* __restrict__ row_start,
                                                                  const long long* __restrict__ rev_ptr, const long long* __restrict__ rev_edge,
                                                                  float* __restrict__ d_state) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= N * S) return;
  const int i = o / S, Dr = 2 * A + 1 + S, c = 2 * A + 1 + (o - i * S);
  float as_recv = 0.f, as_send = 0.f;
  const int e1 = (int)row_start[i + 1];
  for (int e = (int)row_start[i]; e < e1; ++e) as_recv += d_out[(size_t)e * Dr + c];
  const int j1 = (int)rev_ptr[i + 1];
  for (int j = (int)rev_ptr[i]; j < j1; ++j) as_send += d_out[(size_t)rev_edge[j] * Dr + c];
  d_state[o] = as_recv - as_send;
}
}  // namespace gsr_gnn_bwd

extern "C" {
int gsr_gnn_aggregate_backward(int32_t n_rows, int32_t n_sum_rows, int32_t width, const float* rel_part, const float* node_parts, const int64_t* senders,
                               const int64_t* receivers, const int64_t* row_start, const int64_t* rev_ptr, const int64_t* rev_edge, const float* d_agg,
                               float* d_rel_part, float* d_node_parts, void* stream) {
  GsrRange _range("gsr_gnn_aggregate_backward");
  if (n_rows <= 0 || n_sum_rows < 0 || n_sum_rows > n_rows || width <= 0 || (width & 3) || !rel_part || !node_parts || !senders || !receivers || !row_start ||
      !rev_ptr || !rev_edge || !d_agg || !d_rel_part || !d_node_parts) {
    gsr_set_error("gsr_gnn_aggregate_backward: bad argument (width a multiple of 4)");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  { GSR_PROF("gnn_aggregate_backward", st);
    hipLaunchKernelGGL(gsr_gnn_bwd::aggregate_backward_kernel, dim3((n_rows * (width >> 2) + 255) / 256), dim3(256), 0, st, n_rows, n_sum_rows, width, rel_part,
                       node_parts, (const long long*)senders, (const long long*)receivers, (const long long*)row_start, (const long long*)rev_ptr,
                       (const long long*)rev_edge, d_agg, d_rel_part, d_node_parts); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

int gsr_gnn_rel_inputs_backward(int32_t n_rows, int32_t attr_dim, int32_t state_cols, const float* d_out, const int64_t* row_start, const int64_t* rev_ptr,
                                const int64_t* rev_edge, float* d_state, void* stream) {
  GsrRange _range("gsr_gnn_rel_inputs_backward");
  if (n_rows <= 0 || attr_dim < 0 || state_cols <= 0 || !d_out || !row_start || !rev_ptr || !rev_edge || !d_state) {
    gsr_set_error("gsr_gnn_rel_inputs_backward: bad argument");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  { GSR_PROF("gnn_rel_inputs_backward", st);
    hipLaunchKernelGGL(gsr_gnn_bwd::rel_inputs_backward_kernel, dim3((n_rows * state_cols + 255) / 256), dim3(256), 0, st, n_rows, attr_dim, state_cols, d_out,
                       (const long long*)row_start, (const long long*)rev_ptr, (const long long*)rev_edge, d_state); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}
}  // extern "C"
