// gsr_dyn_batch.hip -- the training batches of the propagation network, built on the device (gsdyn.dyn_data.make_dynamics_batch; the
// reference's DynDataset.__getitem__, /root/reference/src/data/dataset.py:332-516, for B samples at once).  Three launches:
//   dyn_sample_kernel    : one workgroup per sample -- farthest point sampling and radius thinning of the sample's cloud in LDS
//                          (gsr_fps_thin.h, the body of fps_thin_small_kernel), then the gather of the n_his + n_future frames, the noise,
//                          the rotation and every dense output of the sample.  Nothing goes through global memory between these steps.
//   dyn_relations_kernel : one workgroup per sample, one WAVE per receiver -- the relations of the noised, rotated last history frame
//                          (gsr_relations.h, four ballot masks per row, per-sample n_obj and threshold, connect_all) as padded lists, the
//                          true count and, on request, the ones of the one-hot Rr / Rs.
//   dyn_graph_kernel     : after the host has read the B counts -- the block-diagonal graph of the batch (receivers, senders, row_start,
//                          rev_ptr, rev_edge of gsdyn.dynamics.SplitGraph) from the padded lists; the sender-side reverse list by a column
//                          walk in a fixed order.
// No atomics, no sort, no float reduction whose order could vary: every output is bit-identical from run to run.  Built with
// -ffp-contract=off: the rotation and the distances are defined one fp32 operation at a time (gsdyn/dyn_data.py).
#include "gsr_common.h"
#include "gsr_relations.h"
#include "gsr_fps_thin.h"

namespace gsr_dyn_batch {

struct DynSampleArgs {
  const float* particles;       // [F, P, 3]
  const float* eef;             // [F, 3]
  const long long* pairs;       // [B, n_his + n_future]
  const int* n_particles;       // [B] or NULL (= P)
  const int* start_idx;         // [B]
  const int* thin_start;        // [B]
  const float* fps_radius;      // [B]
  const float* rot;             // [B, 9]
  const float* noise;           // [B, n_his, N, 3] or NULL
  int F, P, n_his, n_future, max_nobj;
  float* state;                 // [B, n_his, N, 3]
  float* action;                // [B, N, 3]
  float* tool_future;           // [B, n_future - 1, N, 3]
  float* action_future;         // [B, n_future - 1, N, 3]
  float* state_future;          // [B, n_future, max_nobj, 3]
  float* attrs;                 // [B, N, 2]
  float* p_instance;            // [B, max_nobj]
  unsigned char* obj_mask;      // [B, max_nobj]
  int* n_obj;                   // [B]
  long long* fps_idx;           // [B, max_nobj]
};

// x rot, one rounding per operation: out[c] = (x0 r[0][c] + x1 r[1][c]) + x2 r[2][c]
__device__ __forceinline__ void rotate_store(const float* r, float x0, float x1, float x2, float* __restrict__ out) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
    out[c] = __fadd_rn(__fadd_rn(__fmul_rn(x0, r[c]), __fmul_rn(x1, r[3 + c])), __fmul_rn(x2, r[6 + c]));
}

__global__ __launch_bounds__(FT_THREADS) void dyn_sample_kernel(DynSampleArgs a) {
  __shared__ float s_val[2][FT_THREADS / 64];
  __shared__ int s_idx[2][FT_THREADS / 64];
  __shared__ float sa[3 * 1024];          // the sample's cloud
  __shared__ float sp[3 * 256];           // the picked points, in pick order
  __shared__ int s_out[256];              // the picks (particle indices)
  __shared__ int s_thin[256];             // the kept picks, as positions in s_out; afterwards: the kept particles' indices
  __shared__ float s_rot[9];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int T = a.n_his + a.n_future, nobj = a.max_nobj, N = nobj + 1;
  const long long* pair = a.pairs + (size_t)b * T;
  const int n_p = min(max(a.n_particles ? a.n_particles[b] : a.P, 0), a.P);
  const int npoints = min(nobj, n_p);
  auto frame = [&](int t) { return (int)min(max(pair[t], 0ll), (long long)a.F - 1); };
  if (tid < 9) s_rot[tid] = a.rot[(size_t)b * 9 + tid];
  int kept = 0;
  if (npoints > 0) {      // (uniform)
    const int start = min(max(a.start_idx[b], 0), n_p - 1), thin_start = min(max(a.thin_start[b], 0), npoints - 1);
    kept = gsr_fps_thin_block(a.particles + ((size_t)frame(a.n_his - 1) * a.P) * 3, n_p, npoints, start, a.fps_radius[b], thin_start, s_out,
                              s_thin, sa, sp, s_val, s_idx, tid);
  }
  __syncthreads();
  const int src = tid < kept ? s_out[s_thin[tid]] : -1;
  __syncthreads();
  s_thin[tid] = src;
  __syncthreads();
  const float* r = s_rot;
  // ---- history: objects, zero rows, the tool; noise on every row; rotation
  for (int o = tid; o < a.n_his * N; o += FT_THREADS) {
    const int fi = o / N, row = o - fi * N, f = frame(fi);
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    if (row < kept) { const float* p = a.particles + ((size_t)f * a.P + s_thin[row]) * 3; x0 = p[0]; x1 = p[1]; x2 = p[2]; }
    else if (row == nobj) { const float* p = a.eef + (size_t)f * 3; x0 = p[0]; x1 = p[1]; x2 = p[2]; }
    const size_t at = ((size_t)b * a.n_his * N + o) * 3;
    if (a.noise) { x0 = __fadd_rn(x0, a.noise[at]); x1 = __fadd_rn(x1, a.noise[at + 1]); x2 = __fadd_rn(x2, a.noise[at + 2]); }
    rotate_store(r, x0, x1, x2, a.state + at);
  }
  // ---- action: the tool's step between the frames n_his - 1 and n_his, in the tool row
  for (int row = tid; row < N; row += FT_THREADS) {
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    if (row == nobj) {
      const float *p1 = a.eef + (size_t)frame(a.n_his) * 3, *p0 = a.eef + (size_t)frame(a.n_his - 1) * 3;
      x0 = __fsub_rn(p1[0], p0[0]); x1 = __fsub_rn(p1[1], p0[1]); x2 = __fsub_rn(p1[2], p0[2]);
    }
    rotate_store(r, x0, x1, x2, a.action + ((size_t)b * N + row) * 3);
  }
  // ---- the tool's future rows and steps
  for (int o = tid; o < (a.n_future - 1) * N; o += FT_THREADS) {
    const int fi = o / N, row = o - fi * N;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (row == nobj) {
      const float *p0 = a.eef + (size_t)frame(a.n_his + fi) * 3, *p1 = a.eef + (size_t)frame(a.n_his + fi + 1) * 3;
      t0 = p0[0]; t1 = p0[1]; t2 = p0[2];
      d0 = __fsub_rn(p1[0], p0[0]); d1 = __fsub_rn(p1[1], p0[1]); d2 = __fsub_rn(p1[2], p0[2]);
    }
    const size_t at = ((size_t)b * (a.n_future - 1) * N + o) * 3;
    rotate_store(r, t0, t1, t2, a.tool_future + at);
    rotate_store(r, d0, d1, d2, a.action_future + at);
  }
  // ---- the objects' future frames
  for (int o = tid; o < a.n_future * nobj; o += FT_THREADS) {
    const int fi = o / nobj, row = o - fi * nobj;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    if (row < kept) { const float* p = a.particles + ((size_t)frame(a.n_his + fi) * a.P + s_thin[row]) * 3; x0 = p[0]; x1 = p[1]; x2 = p[2]; }
    rotate_store(r, x0, x1, x2, a.state_future + ((size_t)b * a.n_future * nobj + o) * 3);
  }
  // ---- attributes, instance, masks, indices
  for (int row = tid; row < N; row += FT_THREADS) {
    float* at = a.attrs + ((size_t)b * N + row) * 2;
    at[0] = row < kept ? 1.0f : 0.0f;
    at[1] = row == nobj ? 1.0f : 0.0f;
    if (row < nobj) {
      a.p_instance[(size_t)b * nobj + row] = row < kept ? 1.0f : 0.0f;
      a.obj_mask[(size_t)b * nobj + row] = row < kept ? 1 : 0;
      a.fps_idx[(size_t)b * nobj + row] = row < kept ? (long long)s_thin[row] : -1ll;
    }
  }
  if (tid == 0) a.n_obj[b] = kept;
}

#define DR_THREADS 1024
__global__ __launch_bounds__(DR_THREADS) void dyn_relations_kernel(const float* __restrict__ state, int n_his, int max_nobj,
                                                                 const int* __restrict__ n_obj, const float* __restrict__ adj_thresh, int topk,
                                                                 int connect_all, int max_nR, long long* __restrict__ recv,
                                                                 long long* __restrict__ send, int* __restrict__ n_rel, float* __restrict__ Rr,
                                                                 float* __restrict__ Rs) {
  __shared__ float sp[3 * 256];
  __shared__ unsigned long long s_mask[256][4];      // row i: which senders it is related to
  __shared__ int s_base[256];
  __shared__ int s_total;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
  const int N = max_nobj + 1, n_valid = min(max(n_obj[b], 0), max_nobj);
  const float* pos = state + ((size_t)b * n_his + (n_his - 1)) * N * 3;
  const float t = adj_thresh[b], thr2 = __fmul_rn(t, t);
  if (tid < 3 * N) sp[tid] = pos[tid];
  __syncthreads();
  const int k = min(min(topk, GSR_REL_MAXK), n_valid);
  for (int i = wv; i < N; i += DR_THREADS / 64) {
    unsigned long long m[4];
    gsr_rel4_row_masks(sp, i, lane, N, max_nobj, n_valid, thr2, k, connect_all != 0, m);
    if (lane < 4) s_mask[i][lane] = m[lane];
  }
  __syncthreads();
  if (wv == 0) {
    const int tot = gsr_rel4_scan_rows(s_mask, lane, N, s_base);
    if (lane == 63) s_total = tot;
  }
  __syncthreads();
  const int total = s_total;
  long long *rb = recv + (size_t)b * max_nR, *sb = send + (size_t)b * max_nR;
  float *Rrb = Rr ? Rr + (size_t)b * max_nR * N : nullptr, *Rsb = Rs ? Rs + (size_t)b * max_nR * N : nullptr;
  for (int i = wv; i < N; i += DR_THREADS / 64) {
    const unsigned long long m[4] = {s_mask[i][0], s_mask[i][1], s_mask[i][2], s_mask[i][3]};
    gsr_rel4_write_row(m, i, lane, s_base[i], max_nR, N, rb, sb, Rrb, Rsb);
  }
  if (tid == 0) n_rel[b] = total;          // the TRUE count: the caller raises when it exceeds max_nR
  for (int e = total + tid; e < max_nR; e += DR_THREADS) { rb[e] = N; sb[e] = N; }
}

// Block b = sample b: its n = n_rel[b] list entries go to offs[b] .. offs[b] + n of the batch's list, in rows b N + local row.
__global__ __launch_bounds__(256) void dyn_graph_kernel(int B, int N, int max_nR, const long long* __restrict__ recv_pad,
                                                      const long long* __restrict__ send_pad, const int* __restrict__ n_rel,
                                                      const long long* __restrict__ offs, long long* __restrict__ receivers,
                                                      long long* __restrict__ senders, long long* __restrict__ row_start,
                                                      long long* __restrict__ rev_ptr, long long* __restrict__ rev_edge) {
  __shared__ int s_cnt[256];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n = min(max(n_rel[b], 0), max_nR);
  const long long off = offs[b], row0 = (long long)b * N;
  const long long *rp = recv_pad + (size_t)b * max_nR, *sp = send_pad + (size_t)b * max_nR;
  for (int e = tid; e < n; e += 256) { receivers[off + e] = row0 + rp[e]; senders[off + e] = row0 + sp[e]; }
  // row_start: the first entry whose receiver is not below the row (the list ascends in the receiver)
  int cnt = 0;
  if (tid < N) {
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (rp[mid] < tid) lo = mid + 1; else hi = mid;
    }
    row_start[row0 + tid] = off + lo;
    // column walk: how many entries this row SENDS
    for (int e = 0; e < n; ++e) cnt += sp[e] == tid ? 1 : 0;
  }
  s_cnt[tid] = cnt;
  __syncthreads();
  if (tid < N) {
    int before = 0;
    for (int j = 0; j < tid; ++j) before += s_cnt[j];
    rev_ptr[row0 + tid] = off + before;
    long long* out = rev_edge + off + before;
    int w = 0;
    for (int e = 0; e < n; ++e)
      if (sp[e] == tid) out[w++] = off + e;          // ascending entry ids within a sender, as a stable sort by sender leaves them
  }
  if (b == B - 1 && tid == 0) { row_start[(long long)B * N] = off + n; rev_ptr[(long long)B * N] = off + n; }
}

}  // namespace gsr_dyn_batch
using namespace gsr_dyn_batch;

int gsr_dyn_batch_sample(int32_t B, int32_t F, int32_t P, int32_t n_his, int32_t n_future, int32_t max_nobj, const float* particles,
                         const float* eef, const int64_t* pairs, const int32_t* n_particles, const int32_t* start_idx, const int32_t* thin_start,
                         const float* fps_radius, const float* rot, const float* noise, float* state, float* action, float* tool_future,
                         float* action_future, float* state_future, float* attrs, float* p_instance, uint8_t* obj_mask, int32_t* n_obj,
                         int64_t* fps_idx, void* stream) {
  GsrRange _range("gsr_dyn_batch_sample");
  if (B < 1 || F < 1 || P < 1 || P > GSR_DYN_MAX_P || n_his < 1 || n_future < 1 || max_nobj < 1 || max_nobj > GSR_DYN_MAX_NOBJ) {
    gsr_set_error("gsr_dyn_batch_sample: bad argument (B, F >= 1, 1 <= P <= %d, n_his, n_future >= 1, 1 <= max_nobj <= %d; got B = %d, F = %d, "
                  "P = %d, n_his = %d, n_future = %d, max_nobj = %d)", GSR_DYN_MAX_P, GSR_DYN_MAX_NOBJ, (int)B, (int)F, (int)P, (int)n_his,
                  (int)n_future, (int)max_nobj);
    return -2;
  }
  if (!particles || !eef || !pairs || !start_idx || !thin_start || !fps_radius || !rot || !state || !action || !state_future || !attrs ||
      !p_instance || !obj_mask || !n_obj || !fps_idx || (n_future > 1 && (!tool_future || !action_future))) {
    gsr_set_error("gsr_dyn_batch_sample: NULL pointer");
    return -2;
  }
  if ((long long)B * (n_his + n_future) * (max_nobj + 1) * 3 > 0x7fffffffll || (long long)F * P * 3 > 0x7fffffffffffll) {
    gsr_set_error("gsr_dyn_batch_sample: the batch exceeds 2^31 elements");
    return -2;
  }
  DynSampleArgs a;
  a.particles = particles; a.eef = eef; a.pairs = (const long long*)pairs; a.n_particles = n_particles; a.start_idx = start_idx;
  a.thin_start = thin_start; a.fps_radius = fps_radius; a.rot = rot; a.noise = noise;
  a.F = F; a.P = P; a.n_his = n_his; a.n_future = n_future; a.max_nobj = max_nobj;
  a.state = state; a.action = action; a.tool_future = tool_future; a.action_future = action_future; a.state_future = state_future;
  a.attrs = attrs; a.p_instance = p_instance; a.obj_mask = obj_mask; a.n_obj = n_obj; a.fps_idx = (long long*)fps_idx;
  hipStream_t st = (hipStream_t)stream;
  { GSR_PROF("dyn_sample", st);
    hipLaunchKernelGGL(dyn_sample_kernel, dim3(B), dim3(FT_THREADS), 0, st, a); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

int gsr_dyn_batch_relations(int32_t B, int32_t n_his, int32_t max_nobj, const float* state, const int32_t* n_obj, const float* adj_thresh,
                            int32_t topk, int32_t connect_all, int32_t max_nR, int64_t* receivers, int64_t* senders, int32_t* n_rel, float* Rr,
                            float* Rs, void* stream) {
  GsrRange _range("gsr_dyn_batch_relations");
  if (B < 1 || n_his < 1 || max_nobj < 1 || max_nobj > GSR_DYN_MAX_NOBJ || topk < 1 || topk > GSR_REL_MAXK || max_nR < 0 ||
      (long long)B * max_nR * (max_nobj + 1) > 0x7fffffffffffll) {
    gsr_set_error("gsr_dyn_batch_relations: bad argument (B, n_his >= 1, 1 <= max_nobj <= %d, 1 <= topk <= %d, max_nR >= 0; got B = %d, "
                  "n_his = %d, max_nobj = %d, topk = %d, max_nR = %d)", GSR_DYN_MAX_NOBJ, GSR_REL_MAXK, (int)B, (int)n_his, (int)max_nobj,
                  (int)topk, (int)max_nR);
    return -2;
  }
  if (!state || !n_obj || !adj_thresh || !n_rel || (max_nR > 0 && (!receivers || !senders)) || ((Rr == nullptr) != (Rs == nullptr))) {
    gsr_set_error("gsr_dyn_batch_relations: NULL pointer (Rr and Rs: both or neither)");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  { GSR_PROF("dyn_relations", st);
    hipLaunchKernelGGL(dyn_relations_kernel, dim3(B), dim3(DR_THREADS), 0, st, state, n_his, max_nobj, n_obj, adj_thresh, topk, connect_all,
                       max_nR, (long long*)receivers, (long long*)senders, n_rel, Rr, Rs); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

int gsr_dyn_batch_graph(int32_t B, int32_t n_rows, int32_t max_nR, const int64_t* receivers_padded, const int64_t* senders_padded,
                        const int32_t* n_rel, const int64_t* offsets, int64_t* receivers, int64_t* senders, int64_t* row_start,
                        int64_t* rev_ptr, int64_t* rev_edge, void* stream) {
  GsrRange _range("gsr_dyn_batch_graph");
  if (B < 1 || n_rows < 2 || n_rows > GSR_DYN_MAX_NOBJ + 1 || max_nR < 0) {
    gsr_set_error("gsr_dyn_batch_graph: bad argument (B >= 1, 2 <= n_rows <= %d, max_nR >= 0; got B = %d, n_rows = %d, max_nR = %d)",
                  GSR_DYN_MAX_NOBJ + 1, (int)B, (int)n_rows, (int)max_nR);
    return -2;
  }
  if (!n_rel || !offsets || !row_start || !rev_ptr || (max_nR > 0 && (!receivers_padded || !senders_padded))) {
    gsr_set_error("gsr_dyn_batch_graph: NULL pointer");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  { GSR_PROF("dyn_graph", st);
    hipLaunchKernelGGL(dyn_graph_kernel, dim3(B), dim3(256), 0, st, B, n_rows, max_nR, (const long long*)receivers_padded,
                       (const long long*)senders_padded, n_rel, (const long long*)offsets, (long long*)receivers, (long long*)senders,
                       (long long*)row_start, (long long*)rev_ptr, (long long*)rev_edge); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}
