// gsr_knn.hip -- exact k-nearest-neighbour search over a point cloud (gsdyn.knn_points).
//
// Definition (include/gsr.h): d2(i, j) = (dx*dx + dy*dy) + dz*dz with dx = p[i].x - p[j].x .., fp32, unfused (this object is built with
// -ffp-contract=off); row i = the k smallest (d2, j) under the total order "d2 ascending, then j ascending", in that order.
//
// Two search kernels, ONE list and ONE order:
//   knn_brute_kernel : a wave per query walks all N points.  Serves every query for N <= KNN_BRUTE_N, the 256 sample queries of the
//                      cell-size rule, and the rows the grid kernel flagged.
//   knn_grid_kernel  : a wave per query (queries in cell order) walks a uniform grid in shells of growing Chebyshev radius.
// The running best-k is a sorted list, one entry per lane (hence k <= 64): lane l < k holds the l-th smallest (d2, j) seen so far, the
// lanes from k on a sentinel (+inf, INT_MAX).  64 candidates are tested at once; one that beats the k-th is inserted with a ballot (who
// beats the k-th), a popcount (how many list entries precede it) and a one-lane shift of the tail.  No array is indexed dynamically.
//
// Grid.  Cell of a point, per axis: c = clamp(int(floor(fl(fl(p - o) * inv_h))), 0, G - 1), o = the exact minimum of the coordinate.
// Cells live in an open-addressing hash table of M = pow2 >= 2 N slots (key = the three 20-bit cell coordinates), so memory is O(N)
// whatever the box's extent.  Build: insert (64-bit compare-and-swap) + count per slot, a range of the sorted array per occupied slot (a
// wave-aggregated integer cursor), scatter.  The order of the cells and of the points inside a cell depends on scheduling and does NOT
// reach the result: every candidate of a visited cell goes through the same total order.
//
// The bound.  After shell r the wave has seen every point whose cell lies in the block [cq - r, cq + r]^3 around the query's cell cq.  A point
// p outside has, on some axis, c_p >= cq + r + 1 or c_p <= cq - r - 1; take the first (the other is symmetric).  Write t(x) = fl(fl(x - o)
// * inv_h): both roundings are monotone, so t is monotone, t >= 0 (o is the minimum), and
//     t(x) = (x - o) inv_h (1 + e1)(1 + e2),  |e| <= 2^-24          (a subnormal difference is exact; a product that underflows is off by
//                                                                     less than 2^-149 cells, far inside the slack below)
// c_p >= B := cq + r + 1 gives t(p) >= B (a coordinate clamped up from a negative t is cell 0, never >= B >= 1), and t(q) < cq + 1 (a query
// clamped down to G - 1 has nobody beyond).  With h' = 1 / inv_h (the real reciprocal of the fp32 number):
//     p - q = h' [ t(p) / ((1+e1)(1+e2)) - t(q) / ((1+e1')(1+e2')) ] >= h' [ B (1 - 2^-22) - (cq + 1)(1 + 2^-22) ] >= h' (r - G 2^-21)
// since B and cq + 1 are at most G.  That is the slack: G 2^-21 cells, at most one half because G <= 2^20.  The fp32 d2 of such a pair is
// at least the rounded square of that one axis (the other terms are >= 0 and every rounding is monotone), and five roundings cost a factor
// >= 1 - 6 2^-24.  Hence
//     bound2[r] = round_down_to_fp32( (h' (r - G 2^-21))^2 (1 - 2^-20) )      (evaluated in fp64 by one thread, 0 if r <= G 2^-21)
// is a lower bound on the COMPUTED d2 of every unvisited point.  The search ends when the list is full and its k-th d2 is STRICTLY below
// bound2[r] (an unvisited tie of lower index cannot exist then), or when the block covers the grid.  A query not finished after KNN_MAXR
// shells is flagged and finished by the brute-force kernel, which is launched over all rows; unflagged rows leave at once.
//
// Cell size: h = scale x median over 256 sample queries (every (N / 256)-th point) of their exact k-th neighbour distance -- measured on
// the cloud itself, so a sheet, a volume and a box stretched by outliers all get cells that hold the k nearest in the first shell or
// two (DESIGN.md section 3k has the measurements).  h is clamped so that no axis has more than 2^20 cells; zero extent gives one cell.
//
// Scratch layout (gsr_knn_scratch_bytes; every part 256-byte aligned): header (256 B) | info u32[N] | samples f32[256] | keys u64[M] |
// count u32[M] | end u32[M] | slot u32[N] | sorted float4[N].  info[i] = shells walked | 0x80000000 if the brute-force pass finished row i
// (read by tools/knn_cost.py through _hip.knn(stats=True)).
#include "gsr_common.h"
#include "gsr_hashgrid.h"
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>

namespace gsr_knn_ns {

#define KNN_THREADS 256
#define KNN_WAVES (KNN_THREADS / 64)
#define KNN_BRUTE_N 2048     // up to here every query takes the brute-force kernel: at most 32 steps of 64 candidates per query, less
                             // than the grid's eight build launches cost
#define KNN_SAMPLES 256
#define KNN_MAXR 3           // shells before a query is handed to the brute-force pass: 27 + 98 + 218 cells
#define KNN_MAXG (1 << 20)
#define KNN_EMPTY GSR_HASH_EMPTY
#define KNN_FLAG 0x80000000u

struct KnnHeader {           // 256 bytes of device memory at the front of the scratch
  float ox, oy, oz, inv_h;
  int gx, gy, gz, pad0;
  float bound2[4];           // [r], r = 1 .. KNN_MAXR
  float h, med_d2;
  uint32_t cursor;           // next free position of the sorted array (range allocation)
  uint32_t occupied;         // occupied cells
};

struct KnnScratch {
  KnnHeader* hdr; uint32_t* info; float* samp; unsigned long long* keys; uint32_t* cnt; uint32_t* endp; uint32_t* slot; float4* sorted;
  uint32_t M;
};
static inline uint32_t knn_table_size(int32_t N) {
  uint32_t M = 1024;
  while (M < 2u * (uint32_t)N) M <<= 1;
  return M;
}
static inline size_t knn_carve(void* base, int32_t N, KnnScratch* s) {
  size_t off = 0, Nn = (size_t)(N > 0 ? N : 1);
  char* b = (char*)base;
  auto take = [&](size_t bytes) { char* p = b ? b + off : nullptr; off += gsr_align(bytes); return p; };
  s->M = knn_table_size((int32_t)Nn);
  s->hdr = (KnnHeader*)take(256);
  s->info = (uint32_t*)take(Nn * 4);
  s->samp = (float*)take(KNN_SAMPLES * 4);
  s->keys = (unsigned long long*)take((size_t)s->M * 8);
  s->cnt = (uint32_t*)take((size_t)s->M * 4);
  s->endp = (uint32_t*)take((size_t)s->M * 4);
  s->slot = (uint32_t*)take(Nn * 4);
  s->sorted = (float4*)take(Nn * 16);
  return off;
}

// ---------------------------------------------------------------- the list
// (d, j) precedes (e, i) in the total order; a NaN distance precedes nothing and is preceded by nothing
__device__ __forceinline__ bool knn_less(float d, int j, float e, int i) { return d < e || (d == e && j < i); }

struct KnnList {
  float d; int j;            // this lane's entry
  float kd; int kj;          // the k-th entry (wave-uniform)
};
__device__ __forceinline__ void knn_init(KnnList& L) { L.d = L.kd = __builtin_inff(); L.j = L.kj = INT_MAX; }

// Offer one candidate per lane (valid: this lane has one).  Must be called by the whole wave.
__device__ __forceinline__ void knn_offer(KnnList& L, float cd, int cj, bool valid, int k, int lane) {
  unsigned long long pend = __ballot(valid && knn_less(cd, cj, L.kd, L.kj));
  while (pend) {
    const int s = __ffsll((long long)pend) - 1;                       // wave-uniform
    const float d = __shfl(cd, s, 64);
    const int j = __shfl(cj, s, 64);
    const int pos = __popcll(__ballot(knn_less(L.d, L.j, d, j)));     // entries in front of it (a sentinel is in front of nothing): pos < k
    const float ud = __shfl_up(L.d, 1, 64);
    const int uj = __shfl_up(L.j, 1, 64);
    if (lane < k) {
      if (lane == pos) { L.d = d; L.j = j; }
      else if (lane > pos) { L.d = ud; L.j = uj; }
    }
    L.kd = __shfl(L.d, k - 1, 64);
    L.kj = __shfl(L.j, k - 1, 64);
    pend &= pend - 1;
    pend &= __ballot(valid && knn_less(cd, cj, L.kd, L.kj));
  }
}
__device__ __forceinline__ void knn_store(const KnnList& L, int N, int k, int lane, int qi, long long* __restrict__ out_idx, float* __restrict__ out_d2) {
  if (lane < k) {
    out_idx[(size_t)qi * k + lane] = (long long)(L.j < N ? L.j : 0);    // (a sentinel only in rows with non-finite coordinates)
    out_d2[(size_t)qi * k + lane] = L.d;
  }
}
__device__ __forceinline__ float knn_d2(float qx, float qy, float qz, float px, float py, float pz) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

// ---------------------------------------------------------------- brute force
// info != nullptr: only the rows with KNN_FLAG set.  sample_stride > 0: query w is point w * sample_stride, w < KNN_SAMPLES, and only the
// k-th d2 is written (samp[w]).
__global__ __launch_bounds__(KNN_THREADS) void knn_brute_kernel(int N, int k, int excl, const float* __restrict__ pts, const uint32_t* __restrict__ info,
                                                               int sample_stride, float* __restrict__ samp, long long* __restrict__ out_idx,
                                                               float* __restrict__ out_d2) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * KNN_WAVES + (threadIdx.x >> 6);
  int qi;
  if (sample_stride > 0) {
    if (w >= KNN_SAMPLES) return;
    qi = (int)w * sample_stride;
    if (qi >= N) qi = N - 1;
  } else {
    if (w >= N) return;
    qi = (int)w;
    if (info && !(info[qi] & KNN_FLAG)) return;
  }
  const float qx = pts[3 * (size_t)qi], qy = pts[3 * (size_t)qi + 1], qz = pts[3 * (size_t)qi + 2];
  KnnList L;
  knn_init(L);
  for (int base = 0; base < N; base += 256) {           // four independent loads per lane in flight
    float cd[4]; int cj[4]; bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = base + u * 64 + lane;
      cj[u] = j;
      ok[u] = j < N && !(excl && j == qi);
      const size_t a = 3 * (size_t)(j < N ? j : N - 1);
      cd[u] = knn_d2(qx, qy, qz, pts[a], pts[a + 1], pts[a + 2]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) knn_offer(L, cd[u], cj[u], ok[u], k, lane);
  }
  if (sample_stride > 0) {
    if (lane == 0) samp[w] = L.kd;
  } else {
    knn_store(L, N, k, lane, qi, out_idx, out_d2);
  }
}

// ---------------------------------------------------------------- grid build
__device__ __forceinline__ int knn_cell(float p, float o, float inv_h, int G) {
  const float t = floorf((p - o) * inv_h);
  int c = 0;                                            // t < 1 and NaN
  if (t >= 1.0f) c = t >= (float)(G - 1) ? G - 1 : (int)t;
  return c;
}
__device__ __forceinline__ unsigned long long knn_key(int cx, int cy, int cz) {
  return ((unsigned long long)cx << 40) | ((unsigned long long)cy << 20) | (unsigned long long)cz;
}

// One workgroup: bounding box, the median of the samples, the header.
#define KNN_SETUP_THREADS 1024
__global__ __launch_bounds__(KNN_SETUP_THREADS) void knn_setup_kernel(int N, const float* __restrict__ pts, const float* __restrict__ samp, float scale,
                                                                      KnnHeader* __restrict__ hdr) {
  __shared__ float s_red[6][KNN_SETUP_THREADS / 64];
  __shared__ float s_samp[KNN_SAMPLES];
  __shared__ float s_med;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float inf = __builtin_inff();
  float v[6] = {inf, inf, inf, -inf, -inf, -inf};
  for (int i = tid; i < N; i += KNN_SETUP_THREADS) {
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    v[0] = fminf(v[0], x); v[1] = fminf(v[1], y); v[2] = fminf(v[2], z);
    v[3] = fmaxf(v[3], x); v[4] = fmaxf(v[4], y); v[5] = fmaxf(v[5], z);
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    float r = v[c];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const float o = __shfl_xor(r, off, 64); r = c < 3 ? fminf(r, o) : fmaxf(r, o); }
    if (lane == 0) s_red[c][wv] = r;
  }
  if (tid < KNN_SAMPLES) s_samp[tid] = samp[tid];
  if (tid == 0) s_med = 0.0f;
  __syncthreads();
  if (tid < KNN_SAMPLES) {                               // rank by counting: the sample of rank 128 is the (upper) median
    const float mine = s_samp[tid];
    int rank = 0;
    for (int j = 0; j < KNN_SAMPLES; ++j) { const float o = s_samp[j]; rank += (o < mine || (o == mine && j < tid)) ? 1 : 0; }
    if (rank == KNN_SAMPLES / 2) s_med = mine;
  }
  __syncthreads();
  if (tid == 0) {
    float b[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      b[c] = s_red[c][0];
      for (int w = 1; w < KNN_SETUP_THREADS / 64; ++w) b[c] = c < 3 ? fminf(b[c], s_red[c][w]) : fmaxf(b[c], s_red[c][w]);
    }
    float ext = fmaxf(fmaxf(b[3] - b[0], b[4] - b[1]), b[5] - b[2]);
    if (!(ext >= 0.0f) || ext == inf) ext = 0.0f;        // nothing finite to build on: one cell
    float h = scale * sqrtf(s_med);
    const float hmin = ext / 1048000.0f;                 // no axis above 2^20 cells
    if (!(h >= hmin)) h = hmin;
    float inv_h = 1.0f / h;
    if (!(h > 0.0f) || h == inf || inv_h == inf || ext == 0.0f) { h = 1.0f; inv_h = 1.0f; }
    hdr->ox = b[0]; hdr->oy = b[1]; hdr->oz = b[2]; hdr->inv_h = inv_h;
    // cells per axis: the cell of the maximum, by the points' own expression (monotone: no point lands beyond it), plus one
    const int gx = knn_cell(b[3], b[0], inv_h, KNN_MAXG) + 1, gy = knn_cell(b[4], b[1], inv_h, KNN_MAXG) + 1, gz = knn_cell(b[5], b[2], inv_h, KNN_MAXG) + 1;
    hdr->gx = gx; hdr->gy = gy; hdr->gz = gz; hdr->pad0 = 0;
    const int gm = max(gx, max(gy, gz));
    const double hp = 1.0 / (double)inv_h;
    hdr->bound2[0] = 0.0f;
    for (int r = 1; r <= KNN_MAXR; ++r) {
      const double s = (double)r - (double)gm * (1.0 / 2097152.0);
      float f = 0.0f;
      if (s > 0.0) {
        const double b2 = (hp * s) * (hp * s) * (1.0 - 1.0 / 1048576.0);
        f = b2 >= (double)FLT_MAX ? FLT_MAX : (float)b2;
        if ((double)f > b2) f = nextafterf(f, 0.0f);      // round down
      }
      hdr->bound2[r] = f;
    }
    hdr->h = h; hdr->med_d2 = s_med; hdr->cursor = 0u; hdr->occupied = 0u;
  }
}

__global__ __launch_bounds__(KNN_THREADS) void knn_insert_kernel(int N, const float* __restrict__ pts, const KnnHeader* __restrict__ hdr,
                                                                unsigned long long* __restrict__ keys, uint32_t* __restrict__ cnt, uint32_t mask,
                                                                uint32_t* __restrict__ slot) {
  const long long i = (long long)blockIdx.x * KNN_THREADS + threadIdx.x;
  if (i >= N) return;
  const float inv_h = hdr->inv_h;
  const unsigned long long key = knn_key(knn_cell(pts[3 * (size_t)i], hdr->ox, inv_h, hdr->gx), knn_cell(pts[3 * (size_t)i + 1], hdr->oy, inv_h, hdr->gy),
                                         knn_cell(pts[3 * (size_t)i + 2], hdr->oz, inv_h, hdr->gz));
  const uint32_t s = gsr_hash_insert(keys, mask, key);   // (gsr_hashgrid.h) at most N <= M / 2 distinct keys: an empty slot always turns up
  atomicAdd(&cnt[s], 1u);
  slot[i] = s;
}

// A range of the sorted array for every occupied slot: a wave adds up its 64 counts and takes ONE step of the cursor.
__global__ __launch_bounds__(KNN_THREADS) void knn_alloc_kernel(uint32_t M, const uint32_t* __restrict__ cnt, uint32_t* __restrict__ endp, KnnHeader* __restrict__ hdr) {
  const uint32_t s = blockIdx.x * KNN_THREADS + threadIdx.x;      // M is a multiple of KNN_THREADS
  const int lane = threadIdx.x & 63;
  const uint32_t c = s < M ? cnt[s] : 0u;
  uint32_t incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
  const unsigned long long occ = __ballot(c > 0u);
  uint32_t base = 0;
  if (lane == 63 && incl > 0u) { base = atomicAdd(&hdr->cursor, incl); atomicAdd(&hdr->occupied, (uint32_t)__popcll(occ)); }
  base = __shfl(base, 63, 64);
  if (s < M) endp[s] = base + incl - c;                            // the range's start; the scatter moves it to the range's end
}

__global__ __launch_bounds__(KNN_THREADS) void knn_scatter_kernel(int N, const float* __restrict__ pts, const uint32_t* __restrict__ slot, uint32_t* __restrict__ endp,
                                                                 float4* __restrict__ sorted) {
  const long long i = (long long)blockIdx.x * KNN_THREADS + threadIdx.x;
  if (i >= N) return;
  uint32_t pos = atomicAdd(&endp[slot[i]], 1u);
  if (pos >= (uint32_t)N) pos = (uint32_t)N - 1u;                  // (cannot happen: the counts add up to N)
  sorted[pos] = make_float4(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], __int_as_float((int)i));
}

// ---------------------------------------------------------------- grid search
__global__ __launch_bounds__(KNN_THREADS) void knn_grid_kernel(int N, int k, int excl, const KnnHeader* __restrict__ hdr, const float4* __restrict__ sorted,
                                                              const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ cnt,
                                                              const uint32_t* __restrict__ endp, uint32_t mask, uint32_t* __restrict__ info,
                                                              long long* __restrict__ out_idx, float* __restrict__ out_d2) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * KNN_WAVES + (threadIdx.x >> 6);
  if (w >= N) return;
  const float4 q = sorted[w];
  int qi = __float_as_int(q.w);
  if ((unsigned)qi >= (unsigned)N) qi = 0;                          // (cannot happen)
  const int gx = hdr->gx, gy = hdr->gy, gz = hdr->gz;
  const float inv_h = hdr->inv_h;
  const int cqx = knn_cell(q.x, hdr->ox, inv_h, gx), cqy = knn_cell(q.y, hdr->oy, inv_h, gy), cqz = knn_cell(q.z, hdr->oz, inv_h, gz);
  KnnList L;
  knn_init(L);
  bool done = false;
  int r = 1;
  for (; r <= KNN_MAXR; ++r) {
    const int side = 2 * r + 1, ncell = side * side * side;
    for (int cb = 0; cb < ncell; cb += 64) {
      // one cell of the shell per lane: its range of the sorted array (r = 1 takes the centre cell along)
      const int c = cb + lane;
      uint32_t count = 0, start = 0;
      if (c < ncell) {
        const int dz = c % side - r, dy = (c / side) % side - r, dx = c / (side * side) - r;
        const int m = max(abs(dx), max(abs(dy), abs(dz)));
        const int x = cqx + dx, y = cqy + dy, z = cqz + dz;
        if ((r == 1 || m == r) && x >= 0 && x < gx && y >= 0 && y < gy && z >= 0 && z < gz) {
          const unsigned long long key = knn_key(x, y, z);
          uint32_t s = gsr_hash64(key, mask);
          for (uint32_t probe = 0; probe <= mask; ++probe) {
            const unsigned long long kk = keys[s];
            if (kk == key) { count = cnt[s]; start = endp[s] - count; break; }
            if (kk == KNN_EMPTY) break;
            s = (s + 1) & mask;
          }
        }
      }
      uint32_t incl = count;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
      const uint32_t T = __shfl(incl, 63, 64);
      const uint32_t excl_sum = incl - count;
      for (uint32_t base = 0; base < T; base += 64) {
        const uint32_t t = base + lane;
        bool valid = t < T;
        int lo = 0;                                                   // lanes whose inclusive sum is <= t: the lane that owns candidate t
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) { const uint32_t v = __shfl(incl, (lo + step - 1) & 63, 64); if (v <= t) lo += step; }
        lo &= 63;
        const uint32_t st = __shfl(start, lo, 64), ex = __shfl(excl_sum, lo, 64);
        uint32_t a = st + (t - ex);
        if (!valid || a >= (uint32_t)N) a = (uint32_t)N - 1u;        // never an address outside the array
        const float4 p = sorted[a];
        const int j = __float_as_int(p.w);
        valid = valid && !(excl && j == qi);
        knn_offer(L, knn_d2(q.x, q.y, q.z, p.x, p.y, p.z), j, valid, k, lane);
      }
    }
    const bool covers = cqx - r <= 0 && cqx + r >= gx - 1 && cqy - r <= 0 && cqy + r >= gy - 1 && cqz - r <= 0 && cqz + r >= gz - 1;
    if ((L.kj != INT_MAX && L.kd < hdr->bound2[r]) || covers) { done = true; break; }
  }
  if (lane == 0) info[qi] = (uint32_t)(done ? r : KNN_MAXR) | (done ? 0u : KNN_FLAG);
  if (done) knn_store(L, N, k, lane, qi, out_idx, out_d2);
}

}  // namespace gsr_knn_ns

extern "C" {

size_t gsr_knn_scratch_bytes(int32_t N) {
  gsr_knn_ns::KnnScratch s;
  return gsr_knn_ns::knn_carve(nullptr, N, &s);
}

int gsr_knn(int32_t N, const float* points, int32_t k, int32_t exclude_self, void* scratch, int64_t* out_idx, float* out_d2, void* stream) {
  using namespace gsr_knn_ns;
  GsrRange _range("gsr_knn");
  if (N < 1 || N > (1 << 28) || k < 1 || k > 64 || (long long)k > (long long)N - (exclude_self ? 1 : 0)) {
    gsr_set_error("gsr_knn: bad argument (1 <= N <= 2^28, 1 <= k <= 64, k <= N - (exclude_self ? 1 : 0); got N = %d, k = %d, exclude_self = %d)", (int)N,
                  (int)k, (int)exclude_self);
    return -2;
  }
  if (!points || !scratch || !out_idx || !out_d2) {
    gsr_set_error("gsr_knn: NULL pointer");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  const int excl = exclude_self ? 1 : 0;
  const unsigned qblocks = (unsigned)(((long long)N + KNN_WAVES - 1) / KNN_WAVES), pblocks = (unsigned)(((long long)N + KNN_THREADS - 1) / KNN_THREADS);
  if (N <= KNN_BRUTE_N) {
    GSR_PROF("knn_brute", st);
    hipLaunchKernelGGL(knn_brute_kernel, dim3(qblocks), dim3(KNN_THREADS), 0, st, N, k, excl, points, (const uint32_t*)nullptr, 0, (float*)nullptr,
                       (long long*)out_idx, out_d2);
    GSR_HIP_CHECK(hipGetLastError());
    return 0;
  }
  float scale = 1.0f;                                     // the cell-size rule's factor; the override is for measuring
  if (const char* e = getenv("GSR_KNN_CELL_SCALE")) {
    const float v = (float)atof(e);
    if (v >= 0.125f && v <= 16.0f) scale = v;
  }
  KnnScratch s;
  knn_carve(scratch, N, &s);
  const uint32_t mask = s.M - 1u;
  GSR_HIP_CHECK(hipMemsetAsync(s.keys, 0xff, (size_t)s.M * 8, st));
  GSR_HIP_CHECK(hipMemsetAsync(s.cnt, 0, (size_t)((char*)s.slot - (char*)s.cnt), st));      // count and end
  { GSR_PROF("knn_sample", st);
    hipLaunchKernelGGL(knn_brute_kernel, dim3(KNN_SAMPLES / KNN_WAVES), dim3(KNN_THREADS), 0, st, N, k, excl, points, (const uint32_t*)nullptr,
                       N / KNN_SAMPLES, s.samp, (long long*)nullptr, (float*)nullptr); }
  { GSR_PROF("knn_setup", st);
    hipLaunchKernelGGL(knn_setup_kernel, dim3(1), dim3(KNN_SETUP_THREADS), 0, st, N, points, (const float*)s.samp, scale, s.hdr); }
  { GSR_PROF("knn_insert", st);
    hipLaunchKernelGGL(knn_insert_kernel, dim3(pblocks), dim3(KNN_THREADS), 0, st, N, points, (const KnnHeader*)s.hdr, s.keys, s.cnt, mask, s.slot); }
  { GSR_PROF("knn_alloc", st);
    hipLaunchKernelGGL(knn_alloc_kernel, dim3(s.M / KNN_THREADS), dim3(KNN_THREADS), 0, st, s.M, (const uint32_t*)s.cnt, s.endp, s.hdr); }
  { GSR_PROF("knn_scatter", st);
    hipLaunchKernelGGL(knn_scatter_kernel, dim3(pblocks), dim3(KNN_THREADS), 0, st, N, points, (const uint32_t*)s.slot, s.endp, s.sorted); }
  { GSR_PROF("knn_grid", st);
    hipLaunchKernelGGL(knn_grid_kernel, dim3(qblocks), dim3(KNN_THREADS), 0, st, N, k, excl, (const KnnHeader*)s.hdr, (const float4*)s.sorted,
                       (const unsigned long long*)s.keys, (const uint32_t*)s.cnt, (const uint32_t*)s.endp, mask, s.info, (long long*)out_idx, out_d2); }
  { GSR_PROF("knn_brute", st);
    hipLaunchKernelGGL(knn_brute_kernel, dim3(qblocks), dim3(KNN_THREADS), 0, st, N, k, excl, points, (const uint32_t*)s.info, 0, (float*)nullptr,
                       (long long*)out_idx, out_d2); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
