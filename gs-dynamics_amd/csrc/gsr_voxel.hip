// gsr_voxel.hip -- depth images / a point cloud -> one mean point per occupied voxel (gsdyn.depth_to_cloud, gsdyn.voxel_down_sample;
// DESIGN.md section 3l).  The definition is in include/gsr.h; this object is built with -ffp-contract=off because every fp32 and fp64
// operation of it is part of the result's bits.
//
// Passes (all on the caller's stream, no host read-back here; the caller reads *out_m):
//   vox_depth_kernel / vox_points_kernel : a thread per pixel / point: unproject, test, cell and offset of the kept ones, then
//                      vox_accumulate: runs of equal keys among the lanes of a wave are summed in registers (ballot of the run heads +
//                      a segmented shuffle reduction) and the head of each run inserts the key (gsr_hashgrid.h) and issues the atomics
//                      of the whole run.  Every sum is an integer sum, so neither the order of arrival nor the run structure reaches
//                      the result.  The world cloud of the depth entry point is never written.  (GSR_VOXEL_PER_LANE=1, read per
//                      call, makes every kept point a run of its own: the form that was measured and not kept.)
//   vox_mark_kernel  : a thread per table slot: slot_at[first index of the voxel] = slot.
//   vox_count_kernel : a workgroup per VOX_CHUNK input indices counts the marked ones.
//   vox_scan_kernel  : one workgroup turns the chunk counts into exclusive prefixes and writes M.
//   vox_emit_kernel  : a workgroup per chunk ranks its marked indices (rows ascend in the voxel's first index) and evaluates the mean
//                      of each voxel in fp64.
// Each level of the prefix scan is a launch of its own: no workgroup ever waits for another.
//
// Scratch layout (gsr_voxel_scratch_bytes; every part 256-byte aligned): header (256 B) | keys u64[T] | records VoxRec[T] |
// slot_at u32[N rounded up to VOX_CHUNK] | chunk sums u32[chunks + 1].  T = a power of two >= 2 min(N, cells of the box), >= 1024.
// VoxRec keeps the index as its complement (nfirst = ~first, summed by atomicMax), so a record starts as all zero bytes.
#include "gsr_common.h"
#include "gsr_hashgrid.h"
#include <math.h>
#include <stdlib.h>

namespace gsr_voxel_ns {

#define VOX_THREADS 256
#define VOX_PER_THREAD 4
#define VOX_CHUNK (VOX_THREADS * VOX_PER_THREAD)
#define VOX_MAX_N (1 << 24)
#define VOX_MAX_CELLS 2097151.0f                 // 2^21 - 1: (hi - lo) * inv_h must stay below it on every axis
#define VOX_SCAN_THREADS 1024
#define VOX_SCAN_PER_THREAD 16                   // VOX_SCAN_THREADS * VOX_SCAN_PER_THREAD = 2^14 >= VOX_MAX_N / VOX_CHUNK chunks

struct VoxRec {                                  // 48 bytes, zero-initialised
  uint32_t cnt, nfirst;
  unsigned long long s[3];                       // sums of int64(f * 2^32) per axis
  uint32_t col[3], pad;
};
static_assert(sizeof(VoxRec) == 48, "VoxRec layout");

struct VoxGrid {                                 // passed by value
  float lo[3], hi[3];
  float inv_h;
  uint32_t mask;                                 // T - 1
  int per_lane;                                  // 1: no aggregation over the lanes, every kept point issues its own atomics (GSR_VOXEL_PER_LANE=1; for measuring)
};

struct VoxScratch {
  uint32_t* hdr; unsigned long long* keys; VoxRec* rec; uint32_t* slot_at; uint32_t* sums;
  uint32_t T, chunks;
};

// cells of the box per axis by the points' own expression; false: an axis has 2^21 - 1 or more, or the box is not a box
static inline bool vox_cells(const float* lo, const float* hi, float inv_h, double* cells) {
  double c = 1.0;
  for (int a = 0; a < 3; ++a) {
    const float u = (hi[a] - lo[a]) * inv_h;
    if (!(u >= 0.0f) || !(u < VOX_MAX_CELLS)) return false;
    c *= (double)floorf(u) + 1.0;
  }
  *cells = c;
  return true;
}
static inline uint32_t vox_table_size(int32_t N, double cells) {
  const double want = 2.0 * ((double)N < cells ? (double)N : cells);
  uint32_t T = 1024;
  while ((double)T < want) T <<= 1;              // want <= 2^25
  return T;
}
static inline size_t vox_carve(void* base, int32_t N, double cells, VoxScratch* s) {
  size_t off = 0;
  const size_t Nn = (size_t)(N > 0 ? N : 1);
  char* b = (char*)base;
  auto take = [&](size_t bytes) { char* p = b ? b + off : nullptr; off += gsr_align(bytes); return p; };
  s->T = vox_table_size((int32_t)Nn, cells);
  s->chunks = (uint32_t)((Nn + VOX_CHUNK - 1) / VOX_CHUNK);
  s->hdr = (uint32_t*)take(256);
  s->keys = (unsigned long long*)take((size_t)s->T * 8);
  s->rec = (VoxRec*)take((size_t)s->T * sizeof(VoxRec));
  s->slot_at = (uint32_t*)take((size_t)s->chunks * VOX_CHUNK * 4);
  s->sums = (uint32_t*)take(((size_t)s->chunks + 1) * 4);
  return off;
}

// ---------------------------------------------------------------- accumulation
__device__ __forceinline__ unsigned long long vox_shfl_down64(unsigned long long v, int off) {
  const unsigned lo = (unsigned)__shfl_down((int)(unsigned)v, off, 64), hi = (unsigned)__shfl_down((int)(unsigned)(v >> 32), off, 64);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long vox_shfl_up64(unsigned long long v, int off) {
  const unsigned lo = (unsigned)__shfl_up((int)(unsigned)v, off, 64), hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), off, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// Must be called by every lane of the wave.  valid: this lane has a kept point w (inside the box) with input index i and colour rgb
// (r | g << 8 | b << 16).
__device__ __forceinline__ void vox_accumulate(bool valid, float wx, float wy, float wz, uint32_t i, uint32_t rgb, bool has_col, const VoxGrid& g,
                                               unsigned long long* __restrict__ keys, VoxRec* __restrict__ rec) {
  if (__ballot(valid) == 0ull) return;                       // wave-uniform
  const int lane = gsr_lane();
  unsigned long long key = GSR_HASH_EMPTY, q0 = 0, q1 = 0, q2 = 0, pk = 0;
  if (valid) {
    const float ux = (wx - g.lo[0]) * g.inv_h, uy = (wy - g.lo[1]) * g.inv_h, uz = (wz - g.lo[2]) * g.inv_h;
    const float cx = floorf(ux), cy = floorf(uy), cz = floorf(uz);
    q0 = (unsigned long long)(long long)((ux - cx) * 4294967296.0f);
    q1 = (unsigned long long)(long long)((uy - cy) * 4294967296.0f);
    q2 = (unsigned long long)(long long)((uz - cz) * 4294967296.0f);
    key = ((unsigned long long)(long long)cx << 42) | ((unsigned long long)(long long)cy << 21) | (unsigned long long)(long long)cz;
    key &= 0x7fffffffffffffffull;                            // (cells are below 2^21: nothing to cut)
    // a run is at most 64 long: 14 bits per colour sum, 7 for the count
    pk = (unsigned long long)(rgb & 0xffu) | ((unsigned long long)((rgb >> 8) & 0xffu) << 16) | ((unsigned long long)((rgb >> 16) & 0xffu) << 32) | (1ull << 48);
  }
  // runs of equal keys among neighbouring lanes (lanes without a point carry the empty key and zeros: runs of their own)
  const unsigned long long prev = vox_shfl_up64(key, 1);
  const bool boundary = lane == 0 || prev != key || g.per_lane;
  if (!g.per_lane) {
    const unsigned long long heads = __ballot(boundary);
    const int myhead = 63 - __clzll((long long)(heads & (0xffffffffffffffffull >> (63 - lane))));
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int oh = __shfl_down(myhead, off, 64);
      const unsigned long long o0 = vox_shfl_down64(q0, off), o1 = vox_shfl_down64(q1, off), o2 = vox_shfl_down64(q2, off), op = vox_shfl_down64(pk, off);
      if (lane + off < 64 && oh == myhead) { q0 += o0; q1 += o1; q2 += o2; pk += op; }
    }
  }
  if (boundary && valid) {
    const uint32_t s = gsr_hash_insert(keys, g.mask, key);
    VoxRec* r = rec + s;
    atomicAdd(&r->cnt, (uint32_t)(pk >> 48));
    atomicMax(&r->nfirst, ~i);                               // the head of a run has the run's lowest index
    atomicAdd(&r->s[0], q0);
    atomicAdd(&r->s[1], q1);
    atomicAdd(&r->s[2], q2);
    if (has_col) {
      atomicAdd(&r->col[0], (uint32_t)(pk & 0xffffu));
      atomicAdd(&r->col[1], (uint32_t)((pk >> 16) & 0xffffu));
      atomicAdd(&r->col[2], (uint32_t)((pk >> 32) & 0xffffu));
    }
  }
}

__device__ __forceinline__ bool vox_inside(float x, float y, float z, const VoxGrid& g) {
  return x >= g.lo[0] && x <= g.hi[0] && y >= g.lo[1] && y <= g.hi[1] && z >= g.lo[2] && z <= g.hi[2];
}

__global__ __launch_bounds__(VOX_THREADS) void vox_depth_kernel(int N, int HW, int W, const float* __restrict__ depths, const float* __restrict__ K4,
                                                               const float* __restrict__ R, const float* __restrict__ t, const uint8_t* __restrict__ colors,
                                                               const uint8_t* __restrict__ masks, float d_lo, float d_hi, VoxGrid g,
                                                               unsigned long long* __restrict__ keys, VoxRec* __restrict__ rec) {
  const long long il = (long long)blockIdx.x * VOX_THREADS + threadIdx.x;
  const uint32_t i = (uint32_t)il;
  bool valid = il < N;
  float d = 0.0f, wx = 0.0f, wy = 0.0f, wz = 0.0f;
  uint32_t rgb = 0;
  if (valid) {
    d = depths[i];
    valid = d > d_lo && d < d_hi;
    if (valid && masks) valid = masks[i] != 0;
  }
  if (valid) {
    const int v = (int)(i / (uint32_t)HW), rem = (int)(i - (uint32_t)v * (uint32_t)HW);
    const int y = rem / W, x = rem - y * W;
    const float* k = K4 + 4 * (size_t)v;
    const float* r = R + 9 * (size_t)v;
    const float* tv = t + 3 * (size_t)v;
    const float xc = (((float)x - k[2]) * (1.0f / k[0])) * d;
    const float yc = (((float)y - k[3]) * (1.0f / k[1])) * d;
    wx = ((r[0] * xc + r[1] * yc) + r[2] * d) + tv[0];
    wy = ((r[3] * xc + r[4] * yc) + r[5] * d) + tv[1];
    wz = ((r[6] * xc + r[7] * yc) + r[8] * d) + tv[2];
    valid = vox_inside(wx, wy, wz, g);
    if (valid && colors) rgb = (uint32_t)colors[3 * (size_t)i] | ((uint32_t)colors[3 * (size_t)i + 1] << 8) | ((uint32_t)colors[3 * (size_t)i + 2] << 16);
  }
  vox_accumulate(valid, wx, wy, wz, i, rgb, colors != nullptr, g, keys, rec);
}

__global__ __launch_bounds__(VOX_THREADS) void vox_points_kernel(int N, const float* __restrict__ pts, const uint8_t* __restrict__ colors, VoxGrid g,
                                                                unsigned long long* __restrict__ keys, VoxRec* __restrict__ rec) {
  const long long il = (long long)blockIdx.x * VOX_THREADS + threadIdx.x;
  const uint32_t i = (uint32_t)il;
  bool valid = il < N;
  float wx = 0.0f, wy = 0.0f, wz = 0.0f;
  uint32_t rgb = 0;
  if (valid) {
    wx = pts[3 * (size_t)i]; wy = pts[3 * (size_t)i + 1]; wz = pts[3 * (size_t)i + 2];
    valid = vox_inside(wx, wy, wz, g);                       // a NaN or an infinity is inside no box
    if (valid && colors) rgb = (uint32_t)colors[3 * (size_t)i] | ((uint32_t)colors[3 * (size_t)i + 1] << 8) | ((uint32_t)colors[3 * (size_t)i + 2] << 16);
  }
  vox_accumulate(valid, wx, wy, wz, i, rgb, colors != nullptr, g, keys, rec);
}

// ---------------------------------------------------------------- compaction in the order of the first index
__global__ __launch_bounds__(VOX_THREADS) void vox_mark_kernel(uint32_t T, int N, const unsigned long long* __restrict__ keys, const VoxRec* __restrict__ rec,
                                                              uint32_t* __restrict__ slot_at) {
  const uint32_t s = blockIdx.x * VOX_THREADS + threadIdx.x;   // T is a multiple of VOX_THREADS
  if (s >= T || keys[s] == GSR_HASH_EMPTY) return;
  const uint32_t i = ~rec[s].nfirst;
  if (i < (uint32_t)N) slot_at[i] = s;                         // (always: an occupied slot has a member)
}

// marked indices of this thread's VOX_PER_THREAD consecutive entries (slot_at is padded to whole chunks and filled with ~0)
__device__ __forceinline__ uint4 vox_load4(const uint32_t* __restrict__ slot_at) {
  return *reinterpret_cast<const uint4*>(slot_at + ((size_t)blockIdx.x * VOX_THREADS + threadIdx.x) * VOX_PER_THREAD);
}
__device__ __forceinline__ uint32_t vox_marked(uint4 v) {
  return (v.x != 0xffffffffu) + (v.y != 0xffffffffu) + (v.z != 0xffffffffu) + (v.w != 0xffffffffu);
}

__global__ __launch_bounds__(VOX_THREADS) void vox_count_kernel(const uint32_t* __restrict__ slot_at, uint32_t* __restrict__ sums) {
  __shared__ uint32_t s_w[VOX_THREADS / 64];
  uint32_t c = vox_marked(vox_load4(slot_at));
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
  if (gsr_lane() == 0) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(VOX_SCAN_THREADS) void vox_scan_kernel(uint32_t chunks, uint32_t* __restrict__ sums, uint32_t* __restrict__ hdr, int32_t* __restrict__ out_m) {
  __shared__ uint32_t s_w[VOX_SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t v[VOX_SCAN_PER_THREAD], tot = 0;
#pragma unroll
  for (int j = 0; j < VOX_SCAN_PER_THREAD; ++j) {
    const uint32_t c = (uint32_t)tid * VOX_SCAN_PER_THREAD + j;
    v[j] = c < chunks ? sums[c] : 0u;
    tot += v[j];
  }
  uint32_t incl = tot;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
  if (lane == 63) s_w[wv] = incl;
  __syncthreads();
  uint32_t base = 0, all = 0;
  for (int w = 0; w < VOX_SCAN_THREADS / 64; ++w) { if (w < wv) base += s_w[w]; all += s_w[w]; }
  uint32_t run = base + incl - tot;
#pragma unroll
  for (int j = 0; j < VOX_SCAN_PER_THREAD; ++j) {
    const uint32_t c = (uint32_t)tid * VOX_SCAN_PER_THREAD + j;
    if (c < chunks) sums[c] = run;
    run += v[j];
  }
  if (tid == 0) { sums[chunks] = all; hdr[0] = all; *out_m = (int32_t)all; }
}

__global__ __launch_bounds__(VOX_THREADS) void vox_emit_kernel(int N, uint32_t cap, const uint32_t* __restrict__ slot_at, const uint32_t* __restrict__ sums,
                                                              const unsigned long long* __restrict__ keys, const VoxRec* __restrict__ rec, VoxGrid g, double h,
                                                              float* __restrict__ out_points, float* __restrict__ out_colors, int32_t* __restrict__ out_counts,
                                                              long long* __restrict__ out_first) {
  __shared__ uint32_t s_w[VOX_THREADS / 64];
  const int lane = gsr_lane(), wv = threadIdx.x >> 6;
  const uint4 v = vox_load4(slot_at);
  const uint32_t mine = vox_marked(v);
  if (__syncthreads_or(mine != 0u) == 0) return;
  uint32_t incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
  if (lane == 63) s_w[wv] = incl;
  __syncthreads();
  uint32_t row = sums[blockIdx.x] + incl - mine;
  for (int w = 0; w < wv; ++w) row += s_w[w];
  const uint32_t slots[VOX_PER_THREAD] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < VOX_PER_THREAD; ++j) {
    const uint32_t s = slots[j];
    if (s == 0xffffffffu) continue;
    const uint32_t i = ((uint32_t)blockIdx.x * VOX_THREADS + threadIdx.x) * VOX_PER_THREAD + j;
    if (s <= g.mask && row < cap && i < (uint32_t)N) {       // (always)
      const unsigned long long key = keys[s];
      const VoxRec r = rec[s];
      const double n = (double)r.cnt, den = n * 4294967296.0;
      const double c[3] = {(double)(key >> 42), (double)((key >> 21) & 0x1fffffull), (double)(key & 0x1fffffull)};
#pragma unroll
      for (int a = 0; a < 3; ++a) out_points[3 * (size_t)row + a] = (float)((c[a] + (double)(long long)r.s[a] / den) * h + (double)g.lo[a]);
      if (out_colors) {
        const double dc = 255.0 * n;
#pragma unroll
        for (int a = 0; a < 3; ++a) out_colors[3 * (size_t)row + a] = (float)((double)r.col[a] / dc);
      }
      out_counts[row] = (int32_t)r.cnt;
      out_first[row] = (long long)i;
    }
    ++row;
  }
}

// ---------------------------------------------------------------- host
struct VoxCall {
  VoxScratch s; VoxGrid g; double h;
};
static int vox_prepare(const char* who, int64_t N, const float* lo, const float* hi, float inv_h, void* scratch, int32_t cap, VoxCall* c) {
  double cells = 0.0;
  if (N < 1 || N > VOX_MAX_N || !lo || !hi || !(inv_h > 0.0f) || !(inv_h < __builtin_inff()) || !vox_cells(lo, hi, inv_h, &cells)) {
    gsr_set_error("%s: bad argument (1 <= N <= 2^24, a box lo <= hi, 0 < inv_h < inf and (hi - lo) * inv_h < 2^21 - 1 on every axis; got N = %lld)", who,
                  (long long)N);
    return -2;
  }
  const double need = (double)N < cells ? (double)N : cells;
  if (!scratch || cap < 1 || (double)cap < need) {
    gsr_set_error("%s: NULL scratch, or cap = %d below min(N, cells of the box) = %.0f", who, (int)cap, need);
    return -2;
  }
  vox_carve(scratch, (int32_t)N, cells, &c->s);
  for (int a = 0; a < 3; ++a) { c->g.lo[a] = lo[a]; c->g.hi[a] = hi[a]; }
  c->g.inv_h = inv_h;
  c->g.mask = c->s.T - 1u;
  const char* e = getenv("GSR_VOXEL_PER_LANE");    // the accumulation without its wave-level aggregation; same results
  c->g.per_lane = e && e[0] == '1';
  c->h = 1.0 / (double)inv_h;
  return 0;
}
static int vox_clear(const VoxCall& c, hipStream_t st) {
  GSR_HIP_CHECK(hipMemsetAsync(c.s.hdr, 0, 256, st));
  GSR_HIP_CHECK(hipMemsetAsync(c.s.keys, 0xff, (size_t)c.s.T * 8, st));
  GSR_HIP_CHECK(hipMemsetAsync(c.s.rec, 0, (size_t)c.s.T * sizeof(VoxRec), st));
  GSR_HIP_CHECK(hipMemsetAsync(c.s.slot_at, 0xff, (size_t)c.s.chunks * VOX_CHUNK * 4, st));
  return 0;
}
static int vox_finish(const VoxCall& c, int32_t N, int32_t cap, float* out_points, float* out_colors, int32_t* out_counts, int64_t* out_first, int32_t* out_m,
                      hipStream_t st) {
  { GSR_PROF("vox_mark", st);
    hipLaunchKernelGGL(vox_mark_kernel, dim3(c.s.T / VOX_THREADS), dim3(VOX_THREADS), 0, st, c.s.T, (int)N, (const unsigned long long*)c.s.keys,
                       (const VoxRec*)c.s.rec, c.s.slot_at); }
  { GSR_PROF("vox_count", st);
    hipLaunchKernelGGL(vox_count_kernel, dim3(c.s.chunks), dim3(VOX_THREADS), 0, st, (const uint32_t*)c.s.slot_at, c.s.sums); }
  { GSR_PROF("vox_scan", st);
    hipLaunchKernelGGL(vox_scan_kernel, dim3(1), dim3(VOX_SCAN_THREADS), 0, st, c.s.chunks, c.s.sums, c.s.hdr, out_m); }
  { GSR_PROF("vox_emit", st);
    hipLaunchKernelGGL(vox_emit_kernel, dim3(c.s.chunks), dim3(VOX_THREADS), 0, st, (int)N, (uint32_t)cap, (const uint32_t*)c.s.slot_at, (const uint32_t*)c.s.sums,
                       (const unsigned long long*)c.s.keys, (const VoxRec*)c.s.rec, c.g, c.h, out_points, out_colors, out_counts, (long long*)out_first); }
  GSR_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace gsr_voxel_ns

extern "C" {

size_t gsr_voxel_scratch_bytes(int32_t N, const float* lo, const float* hi, float inv_h) {
  using namespace gsr_voxel_ns;
  double cells = 0.0;
  if (N < 1 || N > VOX_MAX_N || !lo || !hi || !vox_cells(lo, hi, inv_h, &cells)) return 0;
  VoxScratch s;
  return vox_carve(nullptr, N, cells, &s);
}

int gsr_voxel_points(int32_t N, const float* points, const uint8_t* colors, const float* lo, const float* hi, float inv_h, void* scratch, int32_t cap,
                     float* out_points, float* out_colors, int32_t* out_counts, int64_t* out_first, int32_t* out_m, void* stream) {
  using namespace gsr_voxel_ns;
  GsrRange _range("gsr_voxel_points");
  VoxCall c;
  if (int e = vox_prepare("gsr_voxel_points", N, lo, hi, inv_h, scratch, cap, &c)) return e;
  if (!points || !out_points || !out_counts || !out_first || !out_m || (colors != nullptr) != (out_colors != nullptr)) {
    gsr_set_error("gsr_voxel_points: NULL pointer, or colors and out_colors not given together");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  if (int e = vox_clear(c, st)) return e;
  { GSR_PROF("vox_points", st);
    hipLaunchKernelGGL(vox_points_kernel, dim3((unsigned)((N + VOX_THREADS - 1) / VOX_THREADS)), dim3(VOX_THREADS), 0, st, (int)N, points, colors, c.g, c.s.keys,
                       c.s.rec); }
  return vox_finish(c, N, cap, out_points, out_colors, out_counts, out_first, out_m, st);
}

int gsr_voxel_depth_views(int32_t V, int32_t H, int32_t W, const float* depths, const float* K4, const float* R, const float* t, const uint8_t* colors,
                          const uint8_t* masks, const float* lo, const float* hi, float depth_lo, float depth_hi, float inv_h, void* scratch, int32_t cap,
                          float* out_points, float* out_colors, int32_t* out_counts, int64_t* out_first, int32_t* out_m, void* stream) {
  using namespace gsr_voxel_ns;
  GsrRange _range("gsr_voxel_depth_views");
  if (V < 1 || H < 1 || W < 1) {
    gsr_set_error("gsr_voxel_depth_views: bad argument (V, H, W >= 1; got %d, %d, %d)", (int)V, (int)H, (int)W);
    return -2;
  }
  const int64_t N = (int64_t)V * H * W;
  VoxCall c;
  if (int e = vox_prepare("gsr_voxel_depth_views", N, lo, hi, inv_h, scratch, cap, &c)) return e;
  if (!depths || !K4 || !R || !t || !out_points || !out_counts || !out_first || !out_m || (colors != nullptr) != (out_colors != nullptr)) {
    gsr_set_error("gsr_voxel_depth_views: NULL pointer, or colors and out_colors not given together");
    return -2;
  }
  hipStream_t st = (hipStream_t)stream;
  if (int e = vox_clear(c, st)) return e;
  { GSR_PROF("vox_depth", st);
    hipLaunchKernelGGL(vox_depth_kernel, dim3((unsigned)((N + VOX_THREADS - 1) / VOX_THREADS)), dim3(VOX_THREADS), 0, st, (int)N, (int)(H * W), (int)W, depths, K4, R, t,
                       colors, masks, depth_lo, depth_hi, c.g, c.s.keys, c.s.rec); }
  return vox_finish(c, (int32_t)N, cap, out_points, out_colors, out_counts, out_first, out_m, st);
}

}  // extern "C"
