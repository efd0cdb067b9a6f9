// gsr_relations.h -- the relations of one particle graph: object particles 0 .. n_obj_cap - 1, of which the first n_valid are real, and
// ONE tool particle at index n_obj_cap (N = n_obj_cap + 1 <= 128 rows).  Device code only.  Users: construct_edges_kernel
// (gsr_dynamics.hip: one graph) and masks_kernel / rows_kernel (gsr_plan.hip: B graphs as one list).
//
// A pair is related when both ends are real, not both tools, closer than thr (squared distance (dx*dx + dy*dy) + dz*dz < thr2, rounded
// as the torch expression) and -- among objects -- the sender is one of the receiver's k nearest objects (itself included; equal
// distances: the lower index first).  One WAVE per receiver, lane l holds the senders l and l + 64; a row's relations are two ballots;
// the list is the adjacency matrix in row-major order, as torch's nonzero gives it.
#pragma once
#ifdef __HIPCC__
#include "gsr_common.h"

#define GSR_REL_MAXK 16     // the largest topk

// Row i as two ballot masks (bit l of m[h] = sender l + 64 h).  `sp` = the N positions in LDS; every lane of the wave calls it.
// The k nearest objects of the receiver are found as k successive wave minima of the 64-bit keys (distance bits << 32 | sender), each
// above the one before -- ties go to the lower index by construction -- so the k-th key is a threshold and membership one compare.
__device__ __forceinline__ void gsr_rel_row_masks(const float* sp, int i, int lane, int N, int n_obj_cap, int n_valid, float thr2, int k,
                                                  unsigned long long m[2]) {
  const bool i_tool = i == n_obj_cap, i_obj = i < n_valid;
  const float px = sp[3 * i], py = sp[3 * i + 1], pz = sp[3 * i + 2];
  unsigned long long key[2];
  bool near_[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int j = lane + 64 * h;
    float d = __builtin_inff();
    if (j < N) {
      const float dx = px - sp[3 * j], dy = py - sp[3 * j + 1], dz = pz - sp[3 * j + 2];
      d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    }
    near_[h] = d < thr2;
    key[h] = j < n_valid ? (((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j) : ~0ull;   // (d >= 0: its bits order like its value)
  }
  unsigned long long kth = 0ull;
  bool first = true;
  if (i_obj)
    for (int q = 0; q < k; ++q) {
      const unsigned long long c0 = (first || key[0] > kth) ? key[0] : ~0ull, c1 = (first || key[1] > kth) ? key[1] : ~0ull;
      kth = gsr_wave_min64(c0 < c1 ? c0 : c1);
      first = false;
    }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int j = lane + 64 * h;
    const bool j_tool = j == n_obj_cap, j_obj = j < n_valid;
    bool rel = (i_obj || i_tool) && (j_tool || j_obj) && !(i_tool && j_tool) && near_[h];
    if (i_obj && j_obj) rel = rel && key[h] <= kth;
    m[h] = __ballot(rel);
  }
}

// Exclusive scan of the N row counts by ONE wave (two rows per lane): s_base[i] = the list entries before row i, all 128 slots written.
// Returns the graph's total, valid in lane 63.
__device__ __forceinline__ int gsr_rel_scan_rows(const unsigned long long (*s_mask)[2], int lane, int N, int* s_base) {
  const int c0 = lane < N ? __popcll(s_mask[lane][0]) + __popcll(s_mask[lane][1]) : 0;
  const int c1 = lane + 64 < N ? __popcll(s_mask[lane + 64][0]) + __popcll(s_mask[lane + 64][1]) : 0;
  int inc0 = c0, inc1 = c1;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o0 = __shfl_up(inc0, d, 64), o1 = __shfl_up(inc1, d, 64);
    if (lane >= d) { inc0 += o0; inc1 += o1; }
  }
  const int tot0 = __shfl(inc0, 63, 64);
  s_base[lane] = inc0 - c0;
  s_base[lane + 64] = tot0 + inc1 - c1;
  return tot0 + inc1;
}

// Row i's list entries from its two masks, by one wave: entry base + (the row's set bits below the lane's), dropped at e_cap; `row0` is
// added to both indices (the graph's first row in a list of several graphs).
__device__ __forceinline__ void gsr_rel_write_row(unsigned long long m0, unsigned long long m1, int i, int lane, int base, int e_cap,
                                                  long long row0, long long* __restrict__ recv, long long* __restrict__ send) {
  const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  if ((m0 >> lane) & 1ull) { const int e = base + __popcll(m0 & lt); if (e < e_cap) { recv[e] = row0 + i; send[e] = row0 + lane; } }
  if ((m1 >> lane) & 1ull) { const int e = base + __popcll(m0) + __popcll(m1 & lt); if (e < e_cap) { recv[e] = row0 + i; send[e] = row0 + lane + 64; } }
}

// ---------------------------------------------------------------- graphs of up to 256 rows: the training batches (gsr_dyn_batch.hip)
// Siblings of the three functions above for N = n_obj_cap + 1 <= 256 rows (the cloth configurations have 151): lane l holds the senders
// l, l + 64, l + 128, l + 192 and a row is FOUR ballot masks.  The rule is the same, with one addition: `connect_all` relates every real
// object with the tool in both directions whatever the distance (never the tool with itself).  The functions above are untouched, so
// their users' lists keep their bits.
__device__ __forceinline__ void gsr_rel4_row_masks(const float* sp, int i, int lane, int N, int n_obj_cap, int n_valid, float thr2, int k,
                                                   bool connect_all, unsigned long long m[4]) {
  const bool i_tool = i == n_obj_cap, i_obj = i < n_valid;
  const float px = sp[3 * i], py = sp[3 * i + 1], pz = sp[3 * i + 2];
  unsigned long long key[4];
  bool near_[4];
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int j = lane + 64 * h;
    float d = __builtin_inff();
    if (j < N) {
      const float dx = px - sp[3 * j], dy = py - sp[3 * j + 1], dz = pz - sp[3 * j + 2];
      d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    }
    near_[h] = d < thr2;
    key[h] = j < n_valid ? (((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j) : ~0ull;   // (d >= 0: its bits order like its value)
  }
  unsigned long long kth = 0ull;
  bool first = true;
  if (i_obj)
    for (int q = 0; q < k; ++q) {
      unsigned long long c = ~0ull;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const unsigned long long ch = (first || key[h] > kth) ? key[h] : ~0ull;
        c = ch < c ? ch : c;
      }
      kth = gsr_wave_min64(c);
      first = false;
    }
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int j = lane + 64 * h;
    const bool j_tool = j == n_obj_cap, j_obj = j < n_valid;
    bool rel;
    if (i_obj && j_obj) rel = near_[h] && key[h] <= kth;
    else rel = ((i_obj && j_tool) || (i_tool && j_obj)) && (near_[h] || connect_all);
    m[h] = __ballot(rel);
  }
}

// Exclusive scan of the N <= 256 row counts by ONE wave (four rows per lane): s_base[i] = the list entries before row i, all 256 slots
// written.  Returns the graph's total, valid in lane 63.
__device__ __forceinline__ int gsr_rel4_scan_rows(const unsigned long long (*s_mask)[4], int lane, int N, int* s_base) {
  int c[4], inc[4];
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int i = lane + 64 * h;
    c[h] = i < N ? __popcll(s_mask[i][0]) + __popcll(s_mask[i][1]) + __popcll(s_mask[i][2]) + __popcll(s_mask[i][3]) : 0;
    inc[h] = c[h];
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int o = __shfl_up(inc[h], d, 64);
      if (lane >= d) inc[h] += o;
    }
  }
  int before = 0;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    s_base[lane + 64 * h] = before + inc[h] - c[h];
    before += __shfl(inc[h], 63, 64);
  }
  return before;
}

// Row i's list entries from its four masks, by one wave, in LOCAL rows: entry base + (the row's set bits below the sender's), dropped at
// e_cap.  Rr / Rs (both or neither): the one-hot matrices [e_cap, N] of the same list, zeroed by the caller -- only the ones are written.
__device__ __forceinline__ void gsr_rel4_write_row(const unsigned long long m[4], int i, int lane, int base, int e_cap, int N,
                                                   long long* __restrict__ recv, long long* __restrict__ send, float* __restrict__ Rr,
                                                   float* __restrict__ Rs) {
  const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  int before = base;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    if ((m[h] >> lane) & 1ull) {
      const int e = before + __popcll(m[h] & lt), j = lane + 64 * h;
      if (e < e_cap) {
        recv[e] = i; send[e] = j;
        if (Rr) { Rr[(size_t)e * N + i] = 1.0f; Rs[(size_t)e * N + j] = 1.0f; }
      }
    }
    before += __popcll(m[h]);
  }
}

#endif  // __HIPCC__
