// gsr_hashgrid.h -- the open-addressing table of grid cells shared by gsr_knn.hip and gsr_voxel.hip: 64-bit keys, the 64-bit finaliser of
// MurmurHash3, linear probing, insertion by compare-and-swap.  An empty slot holds GSR_HASH_EMPTY, which no packed cell key equals (both
// users keep bit 63 of their keys clear).  The table has mask + 1 = a power of two slots and at most half of them are ever occupied, so a
// probe sequence always meets the key or an empty slot.
#pragma once
#include <stdint.h>

#define GSR_HASH_EMPTY 0xffffffffffffffffull

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t gsr_hash64(unsigned long long x, uint32_t mask) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return (uint32_t)x & mask;
}
// The slot of `key`, which is inserted if it is not there yet.
__device__ __forceinline__ uint32_t gsr_hash_insert(unsigned long long* __restrict__ keys, uint32_t mask, unsigned long long key) {
  uint32_t s = gsr_hash64(key, mask);
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const unsigned long long old = atomicCAS(&keys[s], GSR_HASH_EMPTY, key);
    if (old == GSR_HASH_EMPTY || old == key) break;
    s = (s + 1) & mask;
  }
  return s;
}
#endif
