// Device-side scan primitives shared by swgpu.hip, swseg.hip and swindex.hip.  Wave64 throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned long long ull;

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63; }

// Inclusive scan of one value per lane over the wave (shuffle ladder); lane 63 holds the wave's sum.
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const uint32_t lane = lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T t = __shfl_up(v, d, 64);
    if (lane >= (uint32_t)d) v += t;
  }
  return v;
}

// Block-wide exclusive scan of one value per thread of a WAVES-wave block; returns the prefix and
// the block total (WAVES defaults to the 256-thread block every caller uses).  lds holds WAVES + 1
// values; the trailing barrier lets the caller reuse it at once.  Thread 0 prefixes the wave totals:
// measured against the form where every thread sums them between two barriers, which left the step
// no faster and k_zone_mask 2 % slower (profiles/scan_unify).
template <typename T, int WAVES = 4>
__device__ __forceinline__ T block_excl_scan(T v, T* total, T* lds) {
  const uint32_t wid = threadIdx.x >> 6;
  const T inc = wave_incl_scan(v);
  if (lane_id() == 63) lds[wid] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    T acc = 0;
    for (int w = 0; w < WAVES; ++w) { const T t = lds[w]; lds[w] = acc; acc += t; }
    lds[WAVES] = acc;
  }
  __syncthreads();
  const T res = inc - v + lds[wid];
  *total = lds[WAVES];
  __syncthreads();
  return res;
}

// Sum of v[0 .. k), returned to every thread of the block: the prologue reduce of the per-tile sums
// the PREVIOUS kernel wrote, in place of a separate single-workgroup scan dispatch between the two
// (a few thousand L2-resident u32s: ~1-2 us of loads per block against ~5-8 us per extra dispatch,
// and no flags, fences or counters -- the kernel boundary is the only synchronisation).
template <int WAVES = 4>
__device__ __forceinline__ uint32_t block_sum_prefix(const uint32_t* v, int64_t k, uint32_t* lds) {
  uint32_t s = 0;
  for (int64_t i = threadIdx.x; i < k; i += WAVES * 64) s += v[i];
  uint32_t tot;
  block_excl_scan<uint32_t, WAVES>(s, &tot, lds);
  return tot;
}

// The stable LSD radix sort of swindex.hip, also the engine step's clustering sort (swgpu.hip).
extern "C" int sw_radix_sort_u32(uint32_t* keys, uint32_t* vals, const uint32_t* n_ptr, int64_t cap, int bits, uint32_t* hist,
                      uint32_t* vals_final, hipStream_t s);
