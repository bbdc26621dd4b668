// Device-side scan primitives and the step-snapshot writer shared by swgpu.hip, swseg.hip and
// swindex.hip.  Wave64 throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "swengine.h"

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

// The one writer of the end-of-step snapshot (SwStepSnapshot, swengine.h): thread t stores u32 word t
// of the record in mapped host memory, so a workgroup's first 26 threads write it whole.  A step that
// produced nothing leaves only the carry counts.  block_meta: the encoder's three result words
// (SEG_ST_BYTES.., swseg.h) or null; BLOCK_WORDS = false leaves the block words to the caller
// (k_seg_encode's last workgroup stores them from the values it publishes).
template <bool BLOCK_WORDS>
__device__ __forceinline__ void step_snapshot_write(SwStepSnapshot* rec, uint32_t t, const uint32_t* scalars,
                                                    const uint32_t* block_meta, const uint32_t* rej_cnt,
                                                    const uint32_t* n_carry, bool produced) {
  constexpr uint32_t BLOCK = offsetof(SwStepSnapshot, block_bytes) / 4, CARRY = offsetof(SwStepSnapshot, n_carry) / 4,
                     REJ = offsetof(SwStepSnapshot, rej_refs) / 4, PAD = offsetof(SwStepSnapshot, pad) / 4;
  static_assert(BLOCK == SW_SC_WORDS && CARRY == BLOCK + 6 && REJ == CARRY + 2 && PAD == REJ + 2, "word ladder");
  uint32_t* w = reinterpret_cast<uint32_t*>(rec);
  if (t < BLOCK) w[t] = produced ? scalars[t] : 0u;
  else if (t < CARRY) { if (BLOCK_WORDS) w[t] = (produced && block_meta) ? block_meta[t - BLOCK] : 0u; }
  else if (t == CARRY || t == CARRY + 1) w[t] = n_carry ? n_carry[t - CARRY] : 0u;
  else if (t == REJ || t == REJ + 1) w[t] = (produced && rej_cnt) ? rej_cnt[t - REJ] : 0u;
}

// The stable LSD radix sort of swindex.hip, also the engine step's clustering sort (swgpu.hip).
extern "C" int sw_radix_sort_u32(uint32_t* keys, uint32_t* vals, const uint32_t* n_ptr, int64_t cap, int bits, uint32_t* hist,
                      uint32_t* vals_final, hipStream_t s);
