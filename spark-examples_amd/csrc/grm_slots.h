// grm_slots.h -- what the kernels of grm_bits.hip, grm_multi.hip and grm_lsq.hip share: the decoding of one word of 16 two-bit genotypes (coding
// and layout: grm_bits.hip) into its three slot masks, and the AND mask that spends one of their bits on a double.  Private to
// those translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcoa {
namespace {

constexpr uint32_t kLo = 0x55555555u;        // the low bit of every slot; as a word: 16 slots of 01 (not called)

__device__ __forceinline__ double and_mask(double v, int m) {
  return __hiloint2double(__double2hiint(v) & m, __double2loint(v) & m);
}

// the three slot masks of a word, each at the slots' even bit positions
__device__ __forceinline__ void slot_masks(uint32_t w, uint32_t& hi, uint32_t& both, uint32_t& called) {
  hi = (w >> 1) & kLo;
  both = hi & w;
  called = (hi | ~w) & kLo;
}

}  // namespace
}  // namespace pcoa
