// gram_common.h -- what every translation unit of the packed-operand Gram path uses (pack_packed.hip, gram_packed.hip,
// pack_kbits.hip, gram_kbits.hip, gram_kbits_w4.hip, gram_shape.hip): the operand geometry, the vector and address-space
// types of the LDS-DMA, the counted vmcnt wait, the raw barrier and the tile enumeration.  Private to csrc/.
//
// Everything here sits in pcoa's anonymous namespace: each translation unit gets its own copy, and a kernel that uses one of
// these keeps the mangled name it had when all of them lived in one file.
#ifndef PCOA_GRAM_COMMON_H_
#define PCOA_GRAM_COMMON_H_

#include "pcoa_internal.h"

namespace pcoa {
namespace {

constexpr int TM = 256;        // padding granule of the packed operand (samples)
constexpr int KB = 16;         // variants per k-block (one lane's operand slice)
constexpr int TJ = 256;        // tile width (panel J) in samples

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// s_barrier and nothing else (never __syncthreads, which would drain the DMA queue); the caller has waited for what the
// barrier is to publish
__device__ __forceinline__ void raw_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// Tile enumeration over the upper triangle (any bijection is valid: every tile is computed once).
//   NWM = 2: tiles (ti <= tj) of 256 x 256, visited in BANDS of 16 tile rows; inside a band the order is
//            column by column.  Workgroups that run at the same time (~256 consecutive indices) then
//            cover about a 16 x 16 block of tiles and share 16 + 16 operand panels instead of 1 + 256,
//            which is what keeps the contraction off the HBM roofline when N is large (N = 100k: 77,028
//            tiles, 4 MB of operand per panel and launch).  At N = 2504 there is a single band.
//   NWM = 1: row block r in [0, 2T) of 128 samples, column block c >= r/2: T(T+1) tiles, simple order.
constexpr int BAND = 16;

template <int NWM>
__device__ __forceinline__ void tile_coords(int tile, int ntile, int& row_blk, int& col_blk) {
  if (NWM == 2 && ntile <= BAND) {
    // a single band: plain row-major order (measured at T = 10: 36 % fewer HBM fetches than column order)
    int ti = 0, rem = tile;
    while (rem >= ntile - ti) {
      rem -= ntile - ti;
      ++ti;
    }
    row_blk = ti;
    col_blk = ti + rem;
  } else if (NWM == 2) {
    int r0 = 0, rem = tile;
    for (;;) {
      const int h = (ntile - r0 < BAND) ? (ntile - r0) : BAND;   // rows in this band
      const int in_band = h * (h + 1) / 2 + (ntile - r0 - h) * h;
      if (rem < in_band) {
        const int tri = h * (h + 1) / 2;
        if (rem < tri) {               // triangular head: column c (relative) holds c + 1 tiles
          int c = 0;
          while (rem >= c + 1) {
            rem -= c + 1;
            ++c;
          }
          row_blk = r0 + rem;
          col_blk = r0 + c;
        } else {                       // rectangular part: h tiles per column
          const int q = rem - tri;
          row_blk = r0 + q % h;
          col_blk = r0 + h + q / h;
        }
        return;
      }
      rem -= in_band;
      r0 += h;
    }
  } else {
    int sup = 0, rem = tile;
    while (rem >= 2 * (ntile - sup)) {
      rem -= 2 * (ntile - sup);
      ++sup;
    }
    const int half = rem / (ntile - sup);
    row_blk = 2 * sup + half;
    col_blk = sup + (rem - half * (ntile - sup));
  }
}

}  // namespace
}  // namespace pcoa

#endif  // PCOA_GRAM_COMMON_H_
