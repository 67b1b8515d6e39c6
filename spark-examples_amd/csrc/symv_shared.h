// symv_shared.h -- the pieces of the Lanczos mat-vec that more than one translation unit restates: the row form's dot product
// (row_dot) and the upper-triangle form's tile decomposition, workspace layout and DPP row reduction.  eig_lanczos.hip (the
// shared-count measure) and measure.hip (Jaccard, cosine) include this one copy, so the association of every sum and the
// layout symv_sym_gather_kernel reads are the same in both by construction.  Private, not installed.
#pragma once

#include "pcoa_internal.h"

namespace pcoa {
namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// Row i of a symmetric mat-vec, one wave per row: sum_j entry(i, j) x[j], valid in lane 0.  `quad(j, out)` yields the
// four matrix entries of columns j .. j+3 (n % 4 == 0: 16- / 32-byte loads, four groups = 1024 columns of the row in
// flight per wave -- with 4-byte loads the wave had 2 KB in flight and the kernel ran at 1.9 TB/s out of the Infinity
// Cache); `one(j)` a single entry (any n).  The explicit and the implicit (centred on the fly) kernel share this
// function, i.e. the same association of every sum: their results are identical bit for bit when their entries are.
template <class Quad, class One>
__device__ __forceinline__ double row_dot(Quad quad, One one, const double* __restrict__ x, int n, int lane) {
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
  if ((n & 3) == 0) {
    int j = 4 * lane;
    for (; j + 768 < n; j += 1024) {
      double e0[4], e1[4], e2[4], e3[4];
      quad(j, e0);
      quad(j + 256, e1);
      quad(j + 512, e2);
      quad(j + 768, e3);
      const double2 xa0 = *reinterpret_cast<const double2*>(x + j), xb0 = *reinterpret_cast<const double2*>(x + j + 2);
      const double2 xa1 = *reinterpret_cast<const double2*>(x + j + 256), xb1 = *reinterpret_cast<const double2*>(x + j + 258);
      const double2 xa2 = *reinterpret_cast<const double2*>(x + j + 512), xb2 = *reinterpret_cast<const double2*>(x + j + 514);
      const double2 xa3 = *reinterpret_cast<const double2*>(x + j + 768), xb3 = *reinterpret_cast<const double2*>(x + j + 770);
      acc0 += e0[0] * xa0.x + e2[0] * xa2.x;
      acc1 += e0[1] * xa0.y + e2[1] * xa2.y;
      acc2 += e0[2] * xb0.x + e2[2] * xb2.x;
      acc3 += e0[3] * xb0.y + e2[3] * xb2.y;
      acc0 += e1[0] * xa1.x + e3[0] * xa3.x;
      acc1 += e1[1] * xa1.y + e3[1] * xa3.y;
      acc2 += e1[2] * xb1.x + e3[2] * xb3.x;
      acc3 += e1[3] * xb1.y + e3[3] * xb3.y;
    }
    for (; j < n; j += 256) {
      double e0[4];
      quad(j, e0);
      const double2 xa0 = *reinterpret_cast<const double2*>(x + j), xb0 = *reinterpret_cast<const double2*>(x + j + 2);
      acc0 += e0[0] * xa0.x;
      acc1 += e0[1] * xa0.y;
      acc2 += e0[2] * xb0.x;
      acc3 += e0[3] * xb0.y;
    }
  } else {
    int j = lane;
    for (; j + 448 < n; j += 512) {
      const double r0 = one(j), r1 = one(j + 64), r2 = one(j + 128), r3 = one(j + 192);
      const double r4 = one(j + 256), r5 = one(j + 320), r6 = one(j + 384), r7 = one(j + 448);
      acc0 += r0 * x[j] + r4 * x[j + 256];
      acc1 += r1 * x[j + 64] + r5 * x[j + 320];
      acc2 += r2 * x[j + 128] + r6 * x[j + 384];
      acc3 += r3 * x[j + 192] + r7 * x[j + 448];
    }
    for (; j < n; j += 64) acc0 += one(j) * x[j];
  }
  return wave_sum((acc0 + acc1) + (acc2 + acc3));
}

constexpr int SYT = 1024;

__device__ __forceinline__ int64_t sym_tile_index(int bi, int bj, int nb) {  // bi <= bj
  return (int64_t)bi * nb - (int64_t)bi * (bi - 1) / 2 + (bj - bi);
}

// Sum over the 64 lanes on the VALU (DPP: xor 1, xor 2, mirror within 8, mirror within 16, then row 0 -> 1 / 2 -> 3 and
// rows 0-1 -> 2-3 broadcasts); the total is in LANE 63.  One dependent chain of 18 VALU instructions instead of six LDS
// round trips (ds_bpermute) per row.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const int l2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xF, false);
  const int h2 = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xF, false);
  return v + __hiloint2double(h2, l2);
}
__device__ __forceinline__ double wave_sum_to_lane63(double v) {
  v = dpp_add<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
  v = dpp_add<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
  v = dpp_add<0x141, 0xF>(v);  // row_half_mirror
  v = dpp_add<0x140, 0xF>(v);  // row_mirror: every lane holds the sum of its row of 16
  v = dpp_add<0x142, 0xA>(v);  // row_bcast15 into rows 1 and 3
  v = dpp_add<0x143, 0xC>(v);  // row_bcast31 into rows 2 and 3
  return v;
}

constexpr int SYP = 4 * SYT;   // doubles of `part` per tile: row sums [wc = 0, 1][1024], column sums [wr = 0, 1][1024]
constexpr int SYNB = 4;        // row buffers per wave

}  // namespace
}  // namespace pcoa
