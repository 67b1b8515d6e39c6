// king.hip -- the KING-robust kinship screen over FIVE stored Gram matrices (pcoa_king_pairs), and the .bed
// decode that yields the five genotype-class bitsets.  Per variant every sample is in exactly one class by its .bed code:
// R = 00 (hom A1), M = 01 (missing), H = 10 (het), A = 11 (hom A2).  The planes, in the order of PCOA_KING_*: H, M, H u M, R, A.
// With G_p the finalized S of plane p, lower-case letters its diagonal (h_i = G_H(i, i), ...) and V = r_i + a_i + hm_i:
//
//   hethet  = G_H(i, j)                                                  both heterozygous
//   s_hm    = G_HM(i, j) - G_H(i, j) - G_M(i, j)                         one het, the other missing (H, M disjoint)
//   het_sum = h_i + h_j - s_hm                                           hets of i where j is called + hets of j where i is
//   ibs0    = (V - hm_i - hm_j + G_HM(i, j)) - G_R(i, j) - G_A(i, j)     opposite homozygotes
//   num     = hethet - 2 ibs0                                            (int64, may be negative)
//   the pair (i, j), i < j, is REPORTED iff het_sum > 0 and (double)num >= x * (double)het_sum
//
// -- one fp64 multiplication and one comparison, every integer below 2^53, so numpy's king_pairs_rule (variants_pca.py) gives
// the same answer bit for bit.  The planes were not fed the same rows if V differs between samples or some ibs0, het_sum or
// s_hm is negative: each of the four checks has a flag word of its own, which every lane that sees the violation stores the
// same value to (plain vector stores, no atomics); the host reads the words behind the kernels.
//
// The screen is the twin of pairs.hip over five int32 matrices: the same (band, tile) grid, the same count / scan / write (the
// two scans ARE pairs.hip's, through launch_pairs_scan), the list in increasing (i, j) order without a sort.  A lane owns four
// consecutive columns (one 16-byte load per matrix and row when N % 4 == 0, dword loads otherwise) and keeps their h_j and
// hm_j in registers across the band.  Every offset into a matrix is 64-bit.  No LDS ring, no scratch, no atomics in the order.
#include <algorithm>

#include "pcoa_internal.h"

namespace pcoa {
namespace {

constexpr int kKingThreads = 256;
constexpr int kKingWaves = kKingThreads / kWave;
constexpr int kKingColsPerLane = kPairsTileCols / kKingThreads;
// five matrices: a row in flight is five quads (20 registers) per lane, so two rows carry what four carry in pairs.hip
constexpr int kKingRowsInFlight = 2;
static_assert(kKingColsPerLane == 4, "a lane owns one 16-byte quad of int32 columns");
static_assert(kPairsBandRows % kKingRowsInFlight == 0 && kPairsBandRows <= kKingThreads, "band shape");

__device__ __forceinline__ uint32_t king_squeeze_even(uint64_t m) {
  m = (m | (m >> 1)) & 0x3333333333333333ull;
  m = (m | (m >> 2)) & 0x0f0f0f0f0f0f0f0full;
  m = (m | (m >> 4)) & 0x00ff00ff00ff00ffull;
  m = (m | (m >> 8)) & 0x0000ffff0000ffffull;
  m = (m | (m >> 16)) & 0x00000000ffffffffull;
  return (uint32_t)m;
}

// PLINK 1 .bed rows -> the five class bitsets, one read of the row: the loads and the tail handling of the pair decode
// (complete.hip).  One wave per row, one lane per output word = 32 samples = 8 bytes of the row.  Samples >= N are masked in
// EVERY plane: the padding codes of a row's last byte are 00 and would land in R.
__global__ __launch_bounds__(256) void plink_bed_to_king_planes_kernel(const uint8_t* __restrict__ bed, int64_t row_bytes, int64_t nv,
                                                                       int32_t n, int64_t words, KingPlaneRows out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nv) return;
  const uint8_t* row = bed + r * row_bytes;
  for (int64_t w = lane; w < words; w += 64) {
    const int64_t avail = row_bytes - 8 * w;          // bytes the row still has at this word
    uint64_t x = 0;
    if (avail > 0) {
      const int need = avail < 8 ? (int)avail : 8;
      const uintptr_t a = reinterpret_cast<uintptr_t>(row + 8 * w);
      const int sh = (int)(a & 7);
      const uint64_t* q = reinterpret_cast<const uint64_t*>(a - sh);
      x = q[0] >> (8 * sh);
      if (sh + need > 8) x |= q[1] << (8 * (8 - sh));   // (sh > 0 here)
      if (need < 8) x &= (1ull << (8 * need)) - 1ull;   // what follows the row is not its own
    }
    const uint64_t E = 0x5555555555555555ull;
    const uint64_t lo = x & E, hi = (x >> 1) & E;
    const int64_t first = 32 * w;
    uint32_t keep = 0xffffffffu;
    if (first >= n) keep = 0u;
    else if (first + 32 > n) keep = (1u << (n - (int32_t)first)) - 1u;
    const uint32_t het = king_squeeze_even(hi & ~lo) & keep;
    const uint32_t mis = king_squeeze_even(lo & ~hi) & keep;
    const int64_t at = r * words + w;
    out.p[PCOA_KING_HET][at] = het;
    out.p[PCOA_KING_MISSING][at] = mis;
    out.p[PCOA_KING_HET_OR_MISSING][at] = het | mis;
    out.p[PCOA_KING_HOM_A1][at] = king_squeeze_even(~hi & ~lo & E) & keep;
    out.p[PCOA_KING_HOM_A2][at] = king_squeeze_even(hi & lo) & keep;
  }
}

// h_i and hm_i as int64; V = r_0 + a_0 + hm_0 to vout[0]; flag[kKingFlagV] where a sample's r_i + a_i + hm_i is another number
__global__ __launch_bounds__(256) void king_diag_kernel(KingMatrices g, int32_t n, int64_t* __restrict__ h, int64_t* __restrict__ hm,
                                                        int64_t* __restrict__ vout, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t at = i * (int64_t)n + i;
  const int64_t hmi = g.p[PCOA_KING_HET_OR_MISSING][at];
  const int64_t v = (int64_t)g.p[PCOA_KING_HOM_A1][at] + (int64_t)g.p[PCOA_KING_HOM_A2][at] + hmi;
  const int64_t v0 = (int64_t)g.p[PCOA_KING_HOM_A1][0] + (int64_t)g.p[PCOA_KING_HOM_A2][0] + (int64_t)g.p[PCOA_KING_HET_OR_MISSING][0];
  h[i] = g.p[PCOA_KING_HET][at];
  hm[i] = hmi;
  if (v != v0) flag[kKingFlagV] = 1;
  if (i == 0) vout[0] = v0;
}

// the five entries of one (row, column)
struct KingEntry { int32_t h, m, hm, r, a; };

// the rule, stated once for both passes (variants_pca.py king_counts / king_pairs_rule)
struct KingCounts { int64_t hethet, ibs0, het_sum, s_hm; };
__device__ __forceinline__ KingCounts king_counts(const KingEntry& e, int64_t hi, int64_t hmi, int64_t hj, int64_t hmj, int64_t v) {
  KingCounts c;
  c.hethet = e.h;
  c.s_hm = (int64_t)e.hm - (int64_t)e.h - (int64_t)e.m;
  c.het_sum = hi + hj - c.s_hm;
  c.ibs0 = (v - hmi - hmj + (int64_t)e.hm) - (int64_t)e.r - (int64_t)e.a;
  return c;
}
__device__ __forceinline__ bool king_reported(const KingCounts& c, double x) {
  const int64_t num = c.hethet - 2 * c.ibs0;
  return c.het_sum > 0 && (double)num >= x * (double)c.het_sum;
}

// G(i, c0 .. c0 + 3) of one matrix; columns >= n read as 0 (they are never reported or checked)
template <bool VEC>
__device__ __forceinline__ void king_load_quad(const int32_t* __restrict__ s32, int64_t rowbase, int32_t c0, int32_t n,
                                               int32_t v[kKingColsPerLane]) {
  if (VEC) {   // n % 4 == 0: the quad lies wholly inside the row or wholly outside
    int4 q = make_int4(0, 0, 0, 0);
    if (c0 < n) q = *reinterpret_cast<const int4*>(s32 + rowbase + c0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < kKingColsPerLane; ++j) v[j] = c0 + j < n ? s32[rowbase + c0 + j] : 0;
  }
}

template <bool VEC>
__device__ __forceinline__ void king_load_row(const KingMatrices& g, int64_t rowbase, int32_t c0, int32_t n,
                                              int32_t v[PCOA_KING_PLANES][kKingColsPerLane]) {
#pragma unroll
  for (int p = 0; p < PCOA_KING_PLANES; ++p) king_load_quad<VEC>(g.p[p], rowbase, c0, n, v[p]);
}

__device__ __forceinline__ KingEntry king_entry(const int32_t v[PCOA_KING_PLANES][kKingColsPerLane], int j) {
  KingEntry e;
  e.h = v[PCOA_KING_HET][j];
  e.m = v[PCOA_KING_MISSING][j];
  e.hm = v[PCOA_KING_HET_OR_MISSING][j];
  e.r = v[PCOA_KING_HOM_A1][j];
  e.a = v[PCOA_KING_HOM_A2][j];
  return e;
}

// true when every column of the tile is <= every row of the band: no pair (i, j) with i < j lives there
__device__ __forceinline__ bool king_tile_below_diagonal(int32_t tile0, int32_t a0) {
  return (int64_t)tile0 + kPairsTileCols - 1 <= (int64_t)a0;
}

template <bool VEC>
__global__ __launch_bounds__(kKingThreads) void king_count_kernel(KingMatrices g, int32_t n, const int64_t* __restrict__ h,
                                                                  const int64_t* __restrict__ hm, const int64_t* __restrict__ vptr,
                                                                  double x, int32_t ntiles, int32_t* __restrict__ cnt,
                                                                  int32_t* __restrict__ flag) {
  __shared__ int32_t wcnt[kPairsBandRows][kKingWaves];
  const int32_t tile = (int32_t)blockIdx.x;
  const int32_t tile0 = tile * kPairsTileCols;
  const int32_t c0 = tile0 + (int32_t)threadIdx.x * kKingColsPerLane;
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  const int64_t v = vptr[0];
  int64_t hj[kKingColsPerLane], hmj[kKingColsPerLane];
#pragma unroll
  for (int j = 0; j < kKingColsPerLane; ++j) {
    hj[j] = c0 + j < n ? h[c0 + j] : 0;
    hmj[j] = c0 + j < n ? hm[c0 + j] : 0;
  }
  bool bad_ibs0 = false, bad_het = false, bad_shm = false;
  const int32_t nbands = (n + kPairsBandRows - 1) / kPairsBandRows;
  // grid.y strides over the row bands so that the launch stays inside the grid limits whatever n is
  for (int32_t band = (int32_t)blockIdx.y; band < nbands; band += (int32_t)gridDim.y) {
    const int32_t a0 = band * kPairsBandRows;
    const int32_t a1 = a0 + kPairsBandRows < n ? a0 + kPairsBandRows : n;
    if (king_tile_below_diagonal(tile0, a0)) {
      if ((int32_t)threadIdx.x < a1 - a0) cnt[(int64_t)(a0 + (int32_t)threadIdx.x) * ntiles + tile] = 0;
      continue;
    }
    // kKingRowsInFlight rows at a time: their loads are all issued before the first comparison
    for (int32_t a = a0; a < a1; a += kKingRowsInFlight) {
      int32_t q[kKingRowsInFlight][PCOA_KING_PLANES][kKingColsPerLane];
#pragma unroll
      for (int r = 0; r < kKingRowsInFlight; ++r)
        if (a + r < a1) king_load_row<VEC>(g, (int64_t)(a + r) * (int64_t)n, c0, n, q[r]);   // uniform branch
#pragma unroll
      for (int r = 0; r < kKingRowsInFlight; ++r) {
        if (a + r >= a1) break;
        const int32_t i = a + r;
        const int64_t hi = h[i], hmi = hm[i];   // uniform over the workgroup
        int32_t hits = 0;
#pragma unroll
        for (int j = 0; j < kKingColsPerLane; ++j) {
          const bool upper = c0 + j > i && c0 + j < n;
          const KingCounts c = king_counts(king_entry(q[r], j), hi, hmi, hj[j], hmj[j], v);
          bad_ibs0 |= upper && c.ibs0 < 0;
          bad_het |= upper && c.het_sum < 0;
          bad_shm |= upper && c.s_hm < 0;
          const bool hit = upper && king_reported(c, x);
          hits += (int32_t)__popcll(__ballot(hit));
        }
        if (lane == 0) wcnt[i - a0][wave] = hits;
      }
    }
    __syncthreads();
    if ((int32_t)threadIdx.x < a1 - a0) {
      int32_t total = 0;
#pragma unroll
      for (int w = 0; w < kKingWaves; ++w) total += wcnt[threadIdx.x][w];
      cnt[(int64_t)(a0 + (int32_t)threadIdx.x) * ntiles + tile] = total;
    }
    __syncthreads();   // the next band of this workgroup rewrites wcnt
  }
  if (bad_ibs0) flag[kKingFlagIbs0] = 1;
  if (bad_het) flag[kKingFlagHetSum] = 1;
  if (bad_shm) flag[kKingFlagSHm] = 1;
}

template <bool VEC>
__global__ __launch_bounds__(kKingThreads) void king_write_kernel(KingMatrices g, int32_t n, const int64_t* __restrict__ h,
                                                                  const int64_t* __restrict__ hm, const int64_t* __restrict__ vptr,
                                                                  double x, int32_t ntiles, const int32_t* __restrict__ prefix,
                                                                  const int64_t* __restrict__ rowoff, int64_t capacity,
                                                                  pcoa_king_pair* __restrict__ out,
                                                                  unsigned long long* __restrict__ entries_read) {
  __shared__ int32_t wtot[2][kKingWaves];
  const int32_t tile = (int32_t)blockIdx.x;
  const int32_t tile0 = tile * kPairsTileCols;
  const int32_t c0 = tile0 + (int32_t)threadIdx.x * kKingColsPerLane;
  const int wave = (int)threadIdx.x / kWave;
  const int64_t v = vptr[0];
  int64_t hj[kKingColsPerLane], hmj[kKingColsPerLane];
#pragma unroll
  for (int j = 0; j < kKingColsPerLane; ++j) {
    hj[j] = c0 + j < n ? h[c0 + j] : 0;
    hmj[j] = c0 + j < n ? hm[c0 + j] : 0;
  }
  const int32_t nbands = (n + kPairsBandRows - 1) / kPairsBandRows;
  int slot = 0;
  unsigned long long cells = 0;   // the cells this workgroup reads again (uniform)
  for (int32_t band = (int32_t)blockIdx.y; band < nbands; band += (int32_t)gridDim.y) {
    const int32_t a0 = band * kPairsBandRows;
    const int32_t a1 = a0 + kPairsBandRows < n ? a0 + kPairsBandRows : n;
    if (king_tile_below_diagonal(tile0, a0)) continue;
    for (int32_t i = a0; i < a1; ++i) {
      // everything down to the loads is uniform over the workgroup
      const int64_t cell = (int64_t)i * ntiles + tile;
      const int64_t row_first = rowoff[i];
      const int32_t before = prefix[cell];
      const int32_t upto = tile + 1 < ntiles ? prefix[cell + 1] : (int32_t)(rowoff[i + 1] - row_first);
      if (upto == before) continue;              // no hit in this cell: it is not read again
      const int64_t first = row_first + before;  // position of the cell's first hit in the list
      if (first >= capacity) continue;           // the whole cell lies behind the caller's buffer
      ++cells;
      int32_t q[PCOA_KING_PLANES][kKingColsPerLane];
      king_load_row<VEC>(g, (int64_t)i * (int64_t)n, c0, n, q);
      const int64_t hi = h[i], hmi = hm[i];
      KingCounts c[kKingColsPerLane];
      bool hit[kKingColsPerLane];
      int32_t lanes_before = 0, wave_total = 0;
#pragma unroll
      for (int j = 0; j < kKingColsPerLane; ++j) {
        c[j] = king_counts(king_entry(q, j), hi, hmi, hj[j], hmj[j], v);
        hit[j] = c0 + j > i && c0 + j < n && king_reported(c[j], x);
        const unsigned long long b = __ballot(hit[j]);
        lanes_before += (int32_t)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
        wave_total += (int32_t)__popcll(b);
      }
      slot ^= 1;   // two slots: a wave may write the next visited row's total while another still reads this one's
      if ((threadIdx.x & (kWave - 1)) == 0) wtot[slot][wave] = wave_total;
      __syncthreads();
      int64_t pos = first + lanes_before;
#pragma unroll
      for (int w = 0; w < kKingWaves; ++w)
        if (w < wave) pos += wtot[slot][w];
#pragma unroll
      for (int j = 0; j < kKingColsPerLane; ++j) {
        if (!hit[j]) continue;
        if (pos < capacity) {
          pcoa_king_pair p;
          p.i = i;
          p.j = c0 + j;
          p.hethet = c[j].hethet;
          p.ibs0 = c[j].ibs0;
          p.het_sum = c[j].het_sum;
          out[pos] = p;
        }
        ++pos;
      }
    }
  }
  // an integer count for pcoa_king_stats.king_bytes only: nothing of the result depends on it
  const int64_t width = (int64_t)n - tile0 < kPairsTileCols ? (int64_t)n - tile0 : (int64_t)kPairsTileCols;
  if (entries_read && cells && threadIdx.x == 0) atomicAdd(entries_read, cells * (unsigned long long)width);
}

dim3 king_grid(int32_t n, int32_t ntiles) {
  const unsigned bands = (unsigned)((n + kPairsBandRows - 1) / kPairsBandRows);
  return dim3((unsigned)ntiles, bands < 65535u ? bands : 65535u);
}

bool king_vec_ok(const KingMatrices& g, int32_t n) {
  if (n % 4 != 0) return false;
  for (int p = 0; p < PCOA_KING_PLANES; ++p)
    if ((uintptr_t)g.p[p] & 15u) return false;
  return true;
}

bool king_matrices_ok(const KingMatrices& g) {
  for (int p = 0; p < PCOA_KING_PLANES; ++p)
    if (!g.p[p]) return false;
  return true;
}

}  // namespace

hipError_t launch_plink_bed_to_king_planes(const uint8_t* bed, int64_t row_bytes, int64_t nv, int32_t n, int64_t words,
                                           const KingPlaneRows& out, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  for (int p = 0; p < PCOA_KING_PLANES; ++p)
    if (!out.p[p]) return hipErrorInvalidValue;
  const int64_t blocks = (nv + 3) / 4;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(plink_bed_to_king_planes_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, bed, row_bytes, nv, n, words, out);
  return hipGetLastError();
}

hipError_t launch_king_diag(const KingMatrices& g, int32_t n, int64_t* h, int64_t* hm, int64_t* v, int32_t* flag, hipStream_t stream) {
  if (n <= 0 || !king_matrices_ok(g)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(king_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, g, n, h, hm, v, flag);
  return hipGetLastError();
}

hipError_t launch_king_count(const KingMatrices& g, int32_t n, const int64_t* h, const int64_t* hm, const int64_t* v, double x,
                             int32_t* cnt, int32_t* flag, hipStream_t stream) {
  if (n <= 0 || n > kPairsMaxSamples || !king_matrices_ok(g)) return hipErrorInvalidValue;
  const int32_t ntiles = pairs_tiles(n);
  const dim3 grid = king_grid(n, ntiles);
  if (king_vec_ok(g, n))
    hipLaunchKernelGGL((king_count_kernel<true>), grid, dim3(kKingThreads), 0, stream, g, n, h, hm, v, x, ntiles, cnt, flag);
  else
    hipLaunchKernelGGL((king_count_kernel<false>), grid, dim3(kKingThreads), 0, stream, g, n, h, hm, v, x, ntiles, cnt, flag);
  return hipGetLastError();
}

hipError_t launch_king_write(const KingMatrices& g, int32_t n, const int64_t* h, const int64_t* hm, const int64_t* v, double x,
                             const int32_t* prefix, const int64_t* rowoff, int64_t capacity, pcoa_king_pair* out,
                             unsigned long long* entries_read, hipStream_t stream) {
  if (n <= 0 || n > kPairsMaxSamples || capacity <= 0 || !out || !king_matrices_ok(g)) return hipErrorInvalidValue;
  const int32_t ntiles = pairs_tiles(n);
  const dim3 grid = king_grid(n, ntiles);
  if (king_vec_ok(g, n))
    hipLaunchKernelGGL((king_write_kernel<true>), grid, dim3(kKingThreads), 0, stream, g, n, h, hm, v, x, ntiles, prefix, rowoff,
                       capacity, out, entries_read);
  else
    hipLaunchKernelGGL((king_write_kernel<false>), grid, dim3(kKingThreads), 0, stream, g, n, h, hm, v, x, ntiles, prefix, rowoff,
                       capacity, out, entries_read);
  return hipGetLastError();
}

}  // namespace pcoa
