// grm_pairs.hip -- the relatedness cut-off on K (pcoa_grm_pairs): the screen of one row band of the genetic
// relationship matrix for the pairs (i, j), i < j, with K(i, j) >= cutoff.  The band is the fp64 rectangle that
// launch_grm_dense / launch_grm_dense_finish (grm_dense.hip) leave in the ctx's workspace: rows [r0, r0 + nrows) of K x columns
// [c0, c0 + pitch), row-major at `pitch` doubles, c0 a multiple of 64 at or below r0, so the values compared here are the bits
// pcoa_grm_block returns.  The rule is ONE fp64 comparison on the value already divided; nothing here does arithmetic on K.
//
// Pure memory kernels in the mould of pairs.hip: count, scan, write -- the list comes out in increasing (i, j) order without a
// sort, and a band continues the list of the bands before it:
//   count       a workgroup takes kGrmPairsRows rows of the band x a tile of kGrmPairsTileCols columns; lane t owns the FOUR
//               CONSECUTIVE columns 4 t .. 4 t + 3 of the tile: two 16-byte loads per row where the pitch is a multiple of 4
//               doubles and the band is 16-byte aligned (pcoa_grm_pairs chooses such a pitch), otherwise four 8-byte loads of
//               the same columns.  kGrmPairsRowsInFlight rows' loads are issued before the first comparison.  A (rows, tile)
//               wholly left of the diagonal only writes its zero counts.  Result: cnt[row][tile] = hits of the row in the tile,
//               int32.  The diagonal K(i, i) lies inside the band and is copied out by the lane that holds it.
//   row scan    pairs.hip's (launch_pairs_row_scan): cnt[row][.] becomes its exclusive prefix, the row total goes to rowoff.
//   offset scan one workgroup: rowoff becomes its exclusive prefix STARTING FROM *total, the running count of the bands before,
//               kept in device memory; rowoff[nrows] and *total become the new count.  No host synchronisation between bands.
//   write       the count pass's grid again; a (row, tile) cell whose count is zero is not read a second time.  A hit goes to
//               rowoff[row] + prefix(row, tile) + rank, rank = its order within the row tile from the ballot / mbcnt prefix plus
//               the totals of the lower waves, combined through LDS in wave order.  Positions >= capacity are dropped.
// Content and order are a function of the band's values and the cutoff alone.  No floating-point atomics, no LDS beyond the
// per-wave count exchange, no scratch; every offset into the band is 64-bit.
#include <algorithm>

#include "pcoa_internal.h"

namespace pcoa {
namespace {

constexpr int kGrmPairsThreads = 256;
constexpr int kGrmPairsWaves = kGrmPairsThreads / kWave;
constexpr int kGrmPairsColsPerLane = kGrmPairsTileCols / kGrmPairsThreads;
constexpr int kGrmPairsRowsInFlight = 4;
static_assert(kGrmPairsColsPerLane == 4, "a lane owns two 16-byte pairs of fp64 columns");
static_assert(kGrmPairsRows % kGrmPairsRowsInFlight == 0 && kGrmPairsRows <= kGrmPairsThreads, "workgroup shape");

// the band as the kernels see it (by value in the kernel arguments)
struct GrmBand {
  const double* k;     // [nrows][pitch]
  const int32_t* nb;   // [nrows][pitch] pair counts, or NULL (PCOA_GRM_DIVISOR_USED)
  int64_t pitch;       // doubles between two rows
  int32_t r0, nrows;   // rows [r0, r0 + nrows) of K
  int32_t c0;          // column 0 of the band is sample c0
  int32_t n;           // samples: columns at or behind n - c0 are padding and never reported
  int32_t ntiles;      // column tiles of the band (the grid's x)
};

// K(row, lc .. lc + 3) of the band; lc is a multiple of 4.  Columns that are not loaded read as 0.0 and are never reported
template <bool VEC>
__device__ __forceinline__ void load_quad(const GrmBand& b, int64_t rowbase, int32_t lc, double v[kGrmPairsColsPerLane]) {
  if (VEC) {   // pitch % 4 == 0: the quad lies wholly inside the row or wholly outside
    double2 lo = make_double2(0.0, 0.0), hi = make_double2(0.0, 0.0);
    if ((int64_t)lc < b.pitch) {
      const double2* __restrict__ p = reinterpret_cast<const double2*>(b.k + rowbase + lc);
      lo = p[0];
      hi = p[1];
    }
    v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
  } else {
#pragma unroll
    for (int j = 0; j < kGrmPairsColsPerLane; ++j) v[j] = b.c0 + lc + j < b.n ? b.k[rowbase + lc + j] : 0.0;
  }
}

// the rule, stated once for both passes: sample gj against row sample i
__device__ __forceinline__ bool pair_reported(double k, int32_t i, int32_t gj, int32_t n, double cutoff) {
#pragma clang fp contract(off)
  return gj > i && gj < n && k >= cutoff;
}

// true when every column of the tile is left of every row of the workgroup: neither a pair i < j nor a diagonal entry is there
__device__ __forceinline__ bool tile_left_of_diagonal(const GrmBand& b, int32_t tile, int32_t a0) {
  return (int64_t)b.c0 + ((int64_t)tile + 1) * kGrmPairsTileCols <= (int64_t)b.r0 + a0;
}

template <bool VEC>
__global__ __launch_bounds__(kGrmPairsThreads) void grm_pairs_count_kernel(GrmBand b, double cutoff, int32_t* __restrict__ cnt,
                                                                           double* __restrict__ diag) {
#pragma clang fp contract(off)
  __shared__ int32_t wcnt[kGrmPairsRows][kGrmPairsWaves];
  const int32_t tile = (int32_t)blockIdx.x;
  const int32_t lc = tile * kGrmPairsTileCols + (int32_t)threadIdx.x * kGrmPairsColsPerLane;   // the lane's first band column
  const int32_t gc = b.c0 + lc;                                                                // and its sample
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  const int32_t a0 = (int32_t)blockIdx.y * kGrmPairsRows;
  const int32_t a1 = a0 + kGrmPairsRows < b.nrows ? a0 + kGrmPairsRows : b.nrows;
  if (tile_left_of_diagonal(b, tile, a0)) {
    if ((int32_t)threadIdx.x < a1 - a0) cnt[(int64_t)(a0 + (int32_t)threadIdx.x) * b.ntiles + tile] = 0;
    return;
  }
  // kGrmPairsRowsInFlight rows at a time: their loads are all issued before the first comparison
  for (int32_t a = a0; a < a1; a += kGrmPairsRowsInFlight) {
    double v[kGrmPairsRowsInFlight][kGrmPairsColsPerLane];
#pragma unroll
    for (int r = 0; r < kGrmPairsRowsInFlight; ++r)
      if (a + r < a1) load_quad<VEC>(b, (int64_t)(a + r) * b.pitch, lc, v[r]);   // uniform branch
#pragma unroll
    for (int r = 0; r < kGrmPairsRowsInFlight; ++r) {
      if (a + r >= a1) break;
      const int32_t i = b.r0 + a + r;
      int32_t hits = 0;
#pragma unroll
      for (int j = 0; j < kGrmPairsColsPerLane; ++j) {
        hits += (int32_t)__popcll(__ballot(pair_reported(v[r][j], i, gc + j, b.n, cutoff)));
        if (diag && gc + j == i) diag[i] = v[r][j];
      }
      if (lane == 0) wcnt[a + r - a0][wave] = hits;
    }
  }
  __syncthreads();
  if ((int32_t)threadIdx.x < a1 - a0) {
    int32_t total = 0;
#pragma unroll
    for (int w = 0; w < kGrmPairsWaves; ++w) total += wcnt[threadIdx.x][w];
    cnt[(int64_t)(a0 + (int32_t)threadIdx.x) * b.ntiles + tile] = total;
  }
}

// One workgroup: rowoff[0 .. rows) := *total + its exclusive prefix, rowoff[rows] := *total := the count behind this band
constexpr int kGrmPairsScanThreads = 1024;
__global__ __launch_bounds__(kGrmPairsScanThreads) void grm_pairs_offset_scan_kernel(int64_t* __restrict__ rowoff, int32_t rows,
                                                                                     int64_t* __restrict__ total_io) {
  __shared__ int64_t wsum[kGrmPairsScanThreads / kWave];
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  int64_t carry = *total_io;   // every thread reads it before thread 0 writes it: the chunks below synchronise at least once
  for (int64_t base = 0; base < rows; base += kGrmPairsScanThreads) {
    const int64_t idx = base + threadIdx.x;
    const int64_t v = idx < rows ? rowoff[idx] : 0;
    int64_t incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int64_t up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == kWave - 1) wsum[wave] = incl;
    __syncthreads();
    int64_t below = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kGrmPairsScanThreads / kWave; ++w) {
      const int64_t s = wsum[w];
      if (w < wave) below += s;
      total += s;
    }
    if (idx < rows) rowoff[idx] = carry + below + incl - v;
    carry += total;
    __syncthreads();   // wsum is rewritten by the next chunk
  }
  if (threadIdx.x == 0) {
    rowoff[rows] = carry;
    *total_io = carry;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kGrmPairsThreads) void grm_pairs_write_kernel(GrmBand b, double cutoff, int64_t mprime,
                                                                           const int32_t* __restrict__ prefix,
                                                                           const int64_t* __restrict__ rowoff, int64_t capacity,
                                                                           pcoa_grm_pair* __restrict__ out,
                                                                           unsigned long long* __restrict__ entries_read) {
#pragma clang fp contract(off)
  __shared__ int32_t wtot[2][kGrmPairsWaves];
  const int32_t tile = (int32_t)blockIdx.x;
  const int32_t lc = tile * kGrmPairsTileCols + (int32_t)threadIdx.x * kGrmPairsColsPerLane;
  const int32_t gc = b.c0 + lc;
  const int wave = (int)threadIdx.x / kWave;
  const int32_t a0 = (int32_t)blockIdx.y * kGrmPairsRows;
  const int32_t a1 = a0 + kGrmPairsRows < b.nrows ? a0 + kGrmPairsRows : b.nrows;
  if (tile_left_of_diagonal(b, tile, a0)) return;
  int slot = 0;
  unsigned long long cells = 0;   // the cells this workgroup reads again (uniform)
  for (int32_t a = a0; a < a1; ++a) {
    // everything down to the loads is uniform over the workgroup
    const int64_t cell = (int64_t)a * b.ntiles + tile;
    const int64_t row_first = rowoff[a];
    const int32_t before = prefix[cell];
    const int32_t upto = tile + 1 < b.ntiles ? prefix[cell + 1] : (int32_t)(rowoff[a + 1] - row_first);
    if (upto == before) continue;              // no hit in this cell: it is not read again
    const int64_t first = row_first + before;  // position of the cell's first hit in the list
    if (first >= capacity) continue;           // the whole cell lies behind the caller's buffer
    ++cells;
    const int64_t rowbase = (int64_t)a * b.pitch;
    const int32_t i = b.r0 + a;
    double v[kGrmPairsColsPerLane];
    load_quad<VEC>(b, rowbase, lc, v);
    bool hit[kGrmPairsColsPerLane];
    int32_t lanes_before = 0, wave_total = 0;
#pragma unroll
    for (int j = 0; j < kGrmPairsColsPerLane; ++j) {
      hit[j] = pair_reported(v[j], i, gc + j, b.n, cutoff);
      const unsigned long long m = __ballot(hit[j]);
      lanes_before += (int32_t)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      wave_total += (int32_t)__popcll(m);
    }
    slot ^= 1;   // two slots: a wave may write the next visited row's total while another still reads this one's
    if ((threadIdx.x & (kWave - 1)) == 0) wtot[slot][wave] = wave_total;
    __syncthreads();
    int64_t pos = first + lanes_before;
#pragma unroll
    for (int w = 0; w < kGrmPairsWaves; ++w)
      if (w < wave) pos += wtot[slot][w];
#pragma unroll
    for (int j = 0; j < kGrmPairsColsPerLane; ++j) {
      if (!hit[j]) continue;
      if (pos < capacity) {
        pcoa_grm_pair p;
        p.i = i;
        p.j = gc + j;
        p.k = v[j];
        p.n = b.nb ? (int64_t)b.nb[rowbase + lc + j] : mprime;
        out[pos] = p;
      }
      ++pos;
    }
  }
  // an integer count for pcoa_grm_pairs_stats.grm_pairs_bytes only: nothing of the result depends on it
  const int64_t left = (int64_t)b.n - b.c0 - (int64_t)tile * kGrmPairsTileCols;
  const int64_t width = left < kGrmPairsTileCols ? left : (int64_t)kGrmPairsTileCols;
  if (entries_read && cells && threadIdx.x == 0) atomicAdd(entries_read, cells * (unsigned long long)width);
}

// nrows >= 1, c0 a multiple of 64 in [0, n), c0 <= r0, the band's columns reach the last sample
bool band_ok(const double* k, int64_t pitch, int32_t r0, int32_t nrows, int32_t c0, int32_t n) {
  return k && n > 0 && nrows > 0 && r0 >= 0 && nrows <= n - r0 && c0 >= 0 && c0 % 64 == 0 && c0 <= r0 && pitch >= (int64_t)n - c0;
}

GrmBand make_band(const double* k, const int32_t* nb, int64_t pitch, int32_t r0, int32_t nrows, int32_t c0, int32_t n) {
  GrmBand b;
  b.k = k;
  b.nb = nb;
  b.pitch = pitch;
  b.r0 = r0;
  b.nrows = nrows;
  b.c0 = c0;
  b.n = n;
  b.ntiles = grm_pairs_tiles(n - c0);
  return b;
}

dim3 band_grid(const GrmBand& b) { return dim3((unsigned)b.ntiles, (unsigned)((b.nrows + kGrmPairsRows - 1) / kGrmPairsRows)); }

bool band_vec_ok(const GrmBand& b) { return b.pitch % 4 == 0 && ((uintptr_t)b.k & 15u) == 0; }

}  // namespace

int32_t grm_pairs_tiles(int32_t width) { return (width + kGrmPairsTileCols - 1) / kGrmPairsTileCols; }

int64_t grm_pairs_count_pass_entries(int32_t r0, int32_t nrows, int32_t c0, int32_t n) {
  // the entries of the band the count pass loads: every (rows, tile) that is not wholly left of the diagonal, its rows x the
  // tile's columns inside the matrix
  int64_t entries = 0;
  const int32_t ntiles = grm_pairs_tiles(n - c0);
  for (int32_t a0 = 0; a0 < nrows; a0 += kGrmPairsRows) {
    const int64_t rows = std::min<int64_t>(kGrmPairsRows, (int64_t)nrows - a0);
    for (int32_t tile = 0; tile < ntiles; ++tile) {
      const int64_t tile0 = (int64_t)tile * kGrmPairsTileCols;
      if ((int64_t)c0 + tile0 + kGrmPairsTileCols <= (int64_t)r0 + a0) continue;
      entries += rows * std::min<int64_t>(kGrmPairsTileCols, (int64_t)n - c0 - tile0);
    }
  }
  return entries;
}

hipError_t launch_grm_pairs_count(const double* k, int64_t pitch, int32_t r0, int32_t nrows, int32_t c0, int32_t n, double cutoff,
                                  int32_t* cnt, double* diag_or_null, hipStream_t stream) {
  if (!band_ok(k, pitch, r0, nrows, c0, n) || !cnt) return hipErrorInvalidValue;
  const GrmBand b = make_band(k, nullptr, pitch, r0, nrows, c0, n);
  if (band_vec_ok(b))
    hipLaunchKernelGGL((grm_pairs_count_kernel<true>), band_grid(b), dim3(kGrmPairsThreads), 0, stream, b, cutoff, cnt, diag_or_null);
  else
    hipLaunchKernelGGL((grm_pairs_count_kernel<false>), band_grid(b), dim3(kGrmPairsThreads), 0, stream, b, cutoff, cnt, diag_or_null);
  return hipGetLastError();
}

hipError_t launch_grm_pairs_scan(int32_t* cnt, int32_t nrows, int32_t ntiles, int64_t* rowoff, int64_t* total_io, hipStream_t stream) {
  if (nrows <= 0 || ntiles <= 0 || !cnt || !rowoff || !total_io) return hipErrorInvalidValue;
  hipError_t e = launch_pairs_row_scan(cnt, nrows, ntiles, rowoff, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(grm_pairs_offset_scan_kernel, dim3(1), dim3(kGrmPairsScanThreads), 0, stream, rowoff, nrows, total_io);
  return hipGetLastError();
}

hipError_t launch_grm_pairs_write(const double* k, const int32_t* nb_or_null, int64_t pitch, int32_t r0, int32_t nrows, int32_t c0,
                                  int32_t n, double cutoff, int64_t mprime, const int32_t* prefix, const int64_t* rowoff,
                                  int64_t capacity, pcoa_grm_pair* out, unsigned long long* entries_read, hipStream_t stream) {
  if (!band_ok(k, pitch, r0, nrows, c0, n) || !prefix || !rowoff || capacity <= 0 || !out) return hipErrorInvalidValue;
  const GrmBand b = make_band(k, nb_or_null, pitch, r0, nrows, c0, n);
  if (band_vec_ok(b))
    hipLaunchKernelGGL((grm_pairs_write_kernel<true>), band_grid(b), dim3(kGrmPairsThreads), 0, stream, b, cutoff, mprime, prefix, rowoff,
                       capacity, out, entries_read);
  else
    hipLaunchKernelGGL((grm_pairs_write_kernel<false>), band_grid(b), dim3(kGrmPairsThreads), 0, stream, b, cutoff, mprime, prefix, rowoff,
                       capacity, out, entries_read);
  return hipGetLastError();
}

}  // namespace pcoa
