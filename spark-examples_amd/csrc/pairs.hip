// pairs.hip -- the screen for duplicate and related sample pairs over a stored S (pcoa_similar_pairs).
// With d_i = S(i, i) (the variants sample i carries) and U = d_i + d_j - S(i, j) (the variants either carries), the pair
// (i, j), i < j, is REPORTED iff U > 0 and (double)S(i, j) >= X * (double)U: one fp64 multiplication and one comparison,
// every integer below 2^53, so numpy's related_pairs_rule (variants_pca.py) gives the same answer bit for bit.
//
// Pure memory kernels over the upper triangle of S, in the mould of subset.hip: no LDS ring, no scratch, no atomics in the
// order.  Count, scan, write -- the list comes out in increasing (i, j) order without a sort:
//   diagonal    d[i] = s32[i n + i] (+ s64[i n + i]) as int64.
//   count       a workgroup takes a band of kPairsBandRows rows x a tile of kPairsTileCols columns; lane t owns the FOUR
//               CONSECUTIVE columns tile0 + 4 t .. + 3 (one 16-byte load per row where the row pitch allows: 4 n bytes is
//               16-byte aligned only when n % 4 == 0, otherwise four dword loads of the same columns) and keeps their d_j in
//               registers across the band; d_i is uniform.  A (band, tile) wholly on or below the diagonal only writes its
//               zero counts.  Result: cnt[i][tile] = hits of row i in that tile.
//   row scan    one wave per row: cnt[i][.] becomes its exclusive prefix within the row (an int32: a row has < 2^31 hits),
//               the row total goes to rowoff[i] as int64.
//   offset scan one workgroup: rowoff becomes its exclusive prefix, rowoff[n] = n_found.
//   write       the count pass's grid again; a (row, tile) cell whose count is zero is not read a second time.  A hit goes to
//               rowoff[i] + prefix(i, tile) + rank, rank = its order within the row tile: columns ascend with (lane, column of
//               the lane), so the rank is an mbcnt prefix over the four ballots plus the totals of the lower waves, combined
//               through LDS in wave order.  Positions >= capacity are dropped.
// Content and order are a function of S and X alone.  Every offset into S is 64-bit (i n + j passes 2^31 from N = 46,341).
#include <algorithm>

#include "pcoa_internal.h"

namespace pcoa {
namespace {

constexpr int kPairsThreads = 256;
constexpr int kPairsWaves = kPairsThreads / kWave;
constexpr int kPairsColsPerLane = kPairsTileCols / kPairsThreads;
constexpr int kPairsRowsInFlight = 4;
static_assert(kPairsColsPerLane == 4, "a lane owns one 16-byte quad of int32 columns");
static_assert(kPairsBandRows % kPairsRowsInFlight == 0 && kPairsBandRows <= kPairsThreads, "band shape");

// the rule, stated once for both passes (variants_pca.py related_pairs_rule)
__device__ __forceinline__ bool pair_reported(int64_t s, int64_t di, int64_t dj, double x) {
  const int64_t u = di + dj - s;
  return u > 0 && (double)s >= x * (double)u;
}

// S(i, c0 .. c0 + 3) as int64: the int32 matrix plus the int64 part; columns >= n read as 0 (they are never reported)
template <bool VEC, bool HAS64>
__device__ __forceinline__ void load_quad(const int32_t* __restrict__ s32, const int64_t* __restrict__ s64, int64_t rowbase,
                                          int32_t c0, int32_t n, int64_t v[kPairsColsPerLane]) {
  if (VEC) {   // n % 4 == 0: the quad lies wholly inside the row or wholly outside
    int4 q = make_int4(0, 0, 0, 0);
    if (c0 < n) q = *reinterpret_cast<const int4*>(s32 + rowbase + c0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < kPairsColsPerLane; ++j) v[j] = c0 + j < n ? s32[rowbase + c0 + j] : 0;
  }
  if (HAS64) {
#pragma unroll
    for (int j = 0; j < kPairsColsPerLane; ++j)
      if (c0 + j < n) v[j] += s64[rowbase + c0 + j];
  }
}

__global__ __launch_bounds__(256) void pairs_diag_kernel(const int32_t* __restrict__ s32, const int64_t* __restrict__ s64,
                                                         int32_t n, int64_t* __restrict__ diag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t at = i * (int64_t)n + i;
  diag[i] = (int64_t)s32[at] + (s64 ? s64[at] : 0);
}

// true when every column of the tile is <= every row of the band: no pair (i, j) with i < j lives there
__device__ __forceinline__ bool tile_below_diagonal(int32_t tile0, int32_t a0) {
  return (int64_t)tile0 + kPairsTileCols - 1 <= (int64_t)a0;
}

template <bool VEC, bool HAS64>
__global__ __launch_bounds__(kPairsThreads) void pairs_count_kernel(const int32_t* __restrict__ s32,
                                                                    const int64_t* __restrict__ s64, int32_t n,
                                                                    const int64_t* __restrict__ diag, double x, int32_t ntiles,
                                                                    int32_t* __restrict__ cnt) {
  __shared__ int32_t wcnt[kPairsBandRows][kPairsWaves];
  const int32_t tile = (int32_t)blockIdx.x;
  const int32_t tile0 = tile * kPairsTileCols;
  const int32_t c0 = tile0 + (int32_t)threadIdx.x * kPairsColsPerLane;
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  int64_t dj[kPairsColsPerLane];
#pragma unroll
  for (int j = 0; j < kPairsColsPerLane; ++j) dj[j] = c0 + j < n ? diag[c0 + j] : 0;
  const int32_t nbands = (n + kPairsBandRows - 1) / kPairsBandRows;
  // grid.y strides over the row bands so that the launch stays inside the grid limits whatever n is
  for (int32_t band = (int32_t)blockIdx.y; band < nbands; band += (int32_t)gridDim.y) {
    const int32_t a0 = band * kPairsBandRows;
    const int32_t a1 = a0 + kPairsBandRows < n ? a0 + kPairsBandRows : n;
    if (tile_below_diagonal(tile0, a0)) {
      if ((int32_t)threadIdx.x < a1 - a0) cnt[(int64_t)(a0 + (int32_t)threadIdx.x) * ntiles + tile] = 0;
      continue;
    }
    // kPairsRowsInFlight rows at a time: their loads are all issued before the first comparison
    for (int32_t a = a0; a < a1; a += kPairsRowsInFlight) {
      int64_t v[kPairsRowsInFlight][kPairsColsPerLane];
#pragma unroll
      for (int r = 0; r < kPairsRowsInFlight; ++r)
        if (a + r < a1) load_quad<VEC, HAS64>(s32, s64, (int64_t)(a + r) * (int64_t)n, c0, n, v[r]);   // uniform branch
#pragma unroll
      for (int r = 0; r < kPairsRowsInFlight; ++r) {
        if (a + r >= a1) break;
        const int32_t i = a + r;
        const int64_t di = diag[i];   // uniform over the workgroup
        int32_t hits = 0;
#pragma unroll
        for (int j = 0; j < kPairsColsPerLane; ++j) {
          const bool hit = c0 + j > i && c0 + j < n && pair_reported(v[r][j], di, dj[j], x);
          hits += (int32_t)__popcll(__ballot(hit));
        }
        if (lane == 0) wcnt[i - a0][wave] = hits;
      }
    }
    __syncthreads();
    if ((int32_t)threadIdx.x < a1 - a0) {
      int32_t total = 0;
#pragma unroll
      for (int w = 0; w < kPairsWaves; ++w) total += wcnt[threadIdx.x][w];
      cnt[(int64_t)(a0 + (int32_t)threadIdx.x) * ntiles + tile] = total;
    }
    __syncthreads();   // the next band of this workgroup rewrites wcnt
  }
}

// One wave per row: cnt[i][t] := sum of cnt[i][t'] over t' < t; rowoff[i] := the row's total
__global__ __launch_bounds__(kPairsThreads) void pairs_row_scan_kernel(int32_t* __restrict__ cnt, int32_t n, int32_t ntiles,
                                                                       int64_t* __restrict__ rowoff) {
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  const int64_t i = (int64_t)blockIdx.x * kPairsWaves + wave;
  if (i >= n) return;   // (whole waves leave; nothing below synchronises the workgroup)
  int32_t* __restrict__ row = cnt + i * (int64_t)ntiles;
  int32_t carry = 0;
  for (int32_t t0 = 0; t0 < ntiles; t0 += kWave) {
    const int32_t t = t0 + lane;
    const int32_t c = t < ntiles ? row[t] : 0;
    int32_t incl = c;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int32_t up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (t < ntiles) row[t] = carry + incl - c;
    carry += __shfl(incl, kWave - 1);
  }
  if (lane == 0) rowoff[i] = carry;
}

// One workgroup: rowoff[0 .. n) := its exclusive prefix, rowoff[n] := the total (n_found)
constexpr int kPairsScanThreads = 1024;
__global__ __launch_bounds__(kPairsScanThreads) void pairs_offset_scan_kernel(int64_t* __restrict__ rowoff, int32_t n) {
  __shared__ int64_t wsum[kPairsScanThreads / kWave];
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  int64_t carry = 0;
  for (int64_t base = 0; base < n; base += kPairsScanThreads) {
    const int64_t idx = base + threadIdx.x;
    const int64_t v = idx < n ? rowoff[idx] : 0;
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
    for (int w = 0; w < kPairsScanThreads / kWave; ++w) {
      const int64_t s = wsum[w];
      if (w < wave) below += s;
      total += s;
    }
    if (idx < n) rowoff[idx] = carry + below + incl - v;
    carry += total;
    __syncthreads();   // wsum is rewritten by the next chunk
  }
  if (threadIdx.x == 0) rowoff[n] = carry;
}

template <bool VEC, bool HAS64>
__global__ __launch_bounds__(kPairsThreads) void pairs_write_kernel(const int32_t* __restrict__ s32,
                                                                    const int64_t* __restrict__ s64, int32_t n,
                                                                    const int64_t* __restrict__ diag, double x, int32_t ntiles,
                                                                    const int32_t* __restrict__ prefix,
                                                                    const int64_t* __restrict__ rowoff, int64_t capacity,
                                                                    pcoa_pair* __restrict__ out,
                                                                    unsigned long long* __restrict__ entries_read) {
  __shared__ int32_t wtot[2][kPairsWaves];
  const int32_t tile = (int32_t)blockIdx.x;
  const int32_t tile0 = tile * kPairsTileCols;
  const int32_t c0 = tile0 + (int32_t)threadIdx.x * kPairsColsPerLane;
  const int wave = (int)threadIdx.x / kWave;
  int64_t dj[kPairsColsPerLane];
#pragma unroll
  for (int j = 0; j < kPairsColsPerLane; ++j) dj[j] = c0 + j < n ? diag[c0 + j] : 0;
  const int32_t nbands = (n + kPairsBandRows - 1) / kPairsBandRows;
  int slot = 0;
  unsigned long long cells = 0;   // the cells this workgroup reads again (uniform)
  for (int32_t band = (int32_t)blockIdx.y; band < nbands; band += (int32_t)gridDim.y) {
    const int32_t a0 = band * kPairsBandRows;
    const int32_t a1 = a0 + kPairsBandRows < n ? a0 + kPairsBandRows : n;
    if (tile_below_diagonal(tile0, a0)) continue;
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
      int64_t v[kPairsColsPerLane];
      load_quad<VEC, HAS64>(s32, s64, (int64_t)i * (int64_t)n, c0, n, v);
      const int64_t di = diag[i];
      bool hit[kPairsColsPerLane];
      int32_t lanes_before = 0, wave_total = 0;
#pragma unroll
      for (int j = 0; j < kPairsColsPerLane; ++j) {
        hit[j] = c0 + j > i && c0 + j < n && pair_reported(v[j], di, dj[j], x);
        const unsigned long long b = __ballot(hit[j]);
        lanes_before += (int32_t)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
        wave_total += (int32_t)__popcll(b);
      }
      slot ^= 1;   // two slots: a wave may write the next visited row's total while another still reads this one's
      if ((threadIdx.x & (kWave - 1)) == 0) wtot[slot][wave] = wave_total;
      __syncthreads();
      int64_t pos = first + lanes_before;
#pragma unroll
      for (int w = 0; w < kPairsWaves; ++w)
        if (w < wave) pos += wtot[slot][w];
#pragma unroll
      for (int j = 0; j < kPairsColsPerLane; ++j) {
        if (!hit[j]) continue;
        if (pos < capacity) {
          pcoa_pair p;
          p.i = i;
          p.j = c0 + j;
          p.shared = v[j];
          out[pos] = p;
        }
        ++pos;
      }
    }
  }
  // an integer count for pcoa_pairs_stats.pairs_bytes only: nothing of the result depends on it
  const int64_t width = (int64_t)n - tile0 < kPairsTileCols ? (int64_t)n - tile0 : (int64_t)kPairsTileCols;
  if (entries_read && cells && threadIdx.x == 0) atomicAdd(entries_read, cells * (unsigned long long)width);
}

dim3 pairs_grid(int32_t n, int32_t ntiles) {
  const unsigned bands = (unsigned)((n + kPairsBandRows - 1) / kPairsBandRows);
  return dim3((unsigned)ntiles, bands < 65535u ? bands : 65535u);
}

bool pairs_vec_ok(const int32_t* s32, int32_t n) { return n % 4 == 0 && ((uintptr_t)s32 & 15u) == 0; }

}  // namespace

int32_t pairs_tiles(int32_t n) { return (n + kPairsTileCols - 1) / kPairsTileCols; }

int64_t pairs_count_pass_entries(int32_t n) {
  // the entries of S the count pass loads: every (band, tile) that is not wholly on or below the diagonal, its rows x the
  // tile's columns inside the matrix
  int64_t entries = 0;
  const int32_t ntiles = pairs_tiles(n);
  for (int32_t a0 = 0; a0 < n; a0 += kPairsBandRows) {
    const int64_t rows = std::min<int64_t>(kPairsBandRows, (int64_t)n - a0);
    for (int32_t tile = a0 / kPairsTileCols; tile < ntiles; ++tile) {
      const int64_t tile0 = (int64_t)tile * kPairsTileCols;
      if (tile0 + kPairsTileCols - 1 <= a0) continue;
      entries += rows * std::min<int64_t>(kPairsTileCols, (int64_t)n - tile0);
    }
  }
  return entries;
}

hipError_t launch_pairs_diag(const int32_t* s32, const int64_t* s64_or_null, int32_t n, int64_t* diag, hipStream_t stream) {
  if (n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pairs_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, s32, s64_or_null, n, diag);
  return hipGetLastError();
}

hipError_t launch_pairs_count(const int32_t* s32, const int64_t* s64_or_null, int32_t n, const int64_t* diag, double x,
                              int32_t* cnt, hipStream_t stream) {
  if (n <= 0 || n > kPairsMaxSamples) return hipErrorInvalidValue;
  const int32_t ntiles = pairs_tiles(n);
  const dim3 grid = pairs_grid(n, ntiles);
  const bool vec = pairs_vec_ok(s32, n);
#define PCOA_PAIRS_COUNT(V, H) \
  hipLaunchKernelGGL((pairs_count_kernel<V, H>), grid, dim3(kPairsThreads), 0, stream, s32, s64_or_null, n, diag, x, ntiles, cnt)
  if (vec && s64_or_null) PCOA_PAIRS_COUNT(true, true);
  else if (vec) PCOA_PAIRS_COUNT(true, false);
  else if (s64_or_null) PCOA_PAIRS_COUNT(false, true);
  else PCOA_PAIRS_COUNT(false, false);
#undef PCOA_PAIRS_COUNT
  return hipGetLastError();
}

hipError_t launch_pairs_row_scan(int32_t* cnt, int32_t rows, int32_t ntiles, int64_t* rowoff, hipStream_t stream) {
  if (rows <= 0 || rows > kPairsMaxSamples || ntiles <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pairs_row_scan_kernel, dim3((unsigned)((rows + kPairsWaves - 1) / kPairsWaves)), dim3(kPairsThreads), 0, stream,
                     cnt, rows, ntiles, rowoff);
  return hipGetLastError();
}

hipError_t launch_pairs_scan(int32_t* cnt, int32_t n, int64_t* rowoff, hipStream_t stream) {
  if (n <= 0 || n > kPairsMaxSamples) return hipErrorInvalidValue;
  hipError_t e = launch_pairs_row_scan(cnt, n, pairs_tiles(n), rowoff, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pairs_offset_scan_kernel, dim3(1), dim3(kPairsScanThreads), 0, stream, rowoff, n);
  return hipGetLastError();
}

hipError_t launch_pairs_write(const int32_t* s32, const int64_t* s64_or_null, int32_t n, const int64_t* diag, double x,
                              const int32_t* prefix, const int64_t* rowoff, int64_t capacity, pcoa_pair* out,
                              unsigned long long* entries_read, hipStream_t stream) {
  if (n <= 0 || n > kPairsMaxSamples || capacity <= 0 || !out) return hipErrorInvalidValue;
  const int32_t ntiles = pairs_tiles(n);
  const dim3 grid = pairs_grid(n, ntiles);
  const bool vec = pairs_vec_ok(s32, n);
#define PCOA_PAIRS_WRITE(V, H)                                                                                               \
  hipLaunchKernelGGL((pairs_write_kernel<V, H>), grid, dim3(kPairsThreads), 0, stream, s32, s64_or_null, n, diag, x, ntiles, \
                     prefix, rowoff, capacity, out, entries_read)
  if (vec && s64_or_null) PCOA_PAIRS_WRITE(true, true);
  else if (vec) PCOA_PAIRS_WRITE(true, false);
  else if (s64_or_null) PCOA_PAIRS_WRITE(false, true);
  else PCOA_PAIRS_WRITE(false, false);
#undef PCOA_PAIRS_WRITE
  return hipGetLastError();
}

}  // namespace pcoa
