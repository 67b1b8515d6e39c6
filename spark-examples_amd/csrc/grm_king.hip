// grm_king.hip -- the KING-robust kinship screen on the 2-bit store of a GRM ctx (pcoa_grm_king_block / pcoa_grm_king_pairs,
// DESIGN.md 4.26).  The rule is king.hip's, restated on genotype classes.  A slot of the store (grm_bits.hip) is in one class:
// H = 10 heterozygous, R / A = 00 / 11 the two homozygotes (KING is symmetric in them), M = 01 not called; C = R u H u A.  Over
// the counted rows, all exact integers:
//   hethet(i, j)  = sum_v H_vi H_vj
//   ibs0(i, j)    = sum_v (R_vi A_vj + A_vi R_vj)
//   het_sum(i, j) = sum_v (H_vi C_vj + C_vi H_vj)
//   the pair (i, j), i < j, is REPORTED iff het_sum > 0 and (double)(hethet - 2 ibs0) >= x * (double)het_sum
//
// The count kernel.  Four symmetric products sum_v a_vi a_vj, one int8 operand function each, give the three counts:
//   HH with a = H in {0, 1}, CC with a = C in {0, 1}, Q with a = H + C in {0, 1, 2}, xx with a = A - R in {-1, 0, 1}
//   hethet = HH,  het_sum = Q - HH - CC,  ibs0 = (2 CC + 2 HH - Q - xx) / 2   (always even)
// The instruction is v_mfma_i32_32x32x32_i8: lane l (r = l & 31, h = l >> 5) holds 16 bytes of A's row r and of B's column r, the
// k values of half h, and 16 results D[row (q & 3) + 8 (q >> 2) + 4 h][col r], q = 0 .. 15 (the map of gram_packed.hip's
// epilogue).  Both operands of a product are the SAME function of the same variants, so which 16 of a step's 32 variants the
// instruction takes for half h does not matter as long as A and B agree: here byte j of half h is variant 16 h + j of the step.
// A lane's sample sits in one slot of one word column of the store; the lane loads that word of its 16 rows, gathers the 16
// codes into four dwords of one code per byte and derives the four operands with byte-parallel bit operations: no LDS, no
// scratch.  A dead row of the last step, a row that is not counted (PCOA_GRM_ROWS_USED) and every padding slot are code 01: not
// called, in no class, they contribute nothing.
// Shape: grm_dense.hip's -- a workgroup of four waves owns the 64 x 64 tile (TR, TC) anchored at absolute multiples of 64
// samples, wave (wr, wc) its 32 x 32 quarter with the four int32 accumulators (64 registers); one launch per segment of the
// store.  The three counts are sums over variants themselves, so the epilogue combines the segment's four products and ADDS
// the result to what the launch over the previous segment left in the output (the first one stores).  Integer sums: (i, j) and
// (j, i), any rectangle and any segmentation give the same numbers.  The combination runs in uint32, so Q <= 4 V may wrap where
// het_sum <= 2 V < 2^31 still comes out exactly (the callers refuse 2^30 counted rows).  No atomics.
//
// The screen is the twin of grm_pairs.hip over the band's three int32 arrays: count, row scan, offset scan from the running
// total in device memory (both scans ARE grm_pairs.hip's, through launch_grm_pairs_scan), ordered write of pcoa_king_pair
// records.  A lane owns four consecutive columns: one 16-byte load per array and row.
#include <algorithm>

#include "grm_slots.h"
#include "pcoa_internal.h"

namespace pcoa {
namespace {

typedef int ki32x4 __attribute__((ext_vector_type(4)));
typedef int ki32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t kByteLo = 0x01010101u;   // the low bit of every byte

// the int8 operands of 16 variants of one sample, byte j = variant j
struct KingOperands { ki32x4 h, c, q, x; };

__device__ __forceinline__ void king_operands(const uint32_t (&w)[16], int shift, KingOperands& o) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const uint32_t code = ((w[4 * g] >> shift) & 3u) | (((w[4 * g + 1] >> shift) & 3u) << 8) | (((w[4 * g + 2] >> shift) & 3u) << 16) |
                          (((w[4 * g + 3] >> shift) & 3u) << 24);
    const uint32_t lo = code & kByteLo, hi = (code >> 1) & kByteLo;
    const uint32_t het = hi & ~lo;                   // 10
    const uint32_t called = (lo & ~hi) ^ kByteLo;    // not 01
    const uint32_t hom2 = hi & lo;                   // 11
    const uint32_t hom0 = (hi | lo) ^ kByteLo;       // 00
    o.h[g] = (int)het;
    o.c[g] = (int)called;
    o.q[g] = (int)(het + called);                    // bytes 0, 1, 2: no carry
    o.x[g] = (int)(hom2 | ((hom0 << 8) - hom0));     // (b << 8) - b is 0xff in every byte whose low bit is set: -1
  }
}

// grid: (tile columns, tile rows) of the rectangle; tile0_r / tile0_c: the first tile row / column it touches
template <bool USED>
__global__ __launch_bounds__(256) void grm_king_counts_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch,
                                                              const int32_t* __restrict__ used, int32_t row0, int32_t nrows,
                                                              int32_t col0, int32_t ncols, int32_t tile0_r, int32_t tile0_c, int first,
                                                              int32_t* __restrict__ out_hethet, int32_t* __restrict__ out_ibs0,
                                                              int32_t* __restrict__ out_het_sum) {
  const int32_t tr = tile0_r + (int32_t)blockIdx.y, tc = tile0_c + (int32_t)blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int r = lane & 31, half = lane >> 5;
  const int shift = 2 * (r & 15);
  const int aword = tr * 4 + wr * 2 + (r >> 4), bword = tc * 4 + wc * 2 + (r >> 4);   // both < pitch: a multiple of 4 words

  ki32x16 acc[4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[p][q] = 0;

  for (int32_t rb = 0; rb < rows; rb += 32) {
    uint32_t wa[16], wb[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int32_t v = rb + 16 * half + j;
      const int32_t vc = v < rows ? v : rows - 1;   // loads of a dead row go to a valid row and are discarded
      const uint32_t* __restrict__ p = seg + (int64_t)vc * pitch;
      bool live = v < rows;
      if (USED) live = live && used[vc] != 0;
      const uint32_t a = p[aword], b = p[bword];
      wa[j] = live ? a : kLo;
      wb[j] = live ? b : kLo;
    }
    KingOperands a, b;
    king_operands(wa, shift, a);
    king_operands(wb, shift, b);
    acc[0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a.h, b.h, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a.c, b.c, acc[1], 0, 0, 0);
    acc[2] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a.q, b.q, acc[2], 0, 0, 0);
    acc[3] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a.x, b.x, acc[3], 0, 0, 0);
  }

  const int32_t gj = tc * 64 + wc * 32 + r;
  const int32_t j = gj - col0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int32_t gi = tr * 64 + wr * 32 + (q & 3) + 8 * (q >> 2) + 4 * half;
    const int32_t i = gi - row0;
    if (i < 0 || i >= nrows || j < 0 || j >= ncols) continue;
    const int64_t idx = (int64_t)i * ncols + j;
    const uint32_t hh = (uint32_t)acc[0][q], cc = (uint32_t)acc[1][q], qq = (uint32_t)acc[2][q], xx = (uint32_t)acc[3][q];
    const uint32_t het_sum = qq - hh - cc;
    const uint32_t ibs0 = (2u * cc + 2u * hh - qq - xx) >> 1;
    if (out_hethet) out_hethet[idx] = (int32_t)(hh + (first ? 0u : (uint32_t)out_hethet[idx]));
    if (out_ibs0) out_ibs0[idx] = (int32_t)(ibs0 + (first ? 0u : (uint32_t)out_ibs0[idx]));
    if (out_het_sum) out_het_sum[idx] = (int32_t)(het_sum + (first ? 0u : (uint32_t)out_het_sum[idx]));
  }
}

// ---- the screen ----------------------------------------------------------------------------------------------------------------

constexpr int kKingBandThreads = 256;
constexpr int kKingBandWaves = kKingBandThreads / kWave;
constexpr int kKingBandColsPerLane = kGrmPairsTileCols / kKingBandThreads;
constexpr int kKingBandRowsInFlight = 2;
static_assert(kKingBandColsPerLane == 4, "a lane owns one 16-byte quad of int32 columns");
static_assert(kGrmPairsRows % kKingBandRowsInFlight == 0 && kGrmPairsRows <= kKingBandThreads, "workgroup shape");

// the band as the kernels see it (by value in the kernel arguments)
struct KingBand {
  const int32_t *hethet, *ibs0, *het_sum;   // [nrows][pitch] each
  int64_t pitch;                            // int32 between two rows, a multiple of 4; the arrays are 16-byte aligned
  int32_t r0, nrows;                        // rows [r0, r0 + nrows) of the counts
  int32_t c0;                               // column 0 of the band is sample c0
  int32_t n;                                // samples: columns at or behind n - c0 are padding and never reported
  int32_t ntiles;                           // column tiles of the band (the grid's x)
};

struct KingQuad { int32_t hethet[kKingBandColsPerLane], ibs0[kKingBandColsPerLane], het_sum[kKingBandColsPerLane]; };

// the three counts of (row, lc .. lc + 3); a quad lies wholly inside the row or wholly outside and then reads as 0
__device__ __forceinline__ void king_load_quad(const KingBand& b, int64_t rowbase, int32_t lc, KingQuad& v) {
  int4 h = make_int4(0, 0, 0, 0), s = h, t = h;
  if ((int64_t)lc < b.pitch) {
    h = *reinterpret_cast<const int4*>(b.hethet + rowbase + lc);
    s = *reinterpret_cast<const int4*>(b.ibs0 + rowbase + lc);
    t = *reinterpret_cast<const int4*>(b.het_sum + rowbase + lc);
  }
  v.hethet[0] = h.x; v.hethet[1] = h.y; v.hethet[2] = h.z; v.hethet[3] = h.w;
  v.ibs0[0] = s.x; v.ibs0[1] = s.y; v.ibs0[2] = s.z; v.ibs0[3] = s.w;
  v.het_sum[0] = t.x; v.het_sum[1] = t.y; v.het_sum[2] = t.z; v.het_sum[3] = t.w;
}

// the rule, stated once for both passes: sample gj against row sample i
__device__ __forceinline__ bool king_pair_reported(int32_t hethet, int32_t ibs0, int32_t het_sum, int32_t i, int32_t gj, int32_t n,
                                                   double x) {
#pragma clang fp contract(off)
  const int64_t num = (int64_t)hethet - 2 * (int64_t)ibs0;
  return gj > i && gj < n && het_sum > 0 && (double)num >= x * (double)het_sum;
}

// true when every column of the tile is left of every row of the workgroup: neither a pair i < j nor a diagonal entry is there
__device__ __forceinline__ bool king_tile_left_of_diagonal(const KingBand& b, int32_t tile, int32_t a0) {
  return (int64_t)b.c0 + ((int64_t)tile + 1) * kGrmPairsTileCols <= (int64_t)b.r0 + a0;
}

__global__ __launch_bounds__(kKingBandThreads) void grm_king_screen_count_kernel(KingBand b, double x, int32_t* __restrict__ cnt,
                                                                                int64_t* __restrict__ het) {
  __shared__ int32_t wcnt[kGrmPairsRows][kKingBandWaves];
  const int32_t tile = (int32_t)blockIdx.x;
  const int32_t lc = tile * kGrmPairsTileCols + (int32_t)threadIdx.x * kKingBandColsPerLane;   // the lane's first band column
  const int32_t gc = b.c0 + lc;                                                                // and its sample
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  const int32_t a0 = (int32_t)blockIdx.y * kGrmPairsRows;
  const int32_t a1 = a0 + kGrmPairsRows < b.nrows ? a0 + kGrmPairsRows : b.nrows;
  if (king_tile_left_of_diagonal(b, tile, a0)) {
    if ((int32_t)threadIdx.x < a1 - a0) cnt[(int64_t)(a0 + (int32_t)threadIdx.x) * b.ntiles + tile] = 0;
    return;
  }
  for (int32_t a = a0; a < a1; a += kKingBandRowsInFlight) {
    KingQuad v[kKingBandRowsInFlight];
#pragma unroll
    for (int r = 0; r < kKingBandRowsInFlight; ++r)
      if (a + r < a1) king_load_quad(b, (int64_t)(a + r) * b.pitch, lc, v[r]);   // uniform branch
#pragma unroll
    for (int r = 0; r < kKingBandRowsInFlight; ++r) {
      if (a + r >= a1) break;
      const int32_t i = b.r0 + a + r;
      int32_t hits = 0;
#pragma unroll
      for (int j = 0; j < kKingBandColsPerLane; ++j) {
        hits += (int32_t)__popcll(__ballot(king_pair_reported(v[r].hethet[j], v[r].ibs0[j], v[r].het_sum[j], i, gc + j, b.n, x)));
        if (het && gc + j == i) het[i] = (int64_t)v[r].hethet[j];   // hethet(i, i) = h_i
      }
      if (lane == 0) wcnt[a + r - a0][wave] = hits;
    }
  }
  __syncthreads();
  if ((int32_t)threadIdx.x < a1 - a0) {
    int32_t total = 0;
#pragma unroll
    for (int w = 0; w < kKingBandWaves; ++w) total += wcnt[threadIdx.x][w];
    cnt[(int64_t)(a0 + (int32_t)threadIdx.x) * b.ntiles + tile] = total;
  }
}

__global__ __launch_bounds__(kKingBandThreads) void grm_king_screen_write_kernel(KingBand b, double x, const int32_t* __restrict__ prefix,
                                                                                const int64_t* __restrict__ rowoff, int64_t capacity,
                                                                                pcoa_king_pair* __restrict__ out,
                                                                                unsigned long long* __restrict__ entries_read) {
  __shared__ int32_t wtot[2][kKingBandWaves];
  const int32_t tile = (int32_t)blockIdx.x;
  const int32_t lc = tile * kGrmPairsTileCols + (int32_t)threadIdx.x * kKingBandColsPerLane;
  const int32_t gc = b.c0 + lc;
  const int wave = (int)threadIdx.x / kWave;
  const int32_t a0 = (int32_t)blockIdx.y * kGrmPairsRows;
  const int32_t a1 = a0 + kGrmPairsRows < b.nrows ? a0 + kGrmPairsRows : b.nrows;
  if (king_tile_left_of_diagonal(b, tile, a0)) return;
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
    const int32_t i = b.r0 + a;
    KingQuad v;
    king_load_quad(b, (int64_t)a * b.pitch, lc, v);
    bool hit[kKingBandColsPerLane];
    int32_t lanes_before = 0, wave_total = 0;
#pragma unroll
    for (int j = 0; j < kKingBandColsPerLane; ++j) {
      hit[j] = king_pair_reported(v.hethet[j], v.ibs0[j], v.het_sum[j], i, gc + j, b.n, x);
      const unsigned long long m = __ballot(hit[j]);
      lanes_before += (int32_t)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      wave_total += (int32_t)__popcll(m);
    }
    slot ^= 1;   // two slots: a wave may write the next visited row's total while another still reads this one's
    if ((threadIdx.x & (kWave - 1)) == 0) wtot[slot][wave] = wave_total;
    __syncthreads();
    int64_t pos = first + lanes_before;
#pragma unroll
    for (int w = 0; w < kKingBandWaves; ++w)
      if (w < wave) pos += wtot[slot][w];
#pragma unroll
    for (int j = 0; j < kKingBandColsPerLane; ++j) {
      if (!hit[j]) continue;
      if (pos < capacity) {
        pcoa_king_pair p;
        p.i = i;
        p.j = gc + j;
        p.hethet = v.hethet[j];
        p.ibs0 = v.ibs0[j];
        p.het_sum = v.het_sum[j];
        out[pos] = p;
      }
      ++pos;
    }
  }
  // an integer count for pcoa_grm_king_stats.grm_king_bytes only: nothing of the result depends on it
  const int64_t left = (int64_t)b.n - b.c0 - (int64_t)tile * kGrmPairsTileCols;
  const int64_t width = left < kGrmPairsTileCols ? left : (int64_t)kGrmPairsTileCols;
  if (entries_read && cells && threadIdx.x == 0) atomicAdd(entries_read, cells * (unsigned long long)width);
}

// nrows >= 1, c0 a multiple of 64 in [0, n), c0 <= r0, the band's columns reach the last sample, 16-byte quads
bool king_band_ok(const int32_t* hethet, const int32_t* ibs0, const int32_t* het_sum, int64_t pitch, int32_t r0, int32_t nrows,
                  int32_t c0, int32_t n) {
  if (!hethet || !ibs0 || !het_sum) return false;
  if ((((uintptr_t)hethet | (uintptr_t)ibs0 | (uintptr_t)het_sum) & 15u) != 0 || pitch % 4 != 0) return false;
  return n > 0 && nrows > 0 && r0 >= 0 && nrows <= n - r0 && c0 >= 0 && c0 % 64 == 0 && c0 <= r0 && pitch >= (int64_t)n - c0;
}

KingBand make_king_band(const int32_t* hethet, const int32_t* ibs0, const int32_t* het_sum, int64_t pitch, int32_t r0, int32_t nrows,
                        int32_t c0, int32_t n) {
  KingBand b;
  b.hethet = hethet;
  b.ibs0 = ibs0;
  b.het_sum = het_sum;
  b.pitch = pitch;
  b.r0 = r0;
  b.nrows = nrows;
  b.c0 = c0;
  b.n = n;
  b.ntiles = grm_pairs_tiles(n - c0);
  return b;
}

dim3 king_band_grid(const KingBand& b) { return dim3((unsigned)b.ntiles, (unsigned)((b.nrows + kGrmPairsRows - 1) / kGrmPairsRows)); }

}  // namespace

hipError_t launch_grm_king_counts(const uint32_t* seg, int32_t rows, int32_t n, const int32_t* used_or_null, int32_t row0, int32_t nrows,
                                  int32_t col0, int32_t ncols, int first, int32_t* out_hethet, int32_t* out_ibs0, int32_t* out_het_sum,
                                  hipStream_t stream) {
  if (rows <= 0 || (!out_hethet && !out_ibs0 && !out_het_sum)) return hipSuccess;
  const int32_t pitch = grm_pitch_words(n);
  // every tile the grid touches lies inside the store's word columns: nothing is loaded or stored outside them
  if (!seg || row0 < 0 || col0 < 0 || nrows < 1 || ncols < 1 || ((int64_t)row0 + nrows + 63) / 64 * 4 > pitch ||
      ((int64_t)col0 + ncols + 63) / 64 * 4 > pitch)
    return hipErrorInvalidValue;
  const int32_t tile0_r = row0 / 64, tile0_c = col0 / 64;
  const dim3 grid((unsigned)((col0 + ncols - 1) / 64 - tile0_c + 1), (unsigned)((row0 + nrows - 1) / 64 - tile0_r + 1));
  if (used_or_null)
    hipLaunchKernelGGL((grm_king_counts_kernel<true>), grid, dim3(256), 0, stream, seg, rows, pitch, used_or_null, row0, nrows, col0,
                       ncols, tile0_r, tile0_c, first, out_hethet, out_ibs0, out_het_sum);
  else
    hipLaunchKernelGGL((grm_king_counts_kernel<false>), grid, dim3(256), 0, stream, seg, rows, pitch, used_or_null, row0, nrows, col0,
                       ncols, tile0_r, tile0_c, first, out_hethet, out_ibs0, out_het_sum);
  return hipGetLastError();
}

hipError_t launch_grm_king_screen_count(const int32_t* hethet, const int32_t* ibs0, const int32_t* het_sum, int64_t pitch, int32_t r0,
                                        int32_t nrows, int32_t c0, int32_t n, double x, int32_t* cnt, int64_t* het_or_null,
                                        hipStream_t stream) {
  if (!king_band_ok(hethet, ibs0, het_sum, pitch, r0, nrows, c0, n) || !cnt) return hipErrorInvalidValue;
  const KingBand b = make_king_band(hethet, ibs0, het_sum, pitch, r0, nrows, c0, n);
  hipLaunchKernelGGL(grm_king_screen_count_kernel, king_band_grid(b), dim3(kKingBandThreads), 0, stream, b, x, cnt, het_or_null);
  return hipGetLastError();
}

hipError_t launch_grm_king_screen_write(const int32_t* hethet, const int32_t* ibs0, const int32_t* het_sum, int64_t pitch, int32_t r0,
                                        int32_t nrows, int32_t c0, int32_t n, double x, const int32_t* prefix, const int64_t* rowoff,
                                        int64_t capacity, pcoa_king_pair* out, unsigned long long* entries_read, hipStream_t stream) {
  if (!king_band_ok(hethet, ibs0, het_sum, pitch, r0, nrows, c0, n) || !prefix || !rowoff || capacity <= 0 || !out)
    return hipErrorInvalidValue;
  const KingBand b = make_king_band(hethet, ibs0, het_sum, pitch, r0, nrows, c0, n);
  hipLaunchKernelGGL(grm_king_screen_write_kernel, king_band_grid(b), dim3(kKingBandThreads), 0, stream, b, x, prefix, rowoff, capacity,
                     out, entries_read);
  return hipGetLastError();
}

}  // namespace pcoa
