// grm_dense.hip -- reading K out: a rectangle of the genetic relationship matrix K = A^T diag(d) A / M' (and of the pair counts
// n) as a dense fp64 product on the matrix cores, fed straight from the 2-bit store of grm_bits.hip.  The rule
// (include/pcoa.h, pcoa_grm_block), with a_vi = c_iv ? (double)g_iv - mu_v : 0.0:
//   num(i, j) = sum_v (d_v a_v,lo) a_v,hi    lo = min(i, j), hi = max(i, j): d rides on the operand of the smaller sample index
//   n(i, j)   = sum_v used_v c_iv c_jv
// The instruction is v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], one double
// each, and four results D[row (l >> 4) + 4 q][col l & 15], q = 0 .. 3 (NOT the f32 map).  A row of 16 samples of one operand
// is exactly one word of the store, so the 16 lanes of a k read the same word and each extracts its own slot; a padding slot
// is code 01 and decodes to 0, so nothing is masked on the input side.
// Shape: a workgroup of four waves owns the 64 x 64 tile (TR, TC) of K, anchored at absolute multiples of 64 samples; wave
// (wr, wc) holds 2 x 2 MFMA tiles.  A launch walks ONE segment of the store in k-steps of 4 rows, in order, with the accumulators
// in registers; the entries inside the requested rectangle start from what the launch over the previous segment left in the
// output (the first one starts from 0), entries of edge tiles outside it are dropped.
// Symmetry: a tile strictly above the diagonal (TR < TC: every i < j) scales the row operand, one strictly below scales the
// column operand, a tile on the diagonal runs both forms and selects per element.  (i, j) and (j, i) are then sums of the same
// products -- the multiplicands of a product commute -- added in the same order: the same bits.
// Determinism: the order of the additions into an entry is fixed by the variant's index in its segment alone: not by the
// rectangle, the grid, the CU count or the sizes of the accumulate calls.  No atomics of any kind.
#include "grm_slots.h"
#include "pcoa_internal.h"

namespace pcoa {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// one slot of a word: a = c ? (double)g - mu : 0.0 and c as a double
__device__ __forceinline__ void decode_slot(uint32_t w, int shift, double mu, double& a, double& c) {
#pragma clang fp contract(off)
  const uint32_t code = (w >> shift) & 3u;
  const uint32_t hi = code >> 1;
  const bool called = code != 1u;
  const double g = (double)(int32_t)(hi + (hi & code));
  a = called ? g - mu : 0.0;
  c = called ? 1.0 : 0.0;
}

// MODE 0: the tile is strictly above the diagonal, 1: strictly below, 2: on it
template <int MODE, bool NUM, bool PAIRS>
__device__ __forceinline__ void dense_tile(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch, const double* __restrict__ mu,
                                           const double* __restrict__ d, const int32_t* __restrict__ used, int32_t row0, int32_t nrows,
                                           int32_t col0, int32_t ncols, int32_t tr, int32_t tc, int first, double* __restrict__ out_k,
                                           int32_t* __restrict__ out_n) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int kk = lane >> 4, slot = lane & 15, shift = 2 * slot;
  const int rword = tr * 4 + wr * 2, cword = tc * 4 + wc * 2;   // both + 1 < pitch: the pitch is a multiple of 4 words
  const int ibase = tr * 64 + wr * 32 + kk, jbase = tc * 64 + wc * 32 + slot;

  f64x4 acc[2][2], alt[2][2], cnt[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = ibase + m * 16 + 4 * q - row0, j = jbase + n * 16 - col0;
        const bool in = !first && i >= 0 && i < nrows && j >= 0 && j < ncols;
        const int64_t idx = in ? (int64_t)i * ncols + j : 0;
        double v = 0.0, p = 0.0;
        if (NUM && in) v = out_k[idx];
        if (PAIRS && in) p = (double)out_n[idx];
        acc[m][n][q] = v;
        alt[m][n][q] = v;
        cnt[m][n][q] = p;
      }

  for (int rb = 0; rb < rows; rb += 4) {
    const int r = rb + kk;
    const bool live = r < rows;
    const int rc = live ? r : rows - 1;   // loads of a dead k go to a valid row and are discarded
    const uint32_t* __restrict__ p = seg + (int64_t)rc * pitch;
    uint32_t wa[2], wb[2];
    wa[0] = p[rword];
    wa[1] = p[rword + 1];
    wb[0] = p[cword];
    wb[1] = p[cword + 1];
    const double m_v = mu[rc];
    double d_v = 0.0;
    if (NUM) d_v = live ? d[rc] : 0.0;
    bool u_v = false;
    if (PAIRS) u_v = live && used[rc] != 0;
    double a[2], b[2], ca[2], cb[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      decode_slot(live ? wa[m] : kLo, shift, m_v, a[m], ca[m]);
      decode_slot(live ? wb[m] : kLo, shift, m_v, b[m], cb[m]);
    }
    if (NUM) {
      double as[2], bs[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        as[m] = d_v * a[m];
        bs[m] = d_v * b[m];
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          if (MODE != 1) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[m], b[n], acc[m][n], 0, 0, 0);
          if (MODE == 1) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], bs[n], acc[m][n], 0, 0, 0);
          if (MODE == 2) alt[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], bs[n], alt[m][n], 0, 0, 0);
        }
    }
    if (PAIRS) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const double cu = u_v ? ca[m] : 0.0;
#pragma unroll
        for (int n = 0; n < 2; ++n) cnt[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(cu, cb[n], cnt[m][n], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int gi = ibase + m * 16 + 4 * q, gj = jbase + n * 16;
        const int i = gi - row0, j = gj - col0;
        if (i < 0 || i >= nrows || j < 0 || j >= ncols) continue;
        const int64_t idx = (int64_t)i * ncols + j;
        if (NUM) out_k[idx] = (MODE == 2 && gi > gj) ? alt[m][n][q] : acc[m][n][q];
        if (PAIRS) out_n[idx] = (int32_t)cnt[m][n][q];
      }
}

// grid: (tile columns, tile rows) of the rectangle; tile0_r / tile0_c: the first tile row / column it touches
template <bool NUM, bool PAIRS>
__global__ __launch_bounds__(256) void grm_dense_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch,
                                                        const double* __restrict__ mu, const double* __restrict__ d,
                                                        const int32_t* __restrict__ used, int32_t row0, int32_t nrows, int32_t col0,
                                                        int32_t ncols, int32_t tile0_r, int32_t tile0_c, int first,
                                                        double* __restrict__ out_k, int32_t* __restrict__ out_n) {
  const int32_t tr = tile0_r + (int32_t)blockIdx.y, tc = tile0_c + (int32_t)blockIdx.x;
  if (tr < tc)
    dense_tile<0, NUM, PAIRS>(seg, rows, pitch, mu, d, used, row0, nrows, col0, ncols, tr, tc, first, out_k, out_n);
  else if (tr > tc)
    dense_tile<1, NUM, PAIRS>(seg, rows, pitch, mu, d, used, row0, nrows, col0, ncols, tr, tc, first, out_k, out_n);
  else
    dense_tile<2, NUM, PAIRS>(seg, rows, pitch, mu, d, used, row0, nrows, col0, ncols, tr, tc, first, out_k, out_n);
}

// K = num / M' (divisor 0) or n > 0 ? num / n : 0.0 (divisor 1), in place: one division per entry
__global__ __launch_bounds__(256) void grm_dense_finish_kernel(double* __restrict__ k, const int32_t* __restrict__ n, int64_t total,
                                                               int32_t divisor, double mprime) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const double num = k[i];
  if (divisor == 0) {
    k[i] = num / mprime;
  } else {
    const int32_t c = n[i];
    k[i] = c > 0 ? num / (double)c : 0.0;
  }
}

}  // namespace

hipError_t launch_grm_dense(const uint32_t* seg, int32_t rows, int32_t n, const double* mu, const double* d, const int32_t* used,
                            int32_t row0, int32_t nrows, int32_t col0, int32_t ncols, int first, double* out_k, int32_t* out_n,
                            hipStream_t stream) {
  if (rows <= 0 || (!out_k && !out_n)) return hipSuccess;
  const int32_t tile0_r = row0 / 64, tile0_c = col0 / 64;
  const dim3 grid((unsigned)((col0 + ncols - 1) / 64 - tile0_c + 1), (unsigned)((row0 + nrows - 1) / 64 - tile0_r + 1));
  const int32_t pitch = grm_pitch_words(n);
  if (out_k && out_n)
    hipLaunchKernelGGL((grm_dense_kernel<true, true>), grid, dim3(256), 0, stream, seg, rows, pitch, mu, d, used, row0, nrows, col0,
                       ncols, tile0_r, tile0_c, first, out_k, out_n);
  else if (out_k)
    hipLaunchKernelGGL((grm_dense_kernel<true, false>), grid, dim3(256), 0, stream, seg, rows, pitch, mu, d, used, row0, nrows, col0,
                       ncols, tile0_r, tile0_c, first, out_k, out_n);
  else
    hipLaunchKernelGGL((grm_dense_kernel<false, true>), grid, dim3(256), 0, stream, seg, rows, pitch, mu, d, used, row0, nrows, col0,
                       ncols, tile0_r, tile0_c, first, out_k, out_n);
  return hipGetLastError();
}

hipError_t launch_grm_dense_finish(double* k, const int32_t* n, int64_t total, int32_t divisor, int64_t mprime, hipStream_t stream) {
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(grm_dense_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, k, n, total, divisor,
                     (double)mprime);
  return hipGetLastError();
}

}  // namespace pcoa
