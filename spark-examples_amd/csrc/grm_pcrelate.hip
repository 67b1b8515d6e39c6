// grm_pcrelate.hip -- PC-Relate kinship (Conomos et al. 2016) on the 2-bit store of grm_bits.hip: kinship adjusted
// for the ancestry the axes of K found.  The rule (include/pcoa.h, pcoa_grm_pcrelate_block), per sample i and row v of the store:
//   e_iv  = beta_v0 * basis[0][i];  e_iv = e_iv + beta_vc * basis[c][i], c = 1 .. n_cov - 1        mu_iv = 0.5 * e_iv
//   m_iv  = used_v and c_iv and mu_iv > t and mu_iv < 1 - t
//   a_iv  = m_iv ? (double)g_iv - e_iv : 0.0        b_iv = m_iv ? sqrt(mu_iv * (1.0 - mu_iv)) : 0.0
//   num(i, j) = sum_v a_iv a_jv     den(i, j) = sum_v b_iv b_jv     n(i, j) = sum_v m_iv m_jv     phi = den > 0 ? num / (4 den) : 0
// every product and sum rounded on its own (no contraction).  The three sums are dense fp64 products on the matrix cores in
// grm_dense.hip's shape: v_mfma_f64_16x16x4_f64 (lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], and four
// results D[row (l >> 4) + 4 q][col l & 15]); a workgroup of four waves owns the 64 x 64 tile anchored at absolute multiples of 64
// samples, wave (wr, wc) holds 2 x 2 MFMA tiles, one launch walks ONE segment in k-steps of 4 rows and continues from what the
// launch over the previous segment left in the outputs.  What differs from grm_dense.hip is the operand: it is built per (sample,
// variant) from the low-rank model of the individual's allele frequency, so a lane keeps the basis values of its four samples in
// registers (4 NC doubles) and loads its row's n_cov beta values per k-step (the 16 lanes of a k read the same ones).
// Covariates are padded to a compile-time count NC in {1, 3, 5, 9} with beta = 0, basis = 0: e gains + 0.0 * 0.0 terms, which
// change no bit of it but the sign of a zero, and a zero e is masked (mu = 0 is not above t >= 0).
// Symmetry: nothing scales an operand, so (i, j) and (j, i) are sums of the same commuting products in the same order: the same
// bits, with no tile modes.  Determinism: the order of the additions into an entry is fixed by the variant's index in its
// segment alone, four at a time.  No LDS, no atomics.
#include <algorithm>

#include "grm_slots.h"
#include "pcoa_internal.h"

namespace pcoa {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// one slot of a word under the row's fit: a, b and m (as 0.0 / 1.0)
template <int NC>
__device__ __forceinline__ void pcr_operand(uint32_t w, int shift, const double (&bt)[NC], const double (&bs)[NC], bool row_used, double t,
                                            double one_minus_t, double& a, double& b, double& m) {
#pragma clang fp contract(off)
  const uint32_t code = (w >> shift) & 3u;
  const uint32_t hi = code >> 1;
  const bool called = code != 1u;
  const double g = (double)(int32_t)(hi + (hi & code));
  double e = bt[0] * bs[0];
#pragma unroll
  for (int c = 1; c < NC; ++c) e = e + bt[c] * bs[c];
  const double mu = 0.5 * e;
  const bool ok = row_used && called && mu > t && mu < one_minus_t;
  const double var = ok ? mu * (1.0 - mu) : 0.0;   // inside (0, 0.25] where ok
  a = ok ? g - e : 0.0;
  b = sqrt(var);
  m = ok ? 1.0 : 0.0;
}

// grid: (tile columns, tile rows) of the rectangle; tile0_r / tile0_c: the first tile row / column it touches.  used, beta: the
// segment's first row; basis: [n_cov][n]
template <int NC, bool PAIRS>
__global__ __launch_bounds__(256) void grm_pcrelate_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch,
                                                           const int32_t* __restrict__ used, const double* __restrict__ beta,
                                                           int32_t n_cov, const double* __restrict__ basis, int32_t n, double t,
                                                           double one_minus_t, int32_t row0, int32_t nrows, int32_t col0, int32_t ncols,
                                                           int32_t tile0_r, int32_t tile0_c, int first, double* __restrict__ out_num,
                                                           double* __restrict__ out_den, int32_t* __restrict__ out_n) {
#pragma clang fp contract(off)
  const int32_t tr = tile0_r + (int32_t)blockIdx.y, tc = tile0_c + (int32_t)blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int kk = lane >> 4, slot = lane & 15, shift = 2 * slot;
  const int rword = tr * 4 + wr * 2, cword = tc * 4 + wc * 2;   // both + 1 < pitch: the pitch is a multiple of 4 words
  const int ibase = tr * 64 + wr * 32 + kk, jbase = tc * 64 + wc * 32 + slot;

  // the basis values of the lane's four samples: row-invariant.  A sample behind n or a padded covariate holds 0.0
  double bs_r[2][NC], bs_c[2][NC];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int si = tr * 64 + wr * 32 + m * 16 + slot, sj = tc * 64 + wc * 32 + m * 16 + slot;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const bool have = c < n_cov;
      const int cc = have ? c : 0;
      const double vi = basis[(int64_t)cc * n + (si < n ? si : n - 1)];
      const double vj = basis[(int64_t)cc * n + (sj < n ? sj : n - 1)];
      bs_r[m][c] = (have && si < n) ? vi : 0.0;
      bs_c[m][c] = (have && sj < n) ? vj : 0.0;
    }
  }

  f64x4 num[2][2], den[2][2], cnt[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = ibase + m * 16 + 4 * q - row0, j = jbase + nn * 16 - col0;
        const bool in = !first && i >= 0 && i < nrows && j >= 0 && j < ncols;
        const int64_t idx = in ? (int64_t)i * ncols + j : 0;
        double v = 0.0, d = 0.0, p = 0.0;
        if (in) {
          v = out_num[idx];
          d = out_den[idx];
        }
        if (PAIRS && in) p = (double)out_n[idx];
        num[m][nn][q] = v;
        den[m][nn][q] = d;
        cnt[m][nn][q] = p;
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
    const bool u_v = live && used[rc] != 0;
    double bt[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double v = beta[(int64_t)rc * n_cov + (c < n_cov ? c : 0)];
      bt[c] = c < n_cov ? v : 0.0;
    }
    double ar[2], br[2], mr[2], ac[2], bc[2], mc[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      pcr_operand<NC>(wa[m], shift, bt, bs_r[m], u_v, t, one_minus_t, ar[m], br[m], mr[m]);
      pcr_operand<NC>(wb[m], shift, bt, bs_c[m], u_v, t, one_minus_t, ac[m], bc[m], mc[m]);
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn) {
        num[m][nn] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[m], ac[nn], num[m][nn], 0, 0, 0);
        den[m][nn] = __builtin_amdgcn_mfma_f64_16x16x4f64(br[m], bc[nn], den[m][nn], 0, 0, 0);
        if (PAIRS) cnt[m][nn] = __builtin_amdgcn_mfma_f64_16x16x4f64(mr[m], mc[nn], cnt[m][nn], 0, 0, 0);
      }
  }

#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = ibase + m * 16 + 4 * q - row0, j = jbase + nn * 16 - col0;
        if (i < 0 || i >= nrows || j < 0 || j >= ncols) continue;
        const int64_t idx = (int64_t)i * ncols + j;
        out_num[idx] = num[m][nn][q];
        out_den[idx] = den[m][nn][q];
        if (PAIRS) out_n[idx] = (int32_t)cnt[m][nn][q];
      }
}

// phi = den > 0 ? num / (4.0 * den) : 0.0, in place in num
__global__ __launch_bounds__(256) void grm_pcrelate_finish_kernel(double* __restrict__ num, const double* __restrict__ den, int64_t total) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const double d = den[i];
  num[i] = d > 0.0 ? num[i] / (4.0 * d) : 0.0;
}

// beta[r][c0 + c] = (the groups' partials of (A hat_c)[r] added in group order) + mu[r] * S[c0 + c], c in [0, k)
__global__ __launch_bounds__(256) void grm_pcrelate_beta_kernel(const double* __restrict__ tpart, int64_t vstride, int32_t groups,
                                                                int64_t cstride, int64_t rows, const double* __restrict__ mu,
                                                                const double* __restrict__ s, int32_t c0, int32_t k, int32_t n_cov,
                                                                double* __restrict__ beta) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const double m = mu[r];
  for (int32_t c = 0; c < k; ++c) {
    const double* part = tpart + (int64_t)c * cstride;
    double a = part[r];
    for (int32_t g = 1; g < groups; ++g) a += part[(int64_t)g * vstride + r];
    beta[r * n_cov + c0 + c] = a + m * s[c0 + c];
  }
}

// out[(v - first) * n + i] = mu_iv = 0.5 * e_iv for the rows [first, first + nv), unmasked
__global__ __launch_bounds__(256) void grm_pcrelate_isaf_kernel(const double* __restrict__ beta, int32_t n_cov,
                                                                const double* __restrict__ basis, int32_t n, int64_t first, int64_t nv,
                                                                double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t total = nv * n;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int64_t v = idx / n;
    const int32_t i = (int32_t)(idx - v * n);
    const double* bt = beta + (first + v) * n_cov;
    double e = bt[0] * basis[i];
    for (int32_t c = 1; c < n_cov; ++c) e = e + bt[c] * basis[(int64_t)c * n + i];
    out[idx] = 0.5 * e;
  }
}

template <int NC>
void launch_nc(dim3 grid, hipStream_t stream, const uint32_t* seg, int32_t rows, int32_t pitch, const int32_t* used, const double* beta,
               int32_t n_cov, const double* basis, int32_t n, double t, double omt, int32_t row0, int32_t nrows, int32_t col0,
               int32_t ncols, int32_t tile0_r, int32_t tile0_c, int first, double* out_num, double* out_den, int32_t* out_n) {
  if (out_n)
    hipLaunchKernelGGL((grm_pcrelate_kernel<NC, true>), grid, dim3(256), 0, stream, seg, rows, pitch, used, beta, n_cov, basis, n, t, omt,
                       row0, nrows, col0, ncols, tile0_r, tile0_c, first, out_num, out_den, out_n);
  else
    hipLaunchKernelGGL((grm_pcrelate_kernel<NC, false>), grid, dim3(256), 0, stream, seg, rows, pitch, used, beta, n_cov, basis, n, t, omt,
                       row0, nrows, col0, ncols, tile0_r, tile0_c, first, out_num, out_den, out_n);
}

}  // namespace

int32_t grm_pcrelate_padded_cov(int32_t n_cov) { return n_cov <= 1 ? 1 : n_cov <= 3 ? 3 : n_cov <= 5 ? 5 : 9; }

hipError_t launch_grm_pcrelate(const uint32_t* seg, int32_t rows, int32_t n, const int32_t* used, const double* beta, int32_t n_cov,
                               const double* basis, double t, int32_t row0, int32_t nrows, int32_t col0, int32_t ncols, int first,
                               double* out_num, double* out_den, int32_t* out_n, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if (n_cov < 1 || n_cov > kGrmPcrelateMaxCov || !out_num || !out_den) return hipErrorInvalidValue;
  const int32_t tile0_r = row0 / 64, tile0_c = col0 / 64;
  const dim3 grid((unsigned)((col0 + ncols - 1) / 64 - tile0_c + 1), (unsigned)((row0 + nrows - 1) / 64 - tile0_r + 1));
  const int32_t pitch = grm_pitch_words(n);
  const double omt = 1.0 - t;
  switch (grm_pcrelate_padded_cov(n_cov)) {
    case 1:
      launch_nc<1>(grid, stream, seg, rows, pitch, used, beta, n_cov, basis, n, t, omt, row0, nrows, col0, ncols, tile0_r, tile0_c, first,
                   out_num, out_den, out_n);
      break;
    case 3:
      launch_nc<3>(grid, stream, seg, rows, pitch, used, beta, n_cov, basis, n, t, omt, row0, nrows, col0, ncols, tile0_r, tile0_c, first,
                   out_num, out_den, out_n);
      break;
    case 5:
      launch_nc<5>(grid, stream, seg, rows, pitch, used, beta, n_cov, basis, n, t, omt, row0, nrows, col0, ncols, tile0_r, tile0_c, first,
                   out_num, out_den, out_n);
      break;
    default:
      launch_nc<9>(grid, stream, seg, rows, pitch, used, beta, n_cov, basis, n, t, omt, row0, nrows, col0, ncols, tile0_r, tile0_c, first,
                   out_num, out_den, out_n);
      break;
  }
  return hipGetLastError();
}

hipError_t launch_grm_pcrelate_finish(double* num, const double* den, int64_t total, hipStream_t stream) {
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(grm_pcrelate_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, num, den, total);
  return hipGetLastError();
}

hipError_t launch_grm_pcrelate_beta(const double* tpart, int64_t vstride, int32_t n, int64_t cstride, int64_t rows, const double* mu,
                                    const double* s, int32_t c0, int32_t k, int32_t n_cov, double* beta, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(grm_pcrelate_beta_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, tpart, vstride, grm_groups(n),
                     cstride, rows, mu, s, c0, k, n_cov, beta);
  return hipGetLastError();
}

hipError_t launch_grm_pcrelate_isaf(const double* beta, int32_t n_cov, const double* basis, int32_t n, int64_t first, int64_t nv,
                                    double* out, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>((nv * n + 255) / 256, 65536);
  hipLaunchKernelGGL(grm_pcrelate_isaf_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, beta, n_cov, basis, n, first, nv, out);
  return hipGetLastError();
}

}  // namespace pcoa
