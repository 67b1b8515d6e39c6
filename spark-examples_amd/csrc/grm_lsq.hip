// grm_lsq.hip -- the least-squares projection of sparsely called study samples onto the axes of K (the rule is
// stated at pcoa_grm_project_lsq in pcoa.h).  Per study sample q the normal equations H_q x = P_q are formed and solved:
//   P_q[c]    = sum_v (g_vq - mu_v c_vq) t_vc             grm_multi.hip's pass 2, its partials added here WITHOUT the division
//   p_v[c,c'] = used_v ? (t_vc * t_vc') / d_v : 0.0       grm_lsq_products_kernel, one chunk of J pairs at a time as [J][V]
//   H_q[c,c'] = sum_v c_vq p_v[c,c']                      grm_lsq_pairs_kernel<J> over the STUDY's store: per word only the
//                                                         called mask, per genotype one v_bfe_i32 and J masked adds
//   x_q                                                   grm_lsq_solve_kernel: a lane per sample, square-root-free Cholesky
// A pair's sum is added in the order grm_multi.hip's pass 2 fixes -- the rows of a range in order, the ranges in (segment,
// range) order -- and a lane's J accumulator sets never meet, so the sum has the same bits whatever chunk the pair rode in and
// whatever num_pc was.  J is 4, 2 or 1.  No floating-point atomics anywhere.
#include "grm_slots.h"
#include "pcoa_internal.h"

namespace pcoa {

int grm_lsq_chunk(int32_t remaining) { return remaining >= 4 ? 4 : remaining >= 2 ? 2 : 1; }

namespace {

// p[j][v] of the pairs e0 .. e0 + J - 1 (blockIdx.y = j); pair e = c (c + 1) / 2 + c', c' <= c
__global__ __launch_bounds__(256) void grm_lsq_products_kernel(const double* __restrict__ t, int64_t tstride,
                                                               const double* __restrict__ d, const int32_t* __restrict__ used,
                                                               int64_t rows, int32_t e0, double* __restrict__ p) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= rows) return;
  const int32_t e = e0 + (int32_t)blockIdx.y;
  int32_t c = 0;
  while ((c + 1) * (c + 2) / 2 <= e) ++c;
  const int32_t c2 = e - c * (c + 1) / 2;
  const double a = t[(int64_t)c * tstride + v], b = t[(int64_t)c2 * tstride + v];
  p[(int64_t)blockIdx.y * rows + v] = used[v] ? (a * b) / d[v] : 0.0;
}

// hpart[j][range][pitch * 16] = sum over the range's rows r of c(r, i) p_j[r]
template <int J>
__global__ __launch_bounds__(256, 2) void grm_lsq_pairs_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch,
                                                               int32_t words, const double* __restrict__ p, int64_t pstride,
                                                               double* __restrict__ hpart, int64_t ystride, int64_t cstride) {
#pragma clang fp contract(off)
  constexpr int U = 4;   // rows in flight
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (blockIdx.y * 4 + wave) * 64 + lane;
  if (col >= words) return;
  const int r0 = blockIdx.x * kGrmRangeRows;
  const int r1 = min(rows, r0 + kGrmRangeRows);
  double acc[J][16];
#pragma unroll
  for (int j = 0; j < J; ++j) {
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[j][k] = 0.0;
  }
  for (int rb = r0; rb < r1; rb += U) {
    uint32_t w[U];
    double pv[U][J];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = min(rb + u, r1 - 1);
      const uint32_t v = seg[(int64_t)r * pitch + col];
      w[u] = rb + u < r1 ? v : kLo;   // a row behind the range: nobody called, nothing added
#pragma unroll
      for (int j = 0; j < J; ++j) pv[u][j] = p[(int64_t)j * pstride + r];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t called = ((w[u] >> 1) | ~w[u]) & kLo;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int mc = __builtin_amdgcn_sbfe((int)called, 2u * k, 1u);
#pragma unroll
        for (int j = 0; j < J; ++j) acc[j][k] += and_mask(pv[u][j], mc);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    double* out = hpart + (int64_t)j * cstride + (int64_t)blockIdx.x * ystride + (int64_t)col * 16;
#pragma unroll
    for (int k = 0; k < 16; ++k) out[k] = acc[j][k];
  }
}

// out[c][i] = the ranges' partials of column c added in order, nothing else (blockIdx.y = c)
__global__ __launch_bounds__(256) void grm_lsq_finish_kernel(const double* __restrict__ part, int64_t ystride, int32_t nranges,
                                                             int64_t cstride, int32_t n, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (i >= n) return;
  const double* col = part + (int64_t)c * cstride;
  double a = 0.0;
  for (int32_t g = 0; g < nranges; ++g) a += col[(int64_t)g * ystride + i];
  out[(int64_t)c * n + i] = a;
}

// a: [K (K + 1) / 2 + K][nq], H_q packed (entry c (c + 1) / 2 + c') then P_q; a lane owns sample q and works in place, in the
// operation sequence pcoa.h states.  On return rows K (K + 1) / 2 .. hold the coordinates (NaN for an undetermined sample).
__global__ __launch_bounds__(256) void grm_lsq_solve_kernel(double* a, int32_t nq, int32_t kk, int32_t* __restrict__ determined,
                                                            int32_t* __restrict__ undetermined) {
#pragma clang fp contract(off)
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  const int64_t n = nq;
  double* h = a + q;
  double* b = a + (int64_t)(kk * (kk + 1) / 2) * n + q;
  bool ok = true;
  for (int c = 0; c < kk; ++c) {
    const int rc = c * (c + 1) / 2;
    const double hcc = h[(rc + c) * n];
    if (hcc == 0.0) {
      ok = false;
      break;
    }
    for (int j = 0; j < c; ++j) {   // w[c][j] = L[c][j] D[j]
      const int rj = j * (j + 1) / 2;
      double s = h[(rc + j) * n];
      for (int k = 0; k < j; ++k) s = s - h[(rc + k) * n] * h[(rj + k) * n];
      h[(rc + j) * n] = s;
    }
    double s = hcc;
    for (int k = 0; k < c; ++k) {
      const double w = h[(rc + k) * n];
      const double l = w / h[(k * (k + 1) / 2 + k) * n];
      s = s - w * l;
      h[(rc + k) * n] = l;
    }
    if (s <= 0x1p-40 * hcc) {
      ok = false;
      break;
    }
    h[(rc + c) * n] = s;
  }
  if (!ok) {
    for (int c = 0; c < kk; ++c) b[c * n] = __builtin_nan("");
    determined[q] = 0;
    atomicAdd(undetermined, 1);
    return;
  }
  for (int c = 0; c < kk; ++c) {   // L y = P
    const int rc = c * (c + 1) / 2;
    double s = b[c * n];
    for (int k = 0; k < c; ++k) s = s - h[(rc + k) * n] * b[k * n];
    b[c * n] = s;
  }
  for (int c = 0; c < kk; ++c) b[c * n] = b[c * n] / h[(c * (c + 1) / 2 + c) * n];   // D z = y
  for (int c = kk - 1; c >= 0; --c) {   // L^T x = z
    double s = b[c * n];
    for (int k = c + 1; k < kk; ++k) s = s - h[(k * (k + 1) / 2 + c) * n] * b[k * n];
    b[c * n] = s;
  }
  determined[q] = 1;
}

inline int32_t words_of(int32_t n) { return (n + 15) / 16; }

}  // namespace

hipError_t launch_grm_lsq_products(const double* t, int64_t tstride, const double* d, const int32_t* used, int64_t rows, int32_t e0,
                                   int32_t j, double* p, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(grm_lsq_products_kernel, dim3((unsigned)((rows + 255) / 256), (unsigned)j), dim3(256), 0, stream, t, tstride, d,
                     used, rows, e0, p);
  return hipGetLastError();
}

hipError_t launch_grm_lsq_pairs(const uint32_t* seg, int32_t rows, int32_t n, const double* p, int64_t pstride, int32_t j, double* hpart,
                                int64_t cstride, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if (j != 1 && j != 2 && j != 4) return hipErrorInvalidValue;
  const int32_t pitch = grm_pitch_words(n);
  const dim3 grid((unsigned)((rows + kGrmRangeRows - 1) / kGrmRangeRows), (unsigned)grm_groups(n));
  if (j == 4)
    hipLaunchKernelGGL(grm_lsq_pairs_kernel<4>, grid, dim3(256), 0, stream, seg, rows, pitch, words_of(n), p, pstride, hpart,
                       (int64_t)pitch * 16, cstride);
  else if (j == 2)
    hipLaunchKernelGGL(grm_lsq_pairs_kernel<2>, grid, dim3(256), 0, stream, seg, rows, pitch, words_of(n), p, pstride, hpart,
                       (int64_t)pitch * 16, cstride);
  else
    hipLaunchKernelGGL(grm_lsq_pairs_kernel<1>, grid, dim3(256), 0, stream, seg, rows, pitch, words_of(n), p, pstride, hpart,
                       (int64_t)pitch * 16, cstride);
  return hipGetLastError();
}

hipError_t launch_grm_lsq_finish(const double* part, int32_t nranges, int64_t cstride, int32_t n, int32_t k, double* out,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(grm_lsq_finish_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)k), dim3(256), 0, stream, part,
                     (int64_t)grm_pitch_words(n) * 16, nranges, cstride, n, out);
  return hipGetLastError();
}

hipError_t launch_grm_lsq_solve(double* a, int32_t nq, int32_t num_pc, int32_t* determined, int32_t* undetermined, hipStream_t stream) {
  hipLaunchKernelGGL(grm_lsq_solve_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, a, nq, num_pc, determined,
                     undetermined);
  return hipGetLastError();
}

}  // namespace pcoa
