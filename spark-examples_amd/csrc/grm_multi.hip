// grm_multi.hip -- the two passes of the standardised-genotype operator (grm_bits.hip) for K vectors at once: what SNP weights and
// the projection of new samples onto the axes of K need.  With K u_c = lambda_c u_c:
//   pass 1 over the PANEL's rows   t_vc = d_v sum_i (g_iv - mu_v c_iv) u_c[i]           (grm_ax_multi_kernel, then grm_combine_t)
//   pass 2 over the STUDY's rows   coord(q, c) = (sum_v g_vq t_vc + sum_v c_vq s_vc) / M' / lambda_c,  s_vc = -(mu_v t_vc)
// A word's three slot masks are formed once and every v_bfe_i32 of them is spent on K vectors (the 1 + 3K idiom of loadings.hip).
// Every column is added in exactly the order grm_bits.hip fixes for one vector -- the lane's 16 genotypes in order, a - mu b per
// lane, the tree over the 64 lanes at distances 16, 8, 4, 2, 1, 32, the four waves in wave order, the groups in group order; the
// rows of a range in order, the ranges in (segment, range) order -- so column c of any chunk has the bits of a one-vector run.
// The tree over the lanes is the one of grm_bits.hip's 32-row butterfly run on blocks of 16 rows: its first level is a full
// exchange (both lanes of a pair compute the same sum; IEEE addition commutes), so 16 K partials per lane are live where the
// one-vector kernel holds 32: K = 2 fits 256 VGPRs with no scratch at the price of 2 shuffles per row and vector, not 1.
// K is 1 or 2.  No floating-point atomics anywhere.
#include <algorithm>

#include "grm_slots.h"
#include "pcoa_internal.h"

namespace pcoa {

int grm_multi_chunk(int32_t remaining) { return remaining >= 2 ? 2 : 1; }

namespace {

constexpr int kRowsPerBlockM = 512;   // rows a pass-1 workgroup streams past its x registers (32 butterfly blocks of 16)

// p[j][c] = this lane's partial of row j, vector c -> the total of row (lane & 15) over all 64 lanes in p[0][c], by the tree of
// grm_bits.hip's reduce_rows32: level 1 pairs lanes l and l ^ 16 (here: both keep the sum), levels 2..5 halve the rows a lane
// keeps at distances 8, 4, 2, 1, level 6 pairs l and l ^ 32
template <int K, int H>
__device__ __forceinline__ void halve_rows_multi(double (&p)[16][K], int lane) {
  const bool up = (lane & H) != 0;
#pragma unroll
  for (int j = 0; j < H; ++j) {
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const double keep = up ? p[j + H][c] : p[j][c];
      const double send = up ? p[j][c] : p[j + H][c];
      p[j][c] = keep + __shfl_xor(send, H, 64);
    }
  }
}
template <int K>
__device__ __forceinline__ void reduce_rows16(double (&p)[16][K], int lane) {
#pragma unroll
  for (int j = 0; j < 16; ++j) {
#pragma unroll
    for (int c = 0; c < K; ++c) p[j][c] = p[j][c] + __shfl_xor(p[j][c], 16, 64);
  }
  halve_rows_multi<K, 8>(p, lane);
  halve_rows_multi<K, 4>(p, lane);
  halve_rows_multi<K, 2>(p, lane);
  halve_rows_multi<K, 1>(p, lane);
#pragma unroll
  for (int c = 0; c < K; ++c) p[0][c] = p[0][c] + __shfl_xor(p[0][c], 32, 64);
}

// pass 1 for K vectors: tpart[c][group][row] = sum over the group's 4,096 samples of (g(row, i) - mu[row] c(row, i)) x_c[i]
template <int K>
__global__ __launch_bounds__(256, 2) void grm_ax_multi_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch,
                                                              int32_t words, const double* __restrict__ mu,
                                                              const double* __restrict__ x, int64_t xstride, int32_t n,
                                                              double* __restrict__ tpart, int64_t vstride, int64_t cstride) {
#pragma clang fp contract(off)
  __shared__ double red[4][K][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (blockIdx.y * 4 + wave) * 64 + lane;
  const bool live = col < words;
  const int colc = live ? col : words - 1;   // loads of a dead lane go to a valid address and are discarded
  double xx[K][16];
#pragma unroll
  for (int c = 0; c < K; ++c) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int i = colc * 16 + k;
      const double v = x[(int64_t)c * xstride + (i < n ? i : n - 1)];
      xx[c][k] = (live && i < n) ? v : 0.0;
    }
  }
  const int r0 = blockIdx.x * kRowsPerBlockM;
  const int r1 = min(rows, r0 + kRowsPerBlockM);
  double* out = tpart + (int64_t)blockIdx.y * vstride;
  for (int rb = r0; rb < r1; rb += 16) {
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int r = min(rb + j, r1 - 1);
      const uint32_t v = seg[(int64_t)r * pitch + colc];
      w[j] = (live && rb + j < r1) ? v : kLo;   // a dead lane or row: nobody called, nothing added
    }
    double p[16][K];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      uint32_t hi, both, called;
      slot_masks(w[j], hi, both, called);
      double a[K], b[K];
#pragma unroll
      for (int c = 0; c < K; ++c) a[c] = b[c] = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int mh = __builtin_amdgcn_sbfe((int)hi, 2u * k, 1u);
        const int mb = __builtin_amdgcn_sbfe((int)both, 2u * k, 1u);
        const int mc = __builtin_amdgcn_sbfe((int)called, 2u * k, 1u);
#pragma unroll
        for (int c = 0; c < K; ++c) {
          a[c] += and_mask(xx[c][k], mh);
          a[c] += and_mask(xx[c][k], mb);
          b[c] += and_mask(xx[c][k], mc);
        }
      }
      const double m = mu[min(rb + j, r1 - 1)];
#pragma unroll
      for (int c = 0; c < K; ++c) p[j][c] = a[c] - m * b[c];
    }
    reduce_rows16<K>(p, lane);
    if (lane < 16) {
#pragma unroll
      for (int c = 0; c < K; ++c) red[wave][c][lane] = p[0][c];
    }
    __syncthreads();
    if (wave == 0 && lane < 16 && rb + lane < r1) {
#pragma unroll
      for (int c = 0; c < K; ++c)
        out[(int64_t)c * cstride + rb + lane] = ((red[0][c][lane] + red[1][c][lane]) + red[2][c][lane]) + red[3][c][lane];
    }
    __syncthreads();
  }
}

// pass 2 for K vector pairs: ypart[c][range][pitch * 16] = sum_r g(r, i) t_c[r] + c(r, i) s_c[r]
template <int K>
__global__ __launch_bounds__(256, 2) void grm_at_multi_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch,
                                                              int32_t words, const double* __restrict__ t,
                                                              const double* __restrict__ s, int64_t tstride,
                                                              double* __restrict__ ypart, int64_t ystride, int64_t cstride) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (blockIdx.y * 4 + wave) * 64 + lane;
  if (col >= words) return;
  const int r0 = blockIdx.x * kGrmRangeRows;
  const int r1 = min(rows, r0 + kGrmRangeRows);
  double acc[K][16];
#pragma unroll
  for (int c = 0; c < K; ++c) {
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[c][k] = 0.0;
  }
  for (int rb = r0; rb < r1; rb += 8) {
    uint32_t w[8];
    double tv[8][K], sv[8][K];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = min(rb + u, r1 - 1);
      const uint32_t v = seg[(int64_t)r * pitch + col];
      w[u] = rb + u < r1 ? v : kLo;
#pragma unroll
      for (int c = 0; c < K; ++c) {
        tv[u][c] = t[(int64_t)c * tstride + r];
        sv[u][c] = s[(int64_t)c * tstride + r];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      uint32_t hi, both, called;
      slot_masks(w[u], hi, both, called);
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int mh = __builtin_amdgcn_sbfe((int)hi, 2u * k, 1u);
        const int mb = __builtin_amdgcn_sbfe((int)both, 2u * k, 1u);
        const int mc = __builtin_amdgcn_sbfe((int)called, 2u * k, 1u);
#pragma unroll
        for (int c = 0; c < K; ++c) {
          acc[c][k] += and_mask(tv[u][c], mh);
          acc[c][k] += and_mask(tv[u][c], mb);
          acc[c][k] += and_mask(sv[u][c], mc);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < K; ++c) {
    double* out = ypart + (int64_t)c * cstride + (int64_t)blockIdx.x * ystride + (int64_t)col * 16;
#pragma unroll
    for (int k = 0; k < 16; ++k) out[k] = acc[c][k];
  }
}

// out[c][i] = (the ranges' partials of column c added in order) / M' / lam[c]; the caller has refused M' = 0
__global__ __launch_bounds__(256) void grm_project_finish_kernel(const double* __restrict__ ypart, int64_t ystride, int32_t nranges,
                                                                 int64_t cstride, int32_t n,
                                                                 const unsigned long long* __restrict__ mprime,
                                                                 const double* __restrict__ lam, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (i >= n) return;
  const double* part = ypart + (int64_t)c * cstride;
  double a = 0.0;
  for (int32_t g = 0; g < nranges; ++g) a += part[(int64_t)g * ystride + i];
  a = a / (double)*mprime;
  out[(int64_t)c * n + i] = a / lam[c];
}

// called[i] = the ranges' integer partials added (any order)
__global__ __launch_bounds__(256) void grm_called_sum_kernel(const int32_t* __restrict__ ipart, int64_t ystride, int32_t nranges,
                                                             int32_t n, int32_t* __restrict__ called) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int32_t a = 0;
  for (int32_t g = 0; g < nranges; ++g) a += ipart[(int64_t)g * ystride + i];
  called[i] = a;
}

// the window [first, first + nv) of t as [nv][num_pc]; scaled: the unit weights, in the header's expression (no contraction:
// numpy evaluates the same one)
__global__ __launch_bounds__(256) void grm_weights_out_kernel(const double* __restrict__ t, int64_t tstride,
                                                              const double* __restrict__ d, const int32_t* __restrict__ used,
                                                              const unsigned long long* __restrict__ mprime,
                                                              const double* __restrict__ lam, int scaled, int64_t first, int64_t nv,
                                                              int32_t num_pc, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t total = nv * num_pc;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t v = i / num_pc;
    const int32_t c = (int32_t)(i - v * num_pc);
    const int64_t r = first + v;
    const double tv = t[(int64_t)c * tstride + r];
    double o = tv;
    if (scaled) o = used[r] ? tv / sqrt(d[r] * ((double)*mprime * lam[c])) : 0.0;
    out[i] = o;
  }
}

inline int32_t words_of(int32_t n) { return (n + 15) / 16; }

}  // namespace

hipError_t launch_grm_ax_multi(const uint32_t* seg, int32_t rows, int32_t n, const double* mu, const double* x, int64_t xstride, int32_t k,
                               double* tpart, int64_t vstride, int64_t cstride, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if (k != 1 && k != 2) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((rows + kRowsPerBlockM - 1) / kRowsPerBlockM), (unsigned)grm_groups(n));
  const int32_t pitch = grm_pitch_words(n);
  if (k == 2)
    hipLaunchKernelGGL(grm_ax_multi_kernel<2>, grid, dim3(256), 0, stream, seg, rows, pitch, words_of(n), mu, x, xstride, n, tpart,
                       vstride, cstride);
  else
    hipLaunchKernelGGL(grm_ax_multi_kernel<1>, grid, dim3(256), 0, stream, seg, rows, pitch, words_of(n), mu, x, xstride, n, tpart,
                       vstride, cstride);
  return hipGetLastError();
}

hipError_t launch_grm_at_multi(const uint32_t* seg, int32_t rows, int32_t n, const double* t, const double* s, int64_t tstride, int32_t k,
                               double* ypart, int64_t cstride, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if (k != 1 && k != 2) return hipErrorInvalidValue;
  const int32_t pitch = grm_pitch_words(n);
  const dim3 grid((unsigned)((rows + kGrmRangeRows - 1) / kGrmRangeRows), (unsigned)grm_groups(n));
  if (k == 2)
    hipLaunchKernelGGL(grm_at_multi_kernel<2>, grid, dim3(256), 0, stream, seg, rows, pitch, words_of(n), t, s, tstride, ypart,
                       (int64_t)pitch * 16, cstride);
  else
    hipLaunchKernelGGL(grm_at_multi_kernel<1>, grid, dim3(256), 0, stream, seg, rows, pitch, words_of(n), t, s, tstride, ypart,
                       (int64_t)pitch * 16, cstride);
  return hipGetLastError();
}

hipError_t launch_grm_project_finish(const double* ypart, int32_t nranges, int64_t cstride, int32_t n, int32_t k,
                                     const unsigned long long* mprime, const double* lam, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(grm_project_finish_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)k), dim3(256), 0, stream, ypart,
                     (int64_t)grm_pitch_words(n) * 16, nranges, cstride, n, mprime, lam, out);
  return hipGetLastError();
}

hipError_t launch_grm_called_sum(const int32_t* ipart, int32_t nranges, int32_t n, int32_t* called, hipStream_t stream) {
  hipLaunchKernelGGL(grm_called_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ipart,
                     (int64_t)grm_pitch_words(n) * 16, nranges, n, called);
  return hipGetLastError();
}

hipError_t launch_grm_weights_out(const double* t, int64_t tstride, const double* d, const int32_t* used,
                                  const unsigned long long* mprime, const double* lam, int scaled, int64_t first, int64_t nv,
                                  int32_t num_pc, double* out, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>((nv * num_pc + 255) / 256, 65536);
  hipLaunchKernelGGL(grm_weights_out_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, t, tstride, d, used, mprime, lam, scaled,
                     first, nv, num_pc, out);
  return hipGetLastError();
}

}  // namespace pcoa
