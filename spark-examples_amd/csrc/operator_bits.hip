// operator_bits.hip -- the implicit similarity operator: y = S v = X^T (X v) straight from the carrier bitsets, S never formed
// (DESIGN.md 4.8).  X is the V x N bit matrix of the store (capi_operator.hip): segments of rows at a fixed pitch of
// operator_pitch_words(N) words, sample i = bit (i & 31) of word i >> 5, bits of samples >= N and words beyond ceil(N / 32)
// zero, so no pass masks.  Every kernel below gives each lane ONE word column of the store:
//   pass 1  t = X v      the lane keeps its 32 entries of v in registers, rows stream through as coalesced word loads, a block
//                        of 32 rows is reduced across the lanes by a halving butterfly (one cross-lane move per row), the four
//                        waves of a workgroup (four chunks of 2,048 samples) are combined through LDS in wave order, and the
//                        groups of 8,192 samples by operator_combine_t in group order;
//   pass 2  y = X^T t    the lane keeps 32 accumulators, t_v is wave-uniform; a wave takes a RANGE of kOperatorRangeRows rows of
//                        a segment, and the ranges' partial vectors are added in (segment, range) order by operator_finish, which
//                        also applies the centring terms;
//   the integer twins    popcount per row (int32), then pass 2 with int64 accumulators: rowSums = X^T (X 1), exact.
// Determinism: which additions happen, and in which order, is fixed by N, the segment size and the row's index in the store --
// never by the grid, the CU count or the sizes of the accumulate calls.  No floating-point atomics anywhere.
#include <algorithm>

#include "pcoa_internal.h"

namespace pcoa {

int32_t operator_pitch_words(int32_t n) { return ((n + 31) / 32 + 3) / 4 * 4; }   // rows start 16-byte aligned
int32_t operator_groups(int32_t n) { return ((n + 31) / 32 + kOperatorGroupWords - 1) / kOperatorGroupWords; }

namespace {

constexpr int kRowsPerBlock1 = 512;   // rows a pass-1 workgroup streams past its v registers (16 butterfly blocks)

// Repitch rows [nv][ld] -> [nv][pitch]: words beyond `words` zero, bits of samples >= n cleared.
__global__ __launch_bounds__(256) void operator_append_kernel(const uint32_t* __restrict__ src, int64_t ld, int64_t nv, int32_t n,
                                                              int32_t words, int32_t pitch, uint32_t* __restrict__ dst) {
  const int64_t total = nv * pitch;
  const uint32_t tail = (n & 31) ? ((1u << (n & 31)) - 1u) : 0xffffffffu;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / pitch;
    const int32_t c = (int32_t)(i - r * pitch);
    uint32_t w = 0;
    if (c < words) {
      w = src[r * ld + c];
      if (c == words - 1) w &= tail;
    }
    dst[i] = w;
  }
}

// p[j] = this lane's partial of row j -> the total of row (lane & 31) over all 64 lanes, in a fixed tree: at distance h a lane
// keeps the half of the rows whose bit h equals its own and receives the partner's partials of them
template <int H>
__device__ __forceinline__ void halve_rows(double (&p)[32], int lane) {
  const bool up = (lane & H) != 0;
#pragma unroll
  for (int j = 0; j < H; ++j) {
    const double keep = up ? p[j + H] : p[j];
    const double send = up ? p[j] : p[j + H];
    p[j] = keep + __shfl_xor(send, H, 64);
  }
}
__device__ __forceinline__ double reduce_rows32(double (&p)[32], int lane) {
  halve_rows<16>(p, lane);
  halve_rows<8>(p, lane);
  halve_rows<4>(p, lane);
  halve_rows<2>(p, lane);
  halve_rows<1>(p, lane);
  return p[0] + __shfl_xor(p[0], 32, 64);
}

// pass 1: tpart[group][row] = sum over the group's 8,192 samples of bit(row, i) v[i]
__global__ __launch_bounds__(256, 2) void operator_xv_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch, int32_t words,
                                                          const double* __restrict__ v, int32_t n, double* __restrict__ tpart,
                                                          int64_t vstride) {
  __shared__ double red[4][32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (blockIdx.y * 4 + wave) * 64 + lane;
  const bool live = col < words;
  const int colc = live ? col : words - 1;   // loads of a dead lane go to a valid address and are discarded
  double vv[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const int i = colc * 32 + k;
    const double x = v[i < n ? i : n - 1];
    vv[k] = (live && i < n) ? x : 0.0;
  }
  const int r0 = blockIdx.x * kRowsPerBlock1;
  const int r1 = min(rows, r0 + kRowsPerBlock1);
  double* out = tpart + (int64_t)blockIdx.y * vstride;
  for (int rb = r0; rb < r1; rb += 32) {
    uint32_t w[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const int r = min(rb + j, r1 - 1);
      const uint32_t x = seg[(int64_t)r * pitch + colc];
      w[j] = (live && rb + j < r1) ? x : 0u;
    }
    double p[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < 32; ++k) a += ((w[j] >> k) & 1u) ? vv[k] : 0.0;
      p[j] = a;
    }
    const double tot = reduce_rows32(p, lane);
    if (lane < 32) red[wave][lane] = tot;
    __syncthreads();
    if (wave == 0 && lane < 32 && rb + lane < r1) out[rb + lane] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void operator_combine_t_kernel(const double* __restrict__ tpart, int64_t vstride, int32_t groups,
                                                                 int64_t rows, double* __restrict__ t) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  double s = tpart[r];
  for (int32_t g = 1; g < groups; ++g) s += tpart[(int64_t)g * vstride + r];
  t[r] = s;
}

// pass 2 (T = double) and the column sums of the row sums (T = int64_t, t = the rows' popcounts): the partial vector of one
// range of rows, ypart[range][pitch * 32]
template <typename T, typename TV>
__global__ __launch_bounds__(256, 2) void operator_xt_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch, int32_t words,
                                                          const TV* __restrict__ t, T* __restrict__ ypart, int64_t ystride) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (blockIdx.y * 4 + wave) * 64 + lane;
  if (col >= words) return;
  const int r0 = blockIdx.x * kOperatorRangeRows;
  const int r1 = min(rows, r0 + kOperatorRangeRows);
  T acc[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) acc[k] = T(0);
  for (int rb = r0; rb < r1; rb += 8) {
    uint32_t w[8];
    T tv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = min(rb + u, r1 - 1);
      const uint32_t x = seg[(int64_t)r * pitch + col];
      w[u] = rb + u < r1 ? x : 0u;
      tv[u] = (T)t[r];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
#pragma unroll
      for (int k = 0; k < 32; ++k) acc[k] += ((w[u] >> k) & 1u) ? tv[u] : T(0);
    }
  }
  T* out = ypart + (int64_t)blockIdx.x * ystride + (int64_t)col * 32;
#pragma unroll
  for (int k = 0; k < 32; ++k) out[k] = acc[k];
}

// popcount of every row (one wave per row at a time; integer sums, any order)
__global__ __launch_bounds__(256) void operator_popcount_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch,
                                                                int32_t words, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {
    int32_t a = 0;
    for (int c = lane; c < words; c += 64) a += __popc(seg[(int64_t)r * pitch + c]);
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) a += __shfl_xor(a, h, 64);
    if (lane == 0) cnt[r] = a;
  }
}

// out[0] = 1^T v, out[1] = m^T v: one workgroup, thread t sums the entries t, t + 256, .. in order, then a fixed tree
__global__ __launch_bounds__(256) void operator_dots_kernel(const double* __restrict__ v, const double* __restrict__ means, int32_t n,
                                                            double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double a[256], b[256];
  double sv = 0.0, mv = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    sv += v[i];
    mv += means[i] * v[i];
  }
  a[threadIdx.x] = sv;
  b[threadIdx.x] = mv;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
      a[threadIdx.x] += a[threadIdx.x + h];
      b[threadIdx.x] += b[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = a[0];
    out[1] = b[0];
  }
}

// y[i] = sum of the ranges' partials in order; centred: ((y[i] - m[i] (1^T v)) - m^T v) + mm (1^T v)
__global__ __launch_bounds__(256) void operator_finish_kernel(const double* __restrict__ ypart, int64_t ystride, int32_t nranges,
                                                              int32_t n, const double* __restrict__ means,
                                                              const double* __restrict__ stats, const double* __restrict__ dots,
                                                              int centred, double* __restrict__ y) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int32_t g = 0; g < nranges; ++g) s += ypart[(int64_t)g * ystride + i];
  if (centred) {
    const double sv = dots[0], mv = dots[1], mm = stats[1];
    s = s - means[i] * sv;
    s = s - mv;
    s = s + mm * sv;
  }
  y[i] = s;
}

__global__ __launch_bounds__(256) void operator_row_sums_finish_kernel(const int64_t* __restrict__ ipart, int64_t ystride,
                                                                       int32_t nranges, int32_t n, int64_t* __restrict__ rs_i64,
                                                                       double* __restrict__ rs_f64) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int64_t s = 0;
  for (int32_t g = 0; g < nranges; ++g) s += ipart[(int64_t)g * ystride + i];
  rs_i64[i] = s;
  rs_f64[i] = (double)s;
}

inline int32_t words_of(int32_t n) { return (n + 31) / 32; }

}  // namespace

hipError_t launch_operator_append(const uint32_t* src, int64_t ld_words, int64_t nv, int32_t n, uint32_t* dst, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  const int32_t pitch = operator_pitch_words(n);
  const int64_t blocks = std::min<int64_t>((nv * pitch + 255) / 256, 65536);
  hipLaunchKernelGGL(operator_append_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, ld_words, nv, n, words_of(n), pitch,
                     dst);
  return hipGetLastError();
}

hipError_t launch_operator_xv(const uint32_t* seg, int32_t rows, int32_t n, const double* v, double* tpart, int64_t vstride,
                              hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  const dim3 grid((unsigned)((rows + kRowsPerBlock1 - 1) / kRowsPerBlock1), (unsigned)operator_groups(n));
  hipLaunchKernelGGL(operator_xv_kernel, grid, dim3(256), 0, stream, seg, rows, operator_pitch_words(n), words_of(n), v, n, tpart,
                     vstride);
  return hipGetLastError();
}

hipError_t launch_operator_combine_t(const double* tpart, int64_t vstride, int32_t n, int64_t rows, double* t, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(operator_combine_t_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, tpart, vstride,
                     operator_groups(n), rows, t);
  return hipGetLastError();
}

hipError_t launch_operator_xt_f64(const uint32_t* seg, int32_t rows, int32_t n, const double* t, double* ypart, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  const int32_t pitch = operator_pitch_words(n);
  const dim3 grid((unsigned)((rows + kOperatorRangeRows - 1) / kOperatorRangeRows), (unsigned)operator_groups(n));
  hipLaunchKernelGGL((operator_xt_kernel<double, double>), grid, dim3(256), 0, stream, seg, rows, pitch, words_of(n), t, ypart,
                     (int64_t)pitch * 32);
  return hipGetLastError();
}

hipError_t launch_operator_xt_i64(const uint32_t* seg, int32_t rows, int32_t n, const int32_t* cnt, int64_t* ipart,
                                  hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  const int32_t pitch = operator_pitch_words(n);
  const dim3 grid((unsigned)((rows + kOperatorRangeRows - 1) / kOperatorRangeRows), (unsigned)operator_groups(n));
  hipLaunchKernelGGL((operator_xt_kernel<int64_t, int32_t>), grid, dim3(256), 0, stream, seg, rows, pitch, words_of(n), cnt, ipart,
                     (int64_t)pitch * 32);
  return hipGetLastError();
}

hipError_t launch_operator_popcount(const uint32_t* seg, int32_t rows, int32_t n, int32_t* cnt, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  const int blocks = std::min((rows + 3) / 4, 16384);
  hipLaunchKernelGGL(operator_popcount_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, seg, rows, operator_pitch_words(n),
                     words_of(n), cnt);
  return hipGetLastError();
}

hipError_t launch_operator_dots(const double* v, const double* means, int32_t n, double* dots, hipStream_t stream) {
  hipLaunchKernelGGL(operator_dots_kernel, dim3(1), dim3(256), 0, stream, v, means, n, dots);
  return hipGetLastError();
}

hipError_t launch_operator_finish(const double* ypart, int32_t nranges, int32_t n, const double* means, const double* stats,
                                  const double* dots, int centred, double* y, hipStream_t stream) {
  hipLaunchKernelGGL(operator_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ypart,
                     (int64_t)operator_pitch_words(n) * 32, nranges, n, means, stats, dots, centred, y);
  return hipGetLastError();
}

hipError_t launch_operator_row_sums_finish(const int64_t* ipart, int32_t nranges, int32_t n, int64_t* rs_i64, double* rs_f64,
                                           hipStream_t stream) {
  hipLaunchKernelGGL(operator_row_sums_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ipart,
                     (int64_t)operator_pitch_words(n) * 32, nranges, n, rs_i64, rs_f64);
  return hipGetLastError();
}

}  // namespace pcoa
