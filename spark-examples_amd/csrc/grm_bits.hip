// grm_bits.hip -- the standardised-genotype operator: y = K x with K = A^T diag(d) A / M' straight from 2-bit genotype rows, K
// never formed.  A(v, i) = g_iv - mu_v c_iv: g the dosage of the non-reference allele (0 where the sample is
// not called), c the called indicator, mu_v = a_v / n_v, d_v = 1 / (mu_v (1 - mu_v / 2)) for a used variant and 0 otherwise,
// M' the number of used variants.  The store (capi_grm.hip) holds segments of rows at a fixed pitch of grm_pitch_words(N)
// words of 16 genotypes: sample i = bits 2 (i & 15) and 2 (i & 15) + 1 of word i >> 4, in ONE coding whatever ref_is_a1 was:
//   00 g = 0   01 not called   10 g = 1   11 g = 2
// and every slot at index >= N (the pitch's padding words included) holds 01, so no pass masks.  With lo / hi the two bits of
// a slot: g = hi + (hi & lo), c = hi | ~lo.  The shape is operator_bits.hip's -- every lane owns ONE word column:
//   counts  n_v, h_v, o_v per row by popcounts of the three slot masks (int32), then grm_weights: mu, d, used, M'
//   pass 1  t_v = d_v sum_i (g_iv - mu_v c_iv) x_i: the lane keeps its 16 entries of x in registers, rows stream through as
//           coalesced word loads, a genotype costs three masked adds (hi, hi & lo into the g sum, hi | ~lo into the c sum), the
//           lane's two sums are combined with the row's mu, a block of 32 rows is reduced across the lanes by a halving
//           butterfly, the four waves of a workgroup (four chunks of 1,024 samples) through LDS in wave order, the groups of
//           4,096 samples by grm_combine_t in group order, which applies d_v once and also writes s_v = -(mu_v t_v)
//   pass 2  y_i = (sum_v g_iv t_v + sum_v c_iv s_v) / M': the lane keeps 16 accumulators, t_v and s_v are wave-uniform; a wave
//           takes a RANGE of kGrmRangeRows rows of a segment, and the ranges' partial vectors are added in (segment, range)
//           order by grm_finish, which divides by M'
//   the integer twin of pass 2: the c mask alone with used_v as the vector, int32: the variants at which a sample is called
// Determinism: which additions happen, and in which order, is fixed by N, the segment size and the row's index in the store --
// never by the grid, the CU count or the sizes of the accumulate calls.  No floating-point atomics anywhere (M' is an integer
// count).  The masks are spent as AND masks from a sign-extended bit-field extract, the idiom of loadings.hip.
#include <algorithm>

#include "grm_slots.h"
#include "pcoa_internal.h"

namespace pcoa {

int32_t grm_pitch_words(int32_t n) { return ((n + 15) / 16 + 3) / 4 * 4; }   // ceil(N / 4) bytes rounded up to 16
int32_t grm_groups(int32_t n) { return ((n + 15) / 16 + kGrmGroupWords - 1) / kGrmGroupWords; }

namespace {

constexpr int kRowsPerBlock1 = 512;          // rows a pass-1 workgroup streams past its x registers (16 butterfly blocks)
// (kLo, and_mask and slot_masks: grm_slots.h, shared with grm_multi.hip)

// Repitch raw .bed rows [nv][row_bytes] -> [nv][pitch] words.  Bytes beyond ceil(n / 4) and slots of samples >= n become 01;
// swap (the non-reference allele is A1, ref_is_a1 = 0): 00 <-> 11, so that 11 is the homozygous non-reference code
__global__ __launch_bounds__(256) void grm_append_kernel(const uint8_t* __restrict__ src, int64_t row_bytes, int64_t nv, int32_t n,
                                                         int32_t pitch, int swap, uint32_t* __restrict__ dst) {
  const int64_t total = nv * pitch;
  const int32_t nbytes = (n + 3) / 4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / pitch;
    const int32_t c = (int32_t)(i - r * pitch);
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int32_t b = c * 4 + k;
      const uint32_t x = b < nbytes ? (uint32_t)src[r * row_bytes + b] : 0x55u;
      w |= x << (8 * k);
    }
    const int32_t live = n - c * 16;   // slots of this word that belong to samples
    if (live < 16) {
      const uint32_t keep = live > 0 ? (1u << (2 * live)) - 1u : 0u;
      w = (w & keep) | (kLo & ~keep);
    }
    if (swap) {
      const uint32_t eq = ~(w ^ (w >> 1)) & kLo;   // slots whose two bits agree: 00 and 11
      w ^= eq | (eq << 1);
    }
    dst[i] = w;
  }
}

// cnt[r] = {called, het, hom non-reference} of every row (one wave per row at a time; integer sums, any order)
__global__ __launch_bounds__(256) void grm_counts_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch,
                                                         int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {
    int32_t nc = 0, nh = 0, no = 0;
    for (int c = lane; c < pitch; c += 64) {
      uint32_t hi, both, called;
      slot_masks(seg[(int64_t)r * pitch + c], hi, both, called);
      nc += __popc(called);
      nh += __popc(hi & ~both);
      no += __popc(both);
    }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
      nc += __shfl_xor(nc, h, 64);
      nh += __shfl_xor(nh, h, 64);
      no += __shfl_xor(no, h, 64);
    }
    if (lane == 0) {
      cnt[(int64_t)r * 3 + 0] = nc;
      cnt[(int64_t)r * 3 + 1] = nh;
      cnt[(int64_t)r * 3 + 2] = no;
    }
  }
}

// mu, d, used of every variant from its counts, in the expressions of the definition (no contraction: numpy evaluates the same
// ones); *mprime += the used variants of this launch (an integer count).  keep (may be NULL): the LD keep mask of the store
// (pcoa_grm_ld_prune) -- a removed row is not used: d = 0, mu as it was.  The variant filters:
// a row whose missing share of the n samples exceeds max_missing is not used, nor one whose HWE p-value (hwe_p, may be NULL:
// grm_qc.hip) lies below hwe_min_p; max_missing = 1 and hwe_min_p = 0 leave used as it was without them
__global__ __launch_bounds__(256) void grm_weights_kernel(const int32_t* __restrict__ cnt, int64_t rows, double min_maf,
                                                          const uint8_t* __restrict__ keep, int32_t n, double max_missing,
                                                          double hwe_min_p, const double* __restrict__ hwe_p,
                                                          double* __restrict__ mu, double* __restrict__ d,
                                                          int32_t* __restrict__ used, unsigned long long* __restrict__ mprime) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int u = 0;
  if (r < rows) {
    const int32_t nv = cnt[r * 3], a = cnt[r * 3 + 1] + 2 * cnt[r * 3 + 2];
    double m = 0.0, w = 0.0;
    if (nv > 0) {
      m = (double)a / (double)nv;
      u = (a > 0 && a < 2 * nv && (double)min(a, 2 * nv - a) >= min_maf * (2.0 * (double)nv)) ? 1 : 0;
      if (!((double)(n - nv) <= max_missing * (double)n)) u = 0;
      if (hwe_p && hwe_min_p != 0.0 && !(hwe_p[r] >= hwe_min_p)) u = 0;
      if (keep && !keep[r]) u = 0;
      if (u) w = 1.0 / (m * (1.0 - 0.5 * m));
    }
    mu[r] = m;
    d[r] = w;
    used[r] = u;
  }
  const unsigned long long b = __ballot(u);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(mprime, (unsigned long long)__popcll(b));
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

// pass 1: tpart[group][row] = sum over the group's 4,096 samples of (g(row, i) - mu[row] c(row, i)) x[i]
__global__ __launch_bounds__(256, 2) void grm_ax_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch, int32_t words,
                                                     const double* __restrict__ mu, const double* __restrict__ x, int32_t n,
                                                     double* __restrict__ tpart, int64_t vstride) {
#pragma clang fp contract(off)
  __shared__ double red[4][32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (blockIdx.y * 4 + wave) * 64 + lane;
  const bool live = col < words;
  const int colc = live ? col : words - 1;   // loads of a dead lane go to a valid address and are discarded
  double xx[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int i = colc * 16 + k;
    const double v = x[i < n ? i : n - 1];
    xx[k] = (live && i < n) ? v : 0.0;
  }
  const int r0 = blockIdx.x * kRowsPerBlock1;
  const int r1 = min(rows, r0 + kRowsPerBlock1);
  double* out = tpart + (int64_t)blockIdx.y * vstride;
  for (int rb = r0; rb < r1; rb += 32) {
    uint32_t w[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const int r = min(rb + j, r1 - 1);
      const uint32_t v = seg[(int64_t)r * pitch + colc];
      w[j] = (live && rb + j < r1) ? v : kLo;   // a dead lane or row: nobody called, nothing added
    }
    double p[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      uint32_t hi, both, called;
      slot_masks(w[j], hi, both, called);
      double a = 0.0, b = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        a += and_mask(xx[k], __builtin_amdgcn_sbfe((int)hi, 2u * k, 1u));
        a += and_mask(xx[k], __builtin_amdgcn_sbfe((int)both, 2u * k, 1u));
        b += and_mask(xx[k], __builtin_amdgcn_sbfe((int)called, 2u * k, 1u));
      }
      p[j] = a - mu[min(rb + j, r1 - 1)] * b;
    }
    const double tot = reduce_rows32(p, lane);
    if (lane < 32) red[wave][lane] = tot;
    __syncthreads();
    if (wave == 0 && lane < 32 && rb + lane < r1) out[rb + lane] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    __syncthreads();
  }
}

// t[r] = d[r] (the groups' partials added in order), s[r] = -(mu[r] t[r])
__global__ __launch_bounds__(256) void grm_combine_t_kernel(const double* __restrict__ tpart, int64_t vstride, int32_t groups,
                                                            int64_t rows, const double* __restrict__ mu,
                                                            const double* __restrict__ d, double* __restrict__ t,
                                                            double* __restrict__ s) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  double a = tpart[r];
  for (int32_t g = 1; g < groups; ++g) a += tpart[(int64_t)g * vstride + r];
  a = d[r] * a;
  t[r] = a;
  s[r] = -(mu[r] * a);
}

// pass 2: the partial vector of one range of rows, ypart[range][pitch * 16] = sum_r g(r, i) t[r] + c(r, i) s[r]
__global__ __launch_bounds__(256, 2) void grm_at_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch, int32_t words,
                                                     const double* __restrict__ t, const double* __restrict__ s,
                                                     double* __restrict__ ypart, int64_t ystride) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (blockIdx.y * 4 + wave) * 64 + lane;
  if (col >= words) return;
  const int r0 = blockIdx.x * kGrmRangeRows;
  const int r1 = min(rows, r0 + kGrmRangeRows);
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  for (int rb = r0; rb < r1; rb += 8) {
    uint32_t w[8];
    double tv[8], sv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = min(rb + u, r1 - 1);
      const uint32_t v = seg[(int64_t)r * pitch + col];
      w[u] = rb + u < r1 ? v : kLo;
      tv[u] = t[r];
      sv[u] = s[r];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      uint32_t hi, both, called;
      slot_masks(w[u], hi, both, called);
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        acc[k] += and_mask(tv[u], __builtin_amdgcn_sbfe((int)hi, 2u * k, 1u));
        acc[k] += and_mask(tv[u], __builtin_amdgcn_sbfe((int)both, 2u * k, 1u));
        acc[k] += and_mask(sv[u], __builtin_amdgcn_sbfe((int)called, 2u * k, 1u));
      }
    }
  }
  double* out = ypart + (int64_t)blockIdx.x * ystride + (int64_t)col * 16;
#pragma unroll
  for (int k = 0; k < 16; ++k) out[k] = acc[k];
}

// the integer twin of pass 2: ipart[range][pitch * 16] = sum_r c(r, i) used[r]
__global__ __launch_bounds__(256, 2) void grm_called_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch, int32_t words,
                                                         const int32_t* __restrict__ used, int32_t* __restrict__ ipart,
                                                         int64_t ystride) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (blockIdx.y * 4 + wave) * 64 + lane;
  if (col >= words) return;
  const int r0 = blockIdx.x * kGrmRangeRows;
  const int r1 = min(rows, r0 + kGrmRangeRows);
  int32_t acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0;
  for (int rb = r0; rb < r1; rb += 8) {
    uint32_t w[8];
    int32_t uv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = min(rb + u, r1 - 1);
      const uint32_t v = seg[(int64_t)r * pitch + col];
      w[u] = rb + u < r1 ? v : kLo;
      uv[u] = used[r];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      uint32_t hi, both, called;
      slot_masks(w[u], hi, both, called);
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[k] += uv[u] & __builtin_amdgcn_sbfe((int)called, 2u * k, 1u);
    }
  }
  int32_t* out = ipart + (int64_t)blockIdx.x * ystride + (int64_t)col * 16;
#pragma unroll
  for (int k = 0; k < 16; ++k) out[k] = acc[k];
}

// y[i] = (the ranges' partials added in order) / M'; M' = 0: y = 0
__global__ __launch_bounds__(256) void grm_finish_kernel(const double* __restrict__ ypart, int64_t ystride, int32_t nranges, int32_t n,
                                                         const unsigned long long* __restrict__ mprime, double* __restrict__ y) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long m = *mprime;
  double a = 0.0;
  for (int32_t g = 0; g < nranges; ++g) a += ypart[(int64_t)g * ystride + i];
  y[i] = m ? a / (double)m : 0.0;
}

// *nz = the samples called at one or more used variants (the ranges' integer partials added; any order)
__global__ __launch_bounds__(256) void grm_called_finish_kernel(const int32_t* __restrict__ ipart, int64_t ystride, int32_t nranges,
                                                                int32_t n, int32_t* __restrict__ nz) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int64_t a = 0;
  if (i < n)
    for (int32_t g = 0; g < nranges; ++g) a += ipart[(int64_t)g * ystride + i];
  const unsigned long long b = __ballot(a > 0);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(nz, (int32_t)__popcll(b));
}

inline int32_t words_of(int32_t n) { return (n + 15) / 16; }
inline dim3 range_grid(int32_t rows, int32_t n) {
  return dim3((unsigned)((rows + kGrmRangeRows - 1) / kGrmRangeRows), (unsigned)grm_groups(n));
}

}  // namespace

hipError_t launch_grm_append(const uint8_t* src, int64_t row_bytes, int64_t nv, int32_t n, int swap, uint32_t* dst, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  const int32_t pitch = grm_pitch_words(n);
  const int64_t blocks = std::min<int64_t>((nv * pitch + 255) / 256, 65536);
  hipLaunchKernelGGL(grm_append_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src, row_bytes, nv, n, pitch, swap, dst);
  return hipGetLastError();
}

hipError_t launch_grm_counts(const uint32_t* seg, int32_t rows, int32_t n, int32_t* cnt, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  const int blocks = std::min((rows + 3) / 4, 16384);
  hipLaunchKernelGGL(grm_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, seg, rows, grm_pitch_words(n), cnt);
  return hipGetLastError();
}

hipError_t launch_grm_weights(const int32_t* cnt, int64_t rows, double min_maf, const uint8_t* keep, int32_t n, double max_missing,
                              double hwe_min_p, const double* hwe_p, double* mu, double* d, int32_t* used,
                              unsigned long long* mprime, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(grm_weights_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, cnt, rows, min_maf, keep, n,
                     max_missing, hwe_min_p, hwe_p, mu, d, used, mprime);
  return hipGetLastError();
}

hipError_t launch_grm_ax(const uint32_t* seg, int32_t rows, int32_t n, const double* mu, const double* x, double* tpart,
                         int64_t vstride, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  const dim3 grid((unsigned)((rows + kRowsPerBlock1 - 1) / kRowsPerBlock1), (unsigned)grm_groups(n));
  hipLaunchKernelGGL(grm_ax_kernel, grid, dim3(256), 0, stream, seg, rows, grm_pitch_words(n), words_of(n), mu, x, n, tpart, vstride);
  return hipGetLastError();
}

hipError_t launch_grm_combine_t(const double* tpart, int64_t vstride, int32_t n, int64_t rows, const double* mu, const double* d,
                                double* t, double* s, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(grm_combine_t_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, tpart, vstride, grm_groups(n),
                     rows, mu, d, t, s);
  return hipGetLastError();
}

hipError_t launch_grm_at(const uint32_t* seg, int32_t rows, int32_t n, const double* t, const double* s, double* ypart,
                         hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  const int32_t pitch = grm_pitch_words(n);
  hipLaunchKernelGGL(grm_at_kernel, range_grid(rows, n), dim3(256), 0, stream, seg, rows, pitch, words_of(n), t, s, ypart,
                     (int64_t)pitch * 16);
  return hipGetLastError();
}

hipError_t launch_grm_called(const uint32_t* seg, int32_t rows, int32_t n, const int32_t* used, int32_t* ipart, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  const int32_t pitch = grm_pitch_words(n);
  hipLaunchKernelGGL(grm_called_kernel, range_grid(rows, n), dim3(256), 0, stream, seg, rows, pitch, words_of(n), used, ipart,
                     (int64_t)pitch * 16);
  return hipGetLastError();
}

hipError_t launch_grm_finish(const double* ypart, int32_t nranges, int32_t n, const unsigned long long* mprime, double* y,
                             hipStream_t stream) {
  hipLaunchKernelGGL(grm_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ypart,
                     (int64_t)grm_pitch_words(n) * 16, nranges, n, mprime, y);
  return hipGetLastError();
}

hipError_t launch_grm_called_finish(const int32_t* ipart, int32_t nranges, int32_t n, int32_t* nz, hipStream_t stream) {
  hipLaunchKernelGGL(grm_called_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ipart,
                     (int64_t)grm_pitch_words(n) * 16, nranges, n, nz);
  return hipGetLastError();
}

}  // namespace pcoa
