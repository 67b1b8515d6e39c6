// grm_qc.hip -- quality control on the resident 2-bit store of a GRM ctx (the rule is stated at the block of
// pcoa.h): the Hardy-Weinberg exact test of every variant from its three genotype counts, the variants that fail each of the
// three variant tests, and the per-sample genotype counts -- the column statistics of the store.
//   hwe      p_v of Wigginton, Cutler and Abecasis (2005) without mid-p, one lane per variant: with n called samples, R copies
//            of the rarer allele and k heterozygotes, P(k + 2) = P(k) 4 r c / ((k + 2)(k + 1)), r = (R - k) / 2 rare homozygotes
//            and c = n - (R + k) / 2 common ones.  The lane starts at k0 next to the mode with P(k0) = 1 and walks outward, twice:
//            first from k0 to the observed h for P(h), then over the whole support, where it adds every term to the total and
//            the terms at or below P(h) (1 + 2^-24) to the counted sum.  Both walks take the same steps, so the second meets
//            P(h) with the bits of the first.  No array of terms; a step is one product and one quotient of exact operands.
//   counts   a lane owns ONE word column of 16 samples and the rows of a range of kGrmRangeRows rows stream past it, as in
//            grm_called_kernel (grm_bits.hip).  The three classes of a word are bit planes at the slots' even positions; the
//            missing and the het plane share a word (het moved to the odd positions), hom has one of its own.  A block of 16
//            rows goes through a tree of 15 carry-save adders into bit-sliced counters (ones, twos, fours, eights), the
//            block's sixteens ripple into six wider slices, and the ten slices are spent into int32 once, at the end of the
//            range: 512 rows cannot overflow a ten-bit slice set.  An unused or absent row is a zero word: it has no plane.
//            The finish adds the ranges' int32 partials to int64 in (segment, range) order and writes called = rows - missing.
// No floating-point atomics; the only atomics are the three integer counts of the fails kernel.
#include <algorithm>

#include "grm_slots.h"
#include "pcoa_internal.h"

namespace pcoa {
namespace {

// p of one variant; n called, h het, o hom non-reference
__device__ double hwe_exact(int32_t n, int32_t h, int32_t o) {
#pragma clang fp contract(off)
  const int64_t a = (int64_t)h + 2 * (int64_t)o;
  const int64_t R = min(a, 2 * (int64_t)n - a);
  if (n <= 0 || R <= 0) return 1.0;
  int64_t k0 = R * (2 * (int64_t)n - R) / (2 * (int64_t)n);   // next to the mode, of R's parity, in [0, R]
  if ((k0 ^ R) & 1) k0 += 1;
  const int64_t r0 = (R - k0) / 2, c0 = (int64_t)n - (R + k0) / 2;
  // the first walk: P(h) relative to P(k0) = 1
  double ph = 1.0;
  {
    int64_t k = k0, r = r0, c = c0;
    while (k > h) {   // down
      ph = ph * ((double)k * (double)(k - 1)) / (4.0 * (double)(r + 1) * (double)(c + 1));
      k -= 2; r += 1; c += 1;
    }
    while (k < h) {   // up
      ph = ph * (4.0 * (double)r * (double)c) / ((double)(k + 2) * (double)(k + 1));
      k += 2; r -= 1; c -= 1;
    }
  }
  const double thr = ph * (1.0 + 0x1p-24);
  double total = 1.0, counted = 1.0 <= thr ? 1.0 : 0.0;
  {
    double t = 1.0;
    int64_t k = k0, r = r0, c = c0;
    while (k >= 2) {
      t = t * ((double)k * (double)(k - 1)) / (4.0 * (double)(r + 1) * (double)(c + 1));
      k -= 2; r += 1; c += 1;
      total += t;
      if (t <= thr) counted += t;
    }
  }
  {
    double t = 1.0;
    int64_t k = k0, r = r0, c = c0;
    while (k + 2 <= R) {
      t = t * (4.0 * (double)r * (double)c) / ((double)(k + 2) * (double)(k + 1));
      k += 2; r -= 1; c -= 1;
      total += t;
      if (t <= thr) counted += t;
    }
  }
  return counted / total;
}

__global__ __launch_bounds__(256) void grm_hwe_kernel(const int32_t* __restrict__ cnt, int64_t rows, double* __restrict__ p) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  p[r] = hwe_exact(cnt[r * 3], cnt[r * 3 + 1], cnt[r * 3 + 2]);
}

// fails[0..2] += the rows that fail the MAF test (grm_weights_kernel's first three conjuncts), the missing test and the HWE test,
// each judged alone and in the expressions of grm_weights_kernel (integer counts)
__global__ __launch_bounds__(256) void grm_qc_fails_kernel(const int32_t* __restrict__ cnt, int64_t rows, int32_t n, double min_maf,
                                                           double max_missing, double hwe_min_p, const double* __restrict__ hwe_p,
                                                           unsigned long long* __restrict__ fails) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int f0 = 0, f1 = 0, f2 = 0;
  if (r < rows) {
    const int32_t nv = cnt[r * 3], a = cnt[r * 3 + 1] + 2 * cnt[r * 3 + 2];
    f0 = (nv > 0 && a > 0 && a < 2 * nv && (double)min(a, 2 * nv - a) >= min_maf * (2.0 * (double)nv)) ? 0 : 1;
    f1 = ((double)(n - nv) <= max_missing * (double)n) ? 0 : 1;
    f2 = (hwe_p == nullptr || hwe_min_p == 0.0 || hwe_p[r] >= hwe_min_p) ? 0 : 1;
  }
  const unsigned long long b0 = __ballot(f0), b1 = __ballot(f1), b2 = __ballot(f2);
  if ((threadIdx.x & 63) == 0) {
    if (b0) atomicAdd(fails + 0, (unsigned long long)__popcll(b0));
    if (b1) atomicAdd(fails + 1, (unsigned long long)__popcll(b1));
    if (b2) atomicAdd(fails + 2, (unsigned long long)__popcll(b2));
  }
}

// one carry-save adder over every bit position: a + b + c = 2 h + l
__device__ __forceinline__ void csa(uint32_t& h, uint32_t& l, uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t u = a ^ b;
  h = (a & b) | (u & c);
  l = u ^ c;
}

constexpr int kSlices = 10;   // 2^10 > kGrmRangeRows: a range cannot overflow them
static_assert(kGrmRangeRows < (1 << kSlices) && kGrmRangeRows % 16 == 0, "the slices of grm_sample_counts_kernel hold one range");

// s += the 16 planes x[0 .. 16) at every bit position
__device__ __forceinline__ void add16(uint32_t (&s)[kSlices], const uint32_t (&x)[16]) {
  uint32_t ta, tb, fa, fb, ea, eb, sx;
  csa(ta, s[0], s[0], x[0], x[1]);
  csa(tb, s[0], s[0], x[2], x[3]);
  csa(fa, s[1], s[1], ta, tb);
  csa(ta, s[0], s[0], x[4], x[5]);
  csa(tb, s[0], s[0], x[6], x[7]);
  csa(fb, s[1], s[1], ta, tb);
  csa(ea, s[2], s[2], fa, fb);
  csa(ta, s[0], s[0], x[8], x[9]);
  csa(tb, s[0], s[0], x[10], x[11]);
  csa(fa, s[1], s[1], ta, tb);
  csa(ta, s[0], s[0], x[12], x[13]);
  csa(tb, s[0], s[0], x[14], x[15]);
  csa(fb, s[1], s[1], ta, tb);
  csa(eb, s[2], s[2], fa, fb);
  csa(sx, s[3], s[3], ea, eb);
#pragma unroll
  for (int b = 4; b < kSlices; ++b) {   // the block's sixteens ripple into the wider slices
    const uint32_t carry = s[b] & sx;
    s[b] ^= sx;
    sx = carry;
  }
}

// the count at bit position pos of the slices
__device__ __forceinline__ int32_t spend(const uint32_t (&s)[kSlices], int pos) {
  int32_t v = 0;
#pragma unroll
  for (int b = 0; b < kSlices; ++b) v |= (int32_t)((s[b] >> pos) & 1u) << b;
  return v;
}

// ipart[range][class][pitch * 16], class = missing, het, hom: the rows of the range at which sample i has that class; used (may be
// NULL: every row counts): 0 / 1 per row of the segment
__global__ __launch_bounds__(256, 2) void grm_sample_counts_kernel(const uint32_t* __restrict__ seg, int32_t rows, int32_t pitch,
                                                                int32_t words, const int32_t* __restrict__ used,
                                                                int32_t* __restrict__ ipart, int64_t ystride) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = (blockIdx.y * 4 + wave) * 64 + lane;
  if (col >= words) return;
  const int r0 = blockIdx.x * kGrmRangeRows;
  const int r1 = min(rows, r0 + kGrmRangeRows);
  uint32_t smh[kSlices], so[kSlices];   // missing (even positions) and het (odd) / hom (even)
#pragma unroll
  for (int b = 0; b < kSlices; ++b) smh[b] = so[b] = 0u;
  for (int rb = r0; rb < r1; rb += 16) {
    uint32_t w[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int r = min(rb + u, r1 - 1);
      const uint32_t v = seg[(int64_t)r * pitch + col];
      const int32_t uv = used ? used[r] : 1;
      w[u] = rb + u < r1 ? v & (uint32_t)(0 - uv) : 0u;   // the sign-extended used flag: an unused row is a zero word
    }
    uint32_t mh[16], o[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const uint32_t lo = w[u] & kLo, hi = (w[u] >> 1) & kLo;
      mh[u] = (lo & ~hi) | ((hi & ~lo) << 1);
      o[u] = hi & lo;
    }
    add16(smh, mh);
    add16(so, o);
  }
  int32_t* out = ipart + (int64_t)blockIdx.x * 3 * ystride + (int64_t)col * 16;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    out[k] = spend(smh, 2 * k);
    out[ystride + k] = spend(smh, 2 * k + 1);
    out[2 * ystride + k] = spend(so, 2 * k);
  }
}

// out[i][3] = called, het, hom non-reference: the ranges' partials added in order, called = rows_counted - missing
__global__ __launch_bounds__(256) void grm_sample_counts_finish_kernel(const int32_t* __restrict__ ipart, int64_t ystride,
                                                                       int32_t nranges, int32_t n, int64_t rows_counted,
                                                                       int64_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int64_t m = 0, h = 0, o = 0;
  for (int32_t g = 0; g < nranges; ++g) {
    const int32_t* p = ipart + (int64_t)g * 3 * ystride + i;
    m += p[0];
    h += p[ystride];
    o += p[2 * ystride];
  }
  out[(int64_t)i * 3 + 0] = rows_counted - m;
  out[(int64_t)i * 3 + 1] = h;
  out[(int64_t)i * 3 + 2] = o;
}

}  // namespace

hipError_t launch_grm_hwe(const int32_t* cnt, int64_t rows, double* p, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(grm_hwe_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, cnt, rows, p);
  return hipGetLastError();
}

hipError_t launch_grm_qc_fails(const int32_t* cnt, int64_t rows, int32_t n, double min_maf, double max_missing, double hwe_min_p,
                               const double* hwe_p, unsigned long long* fails, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(grm_qc_fails_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, cnt, rows, n, min_maf,
                     max_missing, hwe_min_p, hwe_p, fails);
  return hipGetLastError();
}

hipError_t launch_grm_sample_counts(const uint32_t* seg, int32_t rows, int32_t n, const int32_t* used, int32_t* ipart,
                                    hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  const int32_t pitch = grm_pitch_words(n);
  const dim3 grid((unsigned)((rows + kGrmRangeRows - 1) / kGrmRangeRows), (unsigned)grm_groups(n));
  hipLaunchKernelGGL(grm_sample_counts_kernel, grid, dim3(256), 0, stream, seg, rows, pitch, (n + 15) / 16, used, ipart,
                     (int64_t)pitch * 16);
  return hipGetLastError();
}

hipError_t launch_grm_sample_counts_finish(const int32_t* ipart, int32_t nranges, int32_t n, int64_t rows_counted, int64_t* out,
                                           hipStream_t stream) {
  hipLaunchKernelGGL(grm_sample_counts_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ipart,
                     (int64_t)grm_pitch_words(n) * 16, nranges, n, rows_counted, out);
  return hipGetLastError();
}

}  // namespace pcoa
