// loadings.hip -- per-variant loadings of the principal coordinates: T[v][c] = sum_i bit(v, i) u'[c][i] over rows
// of carrier bitsets (sample i = bit (i & 31) of word i >> 5, pitch ld words).  u' is the PREPARED vector set of
// pcoa_loadings_begin: [num_pc][npad] doubles, npad = 32 ceil(N / 32), centred where asked and ZERO for i >= N, so a bit of a
// sample >= N adds +0.0 and nothing of a row beyond ceil(N / 32) words is ever loaded: tail bits and pad words are ignored, not
// trusted.
//
// Decomposition.  A GROUP of L lanes (L = loadings_lanes(N): 8, 16, 32 or 64, whichever leaves the fewest idle word slots) owns
// R = 32 / K rows at a time for a chunk of K components; lane g of the group takes the word columns g, g + L, g + 2 L, ...  A
// wave holds 64 / L groups and a workgroup four waves, every one with rows of its own: the split is along ROWS, so a short row
// (79 words at N = 2,504: five passes of a 16-lane group, 79 of 80 slots used) leaves no wave idle.  For one word column the
// lane loads 8 bits x K prepared values at a time and spends them on all R rows: a bit is decoded ONCE (a sign-extended
// bit-field extract: 0 or -1) and used as an AND mask on the two halves of each of the K addends, 1 + 3 K instructions per bit
// against 5 K of operator_xv_kernel's select form.
//
// Determinism.  Entry (v, c) is the sum, by ONE lane each, of the lane's word columns in increasing order and of their bits in
// increasing order into one accumulator from +0.0, then of the L lane totals by a halving butterfly (distance L / 2 .. 1; both
// partners add the same two numbers, so every lane ends with the same bits).  L depends on N only; K, R, the row's place in the
// call, the grid and the CU count decide which lane group computes an entry, never how.  No atomics.
#include <algorithm>

#include "pcoa_internal.h"

namespace pcoa {

int32_t loadings_lanes(int32_t n) {
  const int32_t words = (n + 31) / 32;
  if (words <= 8) return 8;
  int32_t best = 64, slots = (words + 63) / 64 * 64;
  for (int32_t l : {32, 16}) {
    const int32_t s = (words + l - 1) / l * l;
    if (s < slots) { slots = s; best = l; }
  }
  return best;
}

int loadings_chunk(int32_t remaining) { return remaining >= 8 ? 8 : remaining >= 4 ? 4 : remaining >= 2 ? 2 : 1; }

namespace {

// v where m == -1, +0.0 where m == 0
__device__ __forceinline__ double and_mask(double v, int m) {
  return __hiloint2double(__double2hiint(v) & m, __double2loint(v) & m);
}

template <int K, int L>
__global__ __launch_bounds__(256) void loadings_kernel(const uint32_t* __restrict__ bits, int64_t nv, int64_t ld, int32_t words,
                                                       const double* __restrict__ u, int64_t ustride,
                                                       const double* __restrict__ div, double* __restrict__ out, int32_t num_pc) {
  constexpr int R = 32 / K;     // rows a group carries past one load of the prepared values
  constexpr int G = 64 / L;     // groups of a wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane & (L - 1);
  const int64_t row0 = (((int64_t)blockIdx.x * 4 + wave) * G + lane / L) * R;
  double acc[R][K];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int k = 0; k < K; ++k) acc[r][k] = 0.0;
  const int iters = (words + L - 1) / L;
  for (int j = 0; j < iters; ++j) {
    const int w = j * L + g;
    const bool live = w < words;
    const int wc = live ? w : words - 1;   // a slot beyond the row loads a valid word and drops it
    uint32_t x[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = min(row0 + r, nv - 1);   // (rows beyond the call repeat its last row and are not stored)
      const uint32_t t = bits[row * ld + wc];
      x[r] = live ? t : 0u;
    }
    const double* up = u + (int64_t)wc * 32;
#pragma unroll 1
    for (int s = 0; s < 32; s += 8) {
      double uu[8][K];
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int b = 0; b < 8; ++b) uu[b][k] = up[k * ustride + s + b];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          const int m = __builtin_amdgcn_sbfe((int)x[r], (unsigned)(s + b), 1u);
#pragma unroll
          for (int k = 0; k < K; ++k) acc[r][k] += and_mask(uu[b][k], m);
        }
    }
  }
#pragma unroll
  for (int h = L / 2; h >= 1; h >>= 1)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < K; ++k) acc[r][k] += __shfl_xor(acc[r][k], h, 64);
  // every lane of the group holds all R x K totals: lane g stores the entries whose number is g modulo L
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (((r * K + k) & (L - 1)) == g && row0 + r < nv) out[(row0 + r) * num_pc + k] = div ? acc[r][k] / div[k] : acc[r][k];
}

template <int K>
hipError_t launch_k(int32_t lanes, dim3 grid, hipStream_t stream, const uint32_t* bits, int64_t nv, int64_t ld, int32_t words,
                    const double* u, int64_t ustride, const double* div, double* out, int32_t num_pc) {
  switch (lanes) {
    case 8: hipLaunchKernelGGL((loadings_kernel<K, 8>), grid, dim3(256), 0, stream, bits, nv, ld, words, u, ustride, div, out, num_pc); break;
    case 16: hipLaunchKernelGGL((loadings_kernel<K, 16>), grid, dim3(256), 0, stream, bits, nv, ld, words, u, ustride, div, out, num_pc); break;
    case 32: hipLaunchKernelGGL((loadings_kernel<K, 32>), grid, dim3(256), 0, stream, bits, nv, ld, words, u, ustride, div, out, num_pc); break;
    case 64: hipLaunchKernelGGL((loadings_kernel<K, 64>), grid, dim3(256), 0, stream, bits, nv, ld, words, u, ustride, div, out, num_pc); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_loadings(const uint32_t* bits, int64_t nv, int64_t ld_words, int32_t n, const double* u, int64_t ustride, int32_t k,
                           const double* div, double* out, int32_t num_pc, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  const int32_t words = (n + 31) / 32, lanes = loadings_lanes(n);
  const int64_t rows_per_wg = (int64_t)4 * (64 / lanes) * (32 / k);
  const int64_t blocks = (nv + rows_per_wg - 1) / rows_per_wg;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks);
  switch (k) {
    case 1: return launch_k<1>(lanes, grid, stream, bits, nv, ld_words, words, u, ustride, div, out, num_pc);
    case 2: return launch_k<2>(lanes, grid, stream, bits, nv, ld_words, words, u, ustride, div, out, num_pc);
    case 4: return launch_k<4>(lanes, grid, stream, bits, nv, ld_words, words, u, ustride, div, out, num_pc);
    case 8: return launch_k<8>(lanes, grid, stream, bits, nv, ld_words, words, u, ustride, div, out, num_pc);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace pcoa
