// complete.hip -- the pairwise-complete similarity, evaluated on the fly from TWO integer matrices, and the
// .bed decode that yields both bitsets.  computePca (reference VariantsPca.scala:198-231) decomposes the shared-carrier counts
// S(i, j), and hasVariation (VariantsPca.scala:56-60) sees a missing call as a non-carrier: a sample with many missing calls
// has a uniformly smaller row.  With Q the Gram matrix of the MISSING-call bitsets (the companion engine's S) and V the number
// of variants fed, the rule divides each shared count by the number of variants at which both samples were called:
//
//   c_i     = V - Q(i, i)                       (int64; the variants at which sample i is called)
//   M(i, j) = c_i + c_j - V + Q(i, j)           (int64; both called)
//   K(i, j) = M > 0 ? (double)S(i, j) / (double)M : 0.0                                       one fp64 division
//   centred   B(i, j) = ((K(i, j) - r_i / N) - r_j / N) + mm,   r = row sums of K,   mm = (sum_i r_i) / N / N
//
// with S(i, j) the TOTAL entry of the carrier engine (int32 matrix plus the int64 part where there is one; the companion has
// no int64 part), IEEE fp64 and no contraction anywhere: variants_pca.py's call_complete_measure / centred_measure are the
// numpy statement.  K is never in memory; the N x N fp64 B exists only for the dense solver and pcoa_center_read_f64.  The
// kernels are twins of measure.hip's and share their loop shapes through symv_shared.h: the row form is row_dot's
// association, the upper-triangle form writes the partials symv_sym_gather_kernel adds.  Plain HIP, fp64, no floating-point
// atomics, no scratch.
#include "pcoa_internal.h"
#include "symv_shared.h"

namespace pcoa {
namespace {

// the rule: s the total entry of S, sd = (double)s (the caller converts: from the int32 word where there is no int64 part),
// ci / cj the two samples' called counts, q = Q(i, j), v = V
__device__ __forceinline__ double complete_k(double sd, int64_t ci, int64_t cj, int64_t q, int64_t v) {
  const int64_t m = ci + cj - v + q;
  return m > 0 ? sd / (double)m : 0.0;
}

// PLINK 1 .bed rows -> the carrier bitsets AND the missing-call bitsets, one read of the row.  The carrier word is what
// plink_bed_to_bits_kernel (gram_aux.hip) writes, bit for bit: the same aligned 8-byte loads and tail handling, the same
// squeeze of the even bits; the missing word is code 01 (low bit set, high bit clear) squeezed the same way.  Samples >= N are
// masked in both.  One wave per row, one lane per output word = 32 samples = 8 bytes of the row.
__device__ __forceinline__ uint32_t squeeze_even(uint64_t m) {
  m = (m | (m >> 1)) & 0x3333333333333333ull;
  m = (m | (m >> 2)) & 0x0f0f0f0f0f0f0f0full;
  m = (m | (m >> 4)) & 0x00ff00ff00ff00ffull;
  m = (m | (m >> 8)) & 0x0000ffff0000ffffull;
  m = (m | (m >> 16)) & 0x00000000ffffffffull;
  return (uint32_t)m;
}

__global__ __launch_bounds__(256) void plink_bed_to_bits_pair_kernel(const uint8_t* __restrict__ bed, int64_t row_bytes, int64_t nv,
                                                                     int32_t n, int64_t words, int ref_a1,
                                                                     uint32_t* __restrict__ bits, uint32_t* __restrict__ miss) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nv) return;
  const uint8_t* row = bed + r * row_bytes;
  for (int64_t w = lane; w < words; w += 64) {
    const int64_t avail = row_bytes - 8 * w;          // bytes the row still has at this word
    uint64_t x = 0;
    if (avail > 0) {
      const int need = avail < 8 ? (int)avail : 8;
      const uintptr_t a = reinterpret_cast<uintptr_t>(row + 8 * w);
      const int sh = (int)(a & 7);
      const uint64_t* q = reinterpret_cast<const uint64_t*>(a - sh);
      x = q[0] >> (8 * sh);
      if (sh + need > 8) x |= q[1] << (8 * (8 - sh));   // (sh > 0 here)
      if (need < 8) x &= (1ull << (8 * need)) - 1ull;   // what follows the row is not its own
    }
    const uint64_t E = 0x5555555555555555ull;
    const uint64_t lo = x & E, hi = (x >> 1) & E;
    const uint64_t carrier = (hi & ~lo) | (ref_a1 ? (hi & lo) : (~hi & ~lo & E));
    const uint64_t missing = lo & ~hi;
    const int64_t first = 32 * w;
    uint32_t keep = 0xffffffffu;
    if (first >= n) keep = 0u;
    else if (first + 32 > n) keep = (1u << (n - (int32_t)first)) - 1u;
    bits[r * words + w] = squeeze_even(carrier) & keep;
    miss[r * words + w] = squeeze_even(missing) & keep;
  }
}

// c_i = V - Q(i, i); flag[0] = 1 where a sample's missing count exceeds V (every lane that sees it stores the same word)
__global__ __launch_bounds__(256) void complete_diag_kernel(const int32_t* __restrict__ q32, int32_t n, int64_t v,
                                                            int64_t* __restrict__ c, int32_t* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t d = (int64_t)q32[(int64_t)i * n + i];
  c[i] = v - d;
  if (d > v) flag[0] = 1;
}

__global__ __launch_bounds__(256) void complete_fill_kernel(double* __restrict__ x, int32_t n, double value) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = value;
}

// ---- row forms: one wave per row, row_dot's loop shape (16-byte loads of BOTH matrices when N % 4 == 0, 4-byte loads
// otherwise; the same main-loop bounds), c_j loaded beside cm[j].  CENTRE: y = B x.  !CENTRE: y = K x -- with x = 1 the row
// sums of K, added in row_dot's fixed order.
template <bool HAS64, bool CENTRE>
__global__ __launch_bounds__(256) void complete_symv_rows_kernel(const int32_t* __restrict__ s32, const int64_t* __restrict__ s64,
                                                                 const int32_t* __restrict__ q32, int n,
                                                                 const int64_t* __restrict__ cc, int64_t v,
                                                                 const double* __restrict__ cm, const double* __restrict__ stats,
                                                                 const double* __restrict__ x, double* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int64_t base = (int64_t)i * n;
  const int64_t ci = cc[i];
  const double row_mean = CENTRE ? cm[i] : 0.0;
  const double mmean = CENTRE ? stats[1] : 0.0;
  auto entry = [&](double sd, int64_t q, int64_t cj, double col_mean) -> double {
#pragma clang fp contract(off)
    double t = complete_k(sd, ci, cj, q, v);
    if (CENTRE) {
      t = t - row_mean;
      t = t - col_mean;
      t = t + mmean;
    }
    return t;
  };
  auto quad = [&](int j, double* out) {
    const int4 s = *reinterpret_cast<const int4*>(s32 + base + j);
    const int4 q = *reinterpret_cast<const int4*>(q32 + base + j);
    double d0 = (double)s.x, d1 = (double)s.y, d2 = (double)s.z, d3 = (double)s.w;
    if (HAS64) {
      const longlong2 l = *reinterpret_cast<const longlong2*>(s64 + base + j);
      const longlong2 h = *reinterpret_cast<const longlong2*>(s64 + base + j + 2);
      d0 = (double)((int64_t)s.x + l.x); d1 = (double)((int64_t)s.y + l.y);
      d2 = (double)((int64_t)s.z + h.x); d3 = (double)((int64_t)s.w + h.y);
    }
    const longlong2 pa = *reinterpret_cast<const longlong2*>(cc + j), pb = *reinterpret_cast<const longlong2*>(cc + j + 2);
    double2 ca = make_double2(0.0, 0.0), cb = make_double2(0.0, 0.0);
    if (CENTRE) {
      ca = *reinterpret_cast<const double2*>(cm + j);
      cb = *reinterpret_cast<const double2*>(cm + j + 2);
    }
    out[0] = entry(d0, q.x, pa.x, ca.x); out[1] = entry(d1, q.y, pa.y, ca.y);
    out[2] = entry(d2, q.z, pb.x, cb.x); out[3] = entry(d3, q.w, pb.y, cb.y);
  };
  auto one = [&](int j) -> double {
    const double sd = HAS64 ? (double)((int64_t)s32[base + j] + s64[base + j]) : (double)s32[base + j];
    return entry(sd, (int64_t)q32[base + j], cc[j], CENTRE ? cm[j] : 0.0);
  };
  const double acc = row_dot(quad, one, x, n, lane);
  if (lane == 0) y[i] = acc;
}

// ---- upper-triangle form: symv_sym_tile_body's decomposition (1024 x 1024 tiles, a 2 x 2 wave grid, a lane owns 8 columns,
// interior tiles without masks, DPP row sums, partials into `part` for symv_sym_gather_kernel).  Beside x_i and rowMean_i the
// tile's c_i are staged in LDS, the lane's eight c_j stay in registers.  K(i, j) is evaluated ONCE per loaded entry pair and
// used for both triangles.  All offsets into S and Q are 64-bit.  Two matrices stream through the prefetch: CNB = 2 rows of
// EACH in flight per wave -- the 32 load registers of the Jaccard kernel's four rows of one matrix.  The compiler's count for
// the centred kernel by depth: 1 -> 136 VGPRs (3 waves per SIMD), 2 -> 192 (2), 3 -> 240 (2), 4 -> 256 (1); none spills.
// Depth 2 at two waves per SIMD keeps 64 KiB of loads in flight per CU, above the ~50 KiB that 1/256 of the HBM rate times a
// 2 us latency asks for; depth 3 would sit 16 registers under the limit of that occupancy.  Chosen by this arithmetic, not by
// a measurement (profiles/r15a_complete_kernel_resources.txt).
constexpr int CNB = 2;

template <bool CENTRE, bool DIAG, bool EDGE>
__device__ __forceinline__ void complete_sym_tile_body(const int32_t* __restrict__ s32, const int32_t* __restrict__ q32, int n, int nb,
                                                       const int64_t* __restrict__ cc, const int64_t v,
                                                       const double* __restrict__ cm, const double mmean,
                                                       const double* __restrict__ x, double* __restrict__ part, int bi, int bj,
                                                       double* xs, double* ms, int64_t* pr, double (*rs)[SYT]) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int i0 = bi * SYT, j0 = bj * SYT;
  const int jw = j0 + 512 * wc + 4 * lane;   // the lane's 8 columns: jw + 256 q + {0..3}
  const int rows = EDGE ? min(SYT, n - i0) : SYT;
  for (int r = threadIdx.x; r < SYT; r += 256) {
    const bool in = !EDGE || i0 + r < n;
    xs[r] = in ? x[i0 + r] : 0.0;
    if (CENTRE) ms[r] = in ? cm[i0 + r] : 0.0;
    pr[r] = in ? cc[i0 + r] : (int64_t)0;
  }
  double xj[8], mj[8], cacc[8];
  int64_t pj[8];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = jw + 256 * q + e;
      const bool in = !EDGE || j < n;
      xj[4 * q + e] = in ? x[j] : 0.0;
      mj[4 * q + e] = (CENTRE && in) ? cm[j] : 0.0;
      pj[4 * q + e] = in ? cc[j] : (int64_t)0;
      cacc[4 * q + e] = 0.0;
    }
  __syncthreads();
  const int64_t off0 = (int64_t)i0 * n + jw;
  auto load_row = [&](int r, int4 (&sv)[2], int4 (&qv)[2]) {
    const int64_t off = off0 + (int64_t)r * n;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (EDGE) {
        const bool in = r < rows && jw + 256 * q < n;   // n % 4 == 0: a quad is whole or absent
        sv[q] = in ? *reinterpret_cast<const int4*>(s32 + off + 256 * q) : make_int4(0, 0, 0, 0);
        qv[q] = in ? *reinterpret_cast<const int4*>(q32 + off + 256 * q) : make_int4(0, 0, 0, 0);
      } else {
        sv[q] = *reinterpret_cast<const int4*>(s32 + off + 256 * q);
        qv[q] = *reinterpret_cast<const int4*>(q32 + off + 256 * q);
      }
    }
  };
  auto use_row = [&](int r, const int4 (&sv)[2], const int4 (&qv)[2]) {
    const int i = i0 + r;
    const double xi = xs[r], mi = CENTRE ? ms[r] : 0.0;
    const int64_t pi = pr[r];
    double racc = 0.0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int se[4] = {sv[q].x, sv[q].y, sv[q].z, sv[q].w};
      const int qe[4] = {qv[q].x, qv[q].y, qv[q].z, qv[q].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = jw + 256 * q + e;
        const double kij = complete_k((double)se[e], pi, pj[4 * q + e], (int64_t)qe[e], v);
        double bij = kij, bji = kij;
        if (CENTRE) {
#pragma clang fp contract(off)
          bij = kij - mi;
          bij = bij - mj[4 * q + e];
          bij = bij + mmean;
          bji = kij - mj[4 * q + e];
          bji = bji - mi;
          bji = bji + mmean;
        }
        if (DIAG) {  // the tile's own upper triangle: the diagonal counts once (in the row sums)
          const bool in = !EDGE || j < n;
          racc += (j >= i && in) ? bij * xj[4 * q + e] : 0.0;
          cacc[4 * q + e] += (j > i && in) ? bji * xi : 0.0;
        } else if (EDGE) {
          // (columns >= n of the last block column: x, S, Q and c were read as 0 but the centred entry is not 0 -> mask)
          racc += j < n ? bij * xj[4 * q + e] : 0.0;
          cacc[4 * q + e] += j < n ? bji * xi : 0.0;
        } else {
          racc += bij * xj[4 * q + e];
          cacc[4 * q + e] += bji * xi;
        }
      }
    }
    racc = wave_sum_to_lane63(racc);
    if (lane == 63) rs[wc][r] = racc;
    // one row at a time, as in symv_sym_tile_body: the column sums are pinned here, and nothing moves across the barrier
#pragma unroll
    for (int c = 0; c < 8; ++c) asm volatile("" : "+v"(cacc[c]));
    __builtin_amdgcn_sched_barrier(0);
  };
  // rows wr, wr + 2, ..: CNB buffers per matrix, each refilled as soon as its row is used
  int4 sbuf[CNB][2], qbuf[CNB][2];
  const int nr = rows > wr ? (rows - wr + 1) / 2 : 0;   // this wave's row count
#pragma unroll
  for (int b = 0; b < CNB; ++b)
    if (b < nr) load_row(wr + 2 * b, sbuf[b], qbuf[b]);
  int k = 0;
  for (; k + 2 * CNB <= nr; k += CNB) {   // every refill is a row of the tile: no conditions in the steady state
#pragma unroll
    for (int b = 0; b < CNB; ++b) {
      use_row(wr + 2 * (k + b), sbuf[b], qbuf[b]);
      load_row(wr + 2 * (k + b + CNB), sbuf[b], qbuf[b]);
    }
  }
#pragma unroll
  for (int b = 0; b < CNB; ++b)   // the last < 2 CNB rows
    if (k + b < nr) {
      use_row(wr + 2 * (k + b), sbuf[b], qbuf[b]);
      if (k + b + CNB < nr) load_row(wr + 2 * (k + b + CNB), sbuf[b], qbuf[b]);
    }
  k += CNB;
#pragma unroll
  for (int b = 0; b < CNB; ++b)
    if (k + b < nr) use_row(wr + 2 * (k + b), sbuf[b], qbuf[b]);
  double* ptile = part + sym_tile_index(bi, bj, nb) * SYP;
  double* pcol = ptile + 2 * SYT + wr * SYT + 512 * wc + 4 * lane;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    *reinterpret_cast<double2*>(pcol + 256 * q) = make_double2(cacc[4 * q], cacc[4 * q + 1]);
    *reinterpret_cast<double2*>(pcol + 256 * q + 2) = make_double2(cacc[4 * q + 2], cacc[4 * q + 3]);
  }
  __syncthreads();
  for (int r = threadIdx.x; r < SYT; r += 256) {   // rows beyond N in the last block row: 0
    ptile[r] = r < rows ? rs[0][r] : 0.0;
    ptile[SYT + r] = r < rows ? rs[1][r] : 0.0;
  }
}

// One launch for all tiles, the block order of symv_sym_tiles_kernel:
// blockIdx.x: [corner (nb - nbi)] [diagonal nbi] [last block column (nb - nbi) * (nb - 1)] [interior nbi (nbi - 1) / 2, row by row]
// 40 KiB of LDS (x_i, rowMean_i, c_i: 24 KiB; the row sums of the two column halves: 16 KiB)
template <bool CENTRE>
__global__ __launch_bounds__(256) void complete_symv_sym_tiles_kernel(const int32_t* __restrict__ s32, const int32_t* __restrict__ q32,
                                                                      int n, int nb, int nbi, const int64_t* __restrict__ cc, int64_t v,
                                                                      const double* __restrict__ cm, const double* __restrict__ stats,
                                                                      const double* __restrict__ x, double* __restrict__ part) {
  __shared__ double xs[SYT], ms[SYT];
  __shared__ int64_t pr[SYT];
  __shared__ double rs[2][SYT];
  const double mmean = CENTRE ? stats[1] : 0.0;
  int t = blockIdx.x;
  const int edge = nb - nbi;           // 0 or 1
  if (t < edge) {
    complete_sym_tile_body<CENTRE, true, true>(s32, q32, n, nb, cc, v, cm, mmean, x, part, nb - 1, nb - 1, xs, ms, pr, rs);
    return;
  }
  t -= edge;
  if (t < nbi) {
    complete_sym_tile_body<CENTRE, true, false>(s32, q32, n, nb, cc, v, cm, mmean, x, part, t, t, xs, ms, pr, rs);
    return;
  }
  t -= nbi;
  if (t < edge * (nb - 1)) {
    complete_sym_tile_body<CENTRE, false, true>(s32, q32, n, nb, cc, v, cm, mmean, x, part, t, nb - 1, xs, ms, pr, rs);
    return;
  }
  t -= edge * (nb - 1);
  int bi = 0;
  while (t >= nbi - 1 - bi) {
    t -= nbi - 1 - bi;
    ++bi;
  }
  complete_sym_tile_body<CENTRE, false, false>(s32, q32, n, nb, cc, v, cm, mmean, x, part, bi, bi + 1 + t, xs, ms, pr, rs);
}

// B for the dense solver and pcoa_center_read_f64.  One workgroup per row, striding over the columns, as measure_center_kernel
__global__ __launch_bounds__(256) void complete_center_kernel(const int32_t* __restrict__ s32, const int64_t* __restrict__ s64,
                                                              const int32_t* __restrict__ q32, int32_t n,
                                                              const int64_t* __restrict__ cc, int64_t v,
                                                              const double* __restrict__ cm, const double* __restrict__ stats,
                                                              double* __restrict__ b) {
#pragma clang fp contract(off)
  const int i = blockIdx.x;
  const int64_t ci = cc[i];
  const double row_mean = cm[i];
  const double mmean = stats[1];
  for (int j = threadIdx.x; j < n; j += 256) {
    const int64_t idx = (int64_t)i * n + j;
    const int64_t s = (int64_t)s32[idx] + (s64 ? s64[idx] : 0);
    double t = complete_k((double)s, ci, cc[j], (int64_t)q32[idx], v);
    t = t - row_mean;
    t = t - cm[j];
    t = t + mmean;
    b[idx] = t;
  }
}

template <bool CENTRE>
void launch_rows(const int32_t* s32, const int64_t* s64, const int32_t* q32, int n, const int64_t* cc, int64_t v, const double* cm,
                 const double* stats, const double* x, double* y, hipStream_t stream) {
  const unsigned rows4 = (unsigned)((n + 3) / 4);
  if (s64)
    hipLaunchKernelGGL((complete_symv_rows_kernel<true, CENTRE>), dim3(rows4), dim3(256), 0, stream, s32, s64, q32, n, cc, v, cm,
                       stats, x, y);
  else
    hipLaunchKernelGGL((complete_symv_rows_kernel<false, CENTRE>), dim3(rows4), dim3(256), 0, stream, s32, s64, q32, n, cc, v, cm,
                       stats, x, y);
}

template <bool CENTRE>
void launch_tiles(const int32_t* s32, const int32_t* q32, int n, const int64_t* cc, int64_t v, const double* cm, const double* stats,
                  const double* x, double* part, hipStream_t stream) {
  const int nb = (n + SYT - 1) / SYT;
  const int nbi = n / SYT;   // block columns wholly inside N (nb or nb - 1)
  hipLaunchKernelGGL((complete_symv_sym_tiles_kernel<CENTRE>), dim3((unsigned)((int64_t)nb * (nb + 1) / 2)), dim3(256), 0, stream,
                     s32, q32, n, nb, nbi, cc, v, cm, stats, x, part);
}

}  // namespace

hipError_t launch_plink_bed_to_bits_pair(const uint8_t* bed, int64_t row_bytes, int64_t nv, int32_t n, int64_t words, int ref_a1,
                                         uint32_t* bits, uint32_t* miss, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  const int64_t blocks = (nv + 3) / 4;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(plink_bed_to_bits_pair_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, bed, row_bytes, nv, n, words,
                     ref_a1, bits, miss);
  return hipGetLastError();
}

hipError_t launch_complete_diag(const int32_t* q32, int32_t n, int64_t v, int64_t* c, int32_t* flag, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(int32_t), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(complete_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, q32, n, v, c, flag);
  return hipGetLastError();
}

hipError_t launch_complete_row_sums(const int32_t* s32, const int64_t* s64_or_null, const int32_t* q32, int32_t n, const int64_t* c,
                                    int64_t v, double* ones, double* row_sums, hipStream_t stream) {
  hipLaunchKernelGGL(complete_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ones, n, 1.0);
  launch_rows<false>(s32, s64_or_null, q32, n, c, v, nullptr, nullptr, ones, row_sums, stream);
  return hipGetLastError();
}

hipError_t launch_complete_row_sums_sym(const int32_t* s32, const int32_t* q32, int32_t n, const int64_t* c, int64_t v, double* ones,
                                        double* sym_part, double* row_sums, hipStream_t stream) {
  if (n & 3) return hipErrorInvalidValue;
  hipLaunchKernelGGL(complete_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ones, n, 1.0);
  launch_tiles<false>(s32, q32, n, c, v, nullptr, nullptr, ones, sym_part, stream);
  return launch_symv_sym_gather(sym_part, n, row_sums, stream);
}

hipError_t launch_complete_center(const int32_t* s32, const int64_t* s64_or_null, const int32_t* q32, int32_t n, const int64_t* c,
                                  int64_t v, const double* cm, const double* stats, double* b, hipStream_t stream) {
  hipLaunchKernelGGL(complete_center_kernel, dim3((unsigned)n), dim3(256), 0, stream, s32, s64_or_null, q32, n, c, v, cm, stats, b);
  return hipGetLastError();
}

hipError_t launch_complete_symv(const EigWorkspace& ws, int32_t n, const double* x, double* y, hipStream_t stream) {
  if (!ws.comp_q32 || !ws.comp_c) return hipErrorInvalidValue;
  if (!ws.s64 && ws.sym_part && (n & 3) == 0) {
    launch_tiles<true>(ws.s32, ws.comp_q32, n, ws.comp_c, ws.comp_v, ws.colmean, ws.stats, x, ws.sym_part, stream);
    return launch_symv_sym_gather(ws.sym_part, n, y, stream);
  }
  launch_rows<true>(ws.s32, ws.s64, ws.comp_q32, n, ws.comp_c, ws.comp_v, ws.colmean, ws.stats, x, y, stream);
  return hipGetLastError();
}

}  // namespace pcoa
