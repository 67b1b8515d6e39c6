// measure.hip -- principal coordinates of a NORMALISED similarity, evaluated on the fly from the integer S.
// computePca (reference VariantsPca.scala:198-231) centres and decomposes the shared-carrier counts S(i, j); a count scales
// with how many variants each of the two samples carries, d_i = S(i, i).  The kernels here put one per-entry map in front of
// the centring, in the places where the Lanczos forms already evaluate the centred entry from the integer S:
//
//   Jaccard  U = d_i + d_j - S(i, j) (int64);   K(i, j) = U > 0 ? (double)S(i, j) / (double)U : 0.0      one fp64 division
//   cosine   q_i = d_i > 0 ? 1.0 / sqrt((double)d_i) : 0.0;   K(i, j) = ((double)S(i, j) * q_i) * q_j    (Ochiai)
//   centred  B(i, j) = ((K(i, j) - r_i / N) - r_j / N) + mm,   r = row sums of K,   mm = (sum_i r_i) / N / N
//
// with S(i, j) the TOTAL entry (int32 matrix plus the int64 part where there is one), IEEE fp64 and no contraction anywhere:
// variants_pca.py's similarity_measure / centred_measure are the numpy statement.  K is never in memory; the N x N fp64 B
// exists only for the dense solver and pcoa_center_read_f64.  The kernels are twins of the shared-count ones and share their
// loop shapes through symv_shared.h: the row form is row_dot's association, the upper-triangle form writes the partials
// symv_sym_gather_kernel adds.  Plain HIP, fp64, no floating-point atomics, no scratch.
#include "pcoa_internal.h"
#include "symv_shared.h"

namespace pcoa {
namespace {

constexpr int JAC = PCOA_SIMILARITY_JACCARD, COS = PCOA_SIMILARITY_COSINE;

// The rule, once per measure.  T = what a sample contributes (d_i, or q_i): 8 bytes either way, so both are staged and
// loaded alike.  k(s, sd, pi, pj): s the total entry, sd = (double)s (the caller converts: from the int32 word where there is
// no int64 part), pi the ROW's and pj the COLUMN's value.
template <int M> struct Rule;
template <> struct Rule<JAC> {
  typedef int64_t T;
  typedef longlong2 T2;
  static __device__ __forceinline__ const T* per_sample(const int64_t* diag, const double*) { return diag; }
  static __device__ __forceinline__ double k(int64_t s, double sd, T di, T dj) {
    const int64_t u = di + dj - s;
    return u > 0 ? sd / (double)u : 0.0;
  }
};
template <> struct Rule<COS> {
  typedef double T;
  typedef double2 T2;
  static __device__ __forceinline__ const T* per_sample(const int64_t*, const double* q) { return q; }
  static __device__ __forceinline__ double k(int64_t, double sd, T qi, T qj) {
#pragma clang fp contract(off)
    double t = sd * qi;
    t = t * qj;
    return t;
  }
};

// d_i = the total diagonal entry; cosine: q_i as well.  N values, once per centring
__global__ __launch_bounds__(256) void measure_diag_kernel(const int32_t* __restrict__ s32, const int64_t* __restrict__ s64, int32_t n,
                                                           int64_t* __restrict__ diag, double* __restrict__ q) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t idx = (int64_t)i * n + i;
  const int64_t d = (int64_t)s32[idx] + (s64 ? s64[idx] : 0);
  diag[i] = d;
  if (q) q[i] = d > 0 ? 1.0 / sqrt((double)d) : 0.0;
}

__global__ __launch_bounds__(256) void measure_fill_kernel(double* __restrict__ x, int32_t n, double value) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = value;
}

// ---- row forms: one wave per row, row_dot's loop shape (16-byte loads when N % 4 == 0, 4-byte loads otherwise; the same
// main-loop bounds).  CENTRE: y = B x.  !CENTRE: y = K x -- with x = 1 the row sums of K, added in row_dot's order: per lane
// four accumulators over the columns 4 lane + 1024 t + {0, 256, 512, 768} + e (e = accumulator; pairs (0, 512) and (256, 768)
// first), the tail's 256-column groups in order, (acc0 + acc1) + (acc2 + acc3), then the 64 lanes by halving strides.
template <int M, bool HAS64, bool CENTRE>
__global__ __launch_bounds__(256) void measure_symv_rows_kernel(const int32_t* __restrict__ s32, const int64_t* __restrict__ s64,
                                                                int n, const int64_t* __restrict__ diag,
                                                                const double* __restrict__ qv, const double* __restrict__ cm,
                                                                const double* __restrict__ stats, const double* __restrict__ x,
                                                                double* __restrict__ y) {
  typedef typename Rule<M>::T T;
  typedef typename Rule<M>::T2 T2;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const T* __restrict__ ps = Rule<M>::per_sample(diag, qv);
  const int64_t base = (int64_t)i * n;
  const T pi = ps[i];
  const double row_mean = CENTRE ? cm[i] : 0.0;
  const double mmean = CENTRE ? stats[1] : 0.0;
  auto entry = [&](int64_t s, double sd, T pj, double col_mean) -> double {
#pragma clang fp contract(off)
    double t = Rule<M>::k(s, sd, pi, pj);
    if (CENTRE) {
      t = t - row_mean;
      t = t - col_mean;
      t = t + mmean;
    }
    return t;
  };
  auto quad = [&](int j, double* out) {
    const int4 s = *reinterpret_cast<const int4*>(s32 + base + j);
    int64_t t0 = s.x, t1 = s.y, t2 = s.z, t3 = s.w;
    double d0 = (double)s.x, d1 = (double)s.y, d2 = (double)s.z, d3 = (double)s.w;
    if (HAS64) {
      const longlong2 l = *reinterpret_cast<const longlong2*>(s64 + base + j);
      const longlong2 h = *reinterpret_cast<const longlong2*>(s64 + base + j + 2);
      t0 += l.x; t1 += l.y; t2 += h.x; t3 += h.y;
      d0 = (double)t0; d1 = (double)t1; d2 = (double)t2; d3 = (double)t3;
    }
    const T2 pa = *reinterpret_cast<const T2*>(ps + j), pb = *reinterpret_cast<const T2*>(ps + j + 2);
    double2 ca = make_double2(0.0, 0.0), cb = make_double2(0.0, 0.0);
    if (CENTRE) {
      ca = *reinterpret_cast<const double2*>(cm + j);
      cb = *reinterpret_cast<const double2*>(cm + j + 2);
    }
    out[0] = entry(t0, d0, pa.x, ca.x); out[1] = entry(t1, d1, pa.y, ca.y);
    out[2] = entry(t2, d2, pb.x, cb.x); out[3] = entry(t3, d3, pb.y, cb.y);
  };
  auto one = [&](int j) -> double {
    const int64_t s = HAS64 ? (int64_t)s32[base + j] + s64[base + j] : (int64_t)s32[base + j];
    const double sd = HAS64 ? (double)s : (double)s32[base + j];
    return entry(s, sd, ps[j], CENTRE ? cm[j] : 0.0);
  };
  const double acc = row_dot(quad, one, x, n, lane);
  if (lane == 0) y[i] = acc;
}

// ---- upper-triangle form: symv_sym_tile_body's decomposition (1024 x 1024 tiles, a 2 x 2 wave grid, a lane owns 8 columns,
// rows prefetched four deep, interior tiles without masks, DPP row sums, partials into `part` for symv_sym_gather_kernel).
// Beside x_i and rowMean_i the tile's d_i (q_i) are staged in LDS, the lane's eight d_j (q_j) stay in registers.  K(i, j) is
// evaluated ONCE per loaded entry, with i the row: B(i, j) and B(j, i) both come from it (for the cosine, whose two products
// do not commute in the last bit, the lower triangle takes the upper one's K).  All offsets into S are 64-bit.
template <int M, bool CENTRE, bool DIAG, bool EDGE>
__device__ __forceinline__ void measure_sym_tile_body(const int32_t* __restrict__ s32, int n, int nb,
                                                      const typename Rule<M>::T* __restrict__ ps, const double* __restrict__ cm,
                                                      const double mmean, const double* __restrict__ x, double* __restrict__ part,
                                                      int bi, int bj, double* xs, double* ms, typename Rule<M>::T* pr,
                                                      double (*rs)[SYT]) {
  typedef typename Rule<M>::T T;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int i0 = bi * SYT, j0 = bj * SYT;
  const int jw = j0 + 512 * wc + 4 * lane;   // the lane's 8 columns: jw + 256 q + {0..3}
  const int rows = EDGE ? min(SYT, n - i0) : SYT;
  for (int r = threadIdx.x; r < SYT; r += 256) {
    const bool in = !EDGE || i0 + r < n;
    xs[r] = in ? x[i0 + r] : 0.0;
    if (CENTRE) ms[r] = in ? cm[i0 + r] : 0.0;
    pr[r] = in ? ps[i0 + r] : (T)0;
  }
  double xj[8], mj[8], cacc[8];
  T pj[8];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = jw + 256 * q + e;
      const bool in = !EDGE || j < n;
      xj[4 * q + e] = in ? x[j] : 0.0;
      mj[4 * q + e] = (CENTRE && in) ? cm[j] : 0.0;
      pj[4 * q + e] = in ? ps[j] : (T)0;
      cacc[4 * q + e] = 0.0;
    }
  __syncthreads();
  const int32_t* base = s32 + (int64_t)i0 * n + jw;
  auto load_row = [&](int r, int4 (&v)[2]) {
    const int32_t* rowp = base + (int64_t)r * n;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (EDGE) {
        const bool in = r < rows && jw + 256 * q < n;   // n % 4 == 0: a quad is whole or absent
        v[q] = in ? *reinterpret_cast<const int4*>(rowp + 256 * q) : make_int4(0, 0, 0, 0);
      } else {
        v[q] = *reinterpret_cast<const int4*>(rowp + 256 * q);
      }
    }
  };
  auto use_row = [&](int r, const int4 (&v)[2]) {
    const int i = i0 + r;
    const double xi = xs[r], mi = CENTRE ? ms[r] : 0.0;
    const T pi = pr[r];
    double racc = 0.0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int sv[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = jw + 256 * q + e;
        const double kij = Rule<M>::k((int64_t)sv[e], (double)sv[e], pi, pj[4 * q + e]);
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
          // (columns >= n of the last block column: x, S and d were read as 0 but the centred entry is not 0 -> mask)
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
  // rows wr, wr + 2, ..: SYNB buffers, each refilled as soon as its row is used
  int4 buf[SYNB][2];
  const int nr = rows > wr ? (rows - wr + 1) / 2 : 0;   // this wave's row count
#pragma unroll
  for (int b = 0; b < SYNB; ++b)
    if (b < nr) load_row(wr + 2 * b, buf[b]);
  int k = 0;
  for (; k + 2 * SYNB <= nr; k += SYNB) {   // every refill is a row of the tile: no conditions in the steady state
#pragma unroll
    for (int b = 0; b < SYNB; ++b) {
      use_row(wr + 2 * (k + b), buf[b]);
      load_row(wr + 2 * (k + b + SYNB), buf[b]);
    }
  }
#pragma unroll
  for (int b = 0; b < SYNB; ++b)   // the last < 2 SYNB rows
    if (k + b < nr) {
      use_row(wr + 2 * (k + b), buf[b]);
      if (k + b + SYNB < nr) load_row(wr + 2 * (k + b + SYNB), buf[b]);
    }
  k += SYNB;
#pragma unroll
  for (int b = 0; b < SYNB; ++b)
    if (k + b < nr) use_row(wr + 2 * (k + b), buf[b]);
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
// 40 KiB of LDS (x_i, rowMean_i, d_i | q_i: 24 KiB; the row sums of the two column halves: 16 KiB): four workgroups per CU
template <int M, bool CENTRE>
__global__ __launch_bounds__(256) void measure_symv_sym_tiles_kernel(const int32_t* __restrict__ s32, int n, int nb, int nbi,
                                                                     const int64_t* __restrict__ diag, const double* __restrict__ qv,
                                                                     const double* __restrict__ cm, const double* __restrict__ stats,
                                                                     const double* __restrict__ x, double* __restrict__ part) {
  typedef typename Rule<M>::T T;
  __shared__ double xs[SYT], ms[SYT];
  __shared__ T pr[SYT];
  __shared__ double rs[2][SYT];
  const T* __restrict__ ps = Rule<M>::per_sample(diag, qv);
  const double mmean = CENTRE ? stats[1] : 0.0;
  int t = blockIdx.x;
  const int edge = nb - nbi;           // 0 or 1
  if (t < edge) {
    measure_sym_tile_body<M, CENTRE, true, true>(s32, n, nb, ps, cm, mmean, x, part, nb - 1, nb - 1, xs, ms, pr, rs);
    return;
  }
  t -= edge;
  if (t < nbi) {
    measure_sym_tile_body<M, CENTRE, true, false>(s32, n, nb, ps, cm, mmean, x, part, t, t, xs, ms, pr, rs);
    return;
  }
  t -= nbi;
  if (t < edge * (nb - 1)) {
    measure_sym_tile_body<M, CENTRE, false, true>(s32, n, nb, ps, cm, mmean, x, part, t, nb - 1, xs, ms, pr, rs);
    return;
  }
  t -= edge * (nb - 1);
  int bi = 0;
  while (t >= nbi - 1 - bi) {
    t -= nbi - 1 - bi;
    ++bi;
  }
  measure_sym_tile_body<M, CENTRE, false, false>(s32, n, nb, ps, cm, mmean, x, part, bi, bi + 1 + t, xs, ms, pr, rs);
}

// single workgroup: the sum of the row sums in ONE fixed order (thread t adds i = t, t + 256, .. in order; the 64 lanes of a
// wave by halving strides; the four waves left to right), the mean by the two divisions stats_kernel performs, #{r_i > 0}
__global__ __launch_bounds__(256) void measure_stats_kernel(const double* __restrict__ row_sums, int32_t n,
                                                            double* __restrict__ stats, int32_t* __restrict__ nz) {
#pragma clang fp contract(off)
  __shared__ double part[4];
  __shared__ int cnt[4];
  double acc = 0.0;
  int c = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double r = row_sums[i];
    acc += r;
    c += (r > 0.0) ? 1 : 0;
  }
  acc = wave_sum(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6] = acc;
    cnt[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double msum = ((part[0] + part[1]) + part[2]) + part[3];
    const double rc = (double)n;
    stats[0] = msum;
    stats[1] = msum / rc / rc;
    nz[0] = ((cnt[0] + cnt[1]) + cnt[2]) + cnt[3];
  }
}

// B for the dense solver and pcoa_center_read_f64.  One workgroup per row, striding over the columns: the dispatch stays at
// N x 256 work-items (center_kernel's comment: a block per (row, 256-column chunk) overflows the 32-bit work-item count of a
// dispatch at N = 100,000)
template <int M>
__global__ __launch_bounds__(256) void measure_center_kernel(const int32_t* __restrict__ s32, const int64_t* __restrict__ s64,
                                                             int32_t n, const int64_t* __restrict__ diag,
                                                             const double* __restrict__ qv, const double* __restrict__ cm,
                                                             const double* __restrict__ stats, double* __restrict__ b) {
#pragma clang fp contract(off)
  typedef typename Rule<M>::T T;
  const T* __restrict__ ps = Rule<M>::per_sample(diag, qv);
  const int i = blockIdx.x;
  const T pi = ps[i];
  const double row_mean = cm[i];
  const double mmean = stats[1];
  for (int j = threadIdx.x; j < n; j += 256) {
    const int64_t idx = (int64_t)i * n + j;
    const int64_t s = (int64_t)s32[idx] + (s64 ? s64[idx] : 0);
    double t = Rule<M>::k(s, (double)s, pi, ps[j]);
    t = t - row_mean;
    t = t - cm[j];
    t = t + mmean;
    b[idx] = t;
  }
}

template <int M, bool CENTRE>
void launch_rows(const int32_t* s32, const int64_t* s64, int n, const int64_t* diag, const double* q, const double* cm,
                 const double* stats, const double* x, double* y, hipStream_t stream) {
  const unsigned rows4 = (unsigned)((n + 3) / 4);
  if (s64)
    hipLaunchKernelGGL((measure_symv_rows_kernel<M, true, CENTRE>), dim3(rows4), dim3(256), 0, stream, s32, s64, n, diag, q, cm,
                       stats, x, y);
  else
    hipLaunchKernelGGL((measure_symv_rows_kernel<M, false, CENTRE>), dim3(rows4), dim3(256), 0, stream, s32, s64, n, diag, q, cm,
                       stats, x, y);
}

template <int M, bool CENTRE>
void launch_tiles(const int32_t* s32, int n, const int64_t* diag, const double* q, const double* cm, const double* stats,
                  const double* x, double* part, hipStream_t stream) {
  const int nb = (n + SYT - 1) / SYT;
  const int nbi = n / SYT;   // block columns wholly inside N (nb or nb - 1)
  hipLaunchKernelGGL((measure_symv_sym_tiles_kernel<M, CENTRE>), dim3((unsigned)((int64_t)nb * (nb + 1) / 2)), dim3(256), 0, stream,
                     s32, n, nb, nbi, diag, q, cm, stats, x, part);
}

inline bool known(int kind) { return kind == JAC || kind == COS; }

}  // namespace

hipError_t launch_measure_diag(const int32_t* s32, const int64_t* s64_or_null, int32_t n, int kind, int64_t* diag, double* q,
                               hipStream_t stream) {
  if (!known(kind) || (kind == COS && !q)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(measure_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, s32, s64_or_null, n, diag,
                     kind == COS ? q : nullptr);
  return hipGetLastError();
}

hipError_t launch_measure_row_sums(const int32_t* s32, const int64_t* s64_or_null, int32_t n, int kind, const int64_t* diag,
                                   const double* q, double* ones, double* row_sums, hipStream_t stream) {
  if (!known(kind)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(measure_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ones, n, 1.0);
  if (kind == JAC) launch_rows<JAC, false>(s32, s64_or_null, n, diag, q, nullptr, nullptr, ones, row_sums, stream);
  else launch_rows<COS, false>(s32, s64_or_null, n, diag, q, nullptr, nullptr, ones, row_sums, stream);
  return hipGetLastError();
}

hipError_t launch_measure_row_sums_sym(const int32_t* s32, int32_t n, int kind, const int64_t* diag, const double* q,
                                       double* ones, double* sym_part, double* row_sums, hipStream_t stream) {
  if (!known(kind) || (n & 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(measure_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ones, n, 1.0);
  if (kind == JAC) launch_tiles<JAC, false>(s32, n, diag, q, nullptr, nullptr, ones, sym_part, stream);
  else launch_tiles<COS, false>(s32, n, diag, q, nullptr, nullptr, ones, sym_part, stream);
  return launch_symv_sym_gather(sym_part, n, row_sums, stream);
}

hipError_t launch_measure_stats(const double* row_sums, int32_t n, double* stats, int32_t* nz, hipStream_t stream) {
  hipLaunchKernelGGL(measure_stats_kernel, dim3(1), dim3(256), 0, stream, row_sums, n, stats, nz);
  return hipGetLastError();
}

hipError_t launch_measure_center(const int32_t* s32, const int64_t* s64_or_null, int32_t n, int kind, const int64_t* diag,
                                 const double* q, const double* cm, const double* stats, double* b, hipStream_t stream) {
  if (!known(kind)) return hipErrorInvalidValue;
  if (kind == JAC)
    hipLaunchKernelGGL(measure_center_kernel<JAC>, dim3((unsigned)n), dim3(256), 0, stream, s32, s64_or_null, n, diag, q, cm, stats, b);
  else
    hipLaunchKernelGGL(measure_center_kernel<COS>, dim3((unsigned)n), dim3(256), 0, stream, s32, s64_or_null, n, diag, q, cm, stats, b);
  return hipGetLastError();
}

hipError_t launch_measure_symv(const EigWorkspace& ws, int32_t n, const double* x, double* y, hipStream_t stream) {
  if (!known(ws.measure)) return hipErrorInvalidValue;
  if (!ws.s64 && ws.sym_part && (n & 3) == 0) {
    if (ws.measure == JAC) launch_tiles<JAC, true>(ws.s32, n, ws.diag, ws.qcos, ws.colmean, ws.stats, x, ws.sym_part, stream);
    else launch_tiles<COS, true>(ws.s32, n, ws.diag, ws.qcos, ws.colmean, ws.stats, x, ws.sym_part, stream);
    return launch_symv_sym_gather(ws.sym_part, n, y, stream);
  }
  if (ws.measure == JAC) launch_rows<JAC, true>(ws.s32, ws.s64, n, ws.diag, ws.qcos, ws.colmean, ws.stats, x, y, stream);
  else launch_rows<COS, true>(ws.s32, ws.s64, n, ws.diag, ws.qcos, ws.colmean, ws.stats, x, y, stream);
  return hipGetLastError();
}

}  // namespace pcoa
