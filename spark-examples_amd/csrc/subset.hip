// subset.hip -- S of a sample subset: dst[a][b] = src[keep[a]][keep[b]] (pcoa_create_subset).
// For a kept index set I, S[I, I] IS the similarity matrix of the reduced cohort, so an outlier-removal round costs one gather
// of S instead of one Gram.  A pure memory kernel: every entry of dst is written exactly once, no atomics, no LDS, no scratch.
//
// A workgroup takes a band of kSubsetBandRows dst rows x a tile of kSubsetTileCols dst columns.  A lane owns the columns
// tile0 + t + 256 j (j = 0..3): it loads their source columns keep[b] once and keeps them in registers across the band.  The
// source row keep[a] is the same for the whole workgroup (a scalar load).  Every store instruction of a wave writes 64
// consecutive dwords (or qwords) of one dst row: stores are dwords on purpose -- the dst row pitch, 4 m bytes, is 16-byte
// aligned only when m % 4 == 0, and 256 contiguous bytes per wave-instruction already store at the rate of wider ones.  The
// loads are a gather along the source row: for the intended use (keep almost the identity: a few removed samples shift the
// columns by a small offset) a wave's 64 loads fall into two or three consecutive 128-byte lines; for a sparse keep set
// they are only correct, not fast.  Every offset is 64-bit: keep[a] * n + keep[b] and a * m + b pass 2^31 from N = 46,341.
#include "pcoa_internal.h"

namespace pcoa {
namespace {

constexpr int kSubsetThreads = 256;
constexpr int kSubsetColsPerLane = kSubsetTileCols / kSubsetThreads;
constexpr int kSubsetRowsInFlight = 4;
static_assert(kSubsetTileCols % kSubsetThreads == 0, "a lane owns a whole number of columns");

template <typename T>
__global__ __launch_bounds__(kSubsetThreads) void subset_gather_kernel(const T* __restrict__ src, int32_t n,
                                                                       const int32_t* __restrict__ keep, int32_t m,
                                                                       T* __restrict__ dst) {
  const int32_t b0 = (int32_t)blockIdx.x * kSubsetTileCols + (int32_t)threadIdx.x;
  int32_t kc[kSubsetColsPerLane];
#pragma unroll
  for (int j = 0; j < kSubsetColsPerLane; ++j) {
    const int32_t b = b0 + j * kSubsetThreads;
    kc[j] = b < m ? keep[b] : 0;   // (column 0 exists in every source; the store below is masked)
  }
  const int32_t nbands = (m + kSubsetBandRows - 1) / kSubsetBandRows;
  // grid.y strides over the row bands so that the launch stays inside the grid limits whatever m is
  for (int32_t band = (int32_t)blockIdx.y; band < nbands; band += (int32_t)gridDim.y) {
    const int32_t a0 = band * kSubsetBandRows;
    const int32_t a1 = a0 + kSubsetBandRows < m ? a0 + kSubsetBandRows : m;
    int32_t a = a0;
    // kSubsetRowsInFlight rows at a time: their loads are all issued before the first store (16 gathered values per lane in
    // flight), then the rows that are left one by one
    for (; a + kSubsetRowsInFlight <= a1; a += kSubsetRowsInFlight) {
      T v[kSubsetRowsInFlight][kSubsetColsPerLane];
#pragma unroll
      for (int r = 0; r < kSubsetRowsInFlight; ++r) {
        const T* __restrict__ srow = src + (int64_t)keep[a + r] * (int64_t)n;   // uniform over the workgroup
#pragma unroll
        for (int j = 0; j < kSubsetColsPerLane; ++j) v[r][j] = srow[kc[j]];
      }
#pragma unroll
      for (int r = 0; r < kSubsetRowsInFlight; ++r) {
        T* __restrict__ drow = dst + (int64_t)(a + r) * (int64_t)m;
#pragma unroll
        for (int j = 0; j < kSubsetColsPerLane; ++j) {
          const int32_t b = b0 + j * kSubsetThreads;
          if (b < m) drow[b] = v[r][j];
        }
      }
    }
    for (; a < a1; ++a) {
      const T* __restrict__ srow = src + (int64_t)keep[a] * (int64_t)n;
      T* __restrict__ drow = dst + (int64_t)a * (int64_t)m;
      T v[kSubsetColsPerLane];
#pragma unroll
      for (int j = 0; j < kSubsetColsPerLane; ++j) v[j] = srow[kc[j]];
#pragma unroll
      for (int j = 0; j < kSubsetColsPerLane; ++j) {
        const int32_t b = b0 + j * kSubsetThreads;
        if (b < m) drow[b] = v[j];
      }
    }
  }
}

template <typename T>
hipError_t launch_subset_gather(const T* src, int32_t n, const int32_t* keep_dev, int32_t m, T* dst, hipStream_t stream) {
  if (m <= 0 || n <= 0 || m > n) return hipErrorInvalidValue;
  const unsigned gx = (unsigned)((m + kSubsetTileCols - 1) / kSubsetTileCols);
  const unsigned bands = (unsigned)((m + kSubsetBandRows - 1) / kSubsetBandRows);
  const unsigned gy = bands < 65535u ? bands : 65535u;
  hipLaunchKernelGGL(subset_gather_kernel<T>, dim3(gx, gy), dim3(kSubsetThreads), 0, stream, src, n, keep_dev, m, dst);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_subset_gather_i32(const int32_t* src, int32_t n, const int32_t* keep_dev, int32_t m, int32_t* dst,
                                    hipStream_t stream) {
  return launch_subset_gather<int32_t>(src, n, keep_dev, m, dst, stream);
}

hipError_t launch_subset_gather_i64(const int64_t* src, int32_t n, const int32_t* keep_dev, int32_t m, int64_t* dst,
                                    hipStream_t stream) {
  return launch_subset_gather<int64_t>(src, n, keep_dev, m, dst, stream);
}

}  // namespace pcoa
