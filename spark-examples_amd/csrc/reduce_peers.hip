// reduce_peers.hip -- the chunk kernel of pcoa_gram_reduce_peers (capi_reduce.hip): S summed over the k engines of one process
// as a reduce-scatter.  The flat element range [0, N^2) of S is cut into k chunks of whole 16-byte quads (reduce_chunk below,
// the ONE statement of the partition); owner g runs reduce_chunk_kernel on its own stream over chunk g: every lane loads the
// same quad from all k matrices -- its own and the peers' --, sums, and stores into the owner's OWN matrix only.  A kernel that
// pulls from peers and writes local memory asks nothing of how a peer's L2 treats lines another device has written; the
// all-gather that follows is the runtime's copies.  No LDS, no atomics, no scratch: the source table is a kernel argument and is
// only ever indexed by unrolled constants.
#include "pcoa_ctx.h"

namespace pcoa {

void reduce_chunk(int32_t g, int32_t k, int32_t n, int64_t* first, int64_t* count) {
  const int64_t nn = (int64_t)n * n;
  const int64_t q = (nn + 3) / 4;                       // quads, the last one partial when N^2 % 4 != 0
  const int64_t lo = (int64_t)g * q / k * 4;
  const int64_t hi = std::min<int64_t>((int64_t)(g + 1) * q / k * 4, nn);   // the last owner's range ends with the tail elements
  *first = lo;
  *count = hi - lo;
}

namespace {

inline unsigned grid_for(int64_t count, int block, int64_t cap) {
  int64_t g = (count + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (unsigned)g;
}

template <typename OUT>
struct Quad { OUT x, y, z, w; };

__device__ __forceinline__ void store_quad(int32_t* dst, int64_t q, const Quad<int32_t>& a) {
  reinterpret_cast<int4*>(dst)[q] = make_int4(a.x, a.y, a.z, a.w);
}
__device__ __forceinline__ void store_quad(int64_t* dst, int64_t q, const Quad<int64_t>& a) {
  longlong2* d = reinterpret_cast<longlong2*>(dst) + 2 * q;
  d[0] = make_longlong2(a.x, a.y);
  d[1] = make_longlong2(a.z, a.w);
}

// first % 4 == 0: every matrix base is an allocation's start, so quad q0 + i is 16-byte aligned in all of them.  The loads of
// up to four sources (16 B of int32 each, 32 B more where a source has an int64 part) are issued before the first add.
template <typename OUT, bool HAS64>
__global__ __launch_bounds__(256) void reduce_chunk_kernel(ReduceSources src, OUT* dst, int64_t first, int64_t count) {
  const int k = src.k;
  const int64_t q0 = first >> 2, quads = count >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < quads; i += stride) {
    const int64_t q = q0 + i;
    Quad<OUT> a = {0, 0, 0, 0};
#pragma unroll
    for (int g0 = 0; g0 < PCOA_REDUCE_MAX_ENGINES; g0 += 4) {
      if (g0 < k) {
        int4 v[4];
        longlong2 w[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = make_int4(0, 0, 0, 0);
          if (g0 + j < k) v[j] = reinterpret_cast<const int4*>(src.s32[g0 + j])[q];
          if (HAS64) {
            w[j][0] = w[j][1] = make_longlong2(0, 0);
            if (g0 + j < k && src.s64[g0 + j]) {
              const longlong2* p = reinterpret_cast<const longlong2*>(src.s64[g0 + j]) + 2 * q;
              w[j][0] = p[0];
              w[j][1] = p[1];
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a.x += (OUT)v[j].x; a.y += (OUT)v[j].y; a.z += (OUT)v[j].z; a.w += (OUT)v[j].w;
          if (HAS64) {
            a.x += (OUT)w[j][0].x; a.y += (OUT)w[j][0].y; a.z += (OUT)w[j][1].x; a.w += (OUT)w[j][1].y;
          }
        }
      }
    }
    store_quad(dst, q, a);
  }
  // the N^2 % 4 elements behind the last whole quad (the last owner's chunk only), as scalars
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < (count & 3)) {
    const int64_t e = first + (quads << 2) + threadIdx.x;
    OUT a = 0;
#pragma unroll
    for (int g = 0; g < PCOA_REDUCE_MAX_ENGINES; ++g) {
      if (g < k) {
        a += (OUT)src.s32[g][e];
        if (HAS64 && src.s64[g]) a += (OUT)src.s64[g][e];
      }
    }
    dst[e] = a;
  }
}

template <typename OUT, bool HAS64>
hipError_t launch(const ReduceSources& src, OUT* dst, int64_t first, int64_t count, hipStream_t stream) {
  hipLaunchKernelGGL((reduce_chunk_kernel<OUT, HAS64>), dim3(grid_for((count + 3) / 4, 256, 8192)), dim3(256), 0, stream, src, dst,
                     first, count);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_reduce_chunk_i32(const ReduceSources& src, int32_t* dst, int64_t first, int64_t count, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  return launch<int32_t, false>(src, dst, first, count, stream);
}

hipError_t launch_reduce_chunk_i64(const ReduceSources& src, bool has64, int64_t* dst, int64_t first, int64_t count,
                                   hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  return has64 ? launch<int64_t, true>(src, dst, first, count, stream) : launch<int64_t, false>(src, dst, first, count, stream);
}

}  // namespace pcoa
