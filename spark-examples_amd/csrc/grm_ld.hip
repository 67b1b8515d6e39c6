// grm_ld.hip -- LD pruning of a GRM ctx's resident 2-bit store by the r^2 of the DOSAGES.  For two rows u < v of
// the store, over the samples J called at both (g the dosage 0 / 1 / 2, int64 throughout):
//   n = |J|,  s_u = sum g_u,  s_v = sum g_v,  q_u = sum g_u^2,  q_v = sum g_v^2,  p = sum g_u g_v
//   cov = n p - s_u s_v,  var_u = n q_u - s_u^2,  var_v = n q_v - s_v^2
//   exceeds(u, v)  <=>  (double)cov (double)cov > t ((double)var_u (double)var_v)
// -- three fp64 multiplications and one comparison, no sum: nothing a compiler could contract (ld.hip's comparison).  A pair with
// n = 0 or a row constant on J has cov = 0 and never exceeds.
//
// The six sums are popcounts of the store's words (coding: grm_bits.hip; 16 slots of 2 bits, 01 = not called).  With hi / both /
// called the slot masks of grm_slots.h (each at the slots' even bits), a row is DECODED once, on its way into LDS, to two words
//   X  = hi | both << 1       the dosage as a 2-bit number per slot: popc(X) = sum g
//   C2 = called | called << 1 both bits of every called slot
// and the target row of a lane derives  X' = both | hi << 1  (the two bits of X exchanged),  B = both  and  CH = called << 1  from
// them once per word, not once per distance.  Then, u the earlier row and v the target,
//   2 n       = popc(C2_u & C2_v)
//   s_u       = popc(X_u & C2_v)             s_v       = popc(X_v & C2_u)
//   q_u - s_u = 2 popc(X_u & CH_v)           q_v - s_v = 2 popc(B_v & C2_u)        (g^2 - g = 2 where g = 2: the slot's `both` bit)
//   p         = popc(X_u & X_v) + popc(X_u & X'_v)                                 ((hi_u + both_u)(hi_v + both_v) slot by slot)
// seven ANDs and seven popcounts per pair of words, six int32 accumulators per pair.  Slots of samples >= N and the pitch's
// padding hold 01: not called, X = C2 = 0, so nothing is masked.  int32 is enough for N < 2^28 (2 n and q - s stay below 2^31).
//
//   grm_ld_reach_kernel  reach[r] = min(W, rows between row r and the last break at or in front of it): the distances at which an
//                        earlier row exists for r.  Breaks are global row indices, sorted; a binary search per row.
//   grm_ld_band_kernel   the hot path, ld_band_kernel's shape with half its distances: a workgroup of four waves owns 64 target
//                        rows x 32 distances -- ONE band word per row -- and walks the sample axis in steps of GLD_KW = 8 store
//                        words (128 samples), staged decoded in LDS: the 64 target rows and the 95 rows before them that the 32
//                        distances reach.  Lane = target row; wave w takes the distances 8 w + 1 .. 8 w + 8 of the tile: 48
//                        accumulators, so the kernel stays far from spilling at several waves per SIMD (16 distances per wave
//                        would be 96).  A row is fetched once per 64 x 32 tile.  LDS rows are 16 decoded words at a pitch of 20
//                        (4 x odd), read as ds_read_b128 like ld.hip's.  The comparison is evaluated once per pair behind the
//                        last step, the four waves' bytes are joined through LDS, one owner per output word, no atomics.
// The work buffer is capi_ld.hip's arrangement: [W + C][pitch] store rows, the W rows in front of the chunk first (those that
// exist: reach says which).  The band words have ld_band_kernel's format, so the greedy pass and the scan are ld.hip's kernels,
// unchanged.  Integers only up to the comparison; the result is a function of the rows, W, t and the breaks alone, never of the grid.
#include "grm_slots.h"
#include "pcoa_internal.h"

namespace pcoa {

namespace {

constexpr int GLD_TR = 64;      // target rows of a band tile (one per lane)
constexpr int GLD_DT = 32;      // distances of a band tile (8 per wave): one band word
constexpr int GLD_DW = 8;       // distances a wave carries
constexpr int GLD_KW = 8;       // store words (16 samples each) of the sample axis staged per step
constexpr int GLD_PITCH = 20;   // words between LDS rows (2 GLD_KW decoded words + 4)

__global__ __launch_bounds__(256) void grm_ld_reach_kernel(const int64_t* __restrict__ breaks, int64_t n_breaks, int64_t g0, int64_t vc,
                                                           int32_t W, int32_t* __restrict__ reach) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= vc) return;
  const int64_t g = g0 + r;
  int64_t lo = 0, hi = n_breaks;   // the breaks [0, lo) are <= g
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (breaks[mid] <= g) lo = mid + 1; else hi = mid;
  }
  const int64_t start = lo > 0 ? breaks[lo - 1] : 0;
  reach[r] = (int32_t)min((int64_t)W, g - start);
}

struct Target {
  uint32_t x, c2, xs, b, ch;
};
__device__ __forceinline__ Target target_of(uint32_t x, uint32_t c2) {
  Target t;
  t.x = x;
  t.c2 = c2;
  t.b = (x >> 1) & kLo;
  t.xs = t.b | ((x & kLo) << 1);
  t.ch = c2 & ~kLo;
  return t;
}

// wb: [W + vc][pitch] store rows, row W the chunk's first; reach: [vc]; ex: [vc][ew] band words, ew = ceil(W / 32)
__global__ __launch_bounds__(256) void grm_ld_band_kernel(const uint32_t* __restrict__ wb, const int32_t* __restrict__ reach, int64_t vc,
                                                          int32_t pitch, int32_t W, double t, int32_t ew, uint32_t* __restrict__ ex) {
  __shared__ __attribute__((aligned(16))) uint32_t s_t[GLD_TR * GLD_PITCH];
  __shared__ __attribute__((aligned(16))) uint32_t s_p[(GLD_TR + GLD_DT) * GLD_PITCH];
  __shared__ uint32_t s_bits[GLD_TR][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * GLD_TR;
  const int32_t d0 = (int32_t)blockIdx.y * GLD_DT;
  // work-buffer row of LDS earlier-row slot 0: the row of target r0 at distance d0 + 32 (negative where W < d0 + 32)
  const int64_t pbase = (int64_t)W + r0 - d0 - GLD_DT;
  const int64_t wb_rows = (int64_t)W + vc;

  int32_t an[GLD_DW], asu[GLD_DW], aqu[GLD_DW], asv[GLD_DW], aqv[GLD_DW], ap[GLD_DW];
#pragma unroll
  for (int j = 0; j < GLD_DW; ++j) an[j] = asu[j] = aqu[j] = asv[j] = aqv[j] = ap[j] = 0;

  const int lw = tid & (GLD_KW - 1), lr = tid / GLD_KW;   // 32 rows of 8 words per sweep
  for (int32_t k0 = 0; k0 < pitch; k0 += GLD_KW) {
    const int32_t k = k0 + lw;
#pragma unroll
    for (int i = 0; i < (GLD_TR + GLD_TR + GLD_DT) / 32; ++i) {
      const int row = lr + 32 * i;
      int64_t src;
      uint32_t* dst;
      if (row < GLD_TR) {
        src = (int64_t)W + r0 + row;
        dst = s_t + row * GLD_PITCH + 2 * lw;
      } else {
        src = pbase + (row - GLD_TR);
        dst = s_p + (row - GLD_TR) * GLD_PITCH + 2 * lw;
      }
      uint32_t w = kLo;   // a row or a word that does not exist: nobody called
      if (k < pitch && src >= 0 && src < wb_rows) w = wb[src * pitch + k];
      uint32_t hi, both, called;
      slot_masks(w, hi, both, called);
      dst[0] = hi | (both << 1);
      dst[1] = called | (called << 1);
    }
    __syncthreads();
    const uint4* tp = reinterpret_cast<const uint4*>(s_t + lane * GLD_PITCH);
#pragma unroll
    for (int q = 0; q < GLD_KW / 2; ++q) {
      const uint4 tv = tp[q];
      const Target a = target_of(tv.x, tv.y), b = target_of(tv.z, tv.w);
#pragma unroll
      for (int j = 0; j < GLD_DW; ++j) {
        const int lp = lane + GLD_DT - (wv * GLD_DW + j + 1);   // 0 .. 94
        const uint4 u = reinterpret_cast<const uint4*>(s_p + lp * GLD_PITCH)[q];
        an[j] += __popc(u.y & a.c2) + __popc(u.w & b.c2);
        asu[j] += __popc(u.x & a.c2) + __popc(u.z & b.c2);
        aqu[j] += __popc(u.x & a.ch) + __popc(u.z & b.ch);
        asv[j] += __popc(a.x & u.y) + __popc(b.x & u.w);
        aqv[j] += __popc(a.b & u.y) + __popc(b.b & u.w);
        ap[j] += __popc(u.x & a.x) + __popc(u.x & a.xs) + __popc(u.z & b.x) + __popc(u.z & b.xs);
      }
    }
    __syncthreads();
  }

  const int64_t r = r0 + lane;
  uint32_t bits = 0;
  if (r < vc) {
    const int32_t rc = reach[r];
#pragma unroll
    for (int j = 0; j < GLD_DW; ++j) {
      const int32_t d = d0 + wv * GLD_DW + j + 1;
      if (d <= rc) {
        const int64_t n = an[j] >> 1, su = asu[j], sv = asv[j], p = ap[j];
        const int64_t qu = su + 2 * (int64_t)aqu[j], qv = sv + 2 * (int64_t)aqv[j];
        const int64_t cov = n * p - su * sv;
        const int64_t var_u = n * qu - su * su, var_v = n * qv - sv * sv;
        const double lhs = __dmul_rn((double)cov, (double)cov);
        const double rhs = __dmul_rn(t, __dmul_rn((double)var_u, (double)var_v));
        if (lhs > rhs) bits |= 1u << j;
      }
    }
  }
  s_bits[lane][wv] = bits;
  __syncthreads();
  if (tid < GLD_TR) {
    const int32_t word = (int32_t)blockIdx.y;
    if (r0 + tid < vc && word < ew)
      ex[(r0 + tid) * ew + word] = s_bits[tid][0] | (s_bits[tid][1] << 8) | (s_bits[tid][2] << 16) | (s_bits[tid][3] << 24);
  }
}

}  // namespace

int32_t grm_ld_band_tile_rows() { return GLD_TR; }
int32_t grm_ld_band_chunk_samples() { return GLD_KW * 16; }

hipError_t launch_grm_ld_reach(const int64_t* breaks, int64_t n_breaks, int64_t g0, int64_t vc, int32_t window, int32_t* reach,
                               hipStream_t stream) {
  if (vc <= 0) return hipSuccess;
  grm_ld_reach_kernel<<<dim3((unsigned)((vc + 255) / 256)), 256, 0, stream>>>(breaks, n_breaks, g0, vc, window, reach);
  return hipGetLastError();
}

hipError_t launch_grm_ld_band(const uint32_t* wb, const int32_t* reach, int64_t vc, int32_t n, int32_t window, double t, uint32_t* ex,
                              hipStream_t stream) {
  if (vc <= 0) return hipSuccess;
  const int32_t ew = (window + 31) / 32;
  const dim3 grid((unsigned)((vc + GLD_TR - 1) / GLD_TR), (unsigned)((window + GLD_DT - 1) / GLD_DT));
  grm_ld_band_kernel<<<grid, 256, 0, stream>>>(wb, reach, vc, grm_pitch_words(n), window, t, ew, ex);
  return hipGetLastError();
}

}  // namespace pcoa
