// ld.hip -- linkage-disequilibrium pruning of variant rows in front of the accumulation.  Rows are carrier
// bitsets (sample i = bit (i & 31) of word i >> 5).  With n samples, a_v the carrier count of row v and c_uv = popcount(row_u &
// row_v), both over samples < n,
//   D = n c_uv - a_u a_v,  p = a_u (n - a_u),  q = a_v (n - a_v)  (int64),   exceeds(u, v)  <=>  (double)D (double)D > t ((double)p (double)q)
// -- three fp64 multiplications and one comparison, no sum: nothing a compiler could contract, so the bit is the one numpy gives.
//
// The kernels work on the pruner's WORK BUFFER wb: [W + C][words] dense rows, words = ceil(n / 32), tail bits cleared.  Rows
// [0, W) are the carried tail (the last T <= W rows of earlier calls, at [W - T, W)), rows [W, W + vc) the rows of this chunk;
// cnt[W + C] holds the carrier counts the same way.  Row r of the chunk and distance d name the earlier row wb[W + r - d], which
// exists iff d <= r + T.
//
//   ld_count_kernel    one wave per row: the row, last word masked, into wb; a_v into cnt.
//   ld_band_kernel     the hot path.  A workgroup of four waves owns 64 target rows x 64 distances and walks the sample axis in
//                      chunks of LD_KC = 16 words, staged once in LDS: the 64 target rows and the 127 rows before them that the
//                      64 distances reach.  Lane = target row; wave w takes the distances 16 w + 1 .. 16 w + 16 of the tile, one
//                      int32 accumulator each.  A row is therefore fetched once per 64 x 64 tile, not once per distance, and the
//                      inner loop is ds_read_b128 of the earlier row's words, v_and_b32 and an accumulating v_bcnt_u32_b32.
//                      LDS rows have a pitch of 20 words (4 x odd): the 16 lanes of a ds_read_b128 group, on consecutive rows,
//                      cover the 64 banks once.  The comparison is evaluated once per pair behind the last chunk, the 16 bits of
//                      a lane are joined with the other waves' through LDS, and the workgroup stores words 2 y, 2 y + 1 of its
//                      rows' band bits (bit d - 1 of the row: distance d).  No atomics; every output word has one owner.
//   ld_resolve_kernel  the greedy pass, one wave.  Lane j holds the keep flags of the 32-row block B - j (B the current row's
//                      block), the flag of row u at bit 31 - (u & 31); a row's band words are shifted to that alignment from
//                      two plain reads (no cross-lane traffic), ANDed with the flags, and one ballot says whether a kept
//                      earlier row exceeds.  The flags move up one lane every 32 rows.  Band words and counts reach the wave
//                      through LDS a tile at a time, the next tile's loads in flight meanwhile.
//   ld_scan_kernel     one workgroup: the keep flags as bytes, the place of every kept row among the kept rows of the chunk,
//                      the kept and monomorphic counts.
//   ld_gather_kernel   one wave per row: kept rows, in order, into the compacted buffer.
// Integers only; the result of every kernel is a function of the rows, W, t and T alone, never of the grid or the CU count.
#include "pcoa_internal.h"

namespace pcoa {

namespace {

constexpr int LD_TR = 64;      // target rows of a band tile (one per lane)
constexpr int LD_DT = 64;      // distances of a band tile (16 per wave)
constexpr int LD_KC = 16;      // words of the sample axis staged per step
constexpr int LD_PITCH = 20;   // words between LDS rows
constexpr int LD_RS_WORDS = 2048;   // band words of a resolve tile in LDS (and counts: a tile has at most as many rows)
constexpr int LD_SCAN_THREADS = 1024;

__global__ __launch_bounds__(256) void ld_count_kernel(const uint32_t* __restrict__ rows, int64_t ld, int64_t vc, int32_t words,
                                                       uint32_t last_mask, uint32_t* __restrict__ wb_rows, int32_t* __restrict__ cnt_rows) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= vc) return;
  const uint32_t* src = rows + r * ld;
  uint32_t* dst = wb_rows + r * words;
  int32_t a = 0;
  for (int32_t k = lane; k < words; k += 64) {
    uint32_t w = src[k];
    if (k == words - 1) w &= last_mask;
    dst[k] = w;
    a += __popc(w);
  }
  for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
  if (lane == 0) cnt_rows[r] = a;
}

__device__ __forceinline__ int32_t and_popc4(const uint4 a, const uint4 b, int32_t acc) {
  acc += __popc(a.x & b.x);
  acc += __popc(a.y & b.y);
  acc += __popc(a.z & b.z);
  acc += __popc(a.w & b.w);
  return acc;
}

// wb / cnt: the whole work buffer (row 0 = first tail slot).  ex: [vc][ew] band words, ew = ceil(W / 32)
__global__ __launch_bounds__(256) void ld_band_kernel(const uint32_t* __restrict__ wb, const int32_t* __restrict__ cnt, int64_t vc,
                                                      int32_t words, int32_t W, int32_t T, int32_t n, double t, int32_t ew,
                                                      uint32_t* __restrict__ ex) {
  __shared__ __attribute__((aligned(16))) uint32_t s_t[LD_TR * LD_PITCH];
  __shared__ __attribute__((aligned(16))) uint32_t s_p[(LD_TR + LD_DT) * LD_PITCH];
  __shared__ uint32_t s_bits[LD_TR][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * LD_TR;
  const int32_t d0 = (int32_t)blockIdx.y * LD_DT;
  // work-buffer row of LDS earlier-row slot 0: the row of target r0 at distance d0 + 64 (negative where W < d0 + 64)
  const int64_t pbase = (int64_t)W + r0 - d0 - LD_DT;
  const int64_t wb_rows = (int64_t)W + vc;

  int32_t acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0;

  const int lw = tid & 15, lr = tid >> 4;
  for (int32_t k0 = 0; k0 < words; k0 += LD_KC) {
    const int32_t k = k0 + lw;
#pragma unroll
    for (int i = 0; i < (LD_TR + LD_TR + LD_DT) / 16; ++i) {
      const int row = lr + 16 * i;
      int64_t src;
      uint32_t* dst;
      if (row < LD_TR) {
        src = (int64_t)W + r0 + row;
        dst = s_t + row * LD_PITCH + lw;
      } else {
        src = pbase + (row - LD_TR);
        dst = s_p + (row - LD_TR) * LD_PITCH + lw;
      }
      uint32_t w = 0;
      if (k < words && src >= 0 && src < wb_rows) w = wb[src * words + k];
      *dst = w;
    }
    __syncthreads();
    const uint4* tp = reinterpret_cast<const uint4*>(s_t + lane * LD_PITCH);
    const uint4 t0 = tp[0], t1 = tp[1], t2 = tp[2], t3 = tp[3];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int lp = lane + LD_DT - (wv * 16 + j + 1);   // 0 .. 126
      const uint4* pp = reinterpret_cast<const uint4*>(s_p + lp * LD_PITCH);
      int32_t a = acc[j];
      a = and_popc4(t0, pp[0], a);
      a = and_popc4(t1, pp[1], a);
      a = and_popc4(t2, pp[2], a);
      a = and_popc4(t3, pp[3], a);
      acc[j] = a;
    }
    __syncthreads();
  }

  const int64_t r = r0 + lane;
  uint32_t bits = 0;
  if (r < vc) {
    const int64_t av = cnt[W + r];
    const int64_t q = av * ((int64_t)n - av);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int32_t d = d0 + wv * 16 + j + 1;
      if (d <= W && (int64_t)d <= r + T) {
        const int64_t au = cnt[W + r - d];
        const int64_t D = (int64_t)n * acc[j] - au * av;
        const int64_t p = au * ((int64_t)n - au);
        const double lhs = __dmul_rn((double)D, (double)D);
        const double rhs = __dmul_rn(t, __dmul_rn((double)p, (double)q));
        if (lhs > rhs) bits |= 1u << j;
      }
    }
  }
  s_bits[lane][wv] = bits;
  __syncthreads();
  if (tid < 2 * LD_TR) {
    const int row = tid >> 1, wd = tid & 1;
    const int32_t word = 2 * (int32_t)blockIdx.y + wd;
    if (r0 + row < vc && word < ew) ex[(r0 + row) * ew + word] = s_bits[row][2 * wd] | (s_bits[row][2 * wd + 1] << 16);
  }
}

// flags: [64] the wave's keep-flag words, carried between launches; g0: rows fed since the last break in front of this chunk.
// kbits: the keep flags of the chunk, word ((g0 + v) >> 5) - (g0 >> 5), bit 31 - ((g0 + v) & 31) for row v -- lane 0's flag word
// as it stands at the end of every block of 32 rows (ld_scan_kernel spreads them into bytes).
//
// The wave walks whole 32-row blocks of the feed order: it starts `pre` = g0 & 31 rows in front of the chunk and ends at a block
// boundary behind it, and the rows outside the chunk are staged as rows without band bits that are not polymorphic -- they change
// nothing.  So a row's place in its block is a compile-time constant of the unrolled body, and the body has no branch: per row
// two LDS reads, the funnel shift, and the chain v_and_b32 -> v_cmp (the ballot) -> s_cselect -> v_and_or_b32.
// A tile of blocks sits in LDS, rows ew + 1 words apart with a zero word in front of each (lane 0's low word, lane ew's high
// word); the next tile's band words and counts are in flight in registers meanwhile.
__global__ __launch_bounds__(64) void ld_resolve_kernel(const uint32_t* __restrict__ ex, const int32_t* __restrict__ cnt_rows, int64_t vc,
                                                        int32_t ew, int32_t n, int64_t g0, uint32_t* __restrict__ flags,
                                                        uint32_t* __restrict__ kbits) {
  __shared__ uint32_t s_ex[LD_RS_WORDS];
  __shared__ uint32_t s_poly[LD_RS_WORDS / 2];
  const int lane = threadIdx.x;
  uint32_t k = flags[lane];
  const int32_t pitch = ew + 1;
  const int32_t tile_rows = (LD_RS_WORDS - 1) / pitch / 32 * 32;   // 992 rows at ew = 1 .. 32 rows at ew = 32
  const int32_t jj = lane < ew ? lane : ew;                          // lanes beyond ew hold no flags (below): any word of the row serves
  const int64_t pre = g0 & 31, total = pre + vc;                     // rows of the walk, the first `pre` of them in front of the chunk
  uint32_t pe[LD_RS_WORDS / 64];
  int32_t pc[LD_RS_WORDS / 128];
  auto fetch = [&](int64_t u0) {
#pragma unroll
    for (int i = 0; i < LD_RS_WORDS / 64; ++i) {
      const int32_t at = i * 64 + lane, row = at / ew;
      const int64_t v = u0 + row - pre;
      pe[i] = row < tile_rows && v >= 0 && v < vc ? ex[v * ew + (at - row * ew)] : 0u;
    }
#pragma unroll
    for (int i = 0; i < LD_RS_WORDS / 128; ++i) {
      const int64_t v = u0 + i * 64 + lane - pre;
      pc[i] = i * 64 + lane < tile_rows && v >= 0 && v < vc ? cnt_rows[v] : 0;
    }
  };
  for (int i = lane; i < LD_RS_WORDS; i += 64) s_ex[i] = 0u;   // (the zero word in front of every row stays)
  fetch(0);
  for (int64_t u0 = 0; u0 < total; u0 += tile_rows) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < LD_RS_WORDS / 64; ++i) {
      const int32_t at = i * 64 + lane, row = at / ew;
      if (row < tile_rows) s_ex[row * pitch + 1 + (at - row * ew)] = pe[i];
    }
#pragma unroll
    for (int i = 0; i < LD_RS_WORDS / 128; ++i)
      if (i * 64 + lane < tile_rows) s_poly[i * 64 + lane] = pc[i] > 0 && pc[i] < n ? 0xffffffffu : 0u;
    if (u0 + tile_rows < total) fetch(u0 + tile_rows);   // in flight while this tile is resolved
    __syncthreads();
    for (int32_t b0 = 0; b0 < tile_rows && u0 + b0 < total; b0 += 32) {
      if (u0 + b0 > 0 || pre == 0) {   // a new block of 32 rows: every lane's flags move up one lane (the launch before did it when pre > 0)
        const uint32_t up = __shfl_up(k, 1);
        k = lane == 0 || lane > ew ? 0u : up;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t hi[8], lo[8], poly[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int32_t r = b0 + 8 * q + i;
          lo[i] = s_ex[r * pitch + jj];
          hi[i] = s_ex[r * pitch + jj + 1];
          poly[i] = s_poly[r];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const uint32_t o = 8 * q + i;
          // bit b of wd: distance o + 32 lane - b (band bit o + 32 lane - b - 1), the row whose flag is bit b of k
          const uint32_t wd = o ? (lo[i] >> o) | (hi[i] << (32 - o)) : lo[i];
          const uint32_t set = lane == 0 ? poly[i] & (1u << (31 - o)) : 0u;
          const uint32_t open = __ballot((wd & k) != 0) != 0 ? 0u : 0xffffffffu;   // no kept earlier row exceeds
          k |= set & open;
        }
      }
      if (lane == 0) kbits[(u0 + b0) >> 5] = k;
    }
  }
  flags[lane] = k;
}

// keep[r]: the flag of row r out of the resolve wave's words; pos[r]: kept rows in front of r in the chunk; out2 = {kept,
// monomorphic}
__global__ __launch_bounds__(LD_SCAN_THREADS) void ld_scan_kernel(const uint32_t* __restrict__ kbits, int64_t g0,
                                                                  const int32_t* __restrict__ cnt_rows, int64_t vc, int32_t n,
                                                                  uint8_t* __restrict__ keep, int32_t* __restrict__ pos,
                                                                  int64_t* __restrict__ out2) {
  __shared__ int32_t s_kept[LD_SCAN_THREADS];
  __shared__ int32_t s_mono[LD_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int64_t per = (vc + LD_SCAN_THREADS - 1) / LD_SCAN_THREADS;
  const int64_t b = std::min<int64_t>(vc, tid * per), e = std::min<int64_t>(vc, b + per);
  int32_t kept = 0, mono = 0;
  for (int64_t r = b; r < e; ++r) {
    const int64_t g = g0 + r;
    const uint8_t kp = (uint8_t)((kbits[(g >> 5) - (g0 >> 5)] >> (31 - ((uint32_t)g & 31u))) & 1u);
    keep[r] = kp;   // (read back below by this thread alone)
    kept += kp;
    const int32_t a = cnt_rows[r];
    mono += (a == 0 || a == n) ? 1 : 0;
  }
  s_kept[tid] = kept;
  s_mono[tid] = mono;
  __syncthreads();
  for (int off = 1; off < LD_SCAN_THREADS; off <<= 1) {   // inclusive scan of the threads' counts
    const int32_t x = tid >= off ? s_kept[tid - off] : 0, y = tid >= off ? s_mono[tid - off] : 0;
    __syncthreads();
    s_kept[tid] += x;
    s_mono[tid] += y;
    __syncthreads();
  }
  int32_t at = s_kept[tid] - kept;
  for (int64_t r = b; r < e; ++r) {
    pos[r] = at;
    at += keep[r];
  }
  if (tid == LD_SCAN_THREADS - 1) {
    out2[0] = s_kept[tid];
    out2[1] = s_mono[tid];
  }
}

__global__ __launch_bounds__(256) void ld_gather_kernel(const uint32_t* __restrict__ wb_rows, const uint8_t* __restrict__ keep,
                                                        const int32_t* __restrict__ pos, int64_t vc, int32_t words,
                                                        uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= vc || !keep[r]) return;
  const uint32_t* src = wb_rows + r * words;
  uint32_t* dst = out + (int64_t)pos[r] * words;
  for (int32_t k = lane; k < words; k += 64) dst[k] = src[k];
}

}  // namespace

int32_t ld_band_tile_rows() { return LD_TR; }
int32_t ld_band_chunk_words() { return LD_KC; }

hipError_t launch_ld_count(const uint32_t* rows, int64_t ld, int64_t vc, int32_t n, uint32_t* wb_rows, int32_t* cnt_rows,
                           hipStream_t stream) {
  if (vc <= 0) return hipSuccess;
  const int32_t words = (n + 31) / 32;
  const uint32_t last_mask = (n & 31) ? ((1u << (n & 31)) - 1u) : 0xffffffffu;
  ld_count_kernel<<<dim3((unsigned)((vc + 3) / 4)), 256, 0, stream>>>(rows, ld, vc, words, last_mask, wb_rows, cnt_rows);
  return hipGetLastError();
}

hipError_t launch_ld_band(const uint32_t* wb, const int32_t* cnt, int64_t vc, int32_t n, int32_t window, int32_t tail, double t,
                          uint32_t* ex, hipStream_t stream) {
  if (vc <= 0) return hipSuccess;
  const int32_t words = (n + 31) / 32, ew = (window + 31) / 32;
  const dim3 grid((unsigned)((vc + LD_TR - 1) / LD_TR), (unsigned)((window + LD_DT - 1) / LD_DT));
  ld_band_kernel<<<grid, 256, 0, stream>>>(wb, cnt, vc, words, window, tail, n, t, ew, ex);
  return hipGetLastError();
}

hipError_t launch_ld_resolve(const uint32_t* ex, const int32_t* cnt_rows, int64_t vc, int32_t n, int32_t window, int64_t g0,
                             uint32_t* flags, uint32_t* kbits, hipStream_t stream) {
  if (vc <= 0) return hipSuccess;
  ld_resolve_kernel<<<1, 64, 0, stream>>>(ex, cnt_rows, vc, (window + 31) / 32, n, g0, flags, kbits);
  return hipGetLastError();
}

hipError_t launch_ld_scan(const uint32_t* kbits, int64_t g0, const int32_t* cnt_rows, int64_t vc, int32_t n, uint8_t* keep,
                          int32_t* pos, int64_t* out2, hipStream_t stream) {
  ld_scan_kernel<<<1, LD_SCAN_THREADS, 0, stream>>>(kbits, g0, cnt_rows, vc, n, keep, pos, out2);
  return hipGetLastError();
}

hipError_t launch_ld_gather(const uint32_t* wb_rows, const uint8_t* keep, const int32_t* pos, int64_t vc, int32_t n, uint32_t* out,
                            hipStream_t stream) {
  if (vc <= 0) return hipSuccess;
  ld_gather_kernel<<<dim3((unsigned)((vc + 3) / 4)), 256, 0, stream>>>(wb_rows, keep, pos, vc, (n + 31) / 32, out);
  return hipGetLastError();
}

}  // namespace pcoa
