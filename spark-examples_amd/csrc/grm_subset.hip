// grm_subset.hip -- the 2-bit column gather of pcoa_create_grm_subset: dst slot a of every row = src slot keep[a]
// of the same row, in the store's one coding (grm_bits.hip), at the result's own pitch.  Every lane owns ONE output word (16
// samples) and rows stream through it, as in grm_bits.hip:
//   before the row loop the lane reads keep[16 w .. 16 w + 15] once and keeps the 16 source sample indices in registers (word =
//   k >> 4, shift = 2 (k & 15), both row-invariant); the list is increasing, so the lane's source words are non-decreasing, and
//   a bit per slot says whether the slot starts a new source word.  In the row loop a source word is loaded only at those slots
//   and reused while consecutive slots share it: a few samples removed cost one or two loads per output word, neighbouring lanes
//   read neighbouring words; one kept sample per 16 costs 16 loads.
//   kGrmSubsetTileRows rows are in flight per lane, so the loads of a slot are issued together and one wait covers them.
//   slots at index >= n_keep and the pitch's padding words are written as 01 (0x55555555 for a whole word), as the append
//   kernel leaves a store.
// An output word is a pure function of the source row and the list: no atomics, no LDS, no scratch, and nothing depends on the
// grid.  Rows are not staged through LDS for sparse lists: the sparse case reads whole 64-byte sectors for 2 bits each whichever
// way the words travel, so LDS would only save load instructions where the memory traffic is already the cost; the dense case
// (the one that matters) has nothing to save.
#include <algorithm>

#include "grm_slots.h"
#include "pcoa_internal.h"

namespace pcoa {

namespace {

constexpr int kGrmSubsetTileRows = 8;   // rows a lane keeps in flight

// byte offsets inside one launch fit 32 bits (launch_grm_subset cuts the rows accordingly), so a load is the uniform base plus
// one 32-bit lane offset
__device__ __forceinline__ uint32_t word_at(const uint32_t* base, uint32_t byte_off) {
  return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(base) + byte_off);
}

__global__ __launch_bounds__(256) void grm_subset_kernel(const uint32_t* __restrict__ src, int32_t spitch, int32_t rows,
                                                         const int32_t* __restrict__ keep, int32_t n_keep, int32_t dpitch,
                                                         int32_t lanes_rows, uint32_t* __restrict__ dst) {
  constexpr int T = kGrmSubsetTileRows;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t slot64 = gid / dpitch;        // which of the lanes_rows row streams this lane is
  const int32_t w = (int32_t)(gid - slot64 * dpitch);
  if (slot64 >= lanes_rows) return;
  const int32_t slot = (int32_t)slot64;
  const int32_t live = (int32_t)std::min<int64_t>(16, (int64_t)n_keep - (int64_t)w * 16);   // slots of this word that belong to samples (<= 0: none)
  int32_t k[16];
  uint32_t fresh = 0;   // bit j: slot j reads another source word than slot j - 1
  int32_t prev = -1;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    int32_t kj = j > 0 ? k[j - 1] : 0;
    if (j < live) {
      kj = keep[(int64_t)w * 16 + j];
      if ((kj >> 4) != prev) fresh |= 1u << j;
      prev = kj >> 4;
    }
    k[j] = kj;
  }
  const uint32_t mask = live >= 16 ? 0xffffffffu : live > 0 ? (1u << (2 * live)) - 1u : 0u;
  const uint32_t pad = kLo & ~mask;
  const uint32_t sbytes = (uint32_t)spitch * 4u, dbytes = (uint32_t)dpitch * 4u;

  for (int32_t r0 = slot * T; r0 < rows; r0 += lanes_rows * T) {
    uint32_t rb[T], cur[T], out[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      rb[t] = (uint32_t)std::min(r0 + t, rows - 1) * sbytes;   // (a row past the end re-reads the last one; it is not stored)
      cur[t] = out[t] = 0;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if ((fresh >> j) & 1u) {
        const uint32_t so = (uint32_t)(k[j] >> 4) * 4u;
#pragma unroll
        for (int t = 0; t < T; ++t) cur[t] = word_at(src, rb[t] + so);
      }
      const uint32_t sh = (uint32_t)(k[j] & 15) * 2u;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        out[t] |= ((cur[t] >> sh) & 3u) << (2 * j);
        asm volatile("" : "+v"(out[t]));   // the slot is consumed here: without this the compiler sinks the extracts behind all 16
                                           // conditional loads and keeps every loaded word live (186 VGPRs instead of 75)
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t)
      if (r0 + t < rows)
        *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(dst) + ((uint32_t)(r0 + t) * dbytes + (uint32_t)w * 4u)) = (out[t] & mask) | pad;
  }
}

}  // namespace

int32_t grm_subset_tile_rows() { return kGrmSubsetTileRows; }

// rows x grm_pitch_words(n_src) words at src -> rows x grm_pitch_words(n_keep) words at dst; keep: n_keep device indices in
// [0, n_src), strictly increasing (the caller has checked them: a source word index is k >> 4 < the source pitch)
hipError_t launch_grm_subset(const uint32_t* src, int64_t rows, int32_t n_src, const int32_t* keep, int32_t n_keep, uint32_t* dst,
                             int32_t num_cu, hipStream_t stream) {
  const int64_t spitch = grm_pitch_words(n_src), dpitch = grm_pitch_words(n_keep);
  // a launch's rows span less than 2^31 bytes on either side (the kernel's 32-bit byte offsets); a segment of the default size
  // is one launch
  int64_t cut = std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / (std::max(spitch, dpitch) * 4));
  if (cut > kGrmSubsetTileRows) cut -= cut % kGrmSubsetTileRows;
  for (int64_t r = 0; r < rows; r += cut) {
    const int64_t cur = std::min(cut, rows - r);
    // every lane amortises its 16 index loads over 8 tiles or more where the rows allow it; about eight workgroups per CU at most
    const int64_t by_rows = (cur + 8 * kGrmSubsetTileRows - 1) / (8 * kGrmSubsetTileRows);
    const int64_t by_cus = std::max<int64_t>(1, (int64_t)std::max(num_cu, 1) * 2048 / dpitch);
    const int64_t lanes_rows = std::max<int64_t>(1, std::min(by_rows, by_cus));
    const int64_t blocks = (lanes_rows * dpitch + 255) / 256;
    hipLaunchKernelGGL(grm_subset_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, src + r * spitch, (int32_t)spitch, (int32_t)cur,
                       keep, n_keep, (int32_t)dpitch, (int32_t)lanes_rows, dst + r * dpitch);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace pcoa
