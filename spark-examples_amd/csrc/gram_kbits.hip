// gram_kbits.hip -- the k-bits contraction, two waves per SIMD: the operand stays in HBM at ONE BIT per genotype and becomes
// MX-FP4 only in registers, on the way into the matrix cores.  Pre-passes: pack_kbits.hip; the one-wave-per-SIMD form:
// gram_kbits_w4.hip; the operand K1[V/128][Npad][4 words], why it exists and its 8 KiB stage: kbits_layout.h.
//
// A lane's operand of one MFMA (32 FP4 values = 4 dwords) comes from ONE word:
//     d0 = (w << 1) & M,  d1 = w & M,  d2 = (w >> 1) & M,  d3 = (w >> 2) & M,   M = 0x22222222
// i.e. bit b of the word lands in nibble b / 4 of dword b % 4 as 0x2 = E2M1 1.0 -- 7 VALU operations per fragment.  Which
// variant sits in which of the MFMA's 64 k-slots does not matter: X^T X takes A and B from the same words through the
// same function, so every product pairs a variant with itself (the remark on k-order in gram_packed.hip's header).
// The wave layout, the accumulators, the ping-pong phases and the epilogue are those of gram_packed_kernel<1, ...>;
// a wave reads its 6 operand rows of a stage with 6 ds_read_b64 (words of both k-steps at once, 3 KiB instead of the
// 12 KiB of ds_read_b128 fragments) and expands them while its partner on the SIMD issues MFMAs.
#include <algorithm>
#include <utility>

#include "gram_common.h"
#include "gram_mfma.h"
#include "kbits_layout.h"

namespace pcoa {
namespace {

// ---------------------------------------------------------------------------------------------- contraction
// 8 DMA instructions of 1 KiB per stage, one per wave (waves 0-3: the quarters of panel I, 4-7: of panel J); a diagonal
// tile brings in its single panel with waves 0-3 only.
template <bool DIAG>
__device__ __forceinline__ void issue_stage_bits(StageBits* st, const int8_t* __restrict__ p, int npad, int64_t blk,
                                                 int col_i, int col_j, int wave, int lane) {
  if (DIAG && wave >= 4) return;  // wave-uniform
  const bool is_i = wave < 4;
  const int q = wave & 3;
  const int c0 = (is_i ? col_i : col_j) + q * 64;
  const int8_t* src = p + ((size_t)blk * npad + c0 + lane) * 16;
  uint32_t* dst = is_i ? &st->pi[q * 64][0] : &st->pj[q * 64][0];
  __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
}

// the two words (k-steps 0 and 1) of each of the wave's 4 A rows and 2 B rows: 6 ds_read_b64, conflict-free (a half-wave
// reads 32 consecutive 16-byte slots at the same 8-byte offset, the other half the other 8 bytes)
template <bool DIAG>
__device__ __forceinline__ void read_words(const StageBits* st, int wm, int wn, int lane, uint2 (&raw)[6]) {
  const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
    raw[mi] = *reinterpret_cast<const uint2*>(&st->pi[wm * 128 + mi * 32 + l31][2 * hi]);
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    if constexpr (DIAG) raw[4 + ni] = *reinterpret_cast<const uint2*>(&st->pi[wn * 64 + ni * 32 + l31][2 * hi]);
    else raw[4 + ni] = *reinterpret_cast<const uint2*>(&st->pj[wn * 64 + ni * 32 + l31][2 * hi]);
  }
}

// Conjugate weights.  The plain encoding puts both operands in as E2M1 1.0 (nibble 0x2): d_q = ((w << 1) >> q) & 0x22222222,
// 7 VALU operations per word.  E2M1 also has 0.5 (nibble 0x1) and 2.0 (nibble 0x4), and 0.5 x 2.0 = 1.0 x 1.0 = 1, both
// exact; so bit class q = b % 4 may sit at different heights in the A and the B nibble as long as the heights add up:
//   class   A (rows: 4 fragments per k-step)        B (columns: 2 fragments)
//     0     w & 0x1111..        0.5                 (w << 2) & 0x4444..   2.0
//     1     w & 0x2222..        1.0                 w & 0x2222..          1.0
//     2     w & 0x4444..        2.0                 (w >> 2) & 0x1111..   0.5
//     3     (w >> 1) & 0x4444.. 2.0                 (w >> 3) & 0x1111..   0.5
// 5 operations for an A word, 7 for a B word: 34 instead of 42 per k-step.  (The sign bit of a nibble is the one height
// that cannot be used, which is why class 3 always pays a shift.)
template <bool IS_B>
__device__ __forceinline__ i32x4 expand_word_fp4(uint32_t w) {
  i32x4 r;
  if constexpr (!IS_B) {
    r[0] = (int)(w & 0x11111111u);
    r[1] = (int)(w & 0x22222222u);
    r[2] = (int)(w & 0x44444444u);
    r[3] = (int)((w >> 1) & 0x44444444u);
  } else {
    r[0] = (int)((w << 2) & 0x44444444u);
    r[1] = (int)(w & 0x22222222u);
    r[2] = (int)((w >> 2) & 0x11111111u);
    r[3] = (int)((w >> 3) & 0x11111111u);
  }
  return r;
}

// The expansion is split over the two phases: the read phase only expands the fragments of k-step 0 (here); those of k-step 1
// are expanded one per MFMA gap while the wave issues its first six MFMAs (which only need k-step 0).
// The read phase (LDS latency + expansion) is then shorter than the partner's MFMA phase instead of longer.
__device__ __forceinline__ void expand_frags(const uint2 (&raw)[6], FragsI8<2> (&f)[2]) {
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) f[0].a[mi] = expand_word_fp4<false>(raw[mi].x);
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) f[0].b[ni] = expand_word_fp4<true>(raw[4 + ni].x);
  // The expansion is pure arithmetic: left alone, the optimiser sinks it below the phase barrier to just in front of the
  // MFMAs that consume it -- into the phase where the wave should do nothing but feed the matrix pipe.  An empty asm
  // that "modifies" every fragment pins the arithmetic here, in the wave's read phase.
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) asm volatile("" : "+v"(f[0].a[mi]));
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) asm volatile("" : "+v"(f[0].b[ni]));
}

// fragment IDX (in the order the k-step-1 MFMAs need them: a0, b0, b1, a1, a2, a3) of k-step 1, pinned at this point of
// the instruction stream from both sides (its input is "redefined" here, its output "used" here)
template <int IDX>
__device__ __forceinline__ void expand_late(uint2 (&raw)[6], FragsI8<2> (&f)[2]) {
  constexpr int R = IDX == 0 ? 0 : IDX == 1 ? 4 : IDX == 2 ? 5 : IDX - 2;  // row of `raw`
  asm volatile("" : "+v"(raw[R].y));
  if constexpr (R < 4) {
    f[1].a[R] = expand_word_fp4<false>(raw[R].y);
    asm volatile("" : "+v"(f[1].a[R]));
  } else {
    f[1].b[R - 4] = expand_word_fp4<true>(raw[R].y);
    asm volatile("" : "+v"(f[1].b[R - 4]));
  }
}

// MFMA number T of a stage (order (k-step, mi, ni) as mfma_range) with its two wait states in front of it INSIDE the
// asm statement, where nothing can be scheduled between them and the instruction.
template <int T>
__device__ __forceinline__ void mfma_one(const FragsI8<2> (&f)[2], f32x16 (&acc)[4][2]) {
  constexpr int k2 = T / 8, mi = (T % 8) / 2, ni = T % 2;
  asm volatile("s_nop 1\n\tv_mfma_f32_32x32x64_f8f6f4 %0, %1, %2, %0 cbsz:4 blgp:4"
               : "+v"(acc[mi][ni])
               : "v"(f[k2].a[mi]), "v"(f[k2].b[ni]));
}

// MFMAs LO .. HI-1 of a stage, with the six late expansions behind MFMAs 0 .. 5.
// Two hazards of mixing VALU work into an asm MFMA run, both measured (profiles/r03g_kbits_hazards.txt), neither padded by
// the compiler because it cannot see an MFMA inside an asm statement:
//  * an MFMA that issues in the cycle after a VALU instruction comes back with the first two registers of its
//    accumulator wrong (rows 0, 1, 4, 5 of its 32 x 32 tile): MFMA 6 directly behind the last late expansion (~7,000 of
//    6.3 M entries of S at configs[1] size, group-1 waves only), and, once that one was padded, MFMA 0 / 8 behind
//    compiler-placed moves at small shapes.  One wait state is enough (measured); every MFMA of this schedule carries two,
//    inside its own asm statement where nothing can be scheduled between them and the instruction (free behind another
//    MFMA: the pipe is busy for 32 cycles anyway);
//  * an MFMA reads its A / B registers for several cycles after it has issued: a late expansion must never be allocated
//    to the registers of a k-step-0 fragment that died an instruction ago, so all of k-step 0 is kept alive until its last
//    MFMA has issued.
template <int LO, int HI, int T = LO>
__device__ __forceinline__ void mfma_run(uint2 (&raw)[6], FragsI8<2> (&f)[2], f32x16 (&acc)[4][2]) {
  if constexpr (T < HI) {
    mfma_one<T>(f, acc);
    if constexpr (T < 6) expand_late<T>(raw, f);
    if constexpr (T == 7)
      asm volatile("" ::"v"(f[0].a[0]), "v"(f[0].a[1]), "v"(f[0].a[2]), "v"(f[0].a[3]), "v"(f[0].b[0]), "v"(f[0].b[1]));
    mfma_run<LO, HI, T + 1>(raw, f, acc);
  }
}

// One stage of the ping-pong schedule (pp_stage of gram_packed.hip with the operand expanded in registers).  The phases,
// the barriers and the vmcnt book-keeping are the same; PER_WAVE = 1 DMA instruction per wave and stage.
template <int NST, int BUF, int GRP, bool IDLE, bool DIAG>
__device__ __forceinline__ void ppb_stage(StageBits* lds, const int8_t* __restrict__ p, int npad, int64_t blk_begin, int s,
                                          int ns, int col_i, int col_j, int wave, int lane, int wm, int wn,
                                          f32x16 (&acc)[4][2], FragsI8<2> (&f)[2], uint2 (&raw)[6]) {
  constexpr int PER_WAVE = 1;
  constexpr int D = NST - 1;
  static_assert(D == 2, "3-stage ring: at most one stage beyond s+1 in flight");
  constexpr int TOT = 16;  // MFMAs per wave and stage
  // the last LEFT MFMAs of a group's run are issued AFTER the barrier that ends its phase (pp_stage of gram_packed.hip)
  constexpr int LEFT = 2;
  const bool more = s + D < ns;
  if constexpr (GRP == 0) {
    // ---- phase 2s: read + expand stage s, issue the DMA of stage s+D
    if constexpr (!IDLE) read_words<DIAG>(&lds[BUF], wm, wn, lane, raw);
    __builtin_amdgcn_sched_barrier(0);
    if (more) issue_stage_bits<DIAG>(&lds[(BUF + D) % NST], p, npad, blk_begin + s + D, col_i, col_j, wave, lane);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!IDLE) expand_frags(raw, f);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    raw_barrier();
    // ---- phase 2s+1: the MFMAs of stage s
    if constexpr (!IDLE) {
      asm volatile("s_nop 1");  // VALU-written operands -> MFMA (the barrier covers it; this makes it unconditional)
      __builtin_amdgcn_s_setprio(1);
      mfma_run<0, TOT - LEFT>(raw, f, acc);
      __builtin_amdgcn_s_setprio(0);
    }
  } else {
    // ---- phase 2s: issue the DMA of stage s+D, then the MFMAs of stage s-1
    if (more) issue_stage_bits<DIAG>(&lds[(BUF + D) % NST], p, npad, blk_begin + s + D, col_i, col_j, wave, lane);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!IDLE) {
      if (s > 0) {
        asm volatile("s_nop 1");
        __builtin_amdgcn_s_setprio(1);
        mfma_run<0, TOT - LEFT>(raw, f, acc);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    raw_barrier();
    // ---- phase 2s+1: (the leftover MFMAs of stage s-1, then) read + expand stage s
    if constexpr (!IDLE) {
      if (s > 0) {
        __builtin_amdgcn_s_setprio(2);
        mfma_run<TOT - LEFT, TOT>(raw, f, acc);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
      }
      read_words<DIAG>(&lds[BUF], wm, wn, lane, raw);
      expand_frags(raw, f);
    }
  }
  // end of phase 2s+1: stage s+1 must have landed (own share), only the DMA of stage s+2.. may stay in flight
  if (s + 1 < ns) {
    const int rem = ns - 2 - s;  // stages after s+1 whose DMA has been issued: min(rem, D-1)
    const int keep = rem < D - 1 ? rem : D - 1;
    if (keep == 1) wait_vmcnt<PER_WAVE>();
    else wait_vmcnt<0>();
  }
  if constexpr (GRP == 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  raw_barrier();
  if constexpr (GRP == 0 && !IDLE) {  // group 0's leftover MFMAs of stage s, into phase 2(s+1)
    __builtin_amdgcn_s_setprio(2);
    mfma_run<TOT - LEFT, TOT>(raw, f, acc);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int NST, int GRP, bool IDLE, bool DIAG, int... Is>
__device__ __forceinline__ void ppb_round(StageBits* lds, const int8_t* __restrict__ p, int npad, int64_t blk_begin, int s,
                                          int ns, int count, int col_i, int col_j, int wave, int lane, int wm, int wn,
                                          f32x16 (&acc)[4][2], FragsI8<2> (&f)[2], uint2 (&raw)[6],
                                          std::integer_sequence<int, Is...>) {
  ((Is < count ? ppb_stage<NST, Is, GRP, IDLE, DIAG>(lds, p, npad, blk_begin, s + Is, ns, col_i, col_j, wave, lane, wm,
                                                           wn, acc, f, raw)
               : (void)0),
   ...);
}

template <int NST, int GRP, bool IDLE, bool DIAG>
__device__ __forceinline__ void ppb_loop(StageBits* lds, const int8_t* __restrict__ p, int npad, int64_t blk_begin, int ns,
                                         int col_i, int col_j, int wave, int lane, int wm, int wn,
                                         f32x16 (&acc)[4][2]) {
  FragsI8<2> f[2];
  uint2 raw[6];
  // prologue: stages 0 .. NST-2 go in flight; stage 0 must have landed before group 0 reads it in phase 0
#pragma unroll
  for (int i = 0; i < NST - 1; ++i)
    if (i < ns) issue_stage_bits<DIAG>(&lds[i], p, npad, blk_begin + i, col_i, col_j, wave, lane);
  if (ns > 1 && NST > 2) wait_vmcnt<(NST > 2 ? 1 : 0)>();
  else wait_vmcnt<0>();
  raw_barrier();
  int s = 0;
  for (; s + NST - 1 < ns; s += NST)
    ppb_round<NST, GRP, IDLE, DIAG>(lds, p, npad, blk_begin, s, ns, NST, col_i, col_j, wave, lane, wm, wn, acc, f,
                                          raw, std::make_integer_sequence<int, NST>{});
  if (s < ns)
    ppb_round<NST, GRP, IDLE, DIAG>(lds, p, npad, blk_begin, s, ns, ns - s, col_i, col_j, wave, lane, wm, wn, acc, f,
                                          raw, std::make_integer_sequence<int, NST - 1>{});
  if constexpr (GRP == 1 && !IDLE) {  // phase 2*ns: group 1's MFMAs of the last stage, nobody to wait for
    asm volatile("s_nop 1");
    mfma_run<0, 16>(raw, f, acc);
  }
}

// Work decomposition: xcd_map 0 / 1 / 2 as gram_packed_kernel (legacy split-K, split-K with one k-slice per XCD,
// lock-step); xcd_map 4 = even split: `nwork` = ntri * nstages (tile, stage) units in tile-major order are cut into
// gridDim.x equal runs, a workgroup walks its run and pays one epilogue per tile it touches (at most
// ceil(run / nstages) + 1).  Every CU gets the same number of MFMAs whatever ntri is (55 tiles x split-K 4 leaves 36 of
// 256 CUs idle in the lock-step launch).
// The body is a device function wrapped by the kernel below it, which is held to 224 VGPRs per wave (the compiler takes all
// 256 a 2-waves-per-SIMD kernel may have when left alone, and needs 196): two contraction waves then leave a SIMD 64 of its
// 512 registers -- room for the waves of the persistent ring pre-pass (pack_kbits_ring_kernel), which shares the CU with
// this kernel in the fp32 pipeline (DESIGN_HISTORY.md 4.1, profiles/r03s .. r03u_coreside.txt).
#define PCOA_KBITS_CONTRACTION __device__ __forceinline__ void gram_kbits_body
template <int NST>
PCOA_KBITS_CONTRACTION(const int8_t* __restrict__ p, int npad, int64_t nstages, int n,
                                                            int ntile, int ntri, int splitk, int64_t stages_per,
                                                            int32_t* __restrict__ s32, int xcd_map,
                                                            const int32_t* __restrict__ skip, GramStrip strip) {
  __shared__ __attribute__((aligned(16))) StageBits lds[NST];
  if (skip != nullptr && *skip != 0) return;  // auto mode's device-side predicate (gram_packed_kernel)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int b = blockIdx.x;

  // the run of (tile, stage) units of this workgroup: [u, u_end) in tile-major order
  int64_t u, u_end;
  if (xcd_map == 4) {
    const int64_t nwork = (int64_t)ntri * nstages;
    const int64_t nwg = gridDim.x;
    // consecutive runs go to consecutive workgroups of ONE XCD (block b runs on XCD b % 8), so that the workgroups
    // which share a tile's operand panels at about the same k also share an L2
    const int64_t slot = (nwg % kNumXcd == 0) ? (int64_t)(b & 7) * (nwg / kNumXcd) + (b >> 3) : (int64_t)b;
    u = nwork * slot / nwg;
    u_end = nwork * (slot + 1) / nwg;
  } else {
    int tile, ks;
    if (xcd_map == 2) {
      const int g = kNumXcd / splitk;
      const int per = (ntri + g - 1) / g;
      const int xcd = b & 7, slot = b >> 3;
      tile = (xcd % g) * per + slot;
      ks = xcd / g;
      if (slot >= per || tile >= ntri) return;
    } else if (xcd_map) {
      const int q = b >> 3;
      ks = (b & 7) + kNumXcd * (q / ntri);
      tile = q % ntri;
    } else {
      tile = b % ntri;
      ks = b / ntri;
    }
    const int64_t st_begin = (int64_t)ks * stages_per;
    const int64_t st_end = (st_begin + stages_per < nstages) ? (st_begin + stages_per) : nstages;
    if (st_begin >= st_end) return;
    u = (int64_t)tile * nstages + st_begin;
    u_end = (int64_t)tile * nstages + st_end;
  }

  while (u < u_end) {  // workgroup-uniform
    const int tile = (int)(u / nstages);
    const int64_t st_begin = u - (int64_t)tile * nstages;
    const int64_t left = u_end - u;
    const int ns = (int)((nstages - st_begin < left) ? (nstages - st_begin) : left);
    u += ns;

    int row_blk, col_blk;
    if (strip.cols > 0) {  // strip owner: all (row block, column block of the strip) tiles, banded (gram_packed_kernel)
      const int ctiles = ntri / ntile;
      const int per_band = BAND * ctiles;
      const int band = tile / per_band;
      const int r0 = band * BAND;
      const int h = (ntile - r0 < BAND) ? (ntile - r0) : BAND;
      const int rem = tile - band * per_band;
      row_blk = r0 + rem % h;
      col_blk = strip.cb0 + rem / h;
    } else {
      tile_coords<2>(tile, ntile, row_blk, col_blk);
    }
    const int col_i = row_blk * 256, col_j = col_blk * TJ;
    const bool idle = strip.cols == 0 && (col_i + wm * 128) > (col_j + wn * 64 + 63);

    f32x16 acc[4][2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0;

    if (row_blk == col_blk && strip.cols == 0) {  // diagonal tile: one panel (workgroup-uniform branch)
      if (wm == 0) ppb_loop<NST, 0, false, true>(lds, p, npad, st_begin, ns, col_i, col_j, wave, lane, wm, wn, acc);
      else if (idle) ppb_loop<NST, 1, true, true>(lds, p, npad, st_begin, ns, col_i, col_j, wave, lane, wm, wn, acc);
      else ppb_loop<NST, 1, false, true>(lds, p, npad, st_begin, ns, col_i, col_j, wave, lane, wm, wn, acc);
    } else if (wm == 0) {
      ppb_loop<NST, 0, false, false>(lds, p, npad, st_begin, ns, col_i, col_j, wave, lane, wm, wn, acc);
    } else {
      ppb_loop<NST, 1, false, false>(lds, p, npad, st_begin, ns, col_i, col_j, wave, lane, wm, wn, acc);
    }

    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // last asm MFMA -> VALU read of D
    if (!idle) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const int j = col_j + wn * 64 + ni * 32 + (lane & 31);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int i = col_i + wm * 128 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int v = (int)acc[mi][ni][r];  // exact integers below 2^24
            if (strip.cols > 0) {
              if (i < n && j >= strip.col0 && j < strip.col0 + strip.cols && v != 0)
                atomicAdd(&s32[(int64_t)i * strip.cols + (j - strip.col0)], v);
            } else if (j >= i && j < n && v != 0) {
              atomicAdd(&s32[(int64_t)i * n + j], v);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    // the next tile of this run reuses the LDS ring: every wave must be out of this tile's last stage first (the loops
    // end with a barrier after the last reads; the epilogue touches no LDS)
  }
}
#undef PCOA_KBITS_CONTRACTION
// amdgpu_num_vgpr counts halves of the unified register file on gfx90a+: 112 -> at most 224 registers per wave
template <int NST, int LEFT, int ENC>
__global__ __launch_bounds__(512, 2) __attribute__((amdgpu_num_vgpr(112))) void gram_kbits_kernel(
    const int8_t* __restrict__ p, int npad, int64_t nstages, int n, int ntile, int ntri, int splitk, int64_t stages_per,
    int32_t* __restrict__ s32, int xcd_map, const int32_t* __restrict__ skip, GramStrip strip) {
  // conjugate weights with the expansion split over the phases (ENC 2), 3-stage ring, two MFMAs behind the barrier: the one
  // schedule there is (the others' numbers: profiles/r03*); the parameter list is the kernel's name
  static_assert(NST == 3 && LEFT == 2 && ENC == 2, "the one shipped instantiation");
  gram_kbits_body<NST>(p, npad, nstages, n, ntile, ntri, splitk, stages_per, s32, xcd_map, skip, strip);
}

}  // namespace

// Contraction of a k-bits operand.  mode: 0 = legacy split-K launch, 2 = lock-step (splitk k-streams on 8 / splitk XCDs,
// fails with hipErrorInvalidValue where the shape does not fit `num_cu`), 4 = even split over `num_cu` workgroups.
hipError_t launch_gram_kbits(const int8_t* p, int64_t nv, int32_t n, int32_t* s32, int num_cu, hipStream_t stream, int mode,
                             const int32_t* skip, GramStrip strip) {
  if (mode == 5) mode = 4;   // (the XCD k-segment split exists in the one-wave-per-SIMD kernel only)
  if (nv <= 0) return hipSuccess;
  const int cus = num_cu > 0 ? num_cu : 256;
  const int npad = (int)gram_packed_npad(n);
  const int ntile = npad / TJ;
  int64_t ntri64 = (int64_t)ntile * (ntile + 1) / 2;
  if (strip.cols > 0) {
    strip.cb0 = strip.col0 / TJ;
    const int cb1 = (strip.col0 + strip.cols + TJ - 1) / TJ;
    ntri64 = (int64_t)ntile * (cb1 - strip.cb0);
  }
  if (ntri64 > (1 << 28)) return hipErrorInvalidValue;
  const int ntri = (int)ntri64;
  const int64_t nstages = gram_kb_pad(nv, 2) / 4;  // blocks of 128 variants (the operand is padded to whole blocks)
  int64_t splitk = 1, stages_per = nstages, nblocks = 0;
  int xcd_map = 0;
  if (mode == 2) {
    if (strip.cols > 0) return hipErrorInvalidValue;
    splitk = gram_lockstep_splitk(n, cus);
    if (splitk == 0) return hipErrorInvalidValue;
    const int g = kNumXcd / (int)splitk;
    const int per = (ntri + g - 1) / g;
    stages_per = (nstages + splitk - 1) / splitk;
    nblocks = (int64_t)per * kNumXcd;
    xcd_map = 2;
  } else if (mode == 4) {
    // one workgroup per CU, but never runs shorter than 8 stages (1,024 variants): an epilogue costs about as much
    const int64_t nwork = (int64_t)ntri * nstages;
    nblocks = std::max<int64_t>(1, std::min<int64_t>(cus, nwork / 8));
    if (nblocks >= kNumXcd) nblocks = nblocks / kNumXcd * kNumXcd;  // the kernel's XCD-aware run order needs a multiple of 8
    xcd_map = 4;
  } else {
    const int64_t target = (int64_t)cus * 7;
    splitk = (target + ntri - 1) / ntri;
    const int64_t max_by_work = nstages * 4 / 64;
    if (splitk > max_by_work) splitk = max_by_work;
    if (splitk < 1) splitk = 1;
    if (splitk >= kNumXcd) {
      splitk = (splitk / kNumXcd) * kNumXcd;
      xcd_map = 1;
    }
    stages_per = (nstages + splitk - 1) / splitk;
    nblocks = (int64_t)ntri * splitk;
  }
  if (nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)nblocks), block(512);
  hipLaunchKernelGGL((gram_kbits_kernel<3, 2, 2>), grid, block, 0, stream, p, npad, nstages, n, ntile, ntri, (int)splitk,
                     stages_per, s32, xcd_map, skip, strip);
  return hipGetLastError();
}

}  // namespace pcoa
