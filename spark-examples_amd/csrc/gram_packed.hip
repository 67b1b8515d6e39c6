// gram_packed.hip -- S += X^T X on the low-precision matrix cores of gfx950, exact.
//
// Same contraction as gram_f32.hip (reference VariantsPca.scala:184-190), computed in the reference's own
// arithmetic: integer counts (`DenseMatrix.zeros[Int]`, :185).  Genotype indicators are 0/1, so nothing is lost in
// low-precision operands as long as the accumulation is exact:
//
//   FMT 1 (default, binary tiles)   MX-FP4 E2M1 operands (0 -> 0x0, 1.0 -> 0x2), v_mfma_f32_32x32x64_f8f6f4 in
//                                   its unscaled form, fp32 accumulators (exact below 2^24; a launch feeds at most
//                                   2^20 variants through one chain), ~10 PFLOP/s dense
//   FMT 0 (carrier multiplicities)  int8 operands (0..127), v_mfma_i32_32x32x32_i8, int32 accumulators, ~5 POP/s
//
// Operand layout P[kb][Npad][16 B], "k-blocked": the 16 bytes at P[kb][i] are sample i's indicators for the 32 (FP4)
// or 16 (int8) variants of k-block kb.  That is exactly one lane's operand slice of the MFMA, for the A operand
// (row i) and for the B operand (column j) alike -- X^T X uses the same k-slot mapping on both sides, so any
// consistent order of the k's inside a block gives the same sum -- and the LDS image IS the global image.
//
// Pre-passes: pack_packed.hip.  The k-bits operand (one bit per genotype, the default for binary tiles) has its own files:
// pack_kbits.hip, gram_kbits.hip, gram_kbits_w4.hip.
//
// gram_packed_kernel<FMT, ...>      P -> S32: upper-triangular 256x256 tiles x split-K, integer atomics.
//   512 threads = 8 waves as 2(M) x 4(N), each wave a 128x64 block = 4x2 MFMA tiles (128 accumulators per lane).
//   One stage = 4 k-blocks x 2 panels x 256 samples x 16 B = 32 KiB, brought in by 32 global_load_lds_dwordx4 (1 KiB
//   each), 3-stage LDS ring (96 KiB), counted vmcnt (two stages stay in flight), raw s_barrier (never
//   __syncthreads, which would drain the DMA queue).  Operand reads are ds_read_b128 of 32 consecutive 16-B slots per
//   half-wave: conflict-free.  Schedule: ping-pong (two wave groups half a stage apart, see below).
//
// Measured at N = 2504 per 10^6 variants: FP4 1.13-1.16 ms (6 PFLOP/s issued), int8 2.14 ms; DESIGN_HISTORY.md 4.1 / 4.2.
#include <utility>

#include "gram_common.h"
#include "gram_mfma.h"

namespace pcoa {
namespace {

// ---------------------------------------------------------------------------------------------- gemm
// Template parameters
//   NWM  waves along M (tile height 128*NWM); NNI 32-column MFMA tiles per wave along N (wave tile
//        128 x 32*NNI, 8/NNI waves along N); SKB k-blocks (of 16 variants) per stage; NST ring length.
// Measured at N = 2504, 10^6 variants per launch (MI355X):
//   <2,2,4,3> 256x256, 8 waves, 64-variant stages, 3-ring          2.41 ms
//   <1,2,4,3> 128x256, 4 waves, two workgroups per CU              2.88 ms  (more LDS-DMA bytes per MAC)
//   <2,4,4,3> 256x256, 4 waves (one per SIMD), wave tile 128x128   2.61 ms  (LDS latency exposed)

template <int NWM, int SKB>
struct StageI8 {
  int8_t pi[SKB][128 * NWM][KB];  // panel I: [k-block][sample][16 B]
  int8_t pj[SKB][TJ][KB];         // panel J
};

// DMA instructions per stage: SKB * (2*NWM + 4) of 1 KiB each, spread evenly over the waves.
template <int NWM, int SKB, int NWAVES>
__device__ __forceinline__ void issue_stage_i8(StageI8<NWM, SKB>* st, const int8_t* __restrict__ p, int npad,
                                               int64_t kb0, int col_i, int col_j, int wave, int lane) {
  constexpr int QI = 2 * NWM;              // 64-sample quarters in panel I
  constexpr int PER_KB = QI + 4;           // instructions per k-block
  constexpr int TOTAL = SKB * PER_KB;
  constexpr int PER_WAVE = TOTAL / NWAVES;
  static_assert(TOTAL % NWAVES == 0, "DMA instructions must divide evenly over the waves");
#pragma unroll
  for (int q = 0; q < PER_WAVE; ++q) {
    const int id = wave * PER_WAVE + q;
    const int kb = id / PER_KB;
    const int r = id - kb * PER_KB;
    const bool is_i = r < QI;
    const int sq = is_i ? r : r - QI;
    const int c0 = (is_i ? col_i : col_j) + sq * 64;
    const int8_t* src = p + ((size_t)(kb0 + kb) * npad + c0 + lane) * KB;
    int8_t* dst = is_i ? &st->pi[kb][sq * 64][0] : &st->pj[kb][sq * 64][0];
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
  }
}

template <int NWM, int NNI, int SKB>
__device__ __forceinline__ void load_frags_i8(const StageI8<NWM, SKB>* st, int k2, int wm, int wn, int lane,
                                              FragsI8<NNI>& f) {
  const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
    f.a[mi] = *reinterpret_cast<const i32x4*>(&st->pi[2 * k2 + hi][wm * 128 + mi * 32 + l31][0]);
#pragma unroll
  for (int ni = 0; ni < NNI; ++ni)
    f.b[ni] = *reinterpret_cast<const i32x4*>(&st->pj[2 * k2 + hi][wn * 32 * NNI + ni * 32 + l31][0]);
}

// Diagonal tiles (row block == column block): panel J IS panel I, so only panel I is brought in (16 instead of 32
// DMA instructions per stage) and the B fragments are read from it.
template <int NWM, int NNI, int SKB>
__device__ __forceinline__ void load_frags_diag(const StageI8<NWM, SKB>* st, int k2, int wm, int wn, int lane,
                                                FragsI8<NNI>& f) {
  const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
    f.a[mi] = *reinterpret_cast<const i32x4*>(&st->pi[2 * k2 + hi][wm * 128 + mi * 32 + l31][0]);
#pragma unroll
  for (int ni = 0; ni < NNI; ++ni)
    f.b[ni] = *reinterpret_cast<const i32x4*>(&st->pi[2 * k2 + hi][wn * 32 * NNI + ni * 32 + l31][0]);
}

template <int NWM, int SKB, int NWAVES>
__device__ __forceinline__ void issue_stage_diag(StageI8<NWM, SKB>* st, const int8_t* __restrict__ p, int npad,
                                                 int64_t kb0, int col_i, int wave, int lane) {
  constexpr int QI = 2 * NWM;  // 64-sample quarters in panel I
  constexpr int TOTAL = SKB * QI;
  constexpr int PER_WAVE = TOTAL / NWAVES;
  static_assert(TOTAL % NWAVES == 0, "DMA instructions must divide evenly over the waves");
#pragma unroll
  for (int q = 0; q < PER_WAVE; ++q) {
    const int id = wave * PER_WAVE + q;
    const int kb = id / QI;
    const int sq = id - kb * QI;
    const int8_t* src = p + ((size_t)(kb0 + kb) * npad + col_i + sq * 64 + lane) * KB;
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)&st->pi[kb][sq * 64][0], 16, 0, 0);
  }
}

template <int FMT, int NNI>
__device__ __forceinline__ void mfma_step_i8(const FragsI8<NNI>& f, typename AccType<FMT>::type (&acc)[4][NNI]) {
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < NNI; ++ni) {
      if constexpr (FMT == 0) {
        acc[mi][ni] = __builtin_amdgcn_mfma_i32_32x32x32_i8(f.a[mi], f.b[ni], acc[mi][ni], 0, 0, 0);
      } else {
        // 32 FP4 values per lane = 4 VGPRs; cbsz = blgp = 4 selects E2M1.  The UNSCALED form of the instruction:
        // no block scale is applied (bit-exact against the oracle, tests/test_gpu_parity.py) and it saves the
        // ld_scale half of v_mfma_scale_* (1.235 vs 1.259 ms per 10^6 variants).  Written as inline asm because the builtin takes 8-VGPR operand tuples (the FP4 form
        // reads the low 4): materialising them doubles the fragment registers and the kernel spills.
        // Hazards (cdna_hip_programming.md 5.7): operands come from ds_read (the compiler waits lgkmcnt before
        // the statement since it names them as inputs); D feeds only the next MFMA as its whole C (no wait
        // states needed); the epilogue's first VALU read of D is fenced by s_nops after the main loop.
        asm volatile("v_mfma_f32_32x32x64_f8f6f4 %0, %1, %2, %0 cbsz:4 blgp:4"
                     : "+v"(acc[mi][ni])
                     : "v"(f.a[mi]), "v"(f.b[ni]));
      }
    }
}

// ---- ping-pong schedule --------------------------------------------------------------------------------------
// A plain ring keeps all eight waves in phase: after every barrier they all read fragments, then all
// issue MFMAs, and the matrix pipe idles during the read burst (53-64 % MFMA-busy measured).  Here the waves
// form two groups, one wave of each group per SIMD (waves w and w+4 share a SIMD), half a stage apart:
//
//   phase 2s   : group 0 reads the fragments of stage s (12 ds_read_b128)  | group 1 issues the MFMAs of stage s-1
//   phase 2s+1 : group 0 issues the 16 MFMAs of stage s                    | group 1 reads the fragments of stage s
//
// with one raw s_barrier after every phase, so the matrix pipe of every SIMD always has one wave feeding it while
// the other wave's LDS reads are in flight.  Buffer of stage s is read in phases 2s (group 0) and 2s+1 (group 1) and
// is free after the barrier that ends phase 2s+1; the DMA of stage s+NST-1 into the buffer of stage s-1 is issued by
// both groups at the start of phase 2s and has until the barrier that ends phase 2(s+NST-1)-1 to land (counted
// vmcnt: only the following stage's DMA may still be in flight there).  (Moving group 1's DMA issue out of its
// MFMA phase into its read phase was measured 2 % slower: 1.265 vs 1.237 ms per 10^6 variants, commit 4f657f1.)

template <int FMT, int NWM, int NNI, int SKB, int NST, int BUF, int GRP, bool IDLE, int LEFT, bool DIAG>
__device__ __forceinline__ void pp_stage(StageI8<NWM, SKB>* lds, const int8_t* __restrict__ p, int npad,
                                         int64_t kb_begin, int s, int ns, int col_i, int col_j, int wave, int lane,
                                         int wm, int wn, typename AccType<FMT>::type (&acc)[4][NNI],
                                         FragsI8<NNI> (&f)[SKB / 2]) {
  constexpr int NWAVES = NWM * (8 / NNI);
  constexpr int PER_WAVE = SKB * (DIAG ? 2 * NWM : 2 * NWM + 4) / NWAVES;
  constexpr int D = NST - 1;
  static_assert(D >= 1 && D * PER_WAVE < 64, "vmcnt is a 6-bit counter");
  // LEFT: the last LEFT MFMAs of a group's run are issued AFTER the barrier that ends its phase (at raised
  // priority), so the matrix pipe has work while the barrier releases and the other group's first MFMA is on its way
  constexpr int TOT = (SKB / 2) * 4 * NNI;
  const bool more = s + D < ns;  // a DMA is issued during this stage
  if constexpr (GRP == 0) {
    // ---- phase 2s: read stage s, issue the DMA of stage s+D
    if constexpr (!IDLE) {
#pragma unroll
      for (int k2 = 0; k2 < SKB / 2; ++k2) {
        if constexpr (DIAG) load_frags_diag<NWM, NNI, SKB>(&lds[BUF], k2, wm, wn, lane, f[k2]);
        else load_frags_i8<NWM, NNI, SKB>(&lds[BUF], k2, wm, wn, lane, f[k2]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
      if constexpr (DIAG)
        issue_stage_diag<NWM, SKB, NWAVES>(&lds[(BUF + D) % NST], p, npad, kb_begin + (int64_t)(s + D) * SKB, col_i, wave,
                                           lane);
      else
        issue_stage_i8<NWM, SKB, NWAVES>(&lds[(BUF + D) % NST], p, npad, kb_begin + (int64_t)(s + D) * SKB, col_i, col_j,
                                         wave, lane);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    raw_barrier();
    // ---- phase 2s+1: the MFMAs of stage s
    if constexpr (!IDLE) {
      __builtin_amdgcn_s_setprio(1);
      mfma_range<FMT, NNI, SKB, 0, TOT - LEFT>(f, acc);
      __builtin_amdgcn_s_setprio(0);
    }
  } else {
    // ---- phase 2s: issue the DMA of stage s+D, then the MFMAs of stage s-1
    if (more) {
      if constexpr (DIAG)
        issue_stage_diag<NWM, SKB, NWAVES>(&lds[(BUF + D) % NST], p, npad, kb_begin + (int64_t)(s + D) * SKB, col_i, wave,
                                           lane);
      else
        issue_stage_i8<NWM, SKB, NWAVES>(&lds[(BUF + D) % NST], p, npad, kb_begin + (int64_t)(s + D) * SKB, col_i, col_j,
                                         wave, lane);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!IDLE) {
      if (s > 0) {
        __builtin_amdgcn_s_setprio(1);
        mfma_range<FMT, NNI, SKB, 0, TOT - LEFT>(f, acc);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    raw_barrier();
    // ---- phase 2s+1: (the leftover MFMAs of stage s-1, then) read stage s
    if constexpr (!IDLE) {
      if constexpr (LEFT > 0) {
        if (s > 0) {
          __builtin_amdgcn_s_setprio(2);
          mfma_range<FMT, NNI, SKB, TOT - LEFT, TOT>(f, acc);
          __builtin_amdgcn_s_setprio(0);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int k2 = 0; k2 < SKB / 2; ++k2) {
        if constexpr (DIAG) load_frags_diag<NWM, NNI, SKB>(&lds[BUF], k2, wm, wn, lane, f[k2]);
        else load_frags_i8<NWM, NNI, SKB>(&lds[BUF], k2, wm, wn, lane, f[k2]);
      }
    }
  }
  // end of phase 2s+1: stage s+1 must have landed (own share), only the DMA of stage s+2.. may stay in flight
  if (s + 1 < ns) {
    const int rem = ns - 2 - s;  // stages after s+1 whose DMA has been issued: min(rem, D-1)
    const int keep = rem < D - 1 ? rem : D - 1;
    if (keep >= 2) wait_vmcnt<(D >= 3 ? 2 * PER_WAVE : 0)>();
    else if (keep == 1) wait_vmcnt<(D >= 2 ? PER_WAVE : 0)>();
    else wait_vmcnt<0>();
  }
  if constexpr (GRP == 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  raw_barrier();
  if constexpr (GRP == 0 && !IDLE && LEFT > 0) {  // group 0's leftover MFMAs of stage s, into phase 2(s+1)
    __builtin_amdgcn_s_setprio(2);
    mfma_range<FMT, NNI, SKB, TOT - LEFT, TOT>(f, acc);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int FMT, int NWM, int NNI, int SKB, int NST, int GRP, bool IDLE, int LEFT, bool DIAG, int... Is>
__device__ __forceinline__ void pp_round(StageI8<NWM, SKB>* lds, const int8_t* __restrict__ p, int npad,
                                         int64_t kb_begin, int s, int ns, int count, int col_i, int col_j, int wave,
                                         int lane, int wm, int wn, typename AccType<FMT>::type (&acc)[4][NNI],
                                         FragsI8<NNI> (&f)[SKB / 2], std::integer_sequence<int, Is...>) {
  ((Is < count ? pp_stage<FMT, NWM, NNI, SKB, NST, Is, GRP, IDLE, LEFT, DIAG>(lds, p, npad, kb_begin, s + Is, ns, col_i, col_j, wave,
                                                                  lane, wm, wn, acc, f)
               : (void)0),
   ...);
}

template <int FMT, int NWM, int NNI, int SKB, int NST, int GRP, bool IDLE, int LEFT, bool DIAG>
__device__ __forceinline__ void pp_loop(StageI8<NWM, SKB>* lds, const int8_t* __restrict__ p, int npad,
                                        int64_t kb_begin, int ns, int col_i, int col_j, int wave, int lane, int wm,
                                        int wn, typename AccType<FMT>::type (&acc)[4][NNI]) {
  FragsI8<NNI> f[SKB / 2];
  // prologue: stages 0 .. NST-2 go in flight; stage 0 must have landed before group 0 reads it in phase 0
  constexpr int NWAVES = NWM * (8 / NNI);
  constexpr int PER_WAVE = SKB * (DIAG ? 2 * NWM : 2 * NWM + 4) / NWAVES;
#pragma unroll
  for (int i = 0; i < NST - 1; ++i) {
    if (i < ns) {
      if constexpr (DIAG)
        issue_stage_diag<NWM, SKB, NWAVES>(&lds[i], p, npad, kb_begin + (int64_t)i * SKB, col_i, wave, lane);
      else
        issue_stage_i8<NWM, SKB, NWAVES>(&lds[i], p, npad, kb_begin + (int64_t)i * SKB, col_i, col_j, wave, lane);
    }
  }
  if (ns > 1 && NST > 2) wait_vmcnt<(NST > 2 ? PER_WAVE : 0)>();
  else wait_vmcnt<0>();
  raw_barrier();
  int s = 0;
  for (; s + NST - 1 < ns; s += NST)
    pp_round<FMT, NWM, NNI, SKB, NST, GRP, IDLE, LEFT, DIAG>(lds, p, npad, kb_begin, s, ns, NST, col_i, col_j, wave, lane, wm, wn, acc,
                                                 f, std::make_integer_sequence<int, NST>{});
  if (s < ns)
    pp_round<FMT, NWM, NNI, SKB, NST, GRP, IDLE, LEFT, DIAG>(lds, p, npad, kb_begin, s, ns, ns - s, col_i, col_j, wave, lane, wm, wn,
                                                 acc, f, std::make_integer_sequence<int, NST - 1>{});
  if constexpr (GRP == 1 && !IDLE) {  // phase 2*ns: group 1's MFMAs of the last stage, nobody to wait for
#pragma unroll
    for (int k2 = 0; k2 < SKB / 2; ++k2) mfma_step_i8<FMT, NNI>(f[k2], acc);
  }
}

template <int FMT, int NWM, int NNI, int SKB, int NST, bool PP, int LEFT = 0>
__global__ __launch_bounds__(64 * NWM * (8 / NNI), (NNI == 2) ? 2 : 1) void gram_packed_kernel(
    const int8_t* __restrict__ p, int npad, int64_t nstages, int n, int ntile, int ntri, int splitk,
    int64_t stages_per, int32_t* __restrict__ s32, int xcd_map, const int32_t* __restrict__ skip, GramStrip strip) {
  // the one schedule there is (DESIGN_HISTORY.md 4.1 / 4.2 has the others' numbers); the parameter list is the kernel's name
  static_assert(NWM == 2 && NNI == 2 && SKB == 4 && NST == 3 && PP && LEFT == 2, "ping-pong: 8 waves, group = wave / 4 = wm");
  __shared__ __attribute__((aligned(16))) StageI8<NWM, SKB> lds[NST];
  // device-side predicate of the auto mode: a pre-pass met a value other than 0 / 1 in the buffered tiles, so this
  // launch must not add anything to S (the host redoes those tiles on the int8 kernel once it reads the same word)
  if (skip != nullptr && *skip != 0) return;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr int NWN = 8 / NNI;  // waves along N
  const int wm = wave / NWN, wn = wave % NWN;

  int tile, ks;
  int row_blk = -1, col_blk = -1;
  const int b = blockIdx.x;
  if (xcd_map == 2) {
    // lock-step layout: the chip holds ALL tiles of `splitk` k-streams at once, one workgroup per CU for the whole
    // launch.  A k-stream's tiles live on a group of 8 / splitk XCDs, so every operand row is fetched into those L2s
    // once and shared by workgroups that move through k together (no second round that re-reads the slice).
    const int g = kNumXcd / splitk;               // XCDs per k-stream
    const int per = (ntri + g - 1) / g;           // tiles per XCD
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
  if (strip.cols > 0) {
    // strip owner: ALL tiles (row block, column block of the strip), in BANDS of 16 tile rows, column by column inside a
    // band -- workgroups that run together then cover ~16 x 16 tiles and share 16 + 16 operand panels (the ordering
    // that keeps the symmetric job MFMA-bound at N = 100,000, tile_coords)
    const int ctiles = ntri / ntile;
    const int per_band = BAND * ctiles;
    const int band = tile / per_band;
    const int r0 = band * BAND;
    const int h = (ntile - r0 < BAND) ? (ntile - r0) : BAND;
    const int rem = tile - band * per_band;
    row_blk = r0 + rem % h;
    col_blk = strip.cb0 + rem / h;
  } else {
    tile_coords<NWM>(tile, ntile, row_blk, col_blk);
  }

  const int64_t st_begin = (int64_t)ks * stages_per;
  const int64_t st_end = (st_begin + stages_per < nstages) ? (st_begin + stages_per) : nstages;
  if (st_begin >= st_end) return;
  const int ns = (int)(st_end - st_begin);
  const int64_t kb_begin = st_begin * SKB;
  const int col_i = row_blk * 128 * NWM, col_j = col_blk * TJ;
  // Diagonal tiles: a wave whose whole 128 x (32*NNI) sub-tile has row > column holds nothing of the
  // upper triangle; it skips its MFMAs (2 of 8 waves in 10 of 55 tiles at N = 2504).
  // (a strip owner keeps both triangles: nothing is idle there)
  const bool idle = strip.cols == 0 && (col_i + wm * 128) > (col_j + wn * 32 * NNI + 32 * NNI - 1);

  typename AccType<FMT>::type acc[4][NNI];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < NNI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0;

  if (row_blk == col_blk) {  // diagonal tile: one panel, below-diagonal waves idle (workgroup-uniform branch)
    if (wm == 0) {
      pp_loop<FMT, NWM, NNI, SKB, NST, 0, false, LEFT, true>(lds, p, npad, kb_begin, ns, col_i, col_j, wave, lane, wm, wn, acc);
    } else if (idle) {
      pp_loop<FMT, NWM, NNI, SKB, NST, 1, true, LEFT, true>(lds, p, npad, kb_begin, ns, col_i, col_j, wave, lane, wm, wn, acc);
      return;
    } else {
      pp_loop<FMT, NWM, NNI, SKB, NST, 1, false, LEFT, true>(lds, p, npad, kb_begin, ns, col_i, col_j, wave, lane, wm, wn, acc);
    }
  } else if (wm == 0) {
    pp_loop<FMT, NWM, NNI, SKB, NST, 0, false, LEFT, false>(lds, p, npad, kb_begin, ns, col_i, col_j, wave, lane, wm, wn, acc);
  } else {
    pp_loop<FMT, NWM, NNI, SKB, NST, 1, false, LEFT, false>(lds, p, npad, kb_begin, ns, col_i, col_j, wave, lane, wm, wn, acc);
  }

  if constexpr (FMT >= 1) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // last asm MFMA -> VALU read of D
  // epilogue: C/D layout col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
  // Only the upper triangle (j >= i) is authoritative; pcoa_gram_finalize mirrors it.
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int ni = 0; ni < NNI; ++ni) {
      const int j = col_j + wn * 32 * NNI + ni * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = col_i + wm * 128 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int v = (int)acc[mi][ni][r];  // fp32 accumulators hold exact integers below 2^24
        if (strip.cols > 0) {           // S[:, col0 .. col0 + cols): every row, the strip's columns, row length `cols`
          if (i < n && j >= strip.col0 && j < strip.col0 + strip.cols && v != 0)
            atomicAdd(&s32[(int64_t)i * strip.cols + (j - strip.col0)], v);
        } else if (j >= i && j < n && v != 0) {
          atomicAdd(&s32[(int64_t)i * n + j], v);
        }
      }
      // keep the float->int conversions of one MFMA tile next to their atomics: hoisting all 128 of them
      // ahead of the stores would need 128 more registers (the FP4 variant then spills)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

}  // namespace

// Lock-step launch of the FP4 / int8 contraction (gram_packed_kernel with xcd_map = 2): ntri * splitk <= #CUs
// persistent workgroups, splitk in {1, 2, 4, 8} k-streams, each on 8 / splitk XCDs (DESIGN_HISTORY.md 4.1).
hipError_t launch_gram_packed_lockstep(const int8_t* p, int fmt, int64_t nv, int32_t n, int32_t* s32, int num_cu,
                                       hipStream_t stream, const int32_t* skip) {
  if (nv <= 0) return hipSuccess;
  const int splitk = gram_lockstep_splitk(n, num_cu > 0 ? num_cu : 256);
  if (splitk == 0) return hipErrorInvalidValue;
  const int npad = (int)gram_packed_npad(n);
  const int ntile = npad / TJ;
  const int ntri = ntile * (ntile + 1) / 2;
  const int skb = 4;
  const int64_t nstages = gram_kb_pad(nv, fmt) / skb;
  const int64_t stages_per = (nstages + splitk - 1) / splitk;
  const int g = kNumXcd / splitk;
  const int per = (ntri + g - 1) / g;
  const dim3 grid((unsigned)(per * kNumXcd)), block(512);
  if (fmt == 1)
    hipLaunchKernelGGL((gram_packed_kernel<1, 2, 2, 4, 3, true, 2>), grid, block, 0, stream, p, npad, nstages, n, ntile, ntri,
                       splitk, stages_per, s32, 2, skip, GramStrip{});
  else
    hipLaunchKernelGGL((gram_packed_kernel<0, 2, 2, 4, 3, true, 2>), grid, block, 0, stream, p, npad, nstages, n, ntile, ntri,
                       splitk, stages_per, s32, 2, skip, GramStrip{});
  return hipGetLastError();
}

hipError_t launch_gram_packed(const int8_t* p, int fmt, int64_t nv, int32_t n, int32_t* s32, int num_cu,
                              hipStream_t stream, int* splitk_out, const int32_t* skip, GramStrip strip) {
  if (nv <= 0) return hipSuccess;
  // The schedule: ping-pong, 4 k-blocks per stage, 3-stage ring, two MFMAs behind the phase barrier ("243" in
  // DESIGN_HISTORY.md 4.1 / 4.2, measured 1.218 (LEFT 2) / 1.218 (4) / 1.236 (0) ms per 10^6 variants).
  const int skb = 4;
  const int npad = (int)gram_packed_npad(n);
  const int ntile = npad / TJ;
  int64_t ntri64 = (int64_t)ntile * (ntile + 1) / 2;
  if (strip.cols > 0) {  // strip owner: ntile row blocks x the column blocks that touch [col0, col0 + cols)
    strip.cb0 = strip.col0 / TJ;
    const int cb1 = (strip.col0 + strip.cols + TJ - 1) / TJ;
    ntri64 = (int64_t)ntile * (cb1 - strip.cb0);
  }
  if (ntri64 > (1 << 28)) return hipErrorInvalidValue;
  const int ntri = (int)ntri64;
  const int64_t nstages = gram_kb_pad(nv, fmt) / skb;
  // one 512-thread workgroup per CU is resident; aim at ~7 work units per CU, >= 1024 variants each
  const int64_t target = (int64_t)(num_cu > 0 ? num_cu : 256) * 7;
  int64_t splitk = (target + ntri - 1) / ntri;
  const int64_t max_by_work = nstages * skb / 64;
  if (splitk > max_by_work) splitk = max_by_work;
  if (splitk < 1) splitk = 1;
  int xcd_map = 0;
  if (splitk >= kNumXcd) {
    splitk = (splitk / kNumXcd) * kNumXcd;
    xcd_map = 1;
  }
  const int64_t stages_per = (nstages + splitk - 1) / splitk;
  const int64_t nblocks = (int64_t)ntri * splitk;
  if (nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (splitk_out) *splitk_out = (int)splitk;
  const dim3 grid((unsigned)nblocks), block(512);
  if (fmt == 1)
    hipLaunchKernelGGL((gram_packed_kernel<1, 2, 2, 4, 3, true, 2>), grid, block, 0, stream, p, npad, nstages, n, ntile, ntri,
                       (int)splitk, stages_per, s32, xcd_map, skip, strip);
  else
    hipLaunchKernelGGL((gram_packed_kernel<0, 2, 2, 4, 3, true, 2>), grid, block, 0, stream, p, npad, nstages, n, ntile, ntri,
                       (int)splitk, stages_per, s32, xcd_map, skip, strip);
  return hipGetLastError();
}

}  // namespace pcoa
