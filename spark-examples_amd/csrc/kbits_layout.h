// kbits_layout.h -- the k-bits operand and its LDS stage: what pack_kbits.hip writes, and what gram_kbits.hip lends
// gram_kbits_w4.hip.  Private to csrc/; anonymous namespace for the reason given in gram_common.h.
//
// Why (DESIGN_HISTORY.md 4.1): the FP4 operand costs 1.28 GB written by the pre-pass and 4.3 GB re-read by
// the contraction per 10^6 variants at N = 2504, and that L2-hit stream is what slows the fp32 pre-pass beside it.  A
// genotype indicator is one bit; as bits the operand is 0.33 GB written and ~1.1 GB re-read.
//
// Operand layout K1[V/128][Npad][4 words] ("k-bits"): the 16 bytes at K1[blk][i] are sample i's indicators for the 128
// variants of block blk, bit b of word j = variant 128 blk + 32 j + b.  A stage of the contraction is one block: 2 panels x
// 256 samples x 16 B = 8 KiB (the FP4 stage is 32 KiB), one global_load_lds_dwordx4 per wave, and the LDS image IS the
// global image.  (The word -> FP4 expansion is each contraction's own.)
#ifndef PCOA_KBITS_LAYOUT_H_
#define PCOA_KBITS_LAYOUT_H_

#include "gram_common.h"

namespace pcoa {
namespace {

struct StageBits {
  uint32_t pi[256][4];  // panel I: [sample][word]; word 2 * hi + k2 is what lane half `hi` feeds to k-step k2
  uint32_t pj[TJ][4];   // panel J
};

}  // namespace
}  // namespace pcoa

#endif  // PCOA_KBITS_LAYOUT_H_
