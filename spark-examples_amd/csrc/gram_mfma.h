// gram_mfma.h -- what the FP4 / int8 contraction (gram_packed.hip) lends the k-bits contraction (gram_kbits.hip): the
// fragment registers of one k-step, the accumulator type per operand format, and the MFMAs of a stage by number.
// Private to csrc/; anonymous namespace for the reason given in gram_common.h.
#ifndef PCOA_GRAM_MFMA_H_
#define PCOA_GRAM_MFMA_H_

#include "gram_common.h"

namespace pcoa {
namespace {

typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Fragment registers of one k32-step: (4 A + NNI B) x 16 B = 24 VGPRs at NNI = 2.
template <int NNI>
struct FragsI8 {
  i32x4 a[4];
  i32x4 b[NNI];
};

// FMT 0: int8 operands, int32 accumulators.  FMT 1: MX-FP4 operands (scales 2^0), fp32 accumulators.
template <int FMT>
struct AccType { typedef i32x16 type; };
template <>
struct AccType<1> { typedef f32x16 type; };

// MFMAs number LO .. HI-1 of a stage, in the order (k-step, mi, ni).  FMT 1 is the UNSCALED form of the instruction as
// inline asm (mfma_step_i8 of gram_packed.hip says why).
template <int FMT, int NNI, int SKB, int LO, int HI>
__device__ __forceinline__ void mfma_range(const FragsI8<NNI> (&f)[SKB / 2], typename AccType<FMT>::type (&acc)[4][NNI]) {
#pragma unroll
  for (int k2 = 0; k2 < SKB / 2; ++k2)
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < NNI; ++ni) {
        const int t = (k2 * 4 + mi) * NNI + ni;
        if (t < LO || t >= HI) continue;
        if constexpr (FMT == 0) {
          acc[mi][ni] = __builtin_amdgcn_mfma_i32_32x32x32_i8(f[k2].a[mi], f[k2].b[ni], acc[mi][ni], 0, 0, 0);
        } else {
          asm volatile("v_mfma_f32_32x32x64_f8f6f4 %0, %1, %2, %0 cbsz:4 blgp:4"
                       : "+v"(acc[mi][ni])
                       : "v"(f[k2].a[mi]), "v"(f[k2].b[ni]));
        }
      }
}

}  // namespace
}  // namespace pcoa

#endif  // PCOA_GRAM_MFMA_H_
