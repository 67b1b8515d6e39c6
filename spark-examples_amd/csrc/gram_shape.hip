// gram_shape.hip -- host arithmetic on the shape of a packed operand and of its launches, shared by the pre-passes, the
// contractions and the C ABI: padded sizes, workspace bytes, and what the lock-step launch fits.  No kernels.
#include <initializer_list>

#include "gram_common.h"

namespace pcoa {

int64_t gram_packed_npad(int32_t n) { return ((int64_t)n + TM - 1) / TM * TM; }
// k-blocks (16 variants for int8, 32 for FP4; 16 B per sample either way) are padded to a multiple of 24 so
// that every stage depth (4, 6 or 8 k-blocks) divides the count
int64_t gram_kb_pad(int64_t nv, int fmt) {
  const int per = fmt >= 1 ? 32 : KB;
  const int64_t nkb = (nv + per - 1) / per;
  return (nkb + 23) / 24 * 24;
}
int64_t gram_packed_kb_pad_i8(int64_t nv) { return gram_kb_pad(nv, 0); }
size_t gram_packed_workspace_bytes(int32_t n, int64_t nv) {  // the int8 size also covers the (half as large) FP4 operand
  return (size_t)gram_packed_kb_pad_i8(nv) * (size_t)gram_packed_npad(n) * KB;
}

// Lock-step launch of a contraction (gram_packed_kernel / gram_kbits_kernel / gram_kbits_w4_kernel with xcd_map = 2):
// ntri * splitk <= #CUs persistent workgroups, splitk in {1, 2, 4, 8} k-streams, each on 8 / splitk XCDs (DESIGN_HISTORY.md 4.1).
int gram_lockstep_splitk(int32_t n, int cus) {
  const int ntile = (int)(gram_packed_npad(n) / TJ);
  const int64_t ntri = (int64_t)ntile * (ntile + 1) / 2;
  if (cus < kNumXcd) return 0;
  for (int k : {8, 4, 2, 1}) {
    const int g = kNumXcd / k;
    const int64_t per = (ntri + g - 1) / g;
    if (per * kNumXcd <= cus) return k;   // one workgroup per CU, cus / 8 CUs per XCD
  }
  return 0;
}
int gram_lockstep_workgroups(int32_t n, int splitk) {
  const int ntile = (int)(gram_packed_npad(n) / TJ);
  return ntile * (ntile + 1) / 2 * splitk;
}

}  // namespace pcoa
