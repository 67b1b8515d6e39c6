// pack_packed.hip -- the pre-passes into the k-blocked FP4 / int8 operand of gram_packed.hip (layout P[kb][Npad][16 B],
// described there).  HBM-bound, one per boundary of include/pcoa.h; all of them zero the padding:
//   pack_fp4_kernel<float|uint8>   dense tile -> FP4; verifies that every value is exactly 0 or 1 (flag bit 3)
//   pack_u8x8_fp4_kernel           uint8 tile, 8-byte loads, byte-gather + spread8
//   expand_bits_fp4_kernel         carrier bitsets (1 bit per genotype) -> FP4 via v_readlane + lane-mask select
//   pack_f32_i8_kernel / pack_u8_i8_kernel / densify_csr_i8_kernel    -> int8 (values 0..127, flag bit 2 otherwise)
//   densify_csr_fp4_kernel         carrier lists without repeats -> FP4
#include <type_traits>

#include "gram_common.h"

namespace pcoa {
namespace {

// ---------------------------------------------------------------------------------------------- pack
// One thread: 16 variants x 4 samples.  A wave covers 256 consecutive samples of one k-block, so
// every load instruction reads 1 KiB contiguous and the wave writes 4 KiB contiguous.
// flag bit 2 is raised for a value that is not an integer in [0, 127].
template <int VEC>
__global__ __launch_bounds__(256) void pack_f32_i8_kernel(const float* __restrict__ x, int64_t ld, int64_t nv,
                                                          int n, int npad, int64_t nkb_pad,
                                                          int8_t* __restrict__ p, int32_t* __restrict__ flag) {
  const int groups = npad >> 2;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t kb = gid / groups;
  const int g = (int)(gid - kb * groups);
  if (kb >= nkb_pad) return;
  const int i0 = g * 4;
  float v[16][4];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int64_t row = kb * KB + t;
    if (row < nv) {
      const float* src = x + row * ld + i0;
      if (VEC == 4 && i0 + 3 < ld) {
        const float4 f = *reinterpret_cast<const float4*>(src);
        v[t][0] = f.x; v[t][1] = f.y; v[t][2] = f.z; v[t][3] = f.w;
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) v[t][s] = (i0 + s < ld) ? src[s] : 0.0f;
      }
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) v[t][s] = 0.0f;
    }
  }
  bool bad = false;
  uint32_t w[4][4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const bool live = (i0 + s) < n;  // padding columns [n, ld) may hold anything: forced to zero
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t word = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const float f = live ? v[q * 4 + b][s] : 0.0f;
        const int iv = (int)f;
        bad |= !((float)iv == f && iv >= 0 && iv <= 127);
        word |= ((uint32_t)iv & 0xffu) << (8 * b);
      }
      w[s][q] = word;
    }
  }
  uint4* dst = reinterpret_cast<uint4*>(p + ((size_t)kb * npad + i0) * KB);
  uint32_t mx = 0;  // largest multiplicity of this thread's 64 values (bytewise max of the packed words)
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    dst[s] = make_uint4(w[s][0], w[s][1], w[s][2], w[s][3]);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int b = 0; b < 4; ++b) mx = max(mx, (w[s][q] >> (8 * b)) & 0xffu);
  }
  if (bad) atomicOr(flag, 4);
  if (mx > 1) atomicMax(flag + 1, (int32_t)mx);   // binary tiles (the common case) never touch the word
}

// uint8 twin of the pre-pass: X u8 [V][ld] -> P.  One thread = 16 variants x 4 samples (16 coalesced 4-B
// loads, a 16x4 byte transpose with v_perm, 4 x 16-B stores).  2.5 + 2.56 GB per 10^6 variants.
__global__ __launch_bounds__(256) void pack_u8_i8_kernel(const uint8_t* __restrict__ x, int64_t ld, int64_t nv,
                                                         int n, int npad, int64_t nkb_pad, int8_t* __restrict__ p,
                                                         int32_t* __restrict__ flag, int vec_ok) {
  const int groups = npad >> 2;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t kb = gid / groups;
  const int g = (int)(gid - kb * groups);
  if (kb >= nkb_pad) return;
  const int i0 = g * 4;
  uint32_t v[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int64_t row = kb * KB + t;
    uint32_t w = 0;
    if (row < nv) {
      const uint8_t* src = x + row * ld + i0;
      if (vec_ok && i0 + 3 < ld) {
        w = *reinterpret_cast<const uint32_t*>(src);
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (i0 + s < ld) w |= (uint32_t)src[s] << (8 * s);
      }
    }
    // padding columns [n, ld) may hold anything: forced to zero
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (i0 + s >= n) w &= ~(0xffu << (8 * s));
    v[t] = w;
  }
  uint32_t any = 0, mx = 0;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    any |= v[t];
#pragma unroll
    for (int b = 0; b < 4; ++b) mx = max(mx, (v[t] >> (8 * b)) & 0xffu);
  }
  if (mx > 1) atomicMax(flag + 1, (int32_t)min(mx, 127u));
  uint4* dst = reinterpret_cast<uint4*>(p + ((size_t)kb * npad + i0) * KB);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      o[q] = ((v[4 * q] >> (8 * s)) & 0xffu) | (((v[4 * q + 1] >> (8 * s)) & 0xffu) << 8) |
             (((v[4 * q + 2] >> (8 * s)) & 0xffu) << 16) | (((v[4 * q + 3] >> (8 * s)) & 0xffu) << 24);
    dst[s] = make_uint4(o[0], o[1], o[2], o[3]);
  }
  if (any & 0x80808080u) atomicOr(flag, 4);  // a value above 127
}

// CSR carrier lists (RDD[Seq[Int]], VariantsPca.scala:153-168) straight into the k-blocked operand:
// one wave per variant row, +1 into byte (v % 16) of P[v / 16][sample] through a 32-bit atomic on
// the enclosing word (repeated indices count with multiplicity, as the reference's double loop does;
// a byte that would pass 127 raises flag bit 2).  P must be zero-filled beforehand.
__global__ __launch_bounds__(256) void densify_csr_i8_kernel(const int32_t* __restrict__ idx,
                                                             const int64_t* __restrict__ offs, int64_t nv,
                                                             int64_t offs_base, int8_t* __restrict__ p, int npad,
                                                             int32_t n, int32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int64_t b = offs[row] - offs_base, e = offs[row + 1] - offs_base;
  const int64_t kb = row / KB;
  const int t = (int)(row % KB);
  for (int64_t q = b + lane; q < e; q += 64) {
    const int32_t c = idx[q];
    if (c < 0 || c >= n) {
      atomicOr(flag, 1);
      continue;
    }
    uint32_t* word = reinterpret_cast<uint32_t*>(p + ((size_t)kb * npad + c) * KB) + (t >> 2);
    const uint32_t old = atomicAdd(word, 1u << (8 * (t & 3)));
    if (((old >> (8 * (t & 3))) & 0xffu) >= 127u) atomicOr(flag, 4);
  }
}

// CSR carrier lists WITHOUT repeats (the host checks) straight into the FP4 operand: one wave per variant row, the
// nibble of variant (row % 32) in sample c's 16-byte slot of k-block row / 32 is set to 0x2 through a 32-bit atomic
// OR (the 32 rows of a k-block share the slots).  The region must be zero-filled beforehand.
__global__ __launch_bounds__(256) void densify_csr_fp4_kernel(const int32_t* __restrict__ idx,
                                                              const int64_t* __restrict__ offs, int64_t nv,
                                                              int64_t offs_base, int8_t* __restrict__ p, int npad,
                                                              int32_t n, int32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nv) return;
  const int64_t b = offs[row] - offs_base, e = offs[row + 1] - offs_base;
  const int64_t kb = row / 32;
  const int t = (int)(row % 32);
  for (int64_t q = b + lane; q < e; q += 64) {
    const int32_t c = idx[q];
    if (c < 0 || c >= n) {
      atomicOr(flag, 1);
      flag[2] = c;  // one of the offending indices, for the error message (every flag buffer has >= 4 words)
      continue;
    }
    uint32_t* word = reinterpret_cast<uint32_t*>(p + ((size_t)kb * npad + c) * 16) + (t >> 3);
    const uint32_t bit = 2u << (4 * (t & 7));
    if (atomicOr(word, bit) & bit) atomicOr(flag, 32);  // a repeated callset: flag bit 5 (densify_csr_kbits_kernel)
  }
}

// ---- FP4 pre-pass: X (fp32 or uint8, values exactly 0 / 1) -> P4 [V/32][Npad][16 B], 32 nibbles per lane slice.
// One thread: 32 variants x 4 samples, in two halves of 16 variants (8 bytes of each sample's slice per half).
// flag bit 3 (value 8) is raised for a value that is not exactly 0 or 1.

template <typename T, int VEC, bool NT = false>
__global__ __launch_bounds__(256) void pack_fp4_kernel(const T* __restrict__ x, int64_t ld, int64_t nv, int n, int npad,
                                                       int64_t nkb_pad, int8_t* __restrict__ p,
                                                       int32_t* __restrict__ flag) {
  // a wave = 64 consecutive 4-sample groups of ONE k-block (npad / 4 is a multiple of 64): the k-block index is
  // wave-uniform, which keeps the row addresses in SGPRs (scalar base + one per-lane column offset)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gw = npad >> 8;  // waves per k-block
  const int64_t wid = (int64_t)blockIdx.x * 4 + wave;
  const int64_t kb = wid / gw;
  const int g = (int)(wid - kb * gw) * 64 + lane;
  if (kb >= nkb_pad) return;
  const int i0 = g * 4;
  bool bad = false;
  uint32_t badw = 0;
  uint32_t w[4][4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int q = 0; q < 4; ++q) w[s][q] = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint32_t one[16];  // bit s of one[t] = sample i0+s carries at variant 32*kb + 16*h + t
    if constexpr (VEC == 4) {
      // VEC == 4 means ld % 4 == 0: a group of 4 columns is wholly inside the row or wholly padding.  Branch-free
      // (address clamped into the tile, result masked) and in two steps -- all 16 row loads of the half first, then
      // the arithmetic -- so that 16 loads per lane are in flight; left to itself the compiler waits for every row
      // before loading the next one.
      typedef typename std::conditional<sizeof(T) == 4, f32x4_t, uint32_t>::type Raw;
      Raw raw[16];
      const int64_t col = (i0 < ld) ? i0 : 0;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int64_t row = kb * 32 + h * 16 + t;
        const T* src = x + (row < nv ? row : nv - 1) * ld + col;
        if constexpr (NT) raw[t] = __builtin_nontemporal_load(reinterpret_cast<const Raw*>(src));
        else raw[t] = *reinterpret_cast<const Raw*>(src);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int64_t row = kb * 32 + h * 16 + t;
        const uint32_t valid = (uint32_t)(row < nv) & (uint32_t)(i0 < ld);
        uint32_t bits = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {   // integer logic only: `&&` / `||` would come back as branches
          uint32_t is1, is0;
          if constexpr (sizeof(T) == 4) {
            is1 = (uint32_t)(raw[t][s] == 1.0f);
            is0 = (uint32_t)(raw[t][s] == 0.0f);
          } else {
            const uint32_t b = (raw[t] >> (8 * s)) & 0xffu;
            is1 = (uint32_t)(b == 1u);
            is0 = (uint32_t)(b == 0u);
          }
          const uint32_t live = valid & (uint32_t)(i0 + s < n);  // columns [n, ld) may hold anything
          badw |= live & ((is1 | is0) ^ 1u);
          bits |= (live & is1) << s;
        }
        one[t] = bits;
      }
    } else {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int64_t row = kb * 32 + h * 16 + t;
        uint32_t bits = 0;
        if (row < nv) {
          const T* src = x + row * ld + i0;
          T v[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) v[s] = (i0 + s < ld) ? src[s] : (T)0;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            if (i0 + s < n) {  // padding columns [n, ld) may hold anything: ignored
              const bool is1 = (v[s] == (T)1);
              bad |= !(is1 || v[s] == (T)0);
              bits |= (is1 ? 1u : 0u) << s;
            }
          }
        }
        one[t] = bits;
      }
    }
    // nibble of variant t = 0x2 (E2M1 1.0) or 0x0; 8 variants per 32-bit word
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) word |= (((one[q * 8 + b] >> s) & 1u) << 1) << (4 * b);
        w[s][h * 2 + q] = word;
      }
  }
  uint4* dst = reinterpret_cast<uint4*>(p + ((size_t)kb * npad + i0) * 16);
#pragma unroll
  for (int s = 0; s < 4; ++s) dst[s] = make_uint4(w[s][0], w[s][1], w[s][2], w[s][3]);
  if (bad || badw) atomicOr(flag, 8);
}

// uint8 input, 8-byte loads: one thread packs 32 variants x 8 samples (a wave reads 512 contiguous bytes per row
// instead of the 256 of the generic kernel above: 2504-byte rows are not line-aligned, so short segments pay for an
// extra 128-B line each).  Four batches of 8 rows; per batch the 0/1 bytes of row t are OR-ed in at bit t, which
// leaves one byte of 8 row-bits per sample, and `spread8` turns that byte into 8 FP4 nibbles (bit t -> 0x2 << 4t).
__device__ __forceinline__ uint32_t spread8_fp4(uint32_t b) {  // b < 256
  uint32_t x = (b | (b << 12)) & 0x000F000Fu;
  x = (x | (x << 6)) & 0x03030303u;
  x = (x | (x << 3)) & 0x11111111u;
  return x << 1;
}

__global__ __launch_bounds__(256) void pack_u8x8_fp4_kernel(const uint8_t* __restrict__ x, int64_t ld, int64_t nv, int n,
                                                            int npad, int64_t nkb_pad, int8_t* __restrict__ p,
                                                            int32_t* __restrict__ flag) {
  const int groups = npad >> 3;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t kb = gid / groups;
  const int g = (int)(gid - kb * groups);
  if (kb >= nkb_pad) return;
  const int i0 = g * 8;
  // byte masks of the columns that exist (< n); columns in [n, ld) may hold anything
  uint32_t m[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    uint32_t mm = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (i0 + 4 * d + b < n) mm |= 0xffu << (8 * b);
    m[d] = mm;
  }
  const bool in_row = i0 < ld;  // ld is a multiple of 8 on this path, so the whole 8-byte load is inside the row
  uint32_t o[8][4];
  uint32_t bad = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t a0 = 0, a1 = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int64_t row = kb * 32 + q * 8 + t;
      uint2 u = make_uint2(0u, 0u);
      if (row < nv && in_row) u = *reinterpret_cast<const uint2*>(x + row * ld + i0);
      u.x &= m[0];
      u.y &= m[1];
      bad |= (u.x | u.y) & 0xfefefefeu;
      a0 |= (u.x & 0x01010101u) << t;
      a1 |= (u.y & 0x01010101u) << t;
    }
#pragma unroll
    for (int sidx = 0; sidx < 4; ++sidx) {
      o[sidx][q] = spread8_fp4((a0 >> (8 * sidx)) & 0xffu);
      o[4 + sidx][q] = spread8_fp4((a1 >> (8 * sidx)) & 0xffu);
    }
  }
  uint4* dst = reinterpret_cast<uint4*>(p + ((size_t)kb * npad + i0) * 16);
#pragma unroll
  for (int sidx = 0; sidx < 8; ++sidx) dst[sidx] = make_uint4(o[sidx][0], o[sidx][1], o[sidx][2], o[sidx][3]);
  if (bad) atomicOr(flag, 8);
}

// ---- bit-packed boundary: carrier bitsets (1 bit per genotype, row v = variant v, bit i & 31 of word i >> 5 =
// sample i) -> P4.  One wave = one k-block (32 variants) x 256 samples: lane (t, j) loads the 16 bytes of row t
// that hold samples 128 j .. 128 j + 127 of the wave's range (one vector load per wave, 32 contiguous bytes per
// row).  The 32 x 32 bit transposes go through v_readlane: the two dwords of row t that belong to a group of 64
// samples land in an SGPR pair, and an SGPR pair IS a lane mask -- v_cndmask_b32 with it as condition hands every
// lane its own sample's bit as a positioned FP4 nibble.  4 VALU ops per (row, 64 samples), one coalesced 16-B store
// per lane and group.  (A first version with scalar loads instead of the vector load + readlane was 5x slower:
// 1.74 ms per 10^6 variants, scalar-cache bound.)  A bitset cannot repeat a callset, so the tile is binary by
// construction and always takes the FP4 kernel.
template <int VEC>
__global__ __launch_bounds__(256) void expand_bits_fp4_kernel(const uint32_t* __restrict__ bits, int64_t ld_words,
                                                              int64_t nv, int n, int npad, int64_t nkb_pad,
                                                              int8_t* __restrict__ p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gpk = npad >> 8;                                  // 256-sample groups per k-block
  const int64_t wid = (int64_t)blockIdx.x * 4 + wave;
  const int64_t kb = wid / gpk;
  const int G = (int)(wid - kb * gpk);
  if (kb >= nkb_pad) return;
  const int t = lane & 31, j = lane >> 5;
  const int64_t row = kb * 32 + t;
  const int64_t w = 8 * (int64_t)G + 4 * j;                   // first of this lane's four dwords
  uint32_t c[4] = {0u, 0u, 0u, 0u};
  if (row < nv) {
    const uint32_t* r = bits + row * ld_words;
    if (VEC == 4 && w + 3 < ld_words) {
      const uint4 u = *reinterpret_cast<const uint4*>(r + w);
      c[0] = u.x; c[1] = u.y; c[2] = u.z; c[3] = u.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (w + q < ld_words) c[q] = r[w + q];
    }
  }
  // bits of samples >= N (row padding, the tail of the last word) are ignored
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t first = 32 * (w + q);
    if (first >= n) c[q] = 0u;
    else if (first + 32 > n) c[q] &= (1u << (n - (int)first)) - 1u;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {                               // samples 256 G + 64 q + lane
    uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int t2 = 0; t2 < 32; ++t2) {
      const int src = t2 + 32 * (q >> 1);                     // the lane that loaded row t2, half q >> 1
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)c[2 * (q & 1)], src);
      const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)c[2 * (q & 1) + 1], src);
      const uint64_t m = ((uint64_t)hi << 32) | lo;
      uint32_t nib;
      const uint32_t one = 2u << (4 * (t2 & 7));              // E2M1 1.0 at this variant's nibble
      asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(nib) : "v"(one), "s"(m));
      o[t2 >> 3] |= nib;
    }
    *reinterpret_cast<uint4*>(p + ((size_t)kb * npad + (size_t)256 * G + 64 * q + lane) * 16) =
        make_uint4(o[0], o[1], o[2], o[3]);
  }
}

}  // namespace

// nkb_out: k-blocks to write (the tail beyond nv is zero-filled); 0 = the padded count gram_kb_pad(nv, 1)
hipError_t launch_pack_fp4(const void* x, int is_u8, int64_t ld, int64_t nv, int32_t n, int8_t* p, int32_t* flag,
                           hipStream_t stream, int64_t nkb_out) {
  if (nv <= 0) return hipSuccess;
  const int npad = (int)gram_packed_npad(n);
  const int64_t nkb_pad = nkb_out > 0 ? nkb_out : gram_kb_pad(nv, 1);
  const int64_t threads = nkb_pad * (npad >> 2);
  const int64_t blocks = (threads + 255) / 256;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(x);
  const dim3 grid((unsigned)blocks), block(256);
  if (is_u8) {
    const bool vec = ((ld & 3) == 0) && ((addr & 3) == 0);
    const uint8_t* xs = static_cast<const uint8_t*>(x);
    if (((ld & 7) == 0) && ((addr & 7) == 0)) {
      const int64_t blocks8 = (nkb_pad * (npad >> 3) + 255) / 256;
      if (blocks8 > 0x7fffffffLL) return hipErrorInvalidValue;
      hipLaunchKernelGGL(pack_u8x8_fp4_kernel, dim3((unsigned)blocks8), block, 0, stream, xs, ld, nv, n, npad, nkb_pad, p,
                         flag);
      return hipGetLastError();
    }
    if (vec) hipLaunchKernelGGL((pack_fp4_kernel<uint8_t, 4>), grid, block, 0, stream, xs, ld, nv, n, npad, nkb_pad, p, flag);
    else hipLaunchKernelGGL((pack_fp4_kernel<uint8_t, 1>), grid, block, 0, stream, xs, ld, nv, n, npad, nkb_pad, p, flag);
  } else {
    const bool vec = ((ld & 3) == 0) && ((addr & 15) == 0);
    const float* xs = static_cast<const float*>(x);
    // the fp32 tile is streamed once: nontemporal loads (measured 2.07 vs 2.15 ms per 10^6 variants)
    if (vec) hipLaunchKernelGGL((pack_fp4_kernel<float, 4, true>), grid, block, 0, stream, xs, ld, nv, n, npad, nkb_pad, p, flag);
    else hipLaunchKernelGGL((pack_fp4_kernel<float, 1>), grid, block, 0, stream, xs, ld, nv, n, npad, nkb_pad, p, flag);
  }
  return hipGetLastError();
}

// fp32 tiles the LDS-DMA-ring pre-passes (pack_kbits.hip) take: ld % 4 == 0 and a 16-byte aligned base
bool pack_fp4_ring_ok(const void* x, int64_t ld) {
  return ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
}
hipError_t launch_expand_bits_fp4(const uint32_t* bits, int64_t ld_words, int64_t nv, int32_t n, int8_t* p,
                                  hipStream_t stream, int64_t nkb_out) {
  if (nv <= 0) return hipSuccess;
  const int npad = (int)gram_packed_npad(n);
  const int64_t nkb_pad = nkb_out > 0 ? nkb_out : gram_kb_pad(nv, 1);
  const int64_t blocks = (nkb_pad * (npad >> 8) + 3) / 4;  // 4 waves per block, one (k-block, 256 samples) each
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const bool vec = ((ld_words & 3) == 0) && ((reinterpret_cast<uintptr_t>(bits) & 15) == 0);
  if (vec)
    hipLaunchKernelGGL(expand_bits_fp4_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, stream, bits, ld_words, nv, n,
                       npad, nkb_pad, p);
  else
    hipLaunchKernelGGL(expand_bits_fp4_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, stream, bits, ld_words, nv, n,
                       npad, nkb_pad, p);
  return hipGetLastError();
}

hipError_t launch_pack_f32_i8(const float* x, int64_t ld, int64_t nv, int32_t n, int8_t* p, int32_t* flag,
                              hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  const int npad = (int)gram_packed_npad(n);
  const int64_t nkb_pad = gram_packed_kb_pad_i8(nv);
  const int64_t threads = nkb_pad * (npad >> 2);
  const int64_t blocks = (threads + 255) / 256;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const bool vec4 = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
  if (vec4)
    hipLaunchKernelGGL(pack_f32_i8_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, stream, x, ld, nv, n, npad,
                       nkb_pad, p, flag);
  else
    hipLaunchKernelGGL(pack_f32_i8_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, stream, x, ld, nv, n, npad,
                       nkb_pad, p, flag);
  return hipGetLastError();
}

hipError_t launch_pack_u8_i8(const uint8_t* x, int64_t ld, int64_t nv, int32_t n, int8_t* p, int32_t* flag,
                             hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  const int npad = (int)gram_packed_npad(n);
  const int64_t nkb_pad = gram_packed_kb_pad_i8(nv);
  const int64_t threads = nkb_pad * (npad >> 2);
  const int64_t blocks = (threads + 255) / 256;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const int vec_ok = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(x) & 3) == 0);
  hipLaunchKernelGGL(pack_u8_i8_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, ld, nv, n, npad, nkb_pad, p,
                     flag, vec_ok);
  return hipGetLastError();
}

hipError_t launch_densify_csr_i8(const int32_t* idx_dev, const int64_t* offs_dev, int64_t nv, int64_t offs_base,
                                 int8_t* p, int32_t n, int32_t* flag, hipStream_t stream) {
  if (nv <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(p, 0, gram_packed_workspace_bytes(n, nv), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(densify_csr_i8_kernel, dim3((unsigned)((nv + 3) / 4)), dim3(256), 0, stream, idx_dev, offs_dev,
                     nv, offs_base, p, (int)gram_packed_npad(n), n, flag);
  return hipGetLastError();
}

// carrier lists without repeated callsets -> nkb_out = ceil(nv / 32) k-blocks of FP4 operand at p
hipError_t launch_densify_csr_fp4(const int32_t* idx_dev, const int64_t* offs_dev, int64_t nv, int64_t offs_base,
                                  int8_t* p, int32_t n, int32_t* flag, hipStream_t stream, int64_t nkb_out) {
  if (nv <= 0) return hipSuccess;
  const int npad = (int)gram_packed_npad(n);
  hipError_t e = hipMemsetAsync(p, 0, (size_t)nkb_out * (size_t)npad * 16, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(densify_csr_fp4_kernel, dim3((unsigned)((nv + 3) / 4)), dim3(256), 0, stream, idx_dev, offs_dev, nv,
                     offs_base, p, npad, n, flag);
  return hipGetLastError();
}

}  // namespace pcoa
