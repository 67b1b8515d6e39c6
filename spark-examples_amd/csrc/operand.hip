// operand.hip -- S and the operands that are contracted into it: the int32 partial and its int64 fold, the operand buffers
// of the binary-tile path (fp4_setup ... fp4_commit) with the int8 fallback, the device-resident input forms
// (gram_device, gram_device_bits), and what every reader of S calls first (finalize_impl, check_device_flags).
#include <algorithm>
#include <cstring>

#include "pcoa_ctx.h"

using namespace pcoa;

namespace pcoa {

// an int64 matrix for a ctx that has none: the one narrow_s64 retired, else a fresh one (contents undefined either way)
int take_s64(pcoa_ctx* c) {
  if (c->s64) return PCOA_OK;
  if (c->s64_spare) {
    c->s64 = c->s64_spare;
    c->s64_spare = nullptr;
    return PCOA_OK;
  }
  HIP_TRY(c, dev_alloc((void**)&c->s64, sizeof(int64_t) * s_count(c), c->device));
  return PCOA_OK;
}

// the int64 matrix is no longer part of S (nothing queued may still touch it): kept as the spare a later fold or import
// takes, or freed -- and a spare the ctx already holds is freed, never overwritten
void retire_s64(pcoa_ctx* c) {
  if (!c->s64) return;
  if (s_count(c) * sizeof(int64_t) <= ((size_t)1 << 30) && !c->s64_spare) {
    c->s64_spare = c->s64;   // kept: a later fold needs one again
  } else {
    dev_free(c->s64);        // large N: 8 N^2 bytes are worth more than the allocation they would save
  }
  c->s64 = nullptr;
}

int fold_now(pcoa_ctx* c) {
  const int64_t count = (int64_t)s_count(c);
  if (!c->s64) {
    const int rc = take_s64(c);
    if (rc != PCOA_OK) return rc;
    HIP_TRY(c, hipMemsetAsync(c->s64, 0, sizeof(int64_t) * (size_t)count, c->stream));
  }
  // s64 is kept symmetric: mirror the partial before it is folded in (a strip holds both triangles already)
  if (!c->is_strip) HIP_TRY(c, launch_symmetrize_i32(c->s32, c->n, c->stream));
  HIP_TRY(c, launch_fold_i32_to_i64(c->s32, c->s64, count, c->stream));
  c->variants_in_s32 = 0;
  c->dirty = false;
  return PCOA_OK;
}


// the exchange buffer, at least `bytes` large (its old contents are never needed across a growth)
int ensure_xfer(pcoa_ctx* c, size_t bytes) {
  if (c->xfer && c->xfer_bytes >= bytes) return PCOA_OK;
  c->xfer_bytes = 0;
  const int rc = regrow(c, (void**)&c->xfer, bytes, true);
  if (rc == PCOA_OK) c->xfer_bytes = bytes;
  return rc;
}

// S has just been handed in or reduced as an int64 matrix (import / load / int64 reductions) and the int32 partial is zero.
// If every entry fits int32 -- any cohort below 2^31 variants: configs[2]'s whole genome is 4 * 10^7 -- S moves back into the
// int32 matrix and the int64 one is retired: half the bytes for every later pass, and the large-N upper-triangle forms of
// computePca (rowsums_sym_tiles_kernel, symv_sym_tiles_kernel) stay available after a multi-GPU reduction or a checkpoint
// resume (VERDICT r05 Weak 3).  One pass over the int64 matrix; synchronises.
int narrow_s64(pcoa_ctx* c) {
  if (!c->s64 || debug_knobs().no_narrow) return PCOA_OK;
  const int64_t count = (int64_t)s_count(c);
  if (!c->narrow_flag) HIP_TRY(c, dev_alloc((void**)&c->narrow_flag, 16, c->device));
  HIP_TRY(c, hipMemsetAsync(c->narrow_flag, 0, 16, c->stream));
  HIP_TRY(c, launch_narrow_i64_to_i32(c->s64, c->s32, count, c->narrow_flag, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->hw->coll, c->narrow_flag, 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int32_t overflow = (int32_t)(c->hw->coll[0] & 0xffffffff);
  const int64_t maxabs = c->hw->coll[1];
  if (overflow) {  // S really needs 64 bits: the int32 matrix goes back to zero
    HIP_TRY(c, hipMemsetAsync(c->s32, 0, sizeof(int32_t) * (size_t)count, c->stream));
    return PCOA_OK;
  }
  retire_s64(c);
  c->variants_in_s32 = maxabs;   // an upper bound of every |entry|, which is what the fold and the int32 reductions go by
  c->narrowed += 1;
  return PCOA_OK;
}

// bookkeeping shared by every Gram launch.  `weight` bounds what one variant can add to an entry of S: 1 for binary
// tiles, m^2 for carrier multiplicities up to m.  variants_in_s32 is therefore an upper bound of every int32 partial;
// the int64 fold and the int32 fast path of the all-reduce go by it.
void account_gram(pcoa_ctx* c, int64_t cur, int64_t weight) {
  c->gram_launches += 1;
  c->gram_variants += cur;
  c->gram_flops += 2.0 * (double)cur * (double)c->n * (double)c->n;
  c->gram_bytes += 4.0 * (double)cur * (double)c->n + 4.0 * (double)c->n * (double)c->n;
  c->variants_in_s32 += cur * weight;
  c->dirty = true;
  c->strip_centering_set = false;  // S changes: the row means of an earlier computePca no longer belong to it
}

int fold_if_needed(pcoa_ctx* c, int64_t cur) {
  if (c->variants_in_s32 + cur > c->fold_threshold) {
    int rc = fp4_quiesce(c);  // contractions queued on the side streams still add into S32
    if (rc != PCOA_OK) return rc;
    ScopedTimer t(c, T_FINALIZE);
    return fold_now(c);
  }
  return PCOA_OK;
}

static int64_t fp4_kb_bytes(const pcoa_ctx* c) { return gram_packed_npad(c->n) * (c->op_fmt == 2 ? 4 : 16); }
// k-blocks (of 32 variants) a chunk of nv variants takes in the operand buffer
int64_t kb_of(const pcoa_ctx* c, int64_t nv) {
  const int64_t kb = (nv + 31) / 32;
  return c->op_fmt == 2 ? round_up(kb, 4) : kb;
}
// the three pre-passes onto the binary-tile operand, in the ctx's operand format
static hipError_t launch_pack_operand(const pcoa_ctx* c, const void* x, int is_u8, int64_t ld, int64_t nv, int8_t* dst, int32_t* flag,
                               hipStream_t s, int64_t kb, int ring_wgs = 0) {
  // ring_wgs > 0: the persistent ring pre-pass of the co-resident fp32 pipeline (fp32 tile, k-bits operand, ring_ok checked)
  if (ring_wgs > 0 && c->op_fmt == 2 && !is_u8)
    return launch_pack_kbits_ring(static_cast<const float*>(x), ld, nv, c->n, dst, flag, s, kb / 4, ring_wgs);
  if (ring_wgs > 0 && c->op_fmt == 2 && is_u8)
    return launch_pack_kbits_ring_u8(static_cast<const uint8_t*>(x), ld, nv, c->n, dst, flag, s, kb / 4, ring_wgs);
  return c->op_fmt == 2 ? launch_pack_kbits(x, is_u8, ld, nv, c->n, dst, flag, s, kb / 4)
                        : launch_pack_fp4(x, is_u8, ld, nv, c->n, dst, flag, s, kb);
}
static hipError_t launch_bits_operand(const pcoa_ctx* c, const uint32_t* bits, int64_t ld_words, int64_t nv, int8_t* dst, hipStream_t s,
                               int64_t kb) {
  return c->op_fmt == 2 ? launch_transpose_bits_kbits(bits, ld_words, nv, c->n, dst, s, kb / 4)
                        : launch_expand_bits_fp4(bits, ld_words, nv, c->n, dst, s, kb);
}
hipError_t launch_csr_operand(const pcoa_ctx* c, const int32_t* idx, const int64_t* offs, int64_t nv, int64_t offs_base,
                              int8_t* dst, hipStream_t s, int64_t kb) {
  return c->op_fmt == 2 ? launch_densify_csr_kbits(idx, offs, nv, offs_base, dst, c->n, c->err_flag, s, kb / 4)
                        : launch_densify_csr_fp4(idx, offs, nv, offs_base, dst, c->n, c->err_flag, s, kb);
}
static int32_t* fb_flag(pcoa_ctx* c, int b) { return c->fb_flags + 16 * b; }

// k-blocks a buffer is meant to hold
int64_t fp4_target_kb(const pcoa_ctx* c) {
  const int64_t per_kb = fp4_kb_bytes(c);
  const int64_t by_launch = (c->fb_count == 2) ? kPipeVariants : kBatchVariants;
  return std::max<int64_t>(1, std::min(std::min(c->max_launch, by_launch) / 32, kBatchBytes / per_kb));
}

// `side` runs behind everything queued on the ctx stream so far
static int fork_to(pcoa_ctx* c, hipStream_t side) {
  if (side == c->stream) return PCOA_OK;
  // an idle ctx stream has nothing to wait for: no marker + barrier packet in front of every pre-pass and contraction of the
  // steady state (they cost 7 % of the fp32 step, profiles/r04w)
  if (hipStreamQuery(c->stream) == hipSuccess) return PCOA_OK;
  (void)hipGetLastError();
  HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
  HIP_TRY(c, hipStreamWaitEvent(side, c->ev_fork, 0));
  return PCOA_OK;
}

// int8 path of one chunk: pre-pass into the workspace and contraction at once, on the ctx stream.  The pre-pass
// reports the largest carrier multiplicity m it met; one variant adds at most m^2 to an entry of S, so the launch is
// cut into pieces of < 2^31 / m^2 variants (int32 accumulators and partials) and the books carry the weight m^2.
static int int8_chunk(pcoa_ctx* c, const void* x_chunk, int is_u8, int64_t cur, int64_t ld) {
  int rc = PCOA_OK;
  // Everything the FP4 side has in flight is resolved BEFORE this chunk touches the shared int8 workspace: resolving a
  // buffer whose pre-pass met a multiplicity re-enters this function (fp4_resolve -> redo), and a redo between this
  // chunk's pre-pass and its contraction -- the int64 fold inside the launch loop below used to trigger one -- would
  // overwrite pack_buf, or reallocate it, under the contraction that is about to read it.  After this
  // point nothing is launched or flagged, so the fold below cannot re-enter.
  if ((rc = fp4_quiesce(c)) != PCOA_OK) return rc;
  const int64_t need = (int64_t)gram_packed_workspace_bytes(c->n, cur);
  if ((rc = ensure(c, &c->pack_buf, &c->pack_cap, need)) != PCOA_OK) return rc;
  HIP_TRY(c, hipMemsetAsync(c->err_flag + 1, 0, sizeof(int32_t), c->stream));
  {
    ScopedTimer t(c, T_PACK);
    hipError_t e = is_u8 ? launch_pack_u8_i8(static_cast<const uint8_t*>(x_chunk), ld, cur, c->n, c->pack_buf,
                                             c->err_flag, c->stream)
                         : launch_pack_f32_i8(static_cast<const float*>(x_chunk), ld, cur, c->n, c->pack_buf,
                                              c->err_flag, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "pack(i8) kernel launch");
    c->pack_launches += 1;
    c->pack_bytes += (is_u8 ? 1.0 : 4.0) * (double)cur * (double)c->n + (double)need;
  }
  HIP_TRY(c, hipMemcpyAsync(&c->hw->mmax, c->err_flag + 1, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int32_t mmax = c->hw->mmax;
  const int64_t weight = (int64_t)std::max(1, mmax) * std::max(1, mmax);
  // (< 2^30 per launch on top of a partial that is folded before it passes 2^30: every int32 stays below 2^31)
  const int64_t per_launch = std::max<int64_t>(24 * KB_I8, ((int64_t)1 << 30) / weight / (24 * KB_I8) * (24 * KB_I8));
  const int64_t row_bytes = gram_packed_npad(c->n) * 16;  // one k-block of 16 variants
  for (int64_t v0 = 0; v0 < cur; v0 += per_launch) {
    const int64_t part = std::min(per_launch, cur - v0);
    if ((rc = fold_if_needed(c, part * weight)) != PCOA_OK) return rc;
    {
      ScopedTimer t(c, T_GRAM);
      hipError_t e = launch_gram_packed(c->pack_buf + (v0 / KB_I8) * row_bytes, 0, part, c->n, c->s32, c->num_cu, c->stream,
                                        nullptr, nullptr, strip_of(c));
      if (e != hipSuccess) return hip_fail(c, e, "packed gram kernel launch");
    }
    c->gram_kind = 2;
    account_gram(c, part, weight);
  }
  return PCOA_OK;
}

// Lazily creates what the FP4 path needs besides the operand memory: the buffer flags (device + pinned host), the
// events, and -- where the shape fits -- the two side streams of the fp32 pipeline.
int fp4_setup(pcoa_ctx* c) {
  if (c->fb_flags) return PCOA_OK;
  HIP_TRY(c, dev_alloc((void**)&c->fb_flags, 256, c->device));
  HIP_TRY(c, hipMemsetAsync(c->fb_flags, 0, 256, c->stream));
  HIP_TRY(c, hipHostMalloc((void**)&c->fb_flags_host, 256, hipHostMallocDefault));
  std::memset(c->fb_flags_host, 0, 256);
  HIP_TRY(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  for (auto& b : c->fb) {
    HIP_TRY(c, hipEventCreateWithFlags(&b.packed, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&b.consumed, hipEventDisableTiming));
  }
  const DebugKnobs& k = debug_knobs();
  // lock-step contraction on the whole chip: used when it fills >= 80 % of the CUs
  const int ls = gram_lockstep_splitk(c->n, c->num_cu);
  c->lockstep_ok = !c->is_strip && ls > 0 && gram_lockstep_workgroups(c->n, ls) * 5 >= c->num_cu * 4;
  if (k.lockstep == 0) c->lockstep_ok = false;
  if (k.lockstep == 1) c->lockstep_ok = !c->is_strip && ls > 0;
  // k-bits operand: the EVEN-SPLIT launch (one workgroup per CU, each an equal run of (tile, 128-variant stage) units)
  // wherever the output has few tiles -- it fills all CUs whatever the tile count is (the lock-step launch leaves 36 of
  // 256 idle at N = 2504), and the 4x smaller operand stream affords the loss of operand sharing.  Large N (many more
  // tiles than CUs) keeps the banded split-K order that shares panels between concurrent workgroups.
  {
    const int64_t ntile = gram_packed_npad(c->n) / 256;
    const int64_t ntri = c->is_strip ? ntile * ((c->s_cols + 255) / 256 + 1) : ntile * (ntile + 1) / 2;
    c->kbits_mode = (ntri <= 4 * (int64_t)c->num_cu) ? 4 : 0;
    if (k.kbits_mode == 0 || k.kbits_mode == 4) c->kbits_mode = k.kbits_mode;
    if (k.kbits_mode == 5 && c->kbits_mode == 4) c->kbits_mode = 5;   // even split per XCD k-segment (gram_kbits_w4.hip, xcd_map 5)
    if (k.kbits_mode == 2 && !c->is_strip && ls > 0) c->kbits_mode = 2;
  }
  // fp32 pipeline: the contraction of one operand buffer beside the pre-pass of the next, on two side streams.
  //  FP4 operand: a lock-step contraction sized for HALF the chip (split-K 2 at N = 2504: 110 workgroups, one per CU)
  //  that fills >= 80 % of that half; k-bits operand: an even-split contraction of `pipe_gram_cus` workgroups.
  // No CU masks: a contraction workgroup takes 2 x 224..256 of a SIMD's 512 VGPRs, a pre-pass wave needs 96..136, so the
  // two never share a CU (sharing one is negative-sum: the CU's vector-memory path returns in order) -- provided the
  // contraction's workgroups are placed FIRST, which a 10-us one-wave spin in front of a generation's first pre-pass
  // ensures (fp4_reserve).  Against static 16 + 16 CU masks (hipExtStreamCreateWithCUMask) this is 5 % faster: the
  // pre-pass gets the CUs the contraction does not use, and the whole chip once the contraction is done
  // (profiles/r02n_overlap_harness.txt; k-bits: profiles/r03*_kbits_harness.txt).
  const int half = c->num_cu / 2;
  const int lsh = gram_lockstep_splitk(c->n, half);
  // (worth it whenever the contraction is a real share of the step: from ~5 tile columns, N > 1024)
  bool want = !c->is_strip && c->num_cu >= 64 && lsh > 0 && gram_packed_npad(c->n) >= 5 * 256;
  // the co-resident form (k-bits operand) does not need a lock-step launch that fits half the chip: any N whose contraction
  // is a real share of the step, up to kCoresideMaxNpad: +25 % at N = 3,072, +30 % at 4,096, +23 % at 8,192 over the serial
  // order, which is what these N had before, +8 .. 9 % at N = 10,240 .. 16,384 where the contraction dominates
  // (profiles/r03zi_coreside_large_n.txt, r03zn_coreside_n10k_16k.txt)
  const bool cores_shape = !c->is_strip && c->num_cu >= 64 && c->op_fmt == 2 && k.kbits_coreside != 0 &&
                           gram_packed_npad(c->n) >= 5 * 256 && gram_packed_npad(c->n) <= kCoresideMaxNpad;
  want = want || cores_shape;
  if (k.pipeline == 0) want = false;
  if (k.pipeline == 1) want = !c->is_strip && (lsh > 0 || cores_shape);
  if (c->flags & PCOA_FLAG_NO_PIPELINE) want = false;
  if (want) {
    hipError_t e1 = hipStreamCreateWithFlags(&c->pack_stream, hipStreamNonBlocking);
    hipError_t e2 = (e1 == hipSuccess) ? hipStreamCreateWithFlags(&c->gram_stream, hipStreamNonBlocking) : e1;
    if (e1 == hipSuccess && e2 == hipSuccess) {
      c->pipe_ok = true;
      c->pipe_gram_cus = half;
      c->fb_count = 2;
      // k-bits operand: the two kernels SHARE every CU instead (r03s .. r03u): the contraction (224 VGPRs per wave, 24 KiB
      // of LDS) takes the whole chip -- lock-step where the shape fits, so that the 36 CUs it leaves at N = 2504 run
      // pre-pass waves only -- and two workgroups per CU of the persistent ring pre-pass (40 VGPRs, 32 KiB) land beside it.
      // The head start still matters: the contraction's workgroups must find every CU able to take one.
      if (c->op_fmt == 2 && k.kbits_coreside != 0) {
        c->coreside = true;
        // (lock-step only where it fills >= 80 % of the CUs: at N = 2048 it has 144 workgroups and the co-resident step
        // loses to the disjoint form, 1.87 vs 1.65 ms, profiles/r03y; the even split always has one workgroup per CU)
        c->coreside_mode = (ls > 0 && gram_lockstep_workgroups(c->n, ls) * 5 >= c->num_cu * 4 && k.kbits_mode != 4) ? 2 : c->kbits_mode;
        if (k.kbits_mode == 2 && ls > 0) c->coreside_mode = 2;
        c->pipe_gram_cus = c->num_cu;
        c->ring_wgs = 2 * c->num_cu;
      }
    } else {
      (void)hipGetLastError();
      if (c->pack_stream) (void)hipStreamDestroy(c->pack_stream);
      c->pack_stream = c->gram_stream = nullptr;
    }
  }
  if (c->op_fmt == 2 && c->kbits_mode != 0) c->fb_count = 2;  // cheap epilogue (<= 2 tiles per workgroup)
  if (!c->pipe_ok && c->lockstep_ok) c->fb_count = 2;  // cheap epilogue: 2^20-variant launches from alternating buffers
  return PCOA_OK;
}

// Queue the contraction of buffer b's current generation.  overlapped: more fp32 pre-passes are coming, so the
// contraction goes to the contraction stream, sized for half the chip; otherwise it takes the whole chip on the ctx stream.
// side_kind: what will run beside it (the chunk that found the buffer full): 1 fp32 tile, 2 uint8 tile, 3 bitset tile.
static int fp4_launch(pcoa_ctx* c, int bi, bool overlapped, int side_kind = 1) {
  pcoa_ctx::Fp4Buf& b = c->fb[bi];
  // carrier lists committed provisionally into this generation are validated (and rolled back, if need be) before the
  // generation can reach S
  int rc = (bi == c->fb_active && !c->csr_pending.empty()) ? csr_validate(c) : PCOA_OK;
  if (rc != PCOA_OK) return rc;
  if (b.kb == 0) return PCOA_OK;
  rc = fold_if_needed(c, b.vars);
  if (rc != PCOA_OK) return rc;
  const int64_t per_kb = fp4_kb_bytes(c);
  const int64_t kb_pad = round_up(b.kb, 24);
  const bool side = overlapped && c->pipe_ok;
  hipStream_t gs = side ? c->gram_stream : c->stream;
  // whole stages only: zero k-blocks behind the data (on the filling stream: moved behind the wait on the contraction's
  // stream it delays the contraction into the next pre-pass, 2.38 vs 2.11 ms per step, profiles/r04w)
  if (kb_pad > b.kb)
    HIP_TRY(c, hipMemsetAsync(b.p + b.kb * per_kb, 0, (size_t)((kb_pad - b.kb) * per_kb), b.fill_stream));
  if (gs != b.fill_stream) {
    HIP_TRY(c, hipEventRecord(b.packed, b.fill_stream));
    HIP_TRY(c, hipStreamWaitEvent(gs, b.packed, 0));
  }
  if ((rc = fork_to(c, gs)) != PCOA_OK) return rc;  // e.g. a pcoa_reset memset of S queued on the ctx stream
  const int cus = side ? c->pipe_gram_cus : c->num_cu;
  const int32_t* skip = b.verify ? fb_flag(c, bi) : nullptr;
  {
    ScopedTimer t(c, T_GRAM, gs);
    hipError_t e = hipErrorInvalidValue;
    if (c->op_fmt == 2) {
      // k-bits: beside the pre-pass an even split over `pipe_gram_cus` workgroups, else the whole-chip form chosen in fp4_setup
      // (beside the short bitset transpose the even split wins: 1.07 vs 1.11 ms per step, profiles/r03zd)
      const int mode = !side ? c->kbits_mode : !c->coreside ? 4 : (side_kind == 3 ? c->kbits_mode : c->coreside_mode);
      // The one-wave-per-SIMD kernel (512 registers per wave, gram_kbits_w4.hip) wherever the contraction has its CUs to
      // itself; beside the ring pre-pass the two-waves-per-SIMD kernel held to 224 registers, which leaves room for it.
      const bool use_w4 = debug_knobs().kbits_w4 != 0 && !(side && c->coreside);
      auto launch = [&](int m) {
        return use_w4 ? launch_gram_kbits_w4(b.p, b.kb * 32, c->n, c->s32, cus, gs, m, skip, strip_of(c), debug_knobs().kbits_w4_diag)
                      : launch_gram_kbits(b.p, b.kb * 32, c->n, c->s32, cus, gs, m, skip, strip_of(c));
      };
      e = launch(mode);
      if (e != hipSuccess && mode != 0) {
        (void)hipGetLastError();
        e = launch(0);
      } else if (e == hipSuccess) {
        if (mode == 2) c->lockstep_launches += 1;
        if (mode == 4 || mode == 5) c->evensplit_launches += 1;
        if (side) c->pipeline_launches += 1;
      }
    } else {
      if (side || c->lockstep_ok) e = launch_gram_packed_lockstep(b.p, 1, b.kb * 32, c->n, c->s32, cus, gs, skip);
      if (e == hipSuccess) {
        c->lockstep_launches += 1;
        if (side) c->pipeline_launches += 1;
      }
      if (e != hipSuccess) {
        (void)hipGetLastError();
        e = launch_gram_packed(b.p, 1, b.kb * 32, c->n, c->s32, cus, gs, nullptr, skip, strip_of(c));
      }
    }
    if (e != hipSuccess) return hip_fail(c, e, "packed gram kernel launch");
  }
  if (b.verify)
    HIP_TRY(c, hipMemcpyAsync(c->fb_flags_host + 16 * bi, fb_flag(c, bi), sizeof(int32_t), hipMemcpyDeviceToHost, gs));
  HIP_TRY(c, hipEventRecord(b.consumed, gs));
  b.launched = true;
  b.launched_vars = b.vars;
  c->gram_kind = 3;
  account_gram(c, b.vars);
  b.kb = 0;
  b.vars = 0;
  return PCOA_OK;
}

// Wait for buffer b's queued contraction and, in auto mode, learn whether its pre-passes met a value other than
// 0 / 1: the contraction then did nothing (device-side predicate) and the generation's chunks are redone on the int8
// kernel -- their inputs are device pointers, valid until the next synchronising call returns (include/pcoa.h).
static int fp4_resolve(pcoa_ctx* c, int bi, bool redo = true) {
  pcoa_ctx::Fp4Buf& b = c->fb[bi];
  if (!b.launched) {
    if (b.kb == 0) b.chunks.clear();
    return PCOA_OK;
  }
  HIP_TRY(c, hipEventSynchronize(b.consumed));
  b.launched = false;
  int rc = PCOA_OK;
  if (b.verify && c->fb_flags_host[16 * bi] != 0) {
    // the skipped launch added nothing: take its variants back out of the books
    c->gram_variants -= b.launched_vars;
    c->gram_flops -= 2.0 * (double)b.launched_vars * (double)c->n * (double)c->n;
    c->gram_bytes -= 4.0 * (double)b.launched_vars * (double)c->n + 4.0 * (double)c->n * (double)c->n;
    c->variants_in_s32 -= b.launched_vars;
    c->fb_flags_host[16 * bi] = 0;
    HIP_TRY(c, hipMemsetAsync(fb_flag(c, bi), 0, sizeof(int32_t), c->stream));
    if (redo) {
      c->fp4_fallbacks += (int64_t)b.chunks.size();
      c->i8_streak = 8;  // then FP4 is tried again
      std::vector<pcoa_ctx::Fp4Chunk> chunks;
      chunks.swap(b.chunks);
      for (const auto& ch : chunks)
        if ((rc = int8_chunk(c, ch.x, ch.is_u8, ch.nv, ch.ld)) != PCOA_OK) break;
    }
  }
  b.chunks.clear();
  return rc;
}

// Everything the FP4 path has queued anywhere has finished (and been verified) when this returns.
int fp4_quiesce(pcoa_ctx* c) {
  int rc = c->csr_pending.empty() ? PCOA_OK : csr_validate(c);  // a synchronising call: the caller may release its arrays next
  for (int bi = 0; bi < 2 && rc == PCOA_OK; ++bi) rc = fp4_resolve(c, bi);
  if (rc != PCOA_OK) return rc;
  for (auto& b : c->fb)   // pre-passes of a generation still being filled on the masked stream
    if (b.kb > 0 && b.fill_stream && b.fill_stream != c->stream) HIP_TRY(c, hipStreamSynchronize(b.fill_stream));
  return PCOA_OK;
}

// Contract what the FP4 operand buffers hold into S32 and wait for it: S is needed.
int fp4_flush(pcoa_ctx* c) {
  int rc = PCOA_OK;
  for (int bi = 0; bi < 2; ++bi)
    if (c->fb[bi].kb > 0 && (rc = fp4_launch(c, bi, false)) != PCOA_OK) return rc;
  return fp4_quiesce(c);
}

// A synchronising call that does not need S (pcoa_sync, timings): afterwards the caller may release the device inputs
// of earlier accumulate calls, so generations whose verification is still owed (auto mode, device pointers) are
// contracted and verified now; generations that owe nothing (host tiles, bitsets, carrier lists) stay buffered.
int fp4_sync_point(pcoa_ctx* c) {
  int rc = PCOA_OK;
  for (int bi = 0; bi < 2; ++bi)
    if (c->fb[bi].kb > 0 && c->fb[bi].verify && (rc = fp4_launch(c, bi, false)) != PCOA_OK) return rc;
  return fp4_quiesce(c);
}

// S is being replaced or zeroed: what is buffered or in flight for the old S goes with it.
int fp4_discard(pcoa_ctx* c) {
  if (!c->csr_pending.empty()) {  // they go with the S they were meant for
    const int rc = staging_wait_all(c, c->cs);
    if (rc != PCOA_OK) return rc;
    c->csr_pending.clear();
    if (c->csr_flag) HIP_TRY(c, hipMemsetAsync(c->csr_flag, 0, 16, c->stream));
  }
  for (int bi = 0; bi < 2; ++bi) {
    pcoa_ctx::Fp4Buf& b = c->fb[bi];
    int rc = fp4_resolve(c, bi, false);
    if (rc != PCOA_OK) return rc;
    if (b.kb > 0 && b.fill_stream && b.fill_stream != c->stream) HIP_TRY(c, hipStreamSynchronize(b.fill_stream));
    b.kb = 0;
    b.vars = 0;
    b.chunks.clear();
  }
  return PCOA_OK;
}

// Capacity for kb more k-blocks in buffer bi (contents kept).  The buffer grows straight to its target size when the
// calls are large, geometrically when they are small.
int fp4_grow(pcoa_ctx* c, int bi, int64_t kb, int64_t chunk_variants) {
  pcoa_ctx::Fp4Buf& b = c->fb[bi];
  if (b.kb + kb <= b.cap_kb) return PCOA_OK;
  const int64_t per_kb = fp4_kb_bytes(c);
  const int64_t target = std::max(fp4_target_kb(c), kb);
  const int64_t floor_kb = std::max<int64_t>(1, std::min<int64_t>(1024, ((int64_t)256 << 20) / per_kb));
  int64_t want = (chunk_variants >= ((int64_t)1 << 18))
                     ? target
                     : std::min(target, std::max(std::max(b.kb + kb, floor_kb), 2 * b.cap_kb));
  int8_t* fresh = nullptr;
  for (;;) {
    hipError_t e = dev_alloc((void**)&fresh, (size_t)((want + 24) * per_kb), c->device);
    if (e == hipSuccess) break;
    (void)hipGetLastError();
    if (want <= b.kb + kb) return hip_fail(c, e, "allocation of the FP4 operand buffer");
    want = std::max(b.kb + kb, want / 2);
  }
  hipStream_t s = b.fill_stream ? b.fill_stream : c->stream;
  if (b.kb > 0) HIP_TRY(c, hipMemcpyAsync(fresh, b.p, (size_t)(b.kb * per_kb), hipMemcpyDeviceToDevice, s));
  HIP_TRY(c, hipStreamSynchronize(s));   // the old buffer may still be read by queued kernels ...
  if (b.launched) HIP_TRY(c, hipEventSynchronize(b.consumed));  // ... or by its last contraction
  if (b.p) dev_free(b.p);
  b.p = fresh;
  b.cap_kb = want;
  // Large calls alternate between the two buffers: size the idle twin now as well, so that the second call of a stream
  // does not allocate inside what the caller may be timing (35 ms on one box: VERDICT r02 Weak 6).
  if (c->fb_count == 2 && chunk_variants >= ((int64_t)1 << 18)) {
    pcoa_ctx::Fp4Buf& o = c->fb[bi ^ 1];
    if (o.cap_kb < want && o.kb == 0 && !o.launched) {
      int8_t* twin = nullptr;
      if (dev_alloc((void**)&twin, (size_t)((want + 24) * per_kb), c->device) == hipSuccess) {
        if (o.p) dev_free(o.p);
        o.p = twin;
        o.cap_kb = want;
      } else {
        (void)hipGetLastError();  // it will be tried again, at its own size, when the buffer is needed
      }
    }
  }
  return PCOA_OK;
}

// Where the next `kb` k-blocks of packed operand go: *dst in the active buffer, to be written on *stream (already
// ordered behind the ctx stream).  deferrable_f32: the chunk is an fp32 device tile whose pre-pass may run on the
// masked stream beside a contraction in flight; verify: its pre-pass reports non-binary values through *flag.
int fp4_reserve(pcoa_ctx* c, int64_t kb, int64_t chunk_variants, int side_kind, bool verify, int8_t** dst,
                hipStream_t* stream, int32_t** flag) {
  int rc = fp4_setup(c);
  if (rc != PCOA_OK) return rc;
  pcoa_ctx::Fp4Buf* b = &c->fb[c->fb_active];
  // side_kind: 0 = the chunk's pre-pass must run on the ctx stream; 1 = fp32 device tile that may run beside a contraction
  // (either pipeline form); 2 / 3 = uint8 / bitset device tile: only the co-resident form has pre-passes that fit beside one
  // (bitsets, r05: their transpose is 0.19 ms per 10^6 variants, and beside it the contraction has to be the kernel held to 224
  // registers: same box, one engine, 1.13-1.15 ms per step co-resident against 1.10-1.14 for the transpose followed by the
  // one-wave-per-SIMD kernel alone on the chip (tools/alt_inputs_ab.py, profiles/r05d) -- and the series does not depend on the
  // two side streams landing on different hardware queues.  Bitsets stay on the ctx stream unless PCOA_BITS_PIPELINE=1.)
  const bool want_side = c->pipe_ok && (side_kind == 1 || (side_kind == 2 && c->coreside) ||
                                        (side_kind == 3 && c->coreside && debug_knobs().bits_pipeline != 0));
  // a generation filling on the masked stream only takes chunks that may run there; a generation that does not report
  // through its flag cannot start to (an earlier launch decision may already have been made without it)
  // (nor the other way round: a skipped launch would drop chunks that cannot be redone)
  const bool misfit = b->kb > 0 && ((b->fill_stream != c->stream && !want_side) || (verify != b->verify));
  const bool full = b->kb > 0 && b->kb + kb > std::max(fp4_target_kb(c), kb);
  if (misfit || full) {
    if ((rc = fp4_launch(c, c->fb_active, want_side, side_kind)) != PCOA_OK) return rc;
    if (c->fb_count == 2) c->fb_active ^= 1;
    b = &c->fb[c->fb_active];
  }
  if (b->kb == 0) {  // a new generation starts in this buffer: the old one must be done and verified
    if ((rc = fp4_resolve(c, c->fb_active)) != PCOA_OK) return rc;
    b->verify = verify;
    b->fill_stream = c->stream;
    if (want_side) {
      const pcoa_ctx::Fp4Buf& o = c->fb[c->fb_active ^ 1];
      if (o.launched && hipEventQuery(o.consumed) == hipErrorNotReady) {
        b->fill_stream = c->pack_stream;
        // head start for the contraction that becomes runnable when the pre-pass queued in front of this one ends: its
        // workgroups must find the CUs empty, the pre-pass then takes the CUs that are left (fp4_setup)
        if ((rc = fork_to(c, c->pack_stream)) != PCOA_OK) return rc;
        constexpr int kHeadstartUs = 10;
        HIP_TRY(c, launch_delay_us(c->pack_stream, kHeadstartUs));
      }
      (void)hipGetLastError();
    }
  }
  if ((rc = fp4_grow(c, c->fb_active, kb, chunk_variants)) != PCOA_OK) return rc;
  if ((rc = fork_to(c, b->fill_stream)) != PCOA_OK) return rc;
  *dst = b->p + b->kb * fp4_kb_bytes(c);
  *stream = b->fill_stream;
  if (flag) *flag = fb_flag(c, c->fb_active);
  return PCOA_OK;
}

void fp4_commit(pcoa_ctx* c, int64_t kb, int64_t vars) {
  pcoa_ctx::Fp4Buf& b = c->fb[c->fb_active];
  b.kb += kb;
  b.vars += vars;
  c->gram_kind = 3;
  c->dirty = true;
  c->strip_centering_set = false;
}

// One chunk (<= pack_chunk variants) of a dense tile resident on the device: re-layout pre-pass into the
// packed operand, then (at once, or when the buffer is full / S is needed) the matrix-core contraction.
//   auto : FP4 pre-pass (it also verifies that every value is exactly 0 or 1); if a tile holds a
//          multiplicity its buffer generation is redone as int8 and contracted on the i8 MFMA instead;
//   fp4  : FP4 only, a non-binary value is an error;   i8 : int8 only (values 0..127).
// can_defer: x_chunk stays valid until the next synchronising call (a caller's device pointer); a staging tile that
// is about to be overwritten is verified at once instead.
static int packed_chunk(pcoa_ctx* c, const void* x_chunk, int is_u8, int64_t cur, int64_t ld, bool can_defer) {
  const double in_bytes = (is_u8 ? 1.0 : 4.0) * (double)cur * (double)c->n;
  int rc = PCOA_OK;
  bool fp4 = c->packed_mode != 2;
  if (fp4 && c->packed_mode == 0 && c->i8_streak > 0) {
    // the last FP4 attempt met multiplicities: do not pay for a second pre-pass on every chunk of such a cohort
    c->i8_streak -= 1;
    fp4 = false;
  }
  if (fp4) {
    const bool autom = c->packed_mode == 0;
    const int64_t kb = kb_of(c, cur);
    int8_t* dst = nullptr;
    hipStream_t ps = nullptr;
    int32_t* bflag = nullptr;
    const bool deferrable_f32 = can_defer && !is_u8 && pack_fp4_ring_ok(x_chunk, ld);
    const bool deferrable_u8 = can_defer && is_u8 && c->coreside && pack_u8_ring_ok(x_chunk, ld);
    const int side_kind = deferrable_f32 ? 1 : deferrable_u8 ? 2 : 0;
    if ((rc = fp4_reserve(c, kb, cur, side_kind, autom && can_defer, &dst, &ps, &bflag)) != PCOA_OK) return rc;
    // where the pre-pass reports a value other than 0 / 1: the generation's flag (auto, deferred), a scratch word that
    // is read back at once (auto, staging tile), or the ctx error word (FP4 forced: an error)
    int32_t* flag = c->err_flag;
    if (autom) flag = can_defer ? bflag : (c->fb_flags + 32);
    if (autom && !can_defer) HIP_TRY(c, hipMemsetAsync(flag, 0, sizeof(int32_t), ps));
    {
      ScopedTimer t(c, T_PACK, ps);
      // co-resident pipeline: the persistent ring pre-pass for every fp32 tile that qualifies -- two workgroups per CU; a
      // ring wave wants several units of 128 variants x 256 samples to stream through (>= 4 per wave, else fewer
      // workgroups; a tiny chunk takes the ordinary kernel).
      // Only BESIDE a contraction (the generation fills on the pre-pass stream): with the chip to itself the ordinary
      // kernel is as fast on big chunks and much faster on small ones (64 x 16,384-variant calls: 270 vs 194 M variants/s,
      // profiles/r03y) -- a persistent wave wants many units to stream through.
      int ring_wgs = 0;
      if (c->coreside && deferrable_f32 && ps == c->pack_stream) {
        const int64_t units = (kb / 4) * (gram_packed_npad(c->n) / 256);
        if (units >= 64) ring_wgs = (int)std::max<int64_t>(1, std::min<int64_t>(c->ring_wgs, units / 16));
      }
      // uint8 tiles: the ring form with one workgroup per CU (94 VGPRs: one wave per SIMD beside the contraction), units
      // of 128 variants x 1,024 samples
      if (c->coreside && deferrable_u8 && ps == c->pack_stream) {
        const int64_t units = (kb / 4) * ((gram_packed_npad(c->n) + 1023) / 1024);
        if (units >= 64) ring_wgs = (int)std::max<int64_t>(1, std::min<int64_t>(c->num_cu, units / 16));
      }
      hipError_t e = launch_pack_operand(c, x_chunk, is_u8, ld, cur, dst, flag, ps, kb, ring_wgs);
      if (e != hipSuccess) return hip_fail(c, e, "operand pre-pass launch");
    }
    c->pack_launches += 1;
    c->pack_bytes += in_bytes + (double)(kb * fp4_kb_bytes(c));
    if (autom && !can_defer) {
      HIP_TRY(c, hipMemcpyAsync(&c->hw->seen, flag, sizeof(int32_t), hipMemcpyDeviceToHost, ps));
      HIP_TRY(c, hipStreamSynchronize(ps));
      if (c->hw->seen) {  // a multiplicity (or garbage): this chunk takes the int8 path, which validates 0..127
        fp4 = false;  // (what was just written behind the buffered k-blocks is simply not kept)
        c->fp4_fallbacks += 1;
        c->i8_streak = 8;  // then FP4 is tried again
      }
    }
    if (fp4) {
      if (autom && can_defer) c->fb[c->fb_active].chunks.push_back(pcoa_ctx::Fp4Chunk{x_chunk, is_u8, cur, ld});
      fp4_commit(c, kb, cur);
      return PCOA_OK;
    }
  }
  return int8_chunk(c, x_chunk, is_u8, cur, ld);
}

// fp32 tile on the fp32-MFMA engine (PCOA_FLAG_GRAM_F32_MFMA): launches that keep the fp32 accumulators exact
static int gram_f32_mfma(pcoa_ctx* c, const float* x_dev, int64_t nv, int64_t ld) {
  for (int64_t done = 0; done < nv;) {
    const int64_t cur = std::min(nv - done, c->max_launch);
    int rc = fold_if_needed(c, cur);
    if (rc != PCOA_OK) return rc;
    GramLaunch g;
    g.x = x_dev + done * ld;
    g.ld = ld;
    g.nv = cur;
    g.n = c->n;
    g.s32 = c->s32;
    g.flag = c->err_flag;
    g.zeros = c->zeros;
    g.num_cu = c->num_cu;
    g.stream = c->stream;
    {
      ScopedTimer t(c, T_GRAM);
      hipError_t e = launch_gram_f32(g, nullptr);
      if (e != hipSuccess) return hip_fail(c, e, "gram kernel launch");
    }
    account_gram(c, cur);
    done += cur;
  }
  return PCOA_OK;
}

// X tile (fp32, or uint8: always a packed-operand path) already resident on the device: split into launches that keep
// fp32 / int32 exact.  fp32 tile -> packed operand (HBM-bound pre-pass); the matrix-core contraction follows at once (int8)
// or when the FP4 operand buffer is full / S is needed (packed_chunk accounts for itself)
int gram_device(pcoa_ctx* c, const void* x_dev, int is_u8, int64_t nv, int64_t ld, bool can_defer) {
  if (!is_u8 && !c->use_i8) return gram_f32_mfma(c, static_cast<const float*>(x_dev), nv, ld);
  const int64_t row_bytes = ld * (is_u8 ? 1 : 4);
  const int64_t max_cur = std::min(c->max_launch, c->pack_chunk);
  for (int64_t done = 0; done < nv;) {
    const int64_t cur = std::min(nv - done, max_cur);
    int rc = packed_chunk(c, static_cast<const char*>(x_dev) + done * row_bytes, is_u8, cur, ld, can_defer);
    if (rc != PCOA_OK) return rc;
    done += cur;
  }
  return PCOA_OK;
}

// bit-packed tile resident on the device -> FP4 operand -> FP4 contraction
// can_defer: a caller's device pointer (valid until the next synchronising call): in the co-resident pipeline its transpose
// (68 VGPRs: one wave per SIMD fits beside the contraction) runs while the previous buffer is contracted
int gram_device_bits(pcoa_ctx* c, const uint32_t* bits_dev, int64_t nv, int64_t ld_words, bool can_defer) {
  if (c->is_operator) return operator_append(c, bits_dev, nv, ld_words);   // the rows join the bit store as they are
  int64_t done = 0;
  const int64_t max_cur = std::min(c->max_launch, c->pack_chunk);
  while (done < nv) {
    const int64_t cur = std::min(nv - done, max_cur);
    const int64_t kb = kb_of(c, cur);
    int8_t* dst = nullptr;
    hipStream_t ps = nullptr;
    int rc = fp4_reserve(c, kb, cur, can_defer ? 3 : 0, false, &dst, &ps, nullptr);  // bitsets are binary by construction
    if (rc != PCOA_OK) return rc;
    {
      ScopedTimer t(c, T_PACK, ps);
      hipError_t e = launch_bits_operand(c, bits_dev + done * ld_words, ld_words, cur, dst, ps, kb);
      if (e != hipSuccess) return hip_fail(c, e, "bitset pre-pass launch");
    }
    c->pack_launches += 1;
    c->pack_bytes += 4.0 * (double)((c->n + 31) / 32) * (double)cur + (double)(kb * fp4_kb_bytes(c));
    fp4_commit(c, kb, cur);
    done += cur;
  }
  return PCOA_OK;
}

// Device-side input checks are asynchronous; they surface at the next synchronising call.
int check_device_flags(pcoa_ctx* c) {
  HIP_TRY(c, hipMemcpyAsync(&c->hw->flag, c->err_flag, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int32_t flag = c->hw->flag;
  if (flag & 1) return fail(c, PCOA_ERR_INDEX_RANGE, "a callset index outside [0, N) reached the device");
  if (flag & 8)
    return fail(c, PCOA_ERR_INVALID_ARG,
                "a genotype tile holds a value other than 0 or 1 and PCOA_FLAG_GRAM_FP4_MFMA was forced; S is "
                "invalid, call pcoa_reset; the default mode falls back to the int8 kernel by itself");
  if (flag & 16)
    return fail(c, PCOA_ERR_INVALID_ARG,
                "an accumulator of the fp32-MFMA kernel left the exact range (a sum of products reached 2^24 inside one "
                "launch, or an int32 partial passed 2^31: carrier multiplicities too large for it); S is invalid, call "
                "pcoa_reset and use the default engine (multiplicities up to 127)");
  if (flag & 4)
    return fail(c, PCOA_ERR_INVALID_ARG,
                "a genotype tile holds a value that is not an integer in [0, 127] (carrier multiplicity); S is "
                "invalid, call pcoa_reset; use PCOA_FLAG_GRAM_F32_MFMA for larger integer multiplicities");
  return PCOA_OK;
}

int finalize_impl(pcoa_ctx* c) {
  int rc0 = fp4_flush(c);  // deferred FP4 contractions land in S32 now
  if (rc0 != PCOA_OK) return rc0;
  if (c->dirty) {
    ScopedTimer t(c, T_FINALIZE);
    if (!c->is_strip) HIP_TRY(c, launch_symmetrize_i32(c->s32, c->n, c->stream));
    c->dirty = false;
  }
  return PCOA_OK;
}

}  // namespace pcoa
