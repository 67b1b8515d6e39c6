// pcoa_capi.hip -- the C ABI of include/pcoa.h on top of the HIP kernels: an engine's life (create / destroy / reset /
// reserve / set_stream / sync), error reporting, and the timings.  The rest of the ABI lives in capi_accumulate.hip,
// capi_reduce.hip, capi_compute.hip, capi_operator.hip, capi_grm.hip, capi_subset.hip, capi_pairs.hip and devmem.hip (map: pcoa_ctx.h).  There is deliberately NO CPU fallback: without a HIP
// device pcoa_create fails with PCOA_ERR_NO_DEVICE.
#include <cstdio>
#include <cstring>
#include <new>

#include "pcoa_ctx.h"

using namespace pcoa;

namespace {

thread_local std::string g_create_error;

// Test hooks (DebugKnobs): PCOA_DEBUG_MAX_LAUNCH / PCOA_DEBUG_FOLD_THRESHOLD shrink the two limits so that the
// multi-launch and int64-fold paths can be exercised with small inputs.
int64_t knob_limit(int64_t x, int64_t dflt) { return (x > 0 && x < dflt) ? x : dflt; }

}  // namespace

namespace pcoa {

int fail(pcoa_ctx* c, int code, const std::string& msg) {
  if (c) c->last_error = msg; else g_create_error = msg;
  return code;
}

int hip_fail(pcoa_ctx* c, hipError_t e, const char* what) {
  std::string m = std::string(what) + ": " + hipGetErrorString(e);
  (void)hipGetLastError();  // clear sticky launch errors
  return fail(c, e == hipErrorOutOfMemory ? PCOA_ERR_OUT_OF_MEMORY : PCOA_ERR_HIP, m);
}

hipEvent_t get_event(pcoa_ctx* c) {
  if (!c->pool.empty()) {
    hipEvent_t e = c->pool.back();
    c->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

// resolves finished (or, if wait, all) event pairs into the per-category sums
void drain_events(pcoa_ctx* c, bool wait) {
  if (wait) {
    (void)hipStreamSynchronize(c->stream);
    if (c->pack_stream) (void)hipStreamSynchronize(c->pack_stream);
    if (c->gram_stream) (void)hipStreamSynchronize(c->gram_stream);
  }
  size_t keep = 0;
  for (size_t i = 0; i < c->pending.size(); ++i) {
    EventPair& p = c->pending[i];
    float ms = 0.f;
    hipError_t e = hipEventElapsedTime(&ms, p.a, p.b);
    if (e == hipSuccess) {
      c->tsec[p.cat] += (double)ms * 1e-3;
      c->pool.push_back(p.a);
      c->pool.push_back(p.b);
    } else if (!wait && e == hipErrorNotReady) {
      c->pending[keep++] = p;
    } else {
      (void)hipGetLastError();
      c->pool.push_back(p.a);
      c->pool.push_back(p.b);
    }
  }
  c->pending.resize(keep);
}

}  // namespace pcoa

// ================================================================================================
// zero_s = false (pcoa_create_subset): S is allocated but not zeroed -- the caller overwrites every entry before anything reads it
static int create_impl(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags, int32_t col0, int32_t cols,
                       bool op = false, bool zero_s = true, bool grm = false, bool grm_study = false) {
  if (!out) return fail(nullptr, PCOA_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  if (n_samples <= 0) return fail(nullptr, PCOA_ERR_INVALID_ARG, "n_samples must be positive");
  if (grm && !grm_study && n_samples < 32)
    return fail(nullptr, PCOA_ERR_INVALID_ARG, "a GRM ctx needs n_samples >= 32: its computePca is the Lanczos iteration, which "
                                               "starts at 32 samples, and there is no matrix for the dense solver below that");
  if (op && n_samples >= 32 && (flags & PCOA_FLAG_EIG_HOUSEHOLDER))
    return fail(nullptr, PCOA_ERR_INVALID_ARG, "an operator ctx has no N x N matrix for the dense Householder solver "
                                               "(PCOA_FLAG_EIG_HOUSEHOLDER); its computePca is the Lanczos iteration");
  if (op && (flags & (PCOA_FLAG_GRAM_F32_MFMA | PCOA_FLAG_GRAM_I8_MFMA | PCOA_FLAG_GRAM_FP4_MFMA | PCOA_FLAG_OPERAND_FP4)))
    return fail(nullptr, PCOA_ERR_INVALID_ARG, "an operator ctx runs no Gram kernel: the PCOA_FLAG_GRAM_* / PCOA_FLAG_OPERAND_FP4 flags do not apply");
  const bool strip = cols >= 0;
  if (strip && (col0 < 0 || cols <= 0 || (int64_t)col0 + cols > n_samples))
    return fail(nullptr, PCOA_ERR_INVALID_ARG, "strip [col0, col0 + cols) must lie inside [0, n_samples) and be non-empty");
  if (strip && (flags & PCOA_FLAG_GRAM_F32_MFMA))
    return fail(nullptr, PCOA_ERR_INVALID_ARG, "a strip owner needs a packed-operand engine (not PCOA_FLAG_GRAM_F32_MFMA)");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(nullptr, PCOA_ERR_NO_DEVICE,
                "no HIP device visible: this engine has no CPU fallback (hipGetDeviceCount failed or returned 0)");
  }
  if (device_ordinal < 0 || device_ordinal >= ndev)
    return fail(nullptr, PCOA_ERR_NO_DEVICE, "device ordinal out of range");
  pcoa_ctx* c = new (std::nothrow) pcoa_ctx();
  if (!c) return fail(nullptr, PCOA_ERR_OUT_OF_MEMORY, "host allocation failed");
  c->n = n_samples;
  c->is_strip = strip;
  c->is_operator = op;
  c->is_grm = grm;
  c->is_grm_study = grm_study;
  c->s_cols = strip ? cols : n_samples;
  c->strip_col0 = strip ? col0 : 0;
  c->device = device_ordinal;
  c->flags = flags;
  c->use_i8 = !(flags & PCOA_FLAG_GRAM_F32_MFMA);
  c->packed_mode = (flags & PCOA_FLAG_GRAM_I8_MFMA) ? 2 : (flags & PCOA_FLAG_GRAM_FP4_MFMA) ? 3 : 0;
  c->op_fmt = (flags & PCOA_FLAG_OPERAND_FP4) ? 1 : 2;
  const DebugKnobs& knobs = debug_knobs();
  if (knobs.gram_kernel == 1) c->use_i8 = false;
  if (knobs.gram_kernel == 2) { c->use_i8 = true; c->packed_mode = 2; }
  if (knobs.gram_kernel == 3) { c->use_i8 = true; c->packed_mode = 3; }
  if (knobs.gram_kernel == 0) { c->use_i8 = true; c->packed_mode = 0; }
  c->gram_kind = c->use_i8 ? (c->packed_mode == 2 ? 2 : 3) : 1;
  if (op) {   // no Gram kernel of any kind; the bitset boundaries only ask for "not the fp32 engine"
    c->use_i8 = true;
    c->packed_mode = 3;
    c->gram_kind = 0;
    // rows per segment: ~256 MiB, whole ranges of the second pass where a segment holds several
    const int64_t row_bytes = store_pitch_words(c) * 4;
    const int64_t align = grm ? kGrmSegmentAlign : kOperatorSegmentAlign, knob = grm ? knobs.grm_segment_rows : knobs.operator_segment_rows;
    int64_t rows = std::max<int64_t>(1, ((int64_t)256 << 20) / row_bytes);
    if (rows >= align) rows -= rows % align;
    if (knob > 0) rows = std::min<int64_t>(knob, (int64_t)1 << 24);
    c->op_seg_rows = rows;
  }
  {
    // keep the int8 workspace at or below ~4 GiB whatever N is (one byte per genotype, Npad columns)
    const int64_t by_mem = (((int64_t)4 << 30) / gram_packed_npad(n_samples)) / 1536 * 1536;
    c->pack_chunk = std::max<int64_t>(1536, std::min<int64_t>(c->pack_chunk, by_mem));
  }
  if (knobs.pack_chunk > 0 && knobs.pack_chunk <= ((int64_t)1 << 24)) c->pack_chunk = knobs.pack_chunk;
  c->max_launch = knob_limit(knobs.max_launch, kMaxLaunchVariants);
  c->fold_threshold = knob_limit(knobs.fold_threshold, kFoldThreshold);
  auto bail = [&](hipError_t err, const char* what) {
    int rc = hip_fail(c, err, what);
    g_create_error = c->last_error;
    pcoa_destroy(c);
    return rc;
  };
  if ((e = hipSetDevice(device_ordinal)) != hipSuccess) return bail(e, "hipSetDevice");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device_ordinal)) != hipSuccess) return bail(e, "hipGetDeviceProperties");
  c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  std::snprintf(c->dev_name, sizeof(c->dev_name), "%s (%s)", prop.name, prop.gcnArchName);
  if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess)
    return bail(e, "hipStreamCreate");
  c->stream = c->own_stream;
  if (strip && !c->use_i8) {
    pcoa_destroy(c);
    return fail(nullptr, PCOA_ERR_INVALID_ARG, "a strip owner needs a packed-operand engine (PCOA_GRAM_KERNEL=f32 is set)");
  }
  const size_t nn = s_count(c);
  if (!op) {
    if ((e = dev_alloc((void**)&c->s32, sizeof(int32_t) * nn, c->device)) != hipSuccess) return bail(e, "allocation of S");
    if (zero_s && (e = hipMemsetAsync(c->s32, 0, sizeof(int32_t) * nn, c->stream)) != hipSuccess) return bail(e, "memset(S)");
  }
  if ((e = dev_alloc((void**)&c->zeros, 4096, c->device)) != hipSuccess) return bail(e, "allocation of the zero page");
  if ((e = hipMemsetAsync(c->zeros, 0, 4096, c->stream)) != hipSuccess) return bail(e, "memset(zeros)");
  if ((e = dev_alloc((void**)&c->err_flag, 16, c->device)) != hipSuccess) return bail(e, "allocation of the flag words");
  if ((e = hipMemsetAsync(c->err_flag, 0, 16, c->stream)) != hipSuccess) return bail(e, "memset(flag)");
  if ((e = hipHostMalloc((void**)&c->hw, sizeof(pcoa_ctx::HostWords), hipHostMallocDefault)) != hipSuccess)
    return bail(e, "hipHostMalloc(landing words)");
  std::memset(c->hw, 0, sizeof(pcoa_ctx::HostWords));
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
  *out = c;
  return PCOA_OK;
}

namespace pcoa {
// pcoa_create's path with S left as allocated: pcoa_create_subset's gather writes every entry (capi_subset.hip)
int create_full_engine_unfilled(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags) {
  return create_impl(out, n_samples, device_ordinal, flags, 0, -1, false, false);
}
// pcoa_create_grm (capi_grm.hip): an operator ctx whose store holds 2-bit genotype rows
int create_grm_engine(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags) {
  return create_impl(out, n_samples, device_ordinal, flags, 0, -1, true, true, true);
}
// pcoa_create_grm_study (capi_grm_project.hip): the same store for study samples; it runs no eigensolver, so any n_samples >= 1
int create_grm_study_engine(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags) {
  return create_impl(out, n_samples, device_ordinal, flags, 0, -1, true, true, true, true);
}
}  // namespace pcoa

extern "C" {

const char* pcoa_version(void) { return "pcoa_hip 0.11 (gfx950)"; }

int pcoa_create(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags) {
  return create_impl(out, n_samples, device_ordinal, flags, 0, -1);
}

int pcoa_create_strip(pcoa_ctx** out, int32_t n_samples, int32_t col0, int32_t cols, int32_t device_ordinal,
                      uint32_t flags) {
  if (cols < 0) return fail(nullptr, PCOA_ERR_INVALID_ARG, "cols must be positive");
  return create_impl(out, n_samples, device_ordinal, flags, col0, cols);
}

int pcoa_create_operator(pcoa_ctx** out, int32_t n_samples, int32_t device_ordinal, uint32_t flags) {
  return create_impl(out, n_samples, device_ordinal, flags, 0, -1, true);
}

void pcoa_destroy(pcoa_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->pack_stream) (void)hipStreamSynchronize(c->pack_stream);
  if (c->gram_stream) (void)hipStreamSynchronize(c->gram_stream);
  if (c->csr_stream) (void)hipStreamSynchronize(c->csr_stream);   // queued copies of carrier lists / .bed rows
  for (auto& p : c->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  for (auto& ev : c->pool) (void)hipEventDestroy(ev);
  for (auto& b : c->fb) {
    if (b.packed) (void)hipEventDestroy(b.packed);
    if (b.consumed) (void)hipEventDestroy(b.consumed);
    if (b.p) dev_free(b.p);
  }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  for (StagingRing* r : {&c->cs, &c->bs, &c->ts}) staging_destroy(*r);
  if (c->csr_stream) (void)hipStreamDestroy(c->csr_stream);
  if (c->csr_flag) dev_free(c->csr_flag);
  if (c->csr_flag_host) (void)hipHostFree(c->csr_flag_host);
  if (c->fb_flags_host) (void)hipHostFree(c->fb_flags_host);
  if (c->hw) (void)hipHostFree(c->hw);
  if (c->ws.host_rec) (void)hipHostFree(c->ws.host_rec);
  void* bufs[] = {c->s32, c->s64, c->s64_spare, c->narrow_flag, c->zeros, c->err_flag, c->tile, c->csr_idx, c->csr_offs, c->thr_dev,
                  c->sample_pop, c->measure_diag, c->measure_q, c->xfer, c->coll, c->fb_flags, c->strip_ws, c->strip_means, c->proj_ws, c->pack_buf, c->lanczos_ws, c->sym_part, c->ws.a, c->ws.d, c->ws.e, c->ws.tau, c->ws.q, c->ws.w, c->ws.lam,
                  c->ws.z, c->ws.wy, c->ws.scratch, c->ws.iscratch, c->row_sums, c->colmean, c->stats, c->nz,
                  c->out_dev};
  for (void* b : bufs)
    if (b) dev_free(b);
  operator_destroy(c);
  grm_destroy(c);
  loadings_destroy(c);
  ld_destroy(c);
  complete_destroy(c);
  king_destroy(c);
  if (c->pack_stream) (void)hipStreamDestroy(c->pack_stream);
  if (c->gram_stream) (void)hipStreamDestroy(c->gram_stream);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

const char* pcoa_last_error(const pcoa_ctx* c) { return c ? c->last_error.c_str() : g_create_error.c_str(); }

int pcoa_n_samples(const pcoa_ctx* c) { return c ? c->n : PCOA_ERR_INVALID_ARG; }

int pcoa_set_stream(pcoa_ctx* c, void* hip_stream) {
  CHECK_CTX(c);
  int rc = fp4_flush(c);  // nothing of the old stream's generation survives the switch half-filled
  if (rc != PCOA_OK) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  drain_events(c, true);
  c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
  return PCOA_OK;
}

int pcoa_sync(pcoa_ctx* c) {
  CHECK_CTX(c);
  int rc = fp4_sync_point(c);
  if (rc != PCOA_OK) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

int pcoa_reserve(pcoa_ctx* c, int64_t variants_per_call, int32_t num_pc) {
  CHECK_CTX(c);
  if (variants_per_call < 0 || num_pc < 0 || num_pc > c->n)
    return fail(c, PCOA_ERR_INVALID_ARG, "reserve: variants_per_call < 0 or num_pc outside [0, n]");
  if (c->is_operator) return operator_reserve(c, num_pc);
  int rc = PCOA_OK;
  if (variants_per_call > 0 && c->use_i8 && c->packed_mode != 2) {
    // the operand buffer(s) of the binary-tile path, at the size fp4_grow would reach after the first large call
    if ((rc = fp4_setup(c)) != PCOA_OK) return rc;
    const int64_t chunk = std::min(std::min(variants_per_call, c->max_launch), c->pack_chunk);
    for (int bi = 0; bi < c->fb_count; ++bi) {
      pcoa_ctx::Fp4Buf& b = c->fb[bi];
      if (b.kb > 0 || b.launched) continue;  // in use: it grows by itself
      const int64_t kb = kb_of(c, chunk);
      if (b.cap_kb >= std::max(kb, chunk >= ((int64_t)1 << 18) ? fp4_target_kb(c) : kb)) continue;
      if ((rc = fp4_grow(c, bi, kb, chunk)) != PCOA_OK) return rc;
    }
  }
  if (num_pc > 0 && !c->is_strip) {
    if ((rc = ensure_workspace(c, num_pc)) != PCOA_OK) return rc;
    if (c->n >= 32 && !(c->flags & PCOA_FLAG_EIG_HOUSEHOLDER)) {
      const int32_t mmax = std::min<int32_t>(c->n, 512);
      if ((rc = ensure(c, &c->lanczos_ws, &c->lanczos_cap, (int64_t)lanczos_workspace_doubles(c->n, num_pc, mmax))) != PCOA_OK)
        return rc;
    } else if ((rc = ensure_b(c)) != PCOA_OK) {
      return rc;
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

int pcoa_reset(pcoa_ctx* c) {
  CHECK_CTX(c);
  int rc = fp4_discard(c);  // buffered or in-flight operands belong to the old S
  if (rc != PCOA_OK) return rc;
  ld_drop_tail(c);   // an LD pruner starts a new window with the new S
  if (c->is_operator) return operator_reset(c);
  const size_t nn = s_count(c);
  HIP_TRY(c, hipMemsetAsync(c->s32, 0, sizeof(int32_t) * nn, c->stream));
  if (c->s64) {
    // S = 0 needs no int64 part (as the non-roots of pcoa_gram_reduce_peers(root_only)): kept zeroed it would stay "live" for
    // the rest of the ctx's life, however small the S fed next -- the int64 kernels, the int64 branch of every reduction, and
    // a companion refused at every centring.  The folds that wrote it are on this stream; the spare's contents are undefined.
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    retire_s64(c);
  }
  HIP_TRY(c, hipMemsetAsync(c->err_flag, 0, 16, c->stream));
  c->variants_in_s32 = 0;
  c->dirty = false;
  c->strip_centering_set = false;  // S changes: the row means of an earlier computePca no longer belong to it
  return PCOA_OK;
}

// The struct grows at its end from release to release; the caller says how many bytes ITS pcoa_timings has (a
// shim built against an older header must not have its stack overwritten by a newer library).
int pcoa_get_timings_sized(pcoa_ctx* c, pcoa_timings* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(double)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  pcoa_timings full;
  pcoa_timings* out = &full;
  std::memset(out, 0, sizeof(*out));
  out->gram_kernel_seconds = c->tsec[T_GRAM];
  out->gram_kernel_launches = c->gram_launches;
  out->gram_variants = c->gram_variants;
  out->gram_flops = c->gram_flops;
  out->gram_bytes = c->gram_bytes;
  out->densify_seconds = c->tsec[T_DENSIFY];
  out->synth_seconds = c->tsec[T_SYNTH];
  out->finalize_seconds = c->tsec[T_FINALIZE];
  out->center_seconds = c->tsec[T_CENTER];
  out->tridiag_seconds = c->tsec[T_TRIDIAG];
  out->eig_seconds = c->tsec[T_EIG];
  out->backtransform_seconds = c->tsec[T_BACK];
  out->compute_total_seconds = c->compute_total;
  out->gram_kernel_kind = c->gram_kind;
  out->lanczos_seconds = c->tsec[T_LANCZOS];
  out->eig_method = c->eig_method;
  out->lanczos_steps = c->lanczos_steps;
  out->fp4_fallbacks = c->fp4_fallbacks;
  out->lockstep_launches = c->lockstep_launches;
  out->pipeline_launches = c->pipeline_launches;
  out->evensplit_launches = c->evensplit_launches;
  out->operand_bits = !c->use_i8 ? 32 : c->gram_kind == 2 ? 8 : c->op_fmt == 2 ? 1 : 4;
  {
    const int ls = c->pipe_ok ? gram_lockstep_splitk(c->n, c->pipe_gram_cus) : 0;
    int wgs = ls > 0 ? gram_lockstep_workgroups(c->n, ls) : 0;   // one workgroup per CU
    if (c->pipe_ok && c->op_fmt == 2 && !(c->coreside && c->coreside_mode == 2)) wgs = c->pipe_gram_cus;  // even split: exactly that many workgroups
    // co-resident form: the ring pre-pass has waves on EVERY CU, the contraction's workgroups share theirs with it
    out->pipeline_pre_pass_cus = c->pipe_ok ? (c->coreside ? c->num_cu : c->num_cu - wgs) : 0;
    out->pipeline_contraction_cus = wgs;
  }
  out->pack_seconds = c->tsec[T_PACK];
  out->pack_launches = c->pack_launches;
  out->pack_bytes = c->pack_bytes;
  out->csr_stage_seconds = c->csr_stage_s;
  out->csr_wait_seconds = c->csr_wait_s;
  out->csr_fast_chunks = c->csr_fast_chunks;
  out->csr_redo_chunks = c->csr_redo_chunks;
  out->allreduce_seconds = c->tsec[T_ALLREDUCE];
  out->allreduce_calls = c->allreduce_calls;
  out->comm_ranks = c->comm_ranks;
  out->allreduce_int32 = c->allreduce_int32;
  out->matvec_form = c->matvec_form;
  out->gram_i64_live = c->s64 ? 1 : 0;
  out->reduce_int32_calls = c->reduce_i32_calls;
  out->narrowed_to_int32 = c->narrowed;
  out->lanczos_block_steps = c->lanczos_block_steps;
  out->eig_dense_form = c->eig_dense_form;
  out->operator_products = c->op_products;
  out->operator_matvec_seconds = c->tsec[T_OPERATOR];
  out->operator_store_bytes = operator_store_bytes(c);
  out->subset_seconds = c->tsec[T_SUBSET];
  out->subset_bytes = c->subset_bytes;
  std::memcpy(out_user, out, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

int pcoa_get_reduce_peers_stats(pcoa_ctx* c, pcoa_reduce_peers_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(int64_t)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  pcoa_reduce_peers_stats full;
  std::memset(&full, 0, sizeof(full));
  full.reduce_peers_calls = c->reduce_peers_calls;
  full.reduce_peers_seconds = c->tsec[T_REDUCE_PEERS];
  full.reduce_peers_bytes_in = c->reduce_peers_bytes_in;
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

static_assert(offsetof(pcoa_timings, csr_stage_seconds) == PCOA_TIMINGS_R03_BYTES, "the r03 prefix of pcoa_timings is frozen");
// the r03 layout (ends behind evensplit_launches), whatever the struct has grown to since
int pcoa_get_timings(pcoa_ctx* c, pcoa_timings* out) { return pcoa_get_timings_sized(c, out, PCOA_TIMINGS_R03_BYTES); }

int pcoa_reset_timings(pcoa_ctx* c) {
  CHECK_CTX(c);
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  for (double& t : c->tsec) t = 0;
  c->csr_stage_s = c->csr_wait_s = 0;
  c->csr_fast_chunks = c->csr_redo_chunks = 0;
  c->allreduce_calls = 0;
  c->reduce_i32_calls = c->narrowed = 0;
  c->gram_launches = 0;
  c->gram_variants = 0;
  c->gram_flops = c->gram_bytes = 0;
  c->compute_total = 0;
  c->pack_launches = 0;
  c->pack_bytes = 0;
  c->lockstep_launches = 0;
  c->pipeline_launches = 0;
  c->evensplit_launches = 0;
  c->op_products = 0;
  c->subset_bytes = 0;
  c->pairs_bytes = c->pairs_calls = 0;
  c->king_bytes = c->king_calls = 0;
  c->grm_block_calls = 0;
  c->grm_block_flops = 0;
  c->grm_pairs_calls = c->grm_pairs_bands = c->grm_pairs_bytes = 0;
  c->grm_pairs_flops = 0;
  c->grm_king_calls = c->grm_king_block_calls = c->grm_king_bands = c->grm_king_bytes = 0;
  c->grm_king_macs = 0;
  c->grm_pcr_fits = c->grm_pcr_block_calls = c->grm_pcr_pairs_calls = c->grm_pcr_bands = c->grm_pcr_bytes = 0;
  c->grm_pcr_flops = 0;
  c->grm_subset_calls = c->grm_subset_bytes = 0;
  c->grm_hwe_calls = c->grm_sample_counts_calls = 0;
  c->grm_lsq_calls = c->grm_lsq_pair_vectors = c->grm_lsq_undetermined = 0;
  c->ld_variants = c->ld_bytes = 0;
  c->ldp_seen = c->ldp_kept = c->ldp_mono = c->ldp_pairs = 0;
  c->reduce_peers_calls = c->reduce_peers_bytes_in = 0;
  return PCOA_OK;
}

int pcoa_device_info(pcoa_ctx* c, char* name_out, int32_t name_cap, int32_t* cu_count_out) {
  CHECK_CTX(c);
  if (name_out && name_cap > 0) {
    std::strncpy(name_out, c->dev_name, (size_t)name_cap - 1);
    name_out[name_cap - 1] = 0;
  }
  if (cu_count_out) *cu_count_out = c->num_cu;
  return PCOA_OK;
}

}  // extern "C"
