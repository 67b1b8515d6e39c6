// capi_accumulate.hip -- the input boundaries of the C ABI: dense fp32 / uint8 tiles, bitsets, PLINK .bed rows, carrier
// lists, the synthetic model.  Device inputs go straight to operand.hip; host inputs are staged, the asynchronous ones
// through a ring of two staging slots (StagingRing, pcoa_ctx.h): host bitsets and .bed rows by the row feed (row_feed.h).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <thread>

#include "pcoa_ctx.h"
#include "row_feed.h"

using namespace pcoa;

namespace pcoa {

// Rows of the fp32 staging tile: 256 MiB for ordinary N; for very wide matrices at least ~16k variants per
// contraction launch (every launch pays one int32-atomic epilogue per output tile), capped at 8 GiB.
static int64_t staging_rows(int64_t n_variants, int64_t ld4) {
  int64_t rows = ((int64_t)64 << 20) / ld4;
  const int64_t want = 16384, cap = ((int64_t)2 << 30) / ld4;
  if (rows < want) rows = std::min(want, cap);
  return std::max<int64_t>(1, std::min(n_variants, rows));
}

// an operator ctx (pcoa_create_operator) stores carrier bitsets: every other boundary names the two that feed it
static int not_a_bitset_boundary(pcoa_ctx* c, const char* call, const char* why = "") {
  return fail(c, PCOA_ERR_STATE, std::string(call) + ": an operator ctx (pcoa_create_operator) stores carrier BITSETS: feed it "
                                 "through pcoa_accumulate_bits or pcoa_accumulate_plink_bed" + why);
}

// a GRM ctx (pcoa_create_grm) stores 2-bit genotypes: carriers alone do not say whether a call is missing or homozygous
static int not_the_bed_boundary(pcoa_ctx* c, const char* call) {
  return fail(c, PCOA_ERR_STATE, std::string(call) + ": a GRM ctx (pcoa_create_grm) stores 2-bit GENOTYPES (dosage and missing "
                                 "calls): feed it through pcoa_accumulate_plink_bed, the .bed boundary, only");
}

// sample -> population map on the device; uploaded again only when the offsets differ from the last call's
static int upload_sample_pop(pcoa_ctx* c, const pcoa_synth_params* p) {
  if (!p || !p->pop_offsets || !p->thresholds || p->n_pops <= 0)
    return fail(c, PCOA_ERR_INVALID_ARG, "synthetic params: null pointer or n_pops <= 0");
  if (p->pop_offsets[0] != 0 || p->pop_offsets[p->n_pops] != c->n)
    return fail(c, PCOA_ERR_INVALID_ARG, "synthetic params: pop_offsets must run from 0 to n_samples");
  for (int32_t q = 0; q < p->n_pops; ++q)
    if (p->pop_offsets[q + 1] < p->pop_offsets[q])
      return fail(c, PCOA_ERR_INVALID_ARG, "synthetic params: pop_offsets not monotone");
  if (c->sample_pop && c->pop_offsets_dev.size() == (size_t)p->n_pops + 1 &&
      std::equal(c->pop_offsets_dev.begin(), c->pop_offsets_dev.end(), p->pop_offsets))
    return PCOA_OK;
  std::vector<int32_t> pop((size_t)c->n);
  for (int32_t q = 0; q < p->n_pops; ++q)
    for (int32_t i = p->pop_offsets[q]; i < p->pop_offsets[q + 1]; ++i) pop[(size_t)i] = q;
  // kernels of earlier calls may still read the old map
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (auto& b : c->fb)
    if (b.fill_stream && b.fill_stream != c->stream) HIP_TRY(c, hipStreamSynchronize(b.fill_stream));
  if (!c->sample_pop) HIP_TRY(c, dev_alloc((void**)&c->sample_pop, sizeof(int32_t) * (size_t)c->n, c->device));
  HIP_TRY(c, hipMemcpyAsync(c->sample_pop, pop.data(), sizeof(int32_t) * (size_t)c->n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // `pop` dies here
  c->pop_offsets_dev.assign(p->pop_offsets, p->pop_offsets + p->n_pops + 1);
  return PCOA_OK;
}

static int upload_synth(pcoa_ctx* c, const pcoa_synth_params* p, int64_t nv) {
  int rc = upload_sample_pop(c, p);
  if (rc != PCOA_OK) return rc;
  rc = ensure(c, &c->thr_dev, &c->thr_cap, nv * p->n_pops);
  if (rc != PCOA_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->thr_dev, p->thresholds, sizeof(uint32_t) * (size_t)(nv * p->n_pops),
                            hipMemcpyHostToDevice, c->stream));
  return PCOA_OK;
}

// pcoa_accumulate_synthetic on the k-bits operand (r06): the genotypes are generated straight into the operand buffer
// (synth_kbits_kernel) -- no fp32 staging tile (6.5 GB at N = 100,000), no pre-pass, and no host synchronisation per chunk:
// the r05 path verified every staging tile like a caller's (a read-back per 16,384 variants) although the generator can
// only produce 0 / 1.  The thresholds travel on the copy stream into one of two slots; the call returns when they have been
// copied (host inputs are consumed when an accumulate call returns), everything else is queued.
static int synth_bits(pcoa_ctx* c, const pcoa_synth_params* p, int64_t first_variant, int64_t nv) {
  int rc = upload_sample_pop(c, p);
  if (rc != PCOA_OK) return rc;
  if ((rc = fp4_setup(c)) != PCOA_OK) return rc;
  const int64_t need = nv * p->n_pops;
  StagingRing::Slot* slp = nullptr;   // (its last readers: the kernels of the call before last)
  if ((rc = staging_acquire(c, c->ts, sizeof(uint32_t) * (size_t)need, sizeof(uint32_t) * (size_t)std::max<int64_t>(need, 1 << 16),
                            &slp)) != PCOA_OK)
    return rc;
  StagingRing::Slot& sl = *slp;
  const uint32_t* thr = static_cast<const uint32_t*>(sl.dev[0]);
  HIP_TRY(c, hipMemcpyAsync(sl.dev[0], p->thresholds, sizeof(uint32_t) * (size_t)need, hipMemcpyHostToDevice, c->csr_stream));
  if ((rc = staging_copied(c, sl)) != PCOA_OK) return rc;
  const int npad = (int)gram_packed_npad(c->n);
  int64_t done = 0;
  hipStream_t last_stream = c->stream;
  while (done < nv) {
    // fill the active operand buffer to exactly its target: a chunk never makes fp4_reserve launch a part-filled buffer
    const pcoa_ctx::Fp4Buf& b = c->fb[c->fb_active];
    const int64_t target = fp4_target_kb(c);
    const int64_t room_kb = (b.kb > 0 && b.kb < target) ? target - b.kb : target;
    const int64_t cur = std::min(std::min(nv - done, room_kb * 32), (int64_t)1 << 20);
    const int64_t kb = kb_of(c, cur);
    int8_t* dst = nullptr;
    hipStream_t ps = nullptr;
    if ((rc = fp4_reserve(c, kb, cur, 0, false, &dst, &ps, nullptr)) != PCOA_OK) return rc;
    HIP_TRY(c, hipStreamWaitEvent(ps, sl.copied, 0));
    {
      ScopedTimer t(c, T_SYNTH, ps);
      HIP_TRY(c, launch_synth_kbits(p->seed, thr + done * p->n_pops, c->sample_pop, p->n_pops, first_variant + done, cur, c->n,
                                    npad, dst, kb / 4, ps));
    }
    fp4_commit(c, kb, cur);
    last_stream = ps;
    done += cur;
  }
  if ((rc = staging_released(c, sl, last_stream)) != PCOA_OK) return rc;
  HIP_TRY(c, hipEventSynchronize(sl.copied));   // the caller's thresholds have been read
  return PCOA_OK;
}

// Host tile of T = float / uint8_t: staged through the (byte-addressed) tile buffer on the ctx stream, rows packed at
// ld4 = round_up(n, 4), in chunks of at most ~256 MiB
template <typename T>
static int dense_host(pcoa_ctx* c, const T* x, int64_t n_variants, int64_t ld) {
  constexpr int is_u8 = sizeof(T) == 1;
  const int64_t ld4 = round_up(c->n, 4);
  const int64_t rows_cap = is_u8 ? std::max<int64_t>(1, std::min<int64_t>(n_variants, ((int64_t)256 << 20) / ld4))
                                 : staging_rows(n_variants, ld4);
  int rc = ensure(c, &c->tile, &c->tile_elems, (rows_cap * ld4 * (int64_t)sizeof(T) + 3) / 4);
  if (rc != PCOA_OK) return rc;
  T* stage = reinterpret_cast<T*>(c->tile);
  for (int64_t v0 = 0; v0 < n_variants; v0 += rows_cap) {
    const int64_t rows = std::min(rows_cap, n_variants - v0);
    if (ld4 != c->n) HIP_TRY(c, hipMemsetAsync(stage, 0, sizeof(T) * (size_t)(rows * ld4), c->stream));
    HIP_TRY(c, hipMemcpy2DAsync(stage, sizeof(T) * (size_t)ld4, x + v0 * ld, sizeof(T) * (size_t)ld, sizeof(T) * (size_t)c->n,
                                (size_t)rows, hipMemcpyHostToDevice, c->stream));
    rc = gram_device(c, stage, is_u8, rows, ld4, false);
    if (rc != PCOA_OK) return rc;
  }
  // the caller may free/overwrite x after we return: pageable copies have been staged, but keep it simple
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

// The r01-r03 form of the carrier-list boundary: one host pass over every entry (range check, repeats and their largest
// multiplicity), then chunk by chunk onto whichever engine the ctx runs.  Since r04 it serves what calls_fast cannot: ctxs
// on the fp32 / int8-only engines, and the chunks in which the device met a repeated callset (rare: nothing a VCF yields).
static int calls_legacy(pcoa_ctx* c, const int32_t* sample_idx, const int64_t* row_offsets, int64_t n_variants) {
  if (n_variants < 0 || !row_offsets) return fail(c, PCOA_ERR_INVALID_ARG, "row_offsets is NULL or n_variants < 0");
  if (n_variants == 0) return PCOA_OK;
  const int64_t nnz_total = row_offsets[n_variants] - row_offsets[0];
  if (nnz_total < 0 || (nnz_total > 0 && !sample_idx))
    return fail(c, PCOA_ERR_INVALID_ARG, "sample_idx is NULL or row_offsets decreasing");
  // validate before touching S: the reference throws on an unknown callset (VariantsPca.scala:59)
  for (int64_t v = 0; v < n_variants; ++v)
    if (row_offsets[v + 1] < row_offsets[v]) return fail(c, PCOA_ERR_INVALID_ARG, "row_offsets not monotone");
  // One pass over the entries: range check, and -- for the packed engines -- whether any carrier list repeats a
  // callset (last[s] remembers the last row that named s).  The reference's double loop counts a repeat with
  // multiplicity (VariantsPca.scala:187), which only the int8 / fp32 kernels can express; lists that are SETS go to the
  // FP4 operand.
  bool any_repeat = false;
  int32_t mult_max = 1;  // largest multiplicity of a callset inside one carrier list
  {
    const bool want_repeats = c->use_i8;
    std::vector<int64_t> last(want_repeats ? (size_t)c->n : 0, (int64_t)-1);
    std::vector<int32_t> cnt(want_repeats ? (size_t)c->n : 0, 0);
    for (int64_t v = 0; v < n_variants; ++v) {
      for (int64_t p = row_offsets[v]; p < row_offsets[v + 1]; ++p) {
        const int32_t s = sample_idx[p];
        if (s < 0 || s >= c->n) {
          char buf[160];
          std::snprintf(buf, sizeof(buf), "callset index %d out of range [0, %d) at entry %lld", s, c->n, (long long)p);
          return fail(c, PCOA_ERR_INDEX_RANGE, buf);
        }
        if (want_repeats) {
          if (last[(size_t)s] == v) {
            any_repeat = true;
            mult_max = std::max(mult_max, ++cnt[(size_t)s]);
          } else {
            last[(size_t)s] = v;
            cnt[(size_t)s] = 1;
          }
        }
      }
    }
    if (any_repeat && c->packed_mode == 3)
      return fail(c, PCOA_ERR_INVALID_ARG,
                  "a carrier list repeats a callset (multiplicity > 1) and PCOA_FLAG_GRAM_FP4_MFMA was forced");
  }
  const bool csr_fp4 = c->use_i8 && c->packed_mode != 2 && !any_repeat;
  const int64_t ld4 = round_up(c->n, 4);
  // one variant adds at most mult_max^2 to an entry of S: int32 launches stay below 2^30 / weight variants
  const int64_t weight = (int64_t)mult_max * mult_max;
  int64_t rows_cap = staging_rows(n_variants, ld4);
  if (c->use_i8 && !csr_fp4) rows_cap = std::max<int64_t>(1, std::min(rows_cap, ((int64_t)1 << 30) / weight));
  int rc = PCOA_OK;
  if (!c->use_i8) {
    rc = ensure(c, &c->tile, &c->tile_elems, rows_cap * ld4);
    if (rc != PCOA_OK) return rc;
  }
  rc = ensure(c, &c->csr_offs, &c->csr_offs_cap, rows_cap + 1);
  if (rc != PCOA_OK) return rc;
  for (int64_t v0 = 0; v0 < n_variants; v0 += rows_cap) {
    const int64_t rows = std::min(rows_cap, n_variants - v0);
    const int64_t b = row_offsets[v0], e = row_offsets[v0 + rows];
    const int64_t nnz = e - b;
    if (nnz == 0) continue;  // only empty rows: they add nothing (filtered at VariantsPca.scala:166)
    rc = ensure(c, &c->csr_idx, &c->csr_idx_cap, nnz);
    if (rc != PCOA_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->csr_idx, sample_idx + b, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice,
                              c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->csr_offs, row_offsets + v0, sizeof(int64_t) * (size_t)(rows + 1),
                              hipMemcpyHostToDevice, c->stream));
    if (csr_fp4) {
      // carrier SETS -> FP4 operand, appended to the operand buffer; the contraction is deferred (fp4_flush)
      const int64_t kb = kb_of(c, rows);
      int8_t* dst = nullptr;
      hipStream_t ps = nullptr;
      if ((rc = fp4_reserve(c, kb, rows, false, false, &dst, &ps, nullptr)) != PCOA_OK) return rc;
      {
        ScopedTimer t(c, T_DENSIFY, ps);
        HIP_TRY(c, launch_csr_operand(c, c->csr_idx, c->csr_offs, rows, b, dst, ps, kb));
      }
      fp4_commit(c, kb, rows);
      continue;
    }
    if (c->use_i8) {
      // carriers -> k-blocked int8 operand directly (no fp32 tile, no pre-pass), then the i8 contraction
      rc = fold_if_needed(c, rows * weight);
      if (rc != PCOA_OK) return rc;
      rc = ensure(c, &c->pack_buf, &c->pack_cap, (int64_t)gram_packed_workspace_bytes(c->n, rows));
      if (rc != PCOA_OK) return rc;
      {
        ScopedTimer t(c, T_DENSIFY);
        HIP_TRY(c, launch_densify_csr_i8(c->csr_idx, c->csr_offs, rows, b, c->pack_buf, c->n, c->err_flag,
                                         c->stream));
      }
      {
        ScopedTimer t(c, T_GRAM);
        HIP_TRY(c, launch_gram_packed(c->pack_buf, 0, rows, c->n, c->s32, c->num_cu, c->stream, nullptr, nullptr, strip_of(c)));
      }
      c->gram_kind = 2;  // a carrier list repeats a callset (or int8 was forced)
      account_gram(c, rows, weight);
      continue;
    }
    {
      ScopedTimer t(c, T_DENSIFY);
      HIP_TRY(c, hipMemsetAsync(c->tile, 0, sizeof(float) * (size_t)(rows * ld4), c->stream));
      HIP_TRY(c, launch_densify_csr(c->csr_idx, c->csr_offs, 0, rows, b, c->tile, ld4, c->n, c->err_flag,
                                    c->stream));
    }
    rc = gram_device(c, c->tile, 0, rows, ld4, false);
    if (rc != PCOA_OK) return rc;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // host arrays may be released by the caller now
  return PCOA_OK;
}

// ---- carrier lists, fast path (r04) ------------------------------------------------------------------
// What bounded the boundary the reference actually has (RDD[Seq[Int]] -> pcoa_accumulate_calls) was the HOST: a serial pass
// over every carrier before the first byte moved, one device staging buffer (copy k+1 could not overlap densify k), pageable
// memcpy, a stream synchronisation per call.  Here the device validates (densify_csr_*_kernel: an index outside [0, N)
// raises bit 0 of csr_flag, a carrier list that names a callset twice -- the atomic OR finds the bit already set -- bit 5),
// chunks of <= 8 M entries travel through two staging slots on a copy stream (pageable sources through pinned twins filled
// by a few host threads), and the chunks are committed into the active operand buffer PROVISIONALLY: csr_validate reads
// the flag before that generation can reach S (fp4_launch), at the end of a synchronous call, and at every synchronising
// call; a bad chunk list is rolled out of the buffer again (S unchanged), a list with repeats is redone by calls_legacy on
// the int8 kernel, which counts multiplicities as the reference's double loop does (VariantsPca.scala:187).
constexpr int64_t kCsrChunkEntries = (int64_t)8 << 20;

static int csr_setup(pcoa_ctx* c) {
  if (c->csr_flag) return PCOA_OK;
  HIP_TRY(c, hipHostMalloc((void**)&c->csr_flag_host, 64, hipHostMallocDefault));
  std::memset(c->csr_flag_host, 0, 64);
  HIP_TRY(c, dev_alloc((void**)&c->csr_flag, 64, c->device));
  HIP_TRY(c, hipMemsetAsync(c->csr_flag, 0, 64, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

// src -> dst by a few host threads (a single memcpy into pinned memory runs at ~10 GB/s; the link takes 50)
static void parallel_copy(void* dst, const void* src, size_t bytes) {
  const size_t kMin = (size_t)4 << 20;
  unsigned nt = std::min<unsigned>(8, std::max<unsigned>(1, std::thread::hardware_concurrency() / 2));
  if (bytes < 2 * kMin) nt = 1;
  nt = (unsigned)std::min<size_t>(nt, (bytes + kMin - 1) / kMin);
  if (nt <= 1) {
    std::memcpy(dst, src, bytes);
    return;
  }
  std::vector<std::thread> th;
  const size_t per = (((bytes + nt - 1) / nt) + 63) & ~(size_t)63;  // nt * per >= bytes (a floor here once lost the last word)
  for (unsigned t = 0; t < nt; ++t) {
    const size_t b0 = std::min(bytes, per * t), b1 = std::min(bytes, per * (t + 1));
    if (b1 > b0) th.emplace_back([=] { std::memcpy((char*)dst + b0, (const char*)src + b0, b1 - b0); });
  }
  for (auto& t : th) t.join();
}

// Validate the provisionally committed carrier-list chunks of the active operand buffer (see above).  Blocks until their
// densify kernels are done.
int csr_validate(pcoa_ctx* c) {
  if (c->csr_pending.empty()) return PCOA_OK;
  pcoa_ctx::Fp4Buf& b = c->fb[c->fb_active];
  hipStream_t s = b.fill_stream ? b.fill_stream : c->stream;
  const double t0 = wall_now();
  HIP_TRY(c, hipMemcpyAsync(c->csr_flag_host, c->csr_flag, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  c->csr_wait_s += wall_now() - t0;
  const int32_t flag = c->csr_flag_host[0], bad_index = c->csr_flag_host[2];
  std::vector<pcoa_ctx::CsrPending> pend;
  pend.swap(c->csr_pending);
  if (flag == 0) return PCOA_OK;
  // roll the chunks out of the buffer again: nothing of this generation has been contracted (fp4_launch validates first)
  int64_t kb = 0, vars = 0;
  for (const auto& q : pend) { kb += q.kb; vars += q.nv; }
  b.kb -= kb;
  b.vars -= vars;
  HIP_TRY(c, hipMemsetAsync(c->csr_flag, 0, 4 * sizeof(int32_t), s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (flag & 1) {
    char msg[256];
    if (bad_index == -2)
      std::snprintf(msg, sizeof(msg), "row_offsets of a carrier-list call are not non-decreasing or run beyond 2^30 entries per 128 "
                    "variants (found by the device-side check); S is unchanged by the calls since the last synchronising call that "
                    "reported no error");
    else
      std::snprintf(msg, sizeof(msg), "callset index %d outside [0, %d) in a carrier list (found by the device-side check); S is "
                    "unchanged by the calls since the last synchronising call that reported no error", bad_index, c->n);
    return fail(c, bad_index == -2 ? PCOA_ERR_INVALID_ARG : PCOA_ERR_INDEX_RANGE, msg);
  }
  if (c->packed_mode == 3)
    return fail(c, PCOA_ERR_INVALID_ARG,
                "a carrier list repeats a callset (multiplicity > 1) and PCOA_FLAG_GRAM_FP4_MFMA was forced");
  // repeats: the same chunks through the int8 kernel, which counts them with multiplicity
  for (const auto& q : pend) {
    c->csr_redo_chunks += 1;
    std::vector<int32_t> hidx;
    std::vector<int64_t> hoffs;
    const int32_t* idx = q.idx;
    const int64_t* offs = q.offs;
    if (q.device) {
      hoffs.resize((size_t)q.nv + 1);
      HIP_TRY(c, hipMemcpy(hoffs.data(), q.offs, sizeof(int64_t) * (size_t)(q.nv + 1), hipMemcpyDeviceToHost));
      const int64_t b0 = hoffs[0], nnz = hoffs[(size_t)q.nv] - b0;
      hidx.resize((size_t)std::max<int64_t>(nnz, 1));
      if (nnz > 0) HIP_TRY(c, hipMemcpy(hidx.data(), q.idx + b0, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost));
      for (auto& o : hoffs) o -= b0;
      idx = hidx.data();
      offs = hoffs.data();
    }
    const int rc = calls_legacy(c, idx, offs, q.nv);
    if (rc != PCOA_OK) return rc;
  }
  return PCOA_OK;
}

static int calls_fast(pcoa_ctx* c, const int32_t* sample_idx, const int64_t* row_offsets, int64_t n_variants, uint32_t flags) {
  const bool device = (flags & PCOA_CALLS_DEVICE_PTR) != 0;
  const bool pinned = (flags & PCOA_CALLS_HOST_PINNED) != 0;
  const bool async = device || (flags & PCOA_CALLS_ASYNC) != 0;
  int rc = csr_setup(c);
  if (rc != PCOA_OK) return rc;
  if ((rc = fp4_setup(c)) != PCOA_OK) return rc;
  // rows per chunk: what one operand buffer takes at most, and (host sources) <= kCsrChunkEntries entries
  const int64_t rows_cap = std::max<int64_t>(128, std::min<int64_t>(fp4_target_kb(c) * 32, (int64_t)1 << 20));
  int64_t v0 = 0;
  c->cs.next = 0;   // every call starts at slot 0
  while (v0 < n_variants) {
    int64_t rows = std::min(rows_cap, n_variants - v0);
    int64_t b0 = 0, nnz = 0;
    if (!device) {
      b0 = row_offsets[v0];
      if (row_offsets[v0 + rows] - b0 > kCsrChunkEntries) {  // largest row count that keeps the chunk under the cap (>= 1)
        const int64_t* lo = row_offsets + v0 + 1;
        const int64_t* up = std::upper_bound(lo, row_offsets + v0 + rows + 1, b0 + kCsrChunkEntries);
        rows = std::max<int64_t>(1, (int64_t)(up - lo));
      }
      nnz = row_offsets[v0 + rows] - b0;
      if (nnz == 0) {  // only empty rows: they add nothing (filtered at VariantsPca.scala:166)
        v0 += rows;
        continue;
      }
    }
    // k-bits operand: chunks are whole blocks of 128 variants except the last of the call
    if (c->op_fmt == 2 && v0 + rows < n_variants && rows >= 128) rows = rows / 128 * 128, nnz = device ? 0 : row_offsets[v0 + rows] - b0;
    const int32_t* idx_dev = sample_idx;
    const int64_t* offs_dev = row_offsets + v0;
    int64_t offs_base = 0;
    StagingRing::Slot* sl = nullptr;
    if (!device) {
      // indices in buffer 0, offsets in buffer 1; both grow by an eighth more than asked, from 2^16 entries
      // (the slot's last reader: its last densify)
      const size_t idx_bytes = sizeof(int32_t) * (size_t)nnz, offs_bytes = sizeof(int64_t) * (size_t)(rows + 1);
      const size_t idx_grow = sizeof(int32_t) * (size_t)std::max<int64_t>(nnz + nnz / 8, 1 << 16);
      const size_t offs_grow = sizeof(int64_t) * (size_t)std::max<int64_t>(rows + 1 + (rows + 1) / 8, 1 << 16);
      if ((rc = staging_acquire(c, c->cs, idx_bytes, idx_grow, &sl, offs_bytes, offs_grow)) != PCOA_OK) return rc;
      const void* src = sample_idx + b0;
      const void* osrc = row_offsets + v0;
      if (!pinned) {
        const double t0 = wall_now();
        if ((rc = staging_pin(c, *sl, 0, idx_bytes, idx_grow)) != PCOA_OK) return rc;
        if ((rc = staging_pin(c, *sl, 1, offs_bytes, offs_grow)) != PCOA_OK) return rc;
        parallel_copy(sl->pin[0], src, idx_bytes);
        std::memcpy(sl->pin[1], osrc, offs_bytes);
        src = sl->pin[0];
        osrc = sl->pin[1];
        c->csr_stage_s += wall_now() - t0;
      }
      HIP_TRY(c, hipMemcpyAsync(sl->dev[0], src, idx_bytes, hipMemcpyHostToDevice, c->csr_stream));
      HIP_TRY(c, hipMemcpyAsync(sl->dev[1], osrc, offs_bytes, hipMemcpyHostToDevice, c->csr_stream));
      if ((rc = staging_copied(c, *sl)) != PCOA_OK) return rc;
      idx_dev = static_cast<const int32_t*>(sl->dev[0]);
      offs_dev = static_cast<const int64_t*>(sl->dev[1]);
      offs_base = b0;
    }
    const int64_t kb = kb_of(c, rows);
    int8_t* dst = nullptr;
    hipStream_t ps = nullptr;
    if ((rc = fp4_reserve(c, kb, rows, 0, false, &dst, &ps, nullptr)) != PCOA_OK) return rc;
    if (sl) HIP_TRY(c, hipStreamWaitEvent(ps, sl->copied, 0));
    {
      ScopedTimer t(c, T_DENSIFY, ps);
      HIP_TRY(c, c->op_fmt == 2 ? launch_densify_csr_kbits(idx_dev, offs_dev, rows, offs_base, dst, c->n, c->csr_flag, ps, kb / 4)
                                : launch_densify_csr_fp4(idx_dev, offs_dev, rows, offs_base, dst, c->n, c->csr_flag, ps, kb));
    }
    if (sl && (rc = staging_released(c, *sl, ps)) != PCOA_OK) return rc;   // the densify is the slot's only reader
    fp4_commit(c, kb, rows);
    c->csr_pending.push_back({device ? sample_idx : sample_idx, row_offsets + v0, rows, kb, device});
    c->csr_fast_chunks += 1;
    v0 += rows;
  }
  if (!async) return csr_validate(c);  // the caller may release (or rewrite) its arrays once this returns
  return PCOA_OK;
}

}  // namespace pcoa

extern "C" {

int pcoa_accumulate_dense_f32(pcoa_ctx* c, const float* x, int64_t n_variants, int64_t ld, int is_device_ptr) {
  CHECK_CTX(c);
  if (c->is_grm) return not_the_bed_boundary(c, "pcoa_accumulate_dense_f32");
  if (c->is_operator) return not_a_bitset_boundary(c, "pcoa_accumulate_dense_f32");
  if (n_variants < 0 || (n_variants > 0 && !x)) return fail(c, PCOA_ERR_INVALID_ARG, "x is NULL or n_variants < 0");
  if (ld < c->n) return fail(c, PCOA_ERR_INVALID_ARG, "ld must be >= n_samples");
  if (n_variants == 0) return PCOA_OK;
  return is_device_ptr ? gram_device(c, x, 0, n_variants, ld, true) : dense_host(c, x, n_variants, ld);
}

int pcoa_accumulate_dense_u8(pcoa_ctx* c, const uint8_t* x, int64_t n_variants, int64_t ld, int is_device_ptr) {
  CHECK_CTX(c);
  if (c->is_grm) return not_the_bed_boundary(c, "pcoa_accumulate_dense_u8");
  if (c->is_operator) return not_a_bitset_boundary(c, "pcoa_accumulate_dense_u8");
  if (n_variants < 0 || (n_variants > 0 && !x)) return fail(c, PCOA_ERR_INVALID_ARG, "x is NULL or n_variants < 0");
  if (ld < c->n) return fail(c, PCOA_ERR_INVALID_ARG, "ld must be >= n_samples");
  if (n_variants == 0) return PCOA_OK;
  return is_device_ptr ? gram_device(c, x, 1, n_variants, ld, true) : dense_host(c, x, n_variants, ld);
}

int pcoa_accumulate_bits(pcoa_ctx* c, const uint32_t* bits, int64_t n_variants, int64_t ld_words, int is_device_ptr) {
  CHECK_CTX(c);
  if (c->is_grm) return not_the_bed_boundary(c, "pcoa_accumulate_bits");
  if (n_variants < 0 || (n_variants > 0 && !bits))
    return fail(c, PCOA_ERR_INVALID_ARG, "bits is NULL or n_variants < 0");
  int rc = check_ld_words(c, "", ld_words);
  if (rc != PCOA_OK) return rc;
  if (!c->use_i8)
    return fail(c, PCOA_ERR_INVALID_ARG, "the bit-packed boundary needs a packed-operand engine (not PCOA_FLAG_GRAM_F32_MFMA)");
  if (n_variants == 0) return PCOA_OK;
  if (is_device_ptr) return gram_device_bits(c, bits, n_variants, ld_words, true);
  // host bitsets: <= 2^17 rows and <= 256 MiB per slot at a time (r06: the copy of chunk k + 1 runs beside the transpose and the
  // contraction of chunk k, as the .bed rows of pcoa_accumulate_plink_bed do; r05 staged 64-MiB-word chunks on the ctx stream,
  // copy and kernels in series).  The byte cap binds only for wide rows: 2^17 rows of N = 250,000 would be 4.1 GB per slot,
  // beside a strip owner's matrix.
  const int64_t slot_rows = std::min<int64_t>((int64_t)1 << 17, ((int64_t)256 << 20) / (words_of(c) * 4));
  const int64_t rows_cap = std::max<int64_t>(1, std::min<int64_t>(n_variants, slot_rows));
  // host rows are consumed once their copy is done; the kernels are queued (the transpose runs on the ctx stream)
  return feed_bits(c, bits, n_variants, ld_words, rows_cap, false, true, [&](const uint32_t* stage, int64_t ld, int64_t, int64_t rows) {
    return gram_device_bits(c, stage, rows, ld, false);
  });
}

// PLINK 1 .bed rows as they lie in the file (r04): decoded on the device.  The host's share of a whole-genome fileset is
// then reading it; 626 B per variant cross PCIe at N = 2504 (a 100 M variants/s link bound) instead of carrier lists or
// host-built bitsets.  Chunks of <= 2^17 rows: raw rows -> plink_bed_to_bits_kernel -> the bitset transpose -> operand.
int pcoa_accumulate_plink_bed(pcoa_ctx* c, const uint8_t* bed_rows, int64_t n_variants, int64_t row_bytes, int ref_is_a1,
                              int is_device_ptr) {
  CHECK_CTX(c);
  if (n_variants < 0 || (n_variants > 0 && !bed_rows)) return fail(c, PCOA_ERR_INVALID_ARG, "bed_rows is NULL or n_variants < 0");
  int rc = check_row_bytes(c, "", row_bytes);
  if (rc != PCOA_OK) return rc;
  if (!c->use_i8)
    return fail(c, PCOA_ERR_INVALID_ARG, "the PLINK boundary needs a packed-operand engine (not PCOA_FLAG_GRAM_F32_MFMA)");
  if ((rc = check_bed_source(c, "", is_device_ptr, true)) != PCOA_OK) return rc;
  if (n_variants == 0) return PCOA_OK;
  if (c->is_grm) return grm_accumulate_bed(c, bed_rows, n_variants, row_bytes, ref_is_a1, is_device_ptr);
  const int64_t words = words_of(c);
  const int64_t rows_cap = std::min<int64_t>(n_variants, (int64_t)1 << 17);
  if ((rc = ensure(c, &c->tile, &c->tile_elems, rows_cap * words)) != PCOA_OK) return rc;
  uint32_t* bits = reinterpret_cast<uint32_t*>(c->tile);
  // r05: a host chunk travels on the copy stream beside the decode, transpose and contraction of the chunk (or the call)
  // before; the r04 form queued everything on the ctx stream and drained it before returning.  Host rows are consumed once
  // their copy is done; a device input (read by the decode kernel only) follows the lifetime rule of every device input
  return feed_bed(c, bed_rows, n_variants, row_bytes, rows_cap, is_device_ptr, true, bed_decoder(c, row_bytes, ref_is_a1, bits),
                  [&](int64_t, int64_t rows) { return gram_device_bits(c, bits, rows, words, false); });
}

int pcoa_accumulate_calls_ex(pcoa_ctx* c, const int32_t* sample_idx, const int64_t* row_offsets, int64_t n_variants,
                             uint32_t flags) {
  CHECK_CTX(c);
  if (c->is_grm) return not_the_bed_boundary(c, "pcoa_accumulate_calls");
  if (c->is_operator) return not_a_bitset_boundary(c, "pcoa_accumulate_calls",
                                                        " (a carrier list can repeat a callset, a bitset cannot)");
  if (n_variants < 0 || !row_offsets) return fail(c, PCOA_ERR_INVALID_ARG, "row_offsets is NULL or n_variants < 0");
  if (flags & ~(uint32_t)(PCOA_CALLS_DEVICE_PTR | PCOA_CALLS_HOST_PINNED | PCOA_CALLS_ASYNC))
    return fail(c, PCOA_ERR_INVALID_ARG, "unknown PCOA_CALLS_* flag");
  if (n_variants == 0) return PCOA_OK;
  const bool device = (flags & PCOA_CALLS_DEVICE_PTR) != 0;
  if (!device) {
    const int64_t nnz_total = row_offsets[n_variants] - row_offsets[0];
    if (nnz_total < 0 || (nnz_total > 0 && !sample_idx))
      return fail(c, PCOA_ERR_INVALID_ARG, "sample_idx is NULL or row_offsets decreasing");
    for (int64_t v = 0; v < n_variants; ++v)  // (8 bytes per variant: not the pass over the entries)
      if (row_offsets[v + 1] < row_offsets[v]) return fail(c, PCOA_ERR_INVALID_ARG, "row_offsets not monotone");
  } else if (!sample_idx) {
    return fail(c, PCOA_ERR_INVALID_ARG, "sample_idx is NULL");
  }
  // the engines with a binary-tile operand take the fast path; fp32-MFMA and int8-only ctxs the host-validated one
  const bool fast = c->use_i8 && c->packed_mode != 2 && !debug_knobs().csr_legacy;
  if (fast) return calls_fast(c, sample_idx, row_offsets, n_variants, flags);
  if (!device) return calls_legacy(c, sample_idx, row_offsets, n_variants);
  // device arrays on an engine without the fast path: through the host
  std::vector<int64_t> hoffs((size_t)n_variants + 1);
  HIP_TRY(c, hipMemcpy(hoffs.data(), row_offsets, sizeof(int64_t) * (size_t)(n_variants + 1), hipMemcpyDeviceToHost));
  const int64_t b0 = hoffs[0], nnz = hoffs[(size_t)n_variants] - b0;
  if (nnz < 0) return fail(c, PCOA_ERR_INVALID_ARG, "row_offsets decreasing");
  std::vector<int32_t> hidx((size_t)std::max<int64_t>(nnz, 1));
  if (nnz > 0) HIP_TRY(c, hipMemcpy(hidx.data(), sample_idx + b0, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost));
  for (auto& o : hoffs) o -= b0;
  return calls_legacy(c, hidx.data(), hoffs.data(), n_variants);
}

int pcoa_accumulate_calls(pcoa_ctx* c, const int32_t* sample_idx, const int64_t* row_offsets, int64_t n_variants) {
  return pcoa_accumulate_calls_ex(c, sample_idx, row_offsets, n_variants, 0);
}

int pcoa_synth_fill_f32(pcoa_ctx* c, const pcoa_synth_params* p, int64_t first_variant, int64_t n_variants,
                        float* x_dev, int64_t ld) {
  CHECK_CTX(c);
  if (n_variants < 0 || first_variant < 0 || (n_variants > 0 && !x_dev) || ld < c->n)
    return fail(c, PCOA_ERR_INVALID_ARG, "synth_fill: bad argument");
  if (n_variants == 0) return PCOA_OK;
  int rc = upload_synth(c, p, n_variants);
  if (rc != PCOA_OK) return rc;
  {
    ScopedTimer t(c, T_SYNTH);
    HIP_TRY(c, launch_synth_fill_f32(p->seed, c->thr_dev, c->sample_pop, p->n_pops, first_variant, n_variants,
                                     c->n, x_dev, ld, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // thresholds were copied from caller memory
  return PCOA_OK;
}

int pcoa_accumulate_synthetic(pcoa_ctx* c, const pcoa_synth_params* p, int64_t first_variant, int64_t n_variants) {
  CHECK_CTX(c);
  if (c->is_grm) return not_the_bed_boundary(c, "pcoa_accumulate_synthetic");
  if (c->is_operator) return not_a_bitset_boundary(c, "pcoa_accumulate_synthetic",
                                                        " (the generator writes the contraction operand, not variant-major bitsets)");
  if (n_variants < 0 || first_variant < 0) return fail(c, PCOA_ERR_INVALID_ARG, "synthetic: negative range");
  if (n_variants == 0) return PCOA_OK;
  if (!p || !p->thresholds) return fail(c, PCOA_ERR_INVALID_ARG, "synthetic params: null");
  if (c->use_i8 && c->packed_mode != 2 && c->op_fmt == 2 && p->n_pops > 0 && p->n_pops <= 64 && !debug_knobs().synth_tile)
    return synth_bits(c, p, first_variant, n_variants);
  const int64_t ld4 = round_up(c->n, 4);
  const int64_t rows_cap = staging_rows(n_variants, ld4);
  int rc = ensure(c, &c->tile, &c->tile_elems, rows_cap * ld4);
  if (rc != PCOA_OK) return rc;
  for (int64_t v0 = 0; v0 < n_variants; v0 += rows_cap) {
    const int64_t rows = std::min(rows_cap, n_variants - v0);
    pcoa_synth_params q = *p;
    q.thresholds = p->thresholds + v0 * p->n_pops;
    rc = upload_synth(c, &q, rows);
    if (rc != PCOA_OK) return rc;
    {
      ScopedTimer t(c, T_SYNTH);
      HIP_TRY(c, launch_synth_fill_f32(q.seed, c->thr_dev, c->sample_pop, q.n_pops, first_variant + v0, rows, c->n,
                                       c->tile, ld4, c->stream));
    }
    rc = gram_device(c, c->tile, 0, rows, ld4, false);
    if (rc != PCOA_OK) return rc;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

}  // extern "C"
