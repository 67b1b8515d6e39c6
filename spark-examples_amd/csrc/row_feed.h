// row_feed.h -- the loop that brings a caller's variant rows onto the device, for every boundary that takes carrier bitsets or
// raw PLINK .bed rows (capi_accumulate, capi_loadings, capi_ld, capi_complete).  [0, n_variants) is cut into chunks of rows_cap
// rows; a host chunk travels on the copy stream (c->csr_stream) into the next slot of the ring c->bs (row_feed.hip), and then,
// in this order:
//   staging_copied                `copied` recorded behind the copy
//   c->stream waits for `copied`
//   the slot's reader             queued on c->stream: the consumer of bitsets, the decode of .bed rows
//   staging_released              `freed` recorded on c->stream behind that reader -- on every exit path once `copied` is
//                                 recorded, a failed reader included (the first error is the one returned); the acquire two
//                                 chunks later is the only host wait for it
//   (.bed rows) the consumer of the decoded rows, behind the release: the next acquire of this slot does not wait for it
// A device source that comes through the feed (.bed rows, the pruner's bitsets) skips the slot: its chunks go to the same
// callables in the same sequence.  Device bitsets of pcoa_accumulate_bits and pcoa_loadings_bits do not come through the feed:
// those boundaries hand the whole range to their consumer.  A call ends with the host waiting
// for the last `copied` where the boundary asks for it (host_waits): a host input is consumed when its copy is done, not when
// its kernels are.  What differs between the boundaries is passed in: rows_cap, the callables (with their decode buffers,
// timers and counters) and the end of the call.  Everything here has internal linkage.
#pragma once

#include <string>

#include "pcoa_ctx.h"

namespace pcoa {
namespace {

// ---- the argument checks the row boundaries share; `fn` is the boundary's message prefix ("" for the two accumulate calls)
int check_ld_words(pcoa_ctx* c, const char* fn, int64_t ld_words) {
  if (ld_words < words_of(c)) return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "ld_words must be >= ceil(n_samples / 32)");
  return PCOA_OK;
}

int check_row_bytes(pcoa_ctx* c, const char* fn, int64_t row_bytes) {
  if (row_bytes < ((int64_t)c->n + 3) / 4) return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "row_bytes must be >= ceil(n_samples / 4)");
  return PCOA_OK;
}

// is_device_ptr of a .bed boundary: 0, 1 and, where the boundary takes queued rows, PCOA_BED_HOST_ASYNC
int check_bed_source(pcoa_ctx* c, const char* fn, int is_device_ptr, bool async_ok) {
  if (is_device_ptr == 0 || is_device_ptr == 1 || (async_ok && is_device_ptr == PCOA_BED_HOST_ASYNC)) return PCOA_OK;
  return fail(c, PCOA_ERR_INVALID_ARG, std::string(fn) + "is_device_ptr must be 0" + (async_ok ? ", 1 or PCOA_BED_HOST_ASYNC" : " or 1"));
}

// The queued form (PCOA_BED_HOST_ASYNC) is only safe for page-locked rows: pageable memory goes through the runtime's staging
// copy, whose timing the "second later call" rule does not cover -- such rows are consumed before the call returns
bool page_locked(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeHost) return true;
  (void)hipGetLastError();
  return false;
}

// `copied` of the slot is recorded: c->stream waits for it, `reader` queues the slot's only reader there, the slot is released
template <typename Reader>
int staging_read(pcoa_ctx* c, StagingRing::Slot& sl, Reader reader) {
  const int rc = [&]() -> int {
    HIP_TRY(c, hipStreamWaitEvent(c->stream, sl.copied, 0));
    return reader();
  }();
  const int rc2 = staging_released(c, sl, c->stream);
  return rc != PCOA_OK ? rc : rc2;
}

int feed_end(pcoa_ctx* c, StagingRing::Slot* last, bool host_waits) {
  if (last && host_waits) HIP_TRY(c, hipEventSynchronize(last->copied));   // (copies complete in order on the copy stream)
  return PCOA_OK;
}

// Carrier bitsets: consume(bits_dev, ld, v0, rows) per chunk.  Host rows arrive dense (ld = ceil(n / 32)) in a slot sized
// rows_cap rows; device rows are read where they lie.
template <typename Consume>
int feed_bits(pcoa_ctx* c, const uint32_t* bits, int64_t n_variants, int64_t ld_words, int64_t rows_cap, bool is_device, bool host_waits,
              Consume consume) {
  const int64_t words = words_of(c);
  StagingRing::Slot* last = nullptr;
  for (int64_t v0 = 0; v0 < n_variants; v0 += rows_cap) {
    const int64_t rows = std::min(rows_cap, n_variants - v0);
    const uint32_t* src = bits + v0 * ld_words;
    int rc;
    if (is_device) {
      rc = consume(src, ld_words, v0, rows);
    } else {
      const size_t bytes = (size_t)(rows * words * 4);
      if ((rc = staging_acquire(c, c->bs, bytes, (size_t)(rows_cap * words * 4), &last)) != PCOA_OK) return rc;
      uint32_t* stage = static_cast<uint32_t*>(last->dev[0]);
      if (ld_words == words)   // dense rows: one linear copy (the strided form crosses the link at ~30 GB/s, this one at ~55)
        HIP_TRY(c, hipMemcpyAsync(stage, src, bytes, hipMemcpyHostToDevice, c->csr_stream));
      else
        HIP_TRY(c, hipMemcpy2DAsync(stage, (size_t)words * 4, src, (size_t)ld_words * 4, (size_t)words * 4, (size_t)rows, hipMemcpyHostToDevice,
                                    c->csr_stream));
      if ((rc = staging_copied(c, *last)) != PCOA_OK) return rc;
      rc = staging_read(c, *last, [&] { return consume(stage, words, v0, rows); });
    }
    if (rc != PCOA_OK) return rc;
  }
  return feed_end(c, last, host_waits);
}

// Raw .bed rows: decode(src_dev, v0, rows) reads the raw rows of a chunk (the slot's only reader), consume(v0, rows) takes what
// it wrote.  source: the boundary's is_device_ptr (0, 1 or PCOA_BED_HOST_ASYNC, which drops the host wait for page-locked rows).
template <typename Decode, typename Consume>
int feed_bed(pcoa_ctx* c, const uint8_t* bed_rows, int64_t n_variants, int64_t row_bytes, int64_t rows_cap, int source, bool host_waits,
             Decode decode, Consume consume) {
  if (source == PCOA_BED_HOST_ASYNC && page_locked(bed_rows)) host_waits = false;
  StagingRing::Slot* last = nullptr;
  for (int64_t v0 = 0; v0 < n_variants; v0 += rows_cap) {
    const int64_t rows = std::min(rows_cap, n_variants - v0);
    const uint8_t* src = bed_rows + v0 * row_bytes;
    int rc;
    if (source == 1) {
      rc = decode(src, v0, rows);
    } else {
      const size_t bytes = (size_t)(rows * row_bytes);
      if ((rc = staging_acquire(c, c->bs, bytes, (size_t)(rows_cap * row_bytes), &last)) != PCOA_OK) return rc;
      HIP_TRY(c, hipMemcpyAsync(last->dev[0], src, bytes, hipMemcpyHostToDevice, c->csr_stream));
      if ((rc = staging_copied(c, *last)) != PCOA_OK) return rc;
      rc = staging_read(c, *last, [&] { return decode(static_cast<const uint8_t*>(last->dev[0]), v0, rows); });
    }
    if (rc == PCOA_OK) rc = consume(v0, rows);
    if (rc != PCOA_OK) return rc;
  }
  return feed_end(c, last, host_waits);
}

// the decode of plain .bed rows for feed_bed: a chunk's carrier bitsets into `dst`, dense, on c->stream
auto bed_decoder(pcoa_ctx* c, int64_t row_bytes, int ref_is_a1, uint32_t* dst) {
  return [=](const uint8_t* src, int64_t, int64_t rows) -> int {
    ScopedTimer t(c, T_DENSIFY);
    HIP_TRY(c, launch_plink_bed_to_bits(src, row_bytes, rows, c->n, words_of(c), ref_is_a1 ? 1 : 0, dst, c->stream));
    return PCOA_OK;
  };
}

}  // namespace
}  // namespace pcoa
