// row_feed.hip -- the staging ring of the host boundaries (protocol: StagingRing, pcoa_ctx.h).  Its users: the row feed of the
// bitset and .bed boundaries (row_feed.h, c->bs), the carrier lists (calls_fast, c->cs) and the thresholds of the synthetic
// generator (synth_bits, c->ts).
#include "pcoa_ctx.h"

namespace pcoa {

// buffer i of a slot whose last reader is done: regrown to grow_to bytes unless it holds `need` already
static int staging_fit(pcoa_ctx* c, StagingRing::Slot& sl, int i, size_t need, size_t grow_to) {
  if (need <= sl.dev_bytes[i]) return PCOA_OK;
  sl.dev_bytes[i] = 0;
  const int rc = regrow(c, &sl.dev[i], grow_to, false);
  if (rc == PCOA_OK) sl.dev_bytes[i] = grow_to;
  return rc;
}

// The next slot of the ring, free to be rewritten, with `need` bytes in buffer 0 (and need1 in buffer 1).  Creates the copy
// stream and the ring's events on first use.
int staging_acquire(pcoa_ctx* c, StagingRing& r, size_t need, size_t grow_to, StagingRing::Slot** out, size_t need1, size_t grow_to1) {
  if (!c->csr_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->csr_stream, hipStreamNonBlocking));
  for (auto& sl : r.slot)
    if (!sl.copied) {
      HIP_TRY(c, hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming));
      HIP_TRY(c, hipEventCreateWithFlags(&sl.freed, hipEventDisableTiming));
    }
  StagingRing::Slot& sl = r.slot[r.next++ & 1];
  if (sl.used) HIP_TRY(c, hipEventSynchronize(sl.freed));   // the kernels that read the slot last are done (its H2D long before)
  int rc = staging_fit(c, sl, 0, need, grow_to);
  if (rc == PCOA_OK) rc = staging_fit(c, sl, 1, need1, grow_to1);
  *out = &sl;
  return rc;
}

// the page-locked twin of buffer i (pageable sources are copied into it by the host before the H2D)
int staging_pin(pcoa_ctx* c, StagingRing::Slot& sl, int i, size_t need, size_t grow_to) {
  if (need <= sl.pin_bytes[i]) return PCOA_OK;
  if (sl.pin[i]) (void)hipHostFree(sl.pin[i]);
  sl.pin[i] = nullptr;
  sl.pin_bytes[i] = 0;
  HIP_TRY(c, hipHostMalloc(&sl.pin[i], grow_to, hipHostMallocDefault));
  sl.pin_bytes[i] = grow_to;
  return PCOA_OK;
}

// the slot's copies have been queued on the copy stream
int staging_copied(pcoa_ctx* c, StagingRing::Slot& sl) {
  HIP_TRY(c, hipEventRecord(sl.copied, c->csr_stream));
  return PCOA_OK;
}

// the last kernel that reads the slot has been queued on `reader`
int staging_released(pcoa_ctx* c, StagingRing::Slot& sl, hipStream_t reader) {
  HIP_TRY(c, hipEventRecord(sl.freed, reader));
  sl.used = true;
  return PCOA_OK;
}

// every reader of every slot is done
int staging_wait_all(pcoa_ctx* c, StagingRing& r) {
  for (auto& sl : r.slot)
    if (sl.used) HIP_TRY(c, hipEventSynchronize(sl.freed));
  return PCOA_OK;
}

void staging_destroy(StagingRing& r) {
  for (auto& sl : r.slot) {
    if (sl.copied) (void)hipEventDestroy(sl.copied);
    if (sl.freed) (void)hipEventDestroy(sl.freed);
    for (void* d : sl.dev)
      if (d) dev_free(d);
    for (void* h : sl.pin)
      if (h) (void)hipHostFree(h);
    sl = StagingRing::Slot();
  }
}

}  // namespace pcoa
