// capi_ld.hip -- pcoa_ld_*: LD pruning of the variant rows in front of the accumulation (the rule is stated at
// the block of pcoa.h and the kernels in ld.hip).  pcoa_ld_begin sizes every buffer once; the calls between begin and end stream
// rows through them a CHUNK (<= ldp_chunk rows) at a time:
//   count (the row, tail bits cleared, into the work buffer behind the carried tail; its carrier count)  ->  band (the exceeds bit
//   of every row against the `window` rows before it)  ->  resolve (the greedy pass, on the device)  ->  scan, gather of the kept
//   rows (PCOA_LD_ACCUMULATE)  ->  the last `window` rows move to the front of the work buffer as the next chunk's tail.
// All of it is queued on the ctx stream; the chunk then ends with ONE host wait, for its kept count and its keep flags, and with
// PCOA_LD_ACCUMULATE the compacted rows go to gram_device_bits as a device input whose pre-pass runs on the ctx stream (can_defer
// = false: no side stream, no second read), so the next chunk's gather, queued on the same stream, cannot overtake its reader.
// The rows reach run_chunk through the row feed (row_feed.h), host and device rows in the same chunks of ldp_chunk; the feed
// ends without a host wait of its own, since every chunk's wait has covered the copy.  Only n, the device, the ctx stream and
// the staging slots of the ctx are used besides: every kind of ctx serves.
#include <cmath>
#include <cstring>
#include <string>

#include "pcoa_ctx.h"
#include "row_feed.h"

using namespace pcoa;

namespace {

constexpr int64_t kLdChunkRows = (int64_t)1 << 16;     // rows per chunk at most
constexpr int64_t kLdChunkBytes = (int64_t)256 << 20;  // and bytes of rows per chunk

int not_begun(pcoa_ctx* c, const char* call) {
  return fail(c, PCOA_ERR_STATE, std::string(call) + ": no pruner is active; call pcoa_ld_begin first");
}

template <typename T>
int ld_alloc(pcoa_ctx* c, T** out, int64_t count) {
  void* p = nullptr;
  const hipError_t e = dev_alloc(&p, sizeof(T) * (size_t)count, c->device);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, PCOA_ERR_OUT_OF_MEMORY, std::string("pcoa_ld_begin: no memory for the pruner's buffers (") + hipGetErrorString(e) + ")");
  }
  *out = static_cast<T*>(p);
  return PCOA_OK;
}

// vc <= ldp_chunk rows on the device, readable on the ctx stream
int run_chunk(pcoa_ctx* c, const uint32_t* rows_dev, int64_t ld, int64_t vc, uint8_t* keep_out, int64_t* kept_out) {
  const int64_t words = words_of(c);
  const int32_t W = c->ldp_window, T = c->ldp_tail;
  uint32_t* wb_rows = c->ldp_wb + (int64_t)W * words;
  int32_t* cnt_rows = c->ldp_cnt + W;
  {
    ScopedTimer t(c, T_LD_COUNT);
    HIP_TRY(c, launch_ld_count(rows_dev, ld, vc, c->n, wb_rows, cnt_rows, c->stream));
  }
  {
    ScopedTimer t(c, T_LD_BAND);
    HIP_TRY(c, launch_ld_band(c->ldp_wb, c->ldp_cnt, vc, c->n, W, T, c->ldp_r2, c->ldp_ex, c->stream));
  }
  {
    ScopedTimer t(c, T_LD_RESOLVE);
    HIP_TRY(c, launch_ld_resolve(c->ldp_ex, cnt_rows, vc, c->n, W, c->ldp_pos, c->ldp_flags, c->ldp_kbits, c->stream));
  }
  const int32_t new_tail = (int32_t)std::min<int64_t>(W, (int64_t)T + vc);
  {
    ScopedTimer t(c, T_LD_COMPACT);
    HIP_TRY(c, launch_ld_scan(c->ldp_kbits, c->ldp_pos, cnt_rows, vc, c->n, c->ldp_keep, c->ldp_scan, c->ldp_out2, c->stream));
    if (c->ldp_accumulate)
      HIP_TRY(c, launch_ld_gather(wb_rows, c->ldp_keep, c->ldp_scan, vc, c->n, c->ldp_compact, c->stream));
    // the last new_tail rows become [W - new_tail, W); a chunk shorter than the window overlaps its destination and goes through tmp
    const int64_t src = (int64_t)W + vc - new_tail, dst = (int64_t)W - new_tail;
    const size_t row_bytes = sizeof(uint32_t) * (size_t)(new_tail * words), cnt_bytes = sizeof(int32_t) * (size_t)new_tail;
    if (vc >= W) {
      HIP_TRY(c, hipMemcpyAsync(c->ldp_wb + dst * words, c->ldp_wb + src * words, row_bytes, hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(c, hipMemcpyAsync(c->ldp_cnt + dst, c->ldp_cnt + src, cnt_bytes, hipMemcpyDeviceToDevice, c->stream));
    } else {
      uint32_t* tmp_cnt = c->ldp_tmp + (int64_t)W * words;
      HIP_TRY(c, hipMemcpyAsync(c->ldp_tmp, c->ldp_wb + src * words, row_bytes, hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(c, hipMemcpyAsync(tmp_cnt, c->ldp_cnt + src, cnt_bytes, hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(c, hipMemcpyAsync(c->ldp_wb + dst * words, c->ldp_tmp, row_bytes, hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(c, hipMemcpyAsync(c->ldp_cnt + dst, tmp_cnt, cnt_bytes, hipMemcpyDeviceToDevice, c->stream));
    }
  }
  HIP_TRY(c, hipMemcpyAsync(c->hw->ld, c->ldp_out2, sizeof(int64_t) * 2, hipMemcpyDeviceToHost, c->stream));
  if (keep_out) HIP_TRY(c, hipMemcpyAsync(keep_out, c->ldp_keep, (size_t)vc, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // the chunk is through: the carried state now describes the rows behind it, whatever the accumulation below says
  const int64_t kept = c->hw->ld[0], k = std::min<int64_t>(vc, W - T);
  c->ldp_pairs += k * T + k * (k - 1) / 2 + (vc - k) * W;
  c->ldp_seen += vc;
  c->ldp_kept += kept;
  c->ldp_mono += c->hw->ld[1];
  c->ldp_tail = new_tail;
  c->ldp_pos += vc;
  *kept_out += kept;
  if (c->ldp_accumulate && kept > 0) return gram_device_bits(c, c->ldp_compact, kept, words, false);
  return PCOA_OK;
}

int check_rows_call(pcoa_ctx* c, const char* call, const void* rows, int64_t n_variants) {
  if (!c->ldp_active) return not_begun(c, call);
  if (n_variants < 0 || (n_variants > 0 && !rows))
    return fail(c, PCOA_ERR_INVALID_ARG, std::string(call) + ": the rows are NULL, or n_variants < 0");
  return PCOA_OK;
}

}  // namespace

namespace pcoa {

void ld_destroy(pcoa_ctx* c) {
  for (void* p : {(void*)c->ldp_wb, (void*)c->ldp_cnt, (void*)c->ldp_tmp, (void*)c->ldp_ex, (void*)c->ldp_flags, (void*)c->ldp_kbits, (void*)c->ldp_keep,
                  (void*)c->ldp_scan, (void*)c->ldp_out2, (void*)c->ldp_compact, (void*)c->ldp_bed})
    if (p) dev_free(p);
  c->ldp_wb = c->ldp_tmp = c->ldp_ex = c->ldp_flags = c->ldp_kbits = c->ldp_compact = c->ldp_bed = nullptr;
  c->ldp_cnt = c->ldp_scan = nullptr;
  c->ldp_keep = nullptr;
  c->ldp_out2 = nullptr;
  c->ldp_bed_cap = 0;
  c->ldp_active = c->ldp_accumulate = false;
  c->ldp_window = c->ldp_tail = 0;
  c->ldp_pos = 0;
}

// the band kernel gives a row no bit against a row that is not among the ldp_tail carried ones, so the flags of the resolve wave
// and the rows in the work buffer need no clearing
void ld_drop_tail(pcoa_ctx* c) {
  c->ldp_tail = 0;
  c->ldp_pos = 0;
}

}  // namespace pcoa

extern "C" {

int pcoa_ld_begin(pcoa_ctx* c, int32_t window, double r2_max, uint32_t flags) {
  CHECK_CTX(c);
  NOT_ON_GRM(c, "pcoa_ld_begin");
  if (window < 1 || window > PCOA_LD_MAX_WINDOW)
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_ld_begin: window = " + std::to_string(window) + " is outside [1, " +
                                             std::to_string(PCOA_LD_MAX_WINDOW) + "]");
  if (!(r2_max >= 0.0 && r2_max <= 1.0))
    return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_ld_begin: r2_max = " + std::to_string(r2_max) + " is outside [0, 1]");
  if (flags & ~(uint32_t)PCOA_LD_ACCUMULATE) return fail(c, PCOA_ERR_INVALID_ARG, "pcoa_ld_begin: unknown PCOA_LD_* flag");
  const bool accumulate = (flags & PCOA_LD_ACCUMULATE) != 0;
  if (accumulate && !c->use_i8)
    return fail(c, PCOA_ERR_INVALID_ARG,
                "pcoa_ld_begin: PCOA_LD_ACCUMULATE feeds the bit-packed boundary, which needs a packed-operand engine (not PCOA_FLAG_GRAM_F32_MFMA)");
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // kernels of an earlier pruner may still run
  ld_destroy(c);
  const int64_t words = words_of(c), W = window, ew = (W + 31) / 32;
  const int64_t chunk = std::max<int64_t>(1, std::min(kLdChunkRows, kLdChunkBytes / (words * 4)));
  int rc = PCOA_OK;
  if ((rc = ld_alloc(c, &c->ldp_wb, (W + chunk) * words)) != PCOA_OK || (rc = ld_alloc(c, &c->ldp_cnt, W + chunk)) != PCOA_OK ||
      (rc = ld_alloc(c, &c->ldp_tmp, W * words + W)) != PCOA_OK || (rc = ld_alloc(c, &c->ldp_ex, chunk * ew)) != PCOA_OK ||
      (rc = ld_alloc(c, &c->ldp_flags, 64)) != PCOA_OK || (rc = ld_alloc(c, &c->ldp_kbits, chunk / 32 + 2)) != PCOA_OK || (rc = ld_alloc(c, &c->ldp_keep, chunk)) != PCOA_OK ||
      (rc = ld_alloc(c, &c->ldp_scan, chunk)) != PCOA_OK || (rc = ld_alloc(c, &c->ldp_out2, 2)) != PCOA_OK ||
      (accumulate && (rc = ld_alloc(c, &c->ldp_compact, chunk * words)) != PCOA_OK)) {
    ld_destroy(c);
    return rc;
  }
  HIP_TRY(c, hipMemsetAsync(c->ldp_flags, 0, sizeof(uint32_t) * 64, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->ldp_wb, 0, sizeof(uint32_t) * (size_t)(W * words), c->stream));
  HIP_TRY(c, hipMemsetAsync(c->ldp_cnt, 0, sizeof(int32_t) * (size_t)W, c->stream));
  c->ldp_window = window;
  c->ldp_r2 = r2_max;
  c->ldp_chunk = chunk;
  c->ldp_accumulate = accumulate;
  c->ldp_active = true;
  return PCOA_OK;
}

int pcoa_ld_break(pcoa_ctx* c) {
  CHECK_CTX(c);
  if (!c->ldp_active) return not_begun(c, "pcoa_ld_break");
  ld_drop_tail(c);
  return PCOA_OK;
}

int pcoa_ld_end(pcoa_ctx* c) {
  CHECK_CTX(c);
  if (!c->ldp_active) return PCOA_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // queued kernels (the pre-pass of the last compacted rows among them) read the buffers
  ld_destroy(c);
  return PCOA_OK;
}

int pcoa_ld_bits(pcoa_ctx* c, const uint32_t* bits, int64_t n_variants, int64_t ld_words, int is_device_ptr, uint8_t* keep_out,
                 int64_t* n_kept_out) {
  CHECK_CTX(c);
  int rc = check_rows_call(c, "pcoa_ld_bits", bits, n_variants);
  if (rc != PCOA_OK) return rc;
  if ((rc = check_ld_words(c, "pcoa_ld_bits: ", ld_words)) != PCOA_OK) return rc;
  int64_t kept = 0;
  if (n_kept_out) *n_kept_out = 0;
  rc = feed_bits(c, bits, n_variants, ld_words, std::min(n_variants, c->ldp_chunk), is_device_ptr != 0, false,
                 [&](const uint32_t* rows_dev, int64_t ld, int64_t v0, int64_t rows) {
                   return run_chunk(c, rows_dev, ld, rows, keep_out ? keep_out + v0 : nullptr, &kept);
                 });
  if (rc == PCOA_OK && n_kept_out) *n_kept_out = kept;
  return rc;
}

int pcoa_ld_plink_bed(pcoa_ctx* c, const uint8_t* bed_rows, int64_t n_variants, int64_t row_bytes, int ref_is_a1, int is_device_ptr,
                      uint8_t* keep_out, int64_t* n_kept_out) {
  CHECK_CTX(c);
  int rc = check_rows_call(c, "pcoa_ld_plink_bed", bed_rows, n_variants);
  if (rc != PCOA_OK) return rc;
  if ((rc = check_row_bytes(c, "pcoa_ld_plink_bed: ", row_bytes)) != PCOA_OK) return rc;
  if ((rc = check_bed_source(c, "pcoa_ld_plink_bed: ", is_device_ptr, false)) != PCOA_OK) return rc;
  int64_t kept = 0;
  if (n_kept_out) *n_kept_out = 0;
  if (n_variants == 0) return PCOA_OK;
  const int64_t words = words_of(c);
  const int64_t rows_cap = std::min(n_variants, c->ldp_chunk);
  if ((rc = ensure(c, &c->ldp_bed, &c->ldp_bed_cap, rows_cap * words)) != PCOA_OK) return rc;
  rc = feed_bed(c, bed_rows, n_variants, row_bytes, rows_cap, is_device_ptr, false, bed_decoder(c, row_bytes, ref_is_a1, c->ldp_bed),
                [&](int64_t v0, int64_t rows) { return run_chunk(c, c->ldp_bed, words, rows, keep_out ? keep_out + v0 : nullptr, &kept); });
  if (rc == PCOA_OK && n_kept_out) *n_kept_out = kept;
  return rc;
}

int pcoa_get_ld_stats(pcoa_ctx* c, pcoa_ld_stats* out_user, size_t out_size) {
  CHECK_CTX(c);
  if (!out_user || out_size < sizeof(int64_t)) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL or out_size too small");
  int rc0 = fp4_sync_point(c);
  if (rc0 != PCOA_OK) return rc0;
  drain_events(c, true);
  pcoa_ld_stats full;
  std::memset(&full, 0, sizeof(full));
  full.ld_variants = c->ldp_seen;
  full.ld_kept = c->ldp_kept;
  full.ld_monomorphic = c->ldp_mono;
  full.ld_pairs = c->ldp_pairs;
  full.ld_count_seconds = c->tsec[T_LD_COUNT];
  full.ld_band_seconds = c->tsec[T_LD_BAND];
  full.ld_resolve_seconds = c->tsec[T_LD_RESOLVE];
  full.ld_compact_seconds = c->tsec[T_LD_COMPACT];
  std::memcpy(out_user, &full, std::min(out_size, sizeof(full)));
  return PCOA_OK;
}

}  // extern "C"
