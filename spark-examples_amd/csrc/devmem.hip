// devmem.hip -- device memory of the library: the guard-page allocator behind dev_alloc / dev_free, the one way a buffer is
// regrown, the environment knobs, and the allocation hooks of the C ABI.
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>

#include "pcoa_ctx.h"

using namespace pcoa;

// ---- device memory ----------------------------------------------------------------------------------------------------
// Every device allocation of the library goes through dev_alloc / dev_free.  Normally that is hipMalloc / hipFree.  With
// PCOA_DEBUG_GUARD=1 (2) every buffer gets a virtual range of its own (HIP virtual-memory API) with the buffer's END
// (START) flush against a page that is never mapped, so that a kernel reading or writing even one element beyond (in front
// of) a workspace faults on the spot -- with AMD_SERIALIZE_KERNEL=3 the runtime names the kernel -- instead of silently
// reading a neighbouring allocation (the unexplained abort of the GPU suite).  Slack: the end is
// aligned down to 16 bytes (the kernels' vector accesses need it), so an overrun by less than 16 bytes of a buffer whose
// size is not a multiple of 16 can pass.
namespace {

struct GuardRec {
  void* va;
  size_t va_size;
  void* map;
  size_t map_size;
  hipMemGenericAllocationHandle_t handle;
};
std::mutex g_guard_mu;
std::unordered_map<void*, GuardRec> g_guard_recs;

hipError_t guard_alloc(void** out, size_t bytes, int device, int mode) {
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = device;
  size_t gran = 0;
  hipError_t e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum);
  if (e != hipSuccess) return e;
  if (gran == 0) return hipErrorNotSupported;
  const size_t need = std::max<size_t>(bytes, 16);
  const size_t map_size = (need + gran - 1) / gran * gran;
  GuardRec r = {};
  r.va_size = map_size + 2 * gran;
  r.map_size = map_size;
  if ((e = hipMemAddressReserve(&r.va, r.va_size, 0, nullptr, 0)) != hipSuccess) return e;
  if ((e = hipMemCreate(&r.handle, map_size, &prop, 0)) != hipSuccess) {
    (void)hipMemAddressFree(r.va, r.va_size);
    return e;
  }
  r.map = static_cast<char*>(r.va) + gran;
  if ((e = hipMemMap(r.map, map_size, 0, r.handle, 0)) != hipSuccess) {
    (void)hipMemRelease(r.handle);
    (void)hipMemAddressFree(r.va, r.va_size);
    return e;
  }
  hipMemAccessDesc acc = {};
  acc.location = prop.location;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  if ((e = hipMemSetAccess(r.map, map_size, &acc, 1)) != hipSuccess) {
    (void)hipMemUnmap(r.map, map_size);
    (void)hipMemRelease(r.handle);
    (void)hipMemAddressFree(r.va, r.va_size);
    return e;
  }
  char* user = static_cast<char*>(r.map);
  if (mode == 1) user += (map_size - need) / 16 * 16;  // the buffer ends (up to 15 bytes) in front of the unmapped page
  *out = user;
  std::lock_guard<std::mutex> lock(g_guard_mu);
  g_guard_recs[user] = r;
  return hipSuccess;
}

bool guard_free(void* p) {
  GuardRec r;
  {
    std::lock_guard<std::mutex> lock(g_guard_mu);
    auto it = g_guard_recs.find(p);
    if (it == g_guard_recs.end()) return false;
    r = it->second;
    g_guard_recs.erase(it);
  }
  (void)hipMemUnmap(r.map, r.map_size);
  (void)hipMemRelease(r.handle);
  // The virtual range is deliberately NOT given back (hipMemAddressFree): a later reservation could get the same
  // addresses with other physical pages behind them, and kernels were then seen to read through stale translations of
  // the old mapping (wrong counts that changed from run to run, profiles/r03n_guard_va_reuse.txt).  A debug process can
  // afford the address space, and a freed buffer's range stays unmapped for good: a use after free faults as well.
  return true;
}

}  // namespace

namespace pcoa {

hipError_t dev_alloc(void** out, size_t bytes, int device) {
  const int mode = debug_knobs().guard;
  if (mode == 1 || mode == 2) return guard_alloc(out, bytes, device, mode);
  return hipMalloc(out, bytes);
}

void dev_free(void* p) {
  if (!p) return;
  if (debug_knobs().guard != 0 && guard_free(p)) return;
  (void)hipFree(p);
}

hipError_t dev_grant_peer(void* p, int owner_device, int peer_device) {
  if (!p || owner_device == peer_device || debug_knobs().guard == 0) return hipSuccess;
  GuardRec r;
  {
    std::lock_guard<std::mutex> lock(g_guard_mu);
    auto it = g_guard_recs.find(p);
    if (it == g_guard_recs.end()) return hipSuccess;   // a plain allocation
    r = it->second;
  }
  hipMemAccessDesc acc = {};
  acc.location.type = hipMemLocationTypeDevice;
  acc.location.id = peer_device;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  return hipMemSetAccess(r.map, r.map_size, &acc, 1);
}

// The one way a device buffer of the library is regrown: *buf is freed and replaced by `bytes` fresh bytes; its old contents
// are not kept, and *buf is null if the allocation fails.  sync_ctx_stream: kernels queued on the ctx stream may still read
// the old buffer (a staging slot's owner has waited for the slot's last reader instead).  Capacities and their growth
// policy are the caller's.
int regrow(pcoa_ctx* c, void** buf, size_t bytes, bool sync_ctx_stream) {
  if (sync_ctx_stream) HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (*buf) dev_free(*buf);
  *buf = nullptr;
  HIP_TRY(c, dev_alloc(buf, bytes, c->device));
  return PCOA_OK;
}

const DebugKnobs& debug_knobs() {
  static const DebugKnobs knobs = [] {
    DebugKnobs k;
    auto num = [](const char* name) -> long long {
      const char* v = std::getenv(name);
      return (v && *v) ? std::atoll(v) : 0;
    };
    if (const char* kk = std::getenv("PCOA_GRAM_KERNEL")) {
      if (!std::strcmp(kk, "f32")) k.gram_kernel = 1;
      if (!std::strcmp(kk, "i8")) k.gram_kernel = 2;
      if (!std::strcmp(kk, "fp4")) k.gram_kernel = 3;
      if (!std::strcmp(kk, "auto")) k.gram_kernel = 0;
    }
    k.pack_chunk = num("PCOA_DEBUG_PACK_CHUNK");
    k.max_launch = num("PCOA_DEBUG_MAX_LAUNCH");
    k.fold_threshold = num("PCOA_DEBUG_FOLD_THRESHOLD");
    if (const char* v = std::getenv("PCOA_PIPELINE")) k.pipeline = std::atoi(v) != 0;
    if (const char* v = std::getenv("PCOA_BITS_PIPELINE")) k.bits_pipeline = std::atoi(v);
    if (const char* v = std::getenv("PCOA_KBITS_W4_DIAG")) k.kbits_w4_diag = std::atoi(v);
    if (const char* v = std::getenv("PCOA_GRAM_LOCKSTEP")) k.lockstep = std::atoi(v) != 0;
    k.explicit_center = std::getenv("PCOA_EXPLICIT_CENTER") != nullptr;
    k.guard = (int)num("PCOA_DEBUG_GUARD");
    if (const char* v = std::getenv("PCOA_KBITS_MODE")) k.kbits_mode = std::atoi(v);
    if (const char* v = std::getenv("PCOA_KBITS_W4")) k.kbits_w4 = std::atoi(v);
    if (const char* v = std::getenv("PCOA_CSR_LEGACY")) k.csr_legacy = std::atoi(v) != 0;
    if (const char* v = std::getenv("PCOA_SYMV_SYM_MIN_N")) k.symv_sym_min_n = std::atoi(v);
    if (const char* v = std::getenv("PCOA_KBITS_CORESIDE")) k.kbits_coreside = std::atoi(v) != 0;
    k.operator_segment_rows = num("PCOA_OPERATOR_SEGMENT_ROWS");
    k.grm_segment_rows = num("PCOA_GRM_SEGMENT_ROWS");
    k.no_narrow = (int)num("PCOA_NO_NARROW");
    k.synth_tile = (int)num("PCOA_SYNTH_TILE");
    if (const char* v = std::getenv("PCOA_LANCZOS_BAND")) k.lanczos_band = std::atoi(v);
    k.lanczos_band_mmax = (int)num("PCOA_LANCZOS_BAND_MMAX");
    return k;
  }();
  return knobs;
}

}  // namespace pcoa

extern "C" {

// ---- test hooks: device memory from the library's own allocator ---------------------------------------------------------
// With PCOA_DEBUG_GUARD set these are guard-page allocations like every workspace of the library, which lets the GPU tests
// place the INPUT tiles of the accumulate calls against an unmapped page as well (a pre-pass reading one row or one word
// too many then faults instead of reading a neighbouring torch allocation).  Not part of the reference-facing boundary.
int pcoa_debug_alloc(int32_t device_ordinal, size_t bytes, void** out) {
  if (!out || bytes == 0) return fail(nullptr, PCOA_ERR_INVALID_ARG, "debug_alloc: out is NULL or bytes == 0");
  hipError_t e = hipSetDevice(device_ordinal);
  if (e == hipSuccess) e = dev_alloc(out, bytes, device_ordinal);
  if (e != hipSuccess) return hip_fail(nullptr, e, "pcoa_debug_alloc");
  return PCOA_OK;
}

int pcoa_debug_free(void* p) {
  dev_free(p);
  return PCOA_OK;
}

int pcoa_debug_guard_mode(void) { return debug_knobs().guard; }

// Page-locked host memory for a host's input blocks (the compiled host streams .bed blocks through two of them: a copy from
// pageable memory crosses the link at ~14 GB/s, from pinned memory at ~50).  Not tied to a ctx.
int pcoa_host_alloc_pinned(size_t bytes, void** out) {
  if (!out || bytes == 0) return PCOA_ERR_INVALID_ARG;
  *out = nullptr;
  return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? PCOA_OK : PCOA_ERR_HIP;
}
int pcoa_host_free_pinned(void* p) {
  if (!p) return PCOA_OK;
  return hipHostFree(p) == hipSuccess ? PCOA_OK : PCOA_ERR_HIP;
}

}  // extern "C"
