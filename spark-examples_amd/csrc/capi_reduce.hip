// capi_reduce.hip -- S leaves or enters an engine: finalize / export / import / read / load, the peer reductions of the
// engines of one process (pair-wise: pcoa_gram_reduce_from; all k at once: pcoa_gram_reduce_peers), and the RCCL all-reduce
// (RCCL is bound at run time).
#include <dlfcn.h>
#include <link.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is bound at run time (rccl_api below), not linked

#include <cstring>
#include <mutex>
#include <string>

#include "pcoa_ctx.h"

using namespace pcoa;

namespace {

// ---- RCCL, bound at run time --------------------------------------------------------------------------------------------
// libpcoa_hip.so does not link librccl.  A PyTorch process already carries an RCCL (torch/lib/librccl.so, no SONAME, so a
// DT_NEEDED librccl.so.1 would map /opt/rocm's copy BESIDE it: two collective runtimes on the same GPUs -- VERDICT r02
// Weak 10).  The first pcoa_comm_* call binds, in this order: an RCCL image the process has already mapped (torch's),
// else librccl.so.1 / librccl.so through the library's RUNPATH (/opt/rocm/lib) -- the Scala / JNI host's case.
struct RcclApi {
  void* handle = nullptr;
  std::string path, error;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*GetVersion)(int*) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;   // optional (telemetry only)
};

// the collective runtime itself, not a plugin of it: the BASENAME starts with "librccl.so" (librccl-net.so and friends carry
// "librccl" in their names too)
int find_mapped_rccl(struct dl_phdr_info* info, size_t, void* data) {
  if (!info->dlpi_name) return 0;
  const char* base = std::strrchr(info->dlpi_name, '/');
  base = base ? base + 1 : info->dlpi_name;
  if (std::strncmp(base, "librccl.so", 10) == 0) {
    *static_cast<std::string*>(data) = info->dlpi_name;
    return 1;
  }
  return 0;
}

const RcclApi& rccl_api() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    std::string mapped;
    dl_iterate_phdr(find_mapped_rccl, &mapped);
    // candidates in order: the image already mapped in this process, then the RUNPATH's; a candidate whose symbols do not
    // bind is dropped and the next one tried
    std::vector<std::pair<std::string, int>> cands;
    if (!mapped.empty()) cands.push_back({mapped, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD});
    cands.push_back({"librccl.so.1", RTLD_NOW | RTLD_GLOBAL});
    cands.push_back({"librccl.so", RTLD_NOW | RTLD_GLOBAL});
    std::string errors;
    for (const auto& cand : cands) {
      void* h = dlopen(cand.first.c_str(), cand.second);
      if (!h) {
        const char* why = dlerror();
        errors += " [" + cand.first + ": " + (why ? why : "not loaded") + "]";
        continue;
      }
      RcclApi t;
      t.handle = h;
      bool ok = true;
      std::string missing;
      auto bind = [&](auto& fn, const char* sym) {
        fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, sym));
        if (!fn) {
          ok = false;
          missing = sym;
        }
      };
      bind(t.GetUniqueId, "ncclGetUniqueId");
      bind(t.CommInitRank, "ncclCommInitRank");
      bind(t.CommDestroy, "ncclCommDestroy");
      bind(t.AllReduce, "ncclAllReduce");
      bind(t.GetErrorString, "ncclGetErrorString");
      bind(t.GetVersion, "ncclGetVersion");
      if (!ok) {
        errors += " [" + cand.first + ": symbol missing: " + missing + "]";
        continue;
      }
      t.CommCount = reinterpret_cast<decltype(t.CommCount)>(dlsym(h, "ncclCommCount"));
      api = t;
      Dl_info di;
      if (dladdr(reinterpret_cast<void*>(api.AllReduce), &di) && di.dli_fname) api.path = di.dli_fname;
      else api.path = cand.first;
      return;
    }
    api.handle = nullptr;
    api.error = "RCCL not found:" + errors;
  });
  return api;
}

}  // namespace

extern "C" {

int pcoa_gram_finalize(pcoa_ctx* c) {
  CHECK_CTX(c);
  int rc = finalize_impl(c);
  if (rc != PCOA_OK) return rc;
  return check_device_flags(c);
}

int pcoa_gram_export_device_i64(pcoa_ctx* c, int64_t* dst_dev) {
  CHECK_CTX(c);
  NOT_ON_OPERATOR(c, "pcoa_gram_export_device_i64");
  if (!dst_dev) return fail(c, PCOA_ERR_INVALID_ARG, "dst_dev is NULL");
  int rc = finalize_impl(c);
  if (rc != PCOA_OK) return rc;
  if ((rc = check_device_flags(c)) != PCOA_OK) return rc;  // never hand out an S that an input check has invalidated
  HIP_TRY(c, launch_export_i64(c->s32, c->s64, dst_dev, (int64_t)s_count(c), c->stream));
  return PCOA_OK;
}

// dst.S += src.S for two engines of ONE process (r04): the reduction step of a host that runs one ctx per GPU from its own
// threads (host/variants_pca_driver --gpus k), without a collective runtime.  src's total leaves as int64 (export), crosses to
// dst's device by hipMemcpyPeerAsync (xGMI between the GPUs of a node; a plain read when both ctxs sit on one device) and is
// added into dst's int64 matrix.  Integer sums: the result does not depend on the order in which partials are reduced.
int pcoa_gram_reduce_from(pcoa_ctx* dst, pcoa_ctx* src) {
  CHECK_CTX(dst);
  if (!src) return fail(dst, PCOA_ERR_INVALID_ARG, "src ctx is NULL");
  if (src == dst) return fail(dst, PCOA_ERR_INVALID_ARG, "src and dst are the same ctx");
  NOT_ON_OPERATOR(dst, "pcoa_gram_reduce_from (dst)");
  if (src->is_operator) return fail(dst, PCOA_ERR_STATE, "pcoa_gram_reduce_from: src is an operator ctx (pcoa_create_operator), which holds no S");
  if (src->n != dst->n || src->s_cols != dst->s_cols || src->strip_col0 != dst->strip_col0 || src->is_strip != dst->is_strip)
    return fail(dst, PCOA_ERR_INVALID_ARG, "reduce_from: the two engines hold different matrices (n / strip)");
  const size_t nn = s_count(dst);
  // src: everything contracted, mirrored, checked, exported as int64 on its own device
  {
    pcoa_ctx* c = src;
    CHECK_CTX(c);
    int rc = finalize_impl(c);
    if (rc == PCOA_OK) rc = check_device_flags(c);   // never reduce an S that an input check has invalidated
    if (rc != PCOA_OK) {
      dst->last_error = "reduce_from: src: " + src->last_error;
      return rc;
    }
  }
  {
    pcoa_ctx* c = dst;
    CHECK_CTX(c);
    int rc = finalize_impl(c);
    if (rc != PCOA_OK) return rc;
    if ((rc = check_device_flags(c)) != PCOA_OK) return rc;
  }
  // r06, the int32 path: neither engine has an int64 part and no sum can leave int32 (variants_in_s32 bounds every entry of a
  // partial; the same test the native all-reduce applies) -> the finalized int32 matrices are added in place.  4 N^2 bytes cross
  // instead of 8, nothing is widened (r05: 80 GB of exchange buffer on src + 80 + 80 on dst at N = 100,000), and dst keeps the
  // upper-triangle forms of computePca.  Both matrices are mirrored (finalize), so the sum is.
  if (!dst->s64 && !src->s64 && dst->variants_in_s32 + src->variants_in_s32 < (((int64_t)1 << 31) - 1) &&
      !debug_knobs().no_narrow) {
    pcoa_ctx* c = dst;
    const int32_t* from = src->s32;
    if (src->device != c->device) {
      int rc = ensure_xfer(c, sizeof(int32_t) * nn);
      if (rc != PCOA_OK) return rc;
      HIP_TRY(c, hipMemcpyPeerAsync(c->xfer, c->device, src->s32, src->device, sizeof(int32_t) * nn, c->stream));
      from = reinterpret_cast<const int32_t*>(c->xfer);
    }
    {
      ScopedTimer t(c, T_FINALIZE);
      HIP_TRY(c, launch_add_i32(c->s32, from, (int64_t)nn, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->variants_in_s32 += src->variants_in_s32;
    c->reduce_i32_calls += 1;
    c->strip_centering_set = false;
    return PCOA_OK;
  }
  {
    pcoa_ctx* c = src;
    CHECK_CTX(c);
    int rc = ensure_xfer(c, sizeof(int64_t) * nn);
    if (rc == PCOA_OK) rc = pcoa_gram_export_device_i64(c, c->xfer);
    if (rc != PCOA_OK) {
      dst->last_error = "reduce_from: src: " + src->last_error;
      return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  pcoa_ctx* c = dst;
  CHECK_CTX(c);
  int rc = PCOA_OK;
  {
    ScopedTimer t(c, T_FINALIZE);
    if ((rc = fold_now(c)) != PCOA_OK) return rc;  // dst's total in its int64 matrix (symmetric), S32 = 0
  }
  const int64_t* from = src->xfer;
  if (src->device != c->device) {
    if ((rc = ensure_xfer(c, sizeof(int64_t) * nn)) != PCOA_OK) return rc;
    HIP_TRY(c, hipMemcpyPeerAsync(c->xfer, c->device, src->xfer, src->device, sizeof(int64_t) * nn, c->stream));
    from = c->xfer;
  }
  HIP_TRY(c, launch_add_i64(c->s64, from, (int64_t)nn, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->strip_centering_set = false;
  return narrow_s64(c);   // the total may fit int32 although the books could not promise it
}

// S of every engine := the sum over the k engines (root_only: of ctxs[0] alone, the others reset), as a reduce-scatter and
// an all-gather over the engines' own matrices.  Phase 1: owner g sums chunk g (reduce_chunk) of all k matrices into its own,
// on its stream.  Phase 2: every receiver copies chunk h from owner h behind owner h's event.  Every link carries 1 / k of the
// matrix at a time, nothing is staged (xfer is not touched) and every engine takes part.
int pcoa_gram_reduce_peers(pcoa_ctx* const* ctxs, int32_t k, int32_t root_only) {
  const char* const me = "pcoa_gram_reduce_peers";
  if (!ctxs) return fail(nullptr, PCOA_ERR_INVALID_ARG, std::string(me) + ": ctxs is NULL");
  if (k < 1 || k > PCOA_REDUCE_MAX_ENGINES)
    return fail(nullptr, PCOA_ERR_INVALID_ARG, std::string(me) + ": k must be in [1, " + std::to_string(PCOA_REDUCE_MAX_ENGINES) + "]");
  pcoa_ctx* const c0 = ctxs[0];   // where errors are reported (NULL: the thread's create error, as pcoa_create_subset does)
  // ---- validation: nothing below touches a device until all of it has passed
  for (int g = 0; g < k; ++g) {
    if (!ctxs[g]) return fail(c0, PCOA_ERR_INVALID_ARG, std::string(me) + ": ctxs[" + std::to_string(g) + "] is NULL");
    for (int h = 0; h < g; ++h)
      if (ctxs[h] == ctxs[g])
        return fail(c0, PCOA_ERR_INVALID_ARG, std::string(me) + ": ctxs[" + std::to_string(g) + "] is the same ctx as ctxs[" + std::to_string(h) + "]");
  }
  for (int g = 0; g < k; ++g) {
    if (ctxs[g]->is_strip)
      return fail(c0, PCOA_ERR_STATE, std::string(me) + ": ctxs[" + std::to_string(g) + "] is a strip owner (pcoa_create_strip): the "
                                      "owners' strips tile S and are never summed");
    if (ctxs[g]->is_operator)
      return fail(c0, PCOA_ERR_STATE, std::string(me) + ": ctxs[" + std::to_string(g) + "] is an operator ctx (pcoa_create_operator), "
                                      "which holds no S");
  }
  for (int g = 1; g < k; ++g)
    if (ctxs[g]->n != c0->n)
      return fail(c0, PCOA_ERR_INVALID_ARG, std::string(me) + ": ctxs[" + std::to_string(g) + "] holds " + std::to_string(ctxs[g]->n) +
                                            " samples, ctxs[0] " + std::to_string(c0->n));
  // engines on different devices: kernels of each must be able to read the other's memory.  Every pair is asked first, then
  // enabled; a pair that cannot be made addressable is the caller's to reduce pair-wise (no staged fallback in here)
  for (int pass = 0; pass < 2; ++pass)
    for (int g = 0; g < k; ++g)
      for (int h = 0; h < k; ++h) {
        const int dg = ctxs[g]->device, dh = ctxs[h]->device;
        if (dg == dh) continue;
        hipError_t e = hipSuccess;
        int can = 0;
        if (pass == 0) {
          e = hipDeviceCanAccessPeer(&can, dg, dh);
        } else {
          can = 1;
          if ((e = hipSetDevice(dg)) == hipSuccess) e = hipDeviceEnablePeerAccess(dh, 0);
          if (e == hipErrorPeerAccessAlreadyEnabled) e = hipSuccess;
        }
        (void)hipGetLastError();
        if (e != hipSuccess || !can)
          return fail(c0, PCOA_ERR_STATE, std::string(me) + ": device " + std::to_string(dg) + " cannot address the memory of device " +
                                          std::to_string(dh) + " (no peer access): reduce these engines pair-wise with "
                                          "pcoa_gram_reduce_from, which stages through a copy");
      }
  // ---- preparation: every engine finalized and its input checks read (synchronises it) before any kernel of the reduction
  for (int g = 0; g < k; ++g) {
    pcoa_ctx* c = ctxs[g];
    CHECK_CTX(c);
    int rc = finalize_impl(c);
    if (rc == PCOA_OK) rc = check_device_flags(c);   // never reduce an S that an input check has invalidated
    if (rc != PCOA_OK) {
      if (g > 0) c0->last_error = std::string(me) + ": ctxs[" + std::to_string(g) + "]: " + c->last_error;
      return rc;
    }
  }
  if (k == 1) return PCOA_OK;
  const int32_t n = c0->n;
  bool any64 = false;
  int64_t sum_bound = 0, sum_variants = 0;
  for (int g = 0; g < k; ++g) {
    any64 = any64 || ctxs[g]->s64 != nullptr;
    sum_bound += ctxs[g]->variants_in_s32;
    sum_variants += ctxs[g]->gram_variants;
  }
  // the test pcoa_gram_reduce_from and the native all-reduce apply: no sum can leave int32
  const bool narrow = !any64 && sum_bound < (((int64_t)1 << 31) - 1) && !debug_knobs().no_narrow;
  ReduceSources src = {};
  src.k = k;
  for (int g = 0; g < k; ++g) {
    src.s32[g] = ctxs[g]->s32;
    src.s64[g] = ctxs[g]->s64;   // as the engine came in: an int64 matrix it is only given below holds nothing yet
  }
  if (!narrow) {   // int64 branch: every engine gets an int64 matrix for the totals; a failure leaves all of them as they were
    bool fresh[PCOA_REDUCE_MAX_ENGINES] = {false};
    for (int g = 0; g < k; ++g) {
      pcoa_ctx* c = ctxs[g];
      if (c->s64) continue;
      int rc = PCOA_OK;
      if (hipSetDevice(c->device) != hipSuccess || (rc = take_s64(c)) != PCOA_OK) {
        if (rc == PCOA_OK) rc = fail(c, PCOA_ERR_HIP, "hipSetDevice");
        if (g > 0) c0->last_error = std::string(me) + ": ctxs[" + std::to_string(g) + "]: " + c->last_error;
        for (int h = 0; h < g; ++h)
          if (fresh[h]) retire_s64(ctxs[h]);
        return rc;
      }
      fresh[g] = true;
    }
  }
  // guard-page mappings name the devices that may touch them (plain allocations are covered by the peer access above)
  for (int g = 0; g < k; ++g)
    for (int h = 0; h < k; ++h) {
      pcoa_ctx* c = ctxs[g];
      if (c->device == ctxs[h]->device) continue;
      HIP_TRY(c0, dev_grant_peer(c->s32, c->device, ctxs[h]->device));
      HIP_TRY(c0, dev_grant_peer(c->s64, c->device, ctxs[h]->device));
    }
  // ---- phase 1: owner g sums chunk g of every matrix into its own, on its stream.  From here on a failure leaves every S
  // undefined (pcoa.h): the error comes back on ctxs[0] and the engines are the caller's to reset.
  const size_t esize = narrow ? sizeof(int32_t) : sizeof(int64_t);
  int64_t first[PCOA_REDUCE_MAX_ENGINES], count[PCOA_REDUCE_MAX_ENGINES];
  hipEvent_t done[PCOA_REDUCE_MAX_ENGINES] = {nullptr};
  for (int g = 0; g < k; ++g) reduce_chunk(g, k, n, &first[g], &count[g]);
  for (int g = 0; g < k; ++g) {
    pcoa_ctx* c = ctxs[g];
    HIP_TRY(c0, hipSetDevice(c->device));
    if (!(done[g] = get_event(c))) return fail(c0, PCOA_ERR_HIP, std::string(me) + ": hipEventCreate failed");
    {
      ScopedTimer t(c, T_REDUCE_PEERS);
      HIP_TRY(c0, narrow ? launch_reduce_chunk_i32(src, c->s32, first[g], count[g], c->stream)
                         : launch_reduce_chunk_i64(src, any64, c->s64, first[g], count[g], c->stream));
    }
    HIP_TRY(c0, hipEventRecord(done[g], c->stream));
    for (int h = 0; h < k; ++h) {   // what the kernel read from OTHER engines
      if (h == g) continue;
      c->reduce_peers_bytes_in += (int64_t)sizeof(int32_t) * count[g];
      if (!narrow && src.s64[h]) c->reduce_peers_bytes_in += (int64_t)sizeof(int64_t) * count[g];
    }
  }
  // ---- phase 2: the all-gather (root_only: the gather to engine 0).  Receiver g copies chunk h from owner h's matrix into its
  // own behind owner h's event; owner h's kernel was the only reader of g's chunk h
  for (int g = 0; g < (root_only ? 1 : k); ++g) {
    pcoa_ctx* c = ctxs[g];
    HIP_TRY(c0, hipSetDevice(c->device));
    ScopedTimer t(c, T_REDUCE_PEERS);
    for (int h = 0; h < k; ++h) {
      if (h == g || count[h] == 0) continue;
      pcoa_ctx* o = ctxs[h];
      HIP_TRY(c0, hipStreamWaitEvent(c->stream, done[h], 0));
      const size_t off = (size_t)first[h] * esize, bytes = (size_t)count[h] * esize;
      char* to = (narrow ? reinterpret_cast<char*>(c->s32) : reinterpret_cast<char*>(c->s64)) + off;
      const char* from = (narrow ? reinterpret_cast<const char*>(o->s32) : reinterpret_cast<const char*>(o->s64)) + off;
      if (o->device == c->device) HIP_TRY(c0, hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToDevice, c->stream));
      else HIP_TRY(c0, hipMemcpyPeerAsync(to, c->device, from, o->device, bytes, c->stream));
      c->reduce_peers_bytes_in += (int64_t)bytes;
    }
  }
  for (int g = 0; g < k; ++g) {
    HIP_TRY(c0, hipSetDevice(ctxs[g]->device));
    HIP_TRY(c0, hipStreamSynchronize(ctxs[g]->stream));
  }
  for (int g = 0; g < k; ++g) ctxs[g]->pool.push_back(done[g]);
  // ---- books.  An engine that holds the total: as after a reduction into it; with root_only every other one: as after pcoa_reset
  for (int g = 0; g < k; ++g) {
    pcoa_ctx* c = ctxs[g];
    HIP_TRY(c0, hipSetDevice(c->device));
    c->reduce_peers_calls += 1;
    c->dirty = false;
    c->strip_centering_set = false;
    if (root_only && g > 0) {
      HIP_TRY(c0, hipMemsetAsync(c->s32, 0, sizeof(int32_t) * s_count(c), c->stream));
      HIP_TRY(c0, hipStreamSynchronize(c->stream));
      retire_s64(c);   // S = 0 needs no int64 part
      c->variants_in_s32 = 0;
      c->gram_variants = 0;
      continue;
    }
    c->gram_variants = sum_variants;
    if (narrow) {
      c->variants_in_s32 = sum_bound;
      c->reduce_i32_calls += 1;
      continue;
    }
    // the hand-over every int64 import makes: the total is in s64, the int32 partial is zero, and a total that fits goes back
    HIP_TRY(c0, hipMemsetAsync(c->s32, 0, sizeof(int32_t) * s_count(c), c->stream));
    c->variants_in_s32 = 0;
    const int rc = narrow_s64(c);
    if (rc != PCOA_OK) {
      if (g > 0) c0->last_error = std::string(me) + ": ctxs[" + std::to_string(g) + "]: " + c->last_error;
      return rc;
    }
  }
  return PCOA_OK;
}

// test hook: the partition pcoa_gram_reduce_peers cuts S by (reduce_chunk, reduce_peers.hip); no GPU
int pcoa_debug_reduce_chunk(int32_t g, int32_t k, int32_t n_samples, int64_t* first_out, int64_t* count_out) {
  if (!first_out || !count_out || k < 1 || k > PCOA_REDUCE_MAX_ENGINES || g < 0 || g >= k || n_samples < 1)
    return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_debug_reduce_chunk: need 0 <= g < k <= PCOA_REDUCE_MAX_ENGINES, n_samples >= 1 and both outputs");
  reduce_chunk(g, k, n_samples, first_out, count_out);
  return PCOA_OK;
}

int pcoa_gram_import_device_i64(pcoa_ctx* c, const int64_t* src_dev) {
  CHECK_CTX(c);
  NOT_ON_OPERATOR(c, "pcoa_gram_import_device_i64");
  if (!src_dev) return fail(c, PCOA_ERR_INVALID_ARG, "src_dev is NULL");
  const size_t nn = s_count(c);
  int rc = fp4_discard(c);  // S is replaced: what was buffered or in flight for the old S goes with it
  if (rc != PCOA_OK) return rc;
  if ((rc = take_s64(c)) != PCOA_OK) return rc;   // the matrix narrow_s64 retired last time, else a fresh one
  HIP_TRY(c, hipMemcpyAsync(c->s64, src_dev, sizeof(int64_t) * nn, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->s32, 0, sizeof(int32_t) * nn, c->stream));
  c->variants_in_s32 = 0;
  c->dirty = false;
  c->strip_centering_set = false;  // (also reached from pcoa_gram_load_i64: checkpoint resume replaces S)
  return narrow_s64(c);   // counts that fit int32 go back into the int32 matrix (synchronises)
}

int pcoa_gram_read_i64(pcoa_ctx* c, int64_t* out_nxn) {
  CHECK_CTX(c);
  NOT_ON_OPERATOR(c, "pcoa_gram_read_i64");
  if (!out_nxn) return fail(c, PCOA_ERR_INVALID_ARG, "out is NULL");
  const size_t nn = s_count(c);
  int rc = ensure_xfer(c, sizeof(int64_t) * nn);
  if (rc != PCOA_OK) return rc;
  if ((rc = pcoa_gram_export_device_i64(c, c->xfer)) != PCOA_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(out_nxn, c->xfer, sizeof(int64_t) * nn, hipMemcpyDeviceToHost, c->stream));
  return check_device_flags(c);
}

int pcoa_gram_read_block_i64(pcoa_ctx* c, int32_t row0, int32_t col0, int32_t rows, int32_t cols, int64_t* out) {
  CHECK_CTX(c);
  NOT_ON_OPERATOR(c, "pcoa_gram_read_block_i64");
  if (!out || rows < 0 || cols < 0 || row0 < 0 || col0 < 0 || (int64_t)row0 + rows > c->n || (int64_t)col0 + cols > c->s_cols)
    return fail(c, PCOA_ERR_INVALID_ARG, "block outside the matrix the ctx holds (N x N, or N x cols of a strip) or out is NULL");
  if (rows == 0 || cols == 0) return PCOA_OK;
  int rc = finalize_impl(c);
  if (rc != PCOA_OK) return rc;
  // int32 partial and (if folded) int64 total are copied as strided blocks and summed on the host:
  // no N x N exchange buffer, so this also works when N^2 * 8 B would not fit (N = 100k: 80 GB)
  std::vector<int32_t> a((size_t)rows * (size_t)cols);
  HIP_TRY(c, hipMemcpy2DAsync(a.data(), sizeof(int32_t) * (size_t)cols, c->s32 + (size_t)row0 * c->s_cols + col0,
                              sizeof(int32_t) * (size_t)c->s_cols, sizeof(int32_t) * (size_t)cols, (size_t)rows,
                              hipMemcpyDeviceToHost, c->stream));
  std::vector<int64_t> b;
  if (c->s64) {
    b.resize(a.size());
    HIP_TRY(c, hipMemcpy2DAsync(b.data(), sizeof(int64_t) * (size_t)cols, c->s64 + (size_t)row0 * c->s_cols + col0,
                                sizeof(int64_t) * (size_t)c->s_cols, sizeof(int64_t) * (size_t)cols, (size_t)rows,
                                hipMemcpyDeviceToHost, c->stream));
  }
  rc = check_device_flags(c);  // synchronises the stream
  if (rc != PCOA_OK) return rc;
  for (size_t i = 0; i < a.size(); ++i) out[i] = (int64_t)a[i] + (c->s64 ? b[i] : 0);
  return PCOA_OK;
}

int pcoa_gram_load_i64(pcoa_ctx* c, const int64_t* in_nxn) {
  CHECK_CTX(c);
  NOT_ON_OPERATOR(c, "pcoa_gram_load_i64");
  if (!in_nxn) return fail(c, PCOA_ERR_INVALID_ARG, "in is NULL");
  const size_t nn = s_count(c);
  int rc = ensure_xfer(c, sizeof(int64_t) * nn);
  if (rc != PCOA_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->xfer, in_nxn, sizeof(int64_t) * nn, hipMemcpyHostToDevice, c->stream));
  rc = pcoa_gram_import_device_i64(c, c->xfer);
  if (rc != PCOA_OK) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PCOA_OK;
}

// RCCL is bound at the first of these calls (rccl_api above); a process that never calls them needs no RCCL at all.
#define RCCL_OR_FAIL(ctx)                                                  \
  const RcclApi& R = rccl_api();                                           \
  if (!R.handle) return fail((ctx), PCOA_ERR_RCCL, R.error)

int pcoa_comm_runtime(char* path_out, int32_t path_cap, int32_t* version_out) {
  RCCL_OR_FAIL(nullptr);
  if (path_out && path_cap > 0) {
    std::strncpy(path_out, R.path.c_str(), (size_t)path_cap - 1);
    path_out[path_cap - 1] = 0;
  }
  if (version_out) {
    int v = 0;
    if (R.GetVersion(&v) != ncclSuccess) v = -1;
    *version_out = v;
  }
  return PCOA_OK;
}

int pcoa_comm_unique_id(uint8_t out_id[128]) {
  if (!out_id) return fail(nullptr, PCOA_ERR_INVALID_ARG, "out_id is NULL");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  RCCL_OR_FAIL(nullptr);
  ncclUniqueId id;
  ncclResult_t r = R.GetUniqueId(&id);
  if (r != ncclSuccess) return fail(nullptr, PCOA_ERR_RCCL, std::string("ncclGetUniqueId: ") + R.GetErrorString(r));
  std::memcpy(out_id, &id, 128);
  return PCOA_OK;
}

int pcoa_comm_init(pcoa_ctx* c, const uint8_t id[128], int32_t rank, int32_t n_ranks, void** comm_out) {
  CHECK_CTX(c);
  if (!id || !comm_out || n_ranks <= 0 || rank < 0 || rank >= n_ranks)
    return fail(c, PCOA_ERR_INVALID_ARG, "comm_init: bad argument");
  RCCL_OR_FAIL(c);
  ncclUniqueId uid;
  std::memcpy(&uid, id, 128);
  ncclComm_t comm = nullptr;
  ncclResult_t r = R.CommInitRank(&comm, n_ranks, uid, rank);
  if (r != ncclSuccess) return fail(c, PCOA_ERR_RCCL, std::string("ncclCommInitRank: ") + R.GetErrorString(r));
  *comm_out = (void*)comm;
  return PCOA_OK;
}

int pcoa_comm_destroy(void* nccl_comm) {
  if (!nccl_comm) return PCOA_OK;
  RCCL_OR_FAIL(nullptr);
  ncclResult_t r = R.CommDestroy((ncclComm_t)nccl_comm);
  return r == ncclSuccess ? PCOA_OK : fail(nullptr, PCOA_ERR_RCCL, std::string("ncclCommDestroy: ") + R.GetErrorString(r));
}

int pcoa_comm_count(void* nccl_comm, int32_t* count_out) {
  if (!nccl_comm || !count_out) return fail(nullptr, PCOA_ERR_INVALID_ARG, "comm_count: NULL argument");
  RCCL_OR_FAIL(nullptr);
  if (!R.CommCount) return fail(nullptr, PCOA_ERR_RCCL, "ncclCommCount is not exported by the bound RCCL");
  int cnt = 0;
  ncclResult_t r = R.CommCount((ncclComm_t)nccl_comm, &cnt);
  if (r != ncclSuccess) return fail(nullptr, PCOA_ERR_RCCL, std::string("ncclCommCount: ") + R.GetErrorString(r));
  *count_out = cnt;
  return PCOA_OK;
}

int pcoa_gram_allreduce_rccl(pcoa_ctx* c, void* nccl_comm) {
  CHECK_CTX(c);
  if (!nccl_comm) return fail(c, PCOA_ERR_INVALID_ARG, "nccl_comm is NULL");
  NOT_ON_OPERATOR(c, "pcoa_gram_allreduce_rccl");
  if (c->is_strip)
    return fail(c, PCOA_ERR_STATE, "a strip owner holds N x cols of S: the owners' strips tile S and are never summed "
                                   "(the exchange step of that layout is the all-gather of pcoa_strip_matvec's results)");
  RCCL_OR_FAIL(c);
  ncclComm_t comm = (ncclComm_t)nccl_comm;
  const size_t nn = s_count(c);
  int rc = finalize_impl(c);
  if (rc != PCOA_OK) return rc;
  c->allreduce_calls += 1;
  if (R.CommCount) {
    int cnt = 0;
    if (R.CommCount(comm, &cnt) == ncclSuccess) c->comm_ranks = cnt;
  }
  ScopedTimer t_all(c, T_ALLREDUCE);   // the agreement words and the S all-reduce, as the ctx stream sees them
  // All ranks must take the same branch: agree on {total variants held in int32 partials, anyone folded}.
  if (!c->coll) HIP_TRY(c, dev_alloc((void**)&c->coll, 64, c->device));
  int64_t* all = c->hw->coll;
  all[0] = c->variants_in_s32;
  all[1] = c->s64 ? 1 : 0;
  HIP_TRY(c, hipMemcpyAsync(c->coll, all, 2 * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  ncclResult_t r = R.AllReduce(c->coll, c->coll, 2, ncclInt64, ncclSum, comm, c->stream);
  if (r != ncclSuccess) return fail(c, PCOA_ERR_RCCL, std::string("ncclAllReduce(meta): ") + R.GetErrorString(r));
  HIP_TRY(c, hipMemcpyAsync(all, c->coll, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (all[1] == 0 && all[0] < (((int64_t)1 << 31) - 1)) {
    // fast path: every count fits int32 even after the sum -> reduce the 4*N^2-byte partial in place
    r = R.AllReduce(c->s32, c->s32, nn, ncclInt32, ncclSum, comm, c->stream);
    if (r != ncclSuccess) return fail(c, PCOA_ERR_RCCL, std::string("ncclAllReduce(int32): ") + R.GetErrorString(r));
    c->variants_in_s32 = all[0];
    c->allreduce_int32 = 1;
    return PCOA_OK;
  }
  c->allreduce_int32 = 0;
  if ((rc = ensure_xfer(c, sizeof(int64_t) * nn)) != PCOA_OK) return rc;
  rc = pcoa_gram_export_device_i64(c, c->xfer);
  if (rc != PCOA_OK) return rc;
  r = R.AllReduce(c->xfer, c->xfer, nn, ncclInt64, ncclSum, comm, c->stream);
  if (r != ncclSuccess) return fail(c, PCOA_ERR_RCCL, std::string("ncclAllReduce: ") + R.GetErrorString(r));
  return pcoa_gram_import_device_i64(c, c->xfer);
}

}  // extern "C"
