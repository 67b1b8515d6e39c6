// capi_subset.hip -- pcoa_create_subset: a new full engine whose S is S[I, I] of another.  The kept index set
// is validated on the host before anything touches a device; the new engine comes from pcoa_create's own path (without the
// zero fill of an S that is overwritten whole), so it is an ordinary engine in every respect; the gathers (subset.hip) run
// on ITS stream, behind src's finalize and input checks.
#include <string>

#include "pcoa_ctx.h"

using namespace pcoa;

extern "C" {

int pcoa_create_subset(pcoa_ctx** out, pcoa_ctx* src, const int32_t* keep, int32_t n_keep) {
  if (!out) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_create_subset: out is NULL");
  *out = nullptr;
  if (!src) return fail(nullptr, PCOA_ERR_INVALID_ARG, "pcoa_create_subset: src ctx is NULL");
  NOT_ON_OPERATOR(src, "pcoa_create_subset");
  if (src->is_strip)
    return fail(src, PCOA_ERR_STATE, "pcoa_create_subset: a strip owner holds N x cols of S, not the rows and columns of a sample "
                                     "subset; use a full engine (pcoa_create) for this call");
  if (!keep || n_keep < 1) return fail(src, PCOA_ERR_INVALID_ARG, "pcoa_create_subset: keep is NULL or n_keep < 1");
  for (int32_t a = 0; a < n_keep; ++a) {
    if (keep[a] < 0 || keep[a] >= src->n)
      return fail(src, PCOA_ERR_INVALID_ARG, "pcoa_create_subset: keep[" + std::to_string(a) + "] = " + std::to_string(keep[a]) +
                                             " is outside [0, " + std::to_string(src->n) + ")");
    if (a > 0 && keep[a] <= keep[a - 1])
      return fail(src, PCOA_ERR_INVALID_ARG, "pcoa_create_subset: keep must be strictly increasing (keep[" + std::to_string(a) +
                                             "] = " + std::to_string(keep[a]) + " follows " + std::to_string(keep[a - 1]) + ")");
  }
  CHECK_CTX(src);
  int rc = finalize_impl(src);
  if (rc == PCOA_OK) rc = check_device_flags(src);   // never subset an S that an input check has invalidated (synchronises src)
  if (rc != PCOA_OK) return rc;

  pcoa_ctx* sub = nullptr;
  rc = create_full_engine_unfilled(&sub, n_keep, src->device, src->flags);   // pcoa_create's path; the gather writes every entry of S
  if (rc != PCOA_OK) return fail(src, rc, std::string("pcoa_create_subset: the new engine: ") + pcoa_last_error(nullptr));
  // from here on a failure is reported on src and takes the half-built engine with it
  int32_t* keep_dev = nullptr;
  auto bail = [&](int code, std::string msg) {   // by value: the message usually lives in the engine destroyed below
    if (keep_dev) {
      (void)hipStreamSynchronize(sub->stream);
      dev_free(keep_dev);
    }
    pcoa_destroy(sub);
    (void)hipSetDevice(src->device);
    return fail(src, code, "pcoa_create_subset: " + msg);
  };
  auto hip_bail = [&](hipError_t e, const char* what) {
    const int code = hip_fail(sub, e, what);
    return bail(code, sub->last_error);
  };
  const size_t m = (size_t)n_keep;
  hipError_t e;
  if ((e = dev_alloc((void**)&keep_dev, sizeof(int32_t) * m, sub->device)) != hipSuccess) return hip_bail(e, "allocation of the kept indices");
  if (src->s64 && (e = dev_alloc((void**)&sub->s64, sizeof(int64_t) * m * m, sub->device)) != hipSuccess)
    return hip_bail(e, "allocation of the int64 part of S");
  if ((e = hipMemcpyAsync(keep_dev, keep, sizeof(int32_t) * m, hipMemcpyHostToDevice, sub->stream)) != hipSuccess)
    return hip_bail(e, "hipMemcpyAsync(keep)");
  {
    ScopedTimer t(sub, T_SUBSET);
    if ((e = launch_subset_gather_i32(src->s32, src->n, keep_dev, n_keep, sub->s32, sub->stream)) != hipSuccess)
      return hip_bail(e, "subset_gather_kernel<int32_t>");
    sub->subset_bytes += (int64_t)(2 * sizeof(int32_t) * m * m);
    if (src->s64) {
      if ((e = launch_subset_gather_i64(src->s64, src->n, keep_dev, n_keep, sub->s64, sub->stream)) != hipSuccess)
        return hip_bail(e, "subset_gather_kernel<int64_t>");
      sub->subset_bytes += (int64_t)(2 * sizeof(int64_t) * m * m);
    }
  }
  if ((e = hipStreamSynchronize(sub->stream)) != hipSuccess) return hip_bail(e, "hipStreamSynchronize");
  dev_free(keep_dev);
  keep_dev = nullptr;
  sub->variants_in_s32 = src->variants_in_s32;   // the bound of every int32 entry holds for a sub-matrix as it stands
  sub->gram_variants = src->gram_variants;
  sub->similarity = src->similarity;             // what computePca decomposes (pcoa_set_similarity) follows the cohort
  sub->dirty = false;                            // both triangles were gathered from a mirrored S
  if (sub->s64) {
    // the int64 hand-over every import makes: the total in the int64 matrix, the int32 partial zero, then back into the
    // int32 matrix if every kept entry fits (the entries that needed 64 bits may all belong to removed samples)
    if ((rc = fold_now(sub)) == PCOA_OK) rc = narrow_s64(sub);
    if (rc == PCOA_OK && (e = hipStreamSynchronize(sub->stream)) != hipSuccess) rc = hip_fail(sub, e, "hipStreamSynchronize");
    if (rc != PCOA_OK) return bail(rc, sub->last_error);
  }
  if (src->companion) {
    // a bound src: the result gets a companion of its own, Q[keep, keep] by the same gather, with the same V; the result owns it
    pcoa_ctx* subq = nullptr;
    rc = pcoa_create_subset(&subq, src->companion, keep, n_keep);
    if (rc != PCOA_OK) return bail(rc, "the call companion: " + src->companion->last_error);
    sub->companion = subq;
    sub->companion_v = src->companion_v;
    sub->companion_owned = true;
  }
  (void)hipSetDevice(src->device);
  *out = sub;
  return PCOA_OK;
}

}  // extern "C"
