"""PcoaEngine -- thin object wrapper over the C ABI (include/pcoa.h).

One engine = one pcoa_ctx = one GPU.  The method names follow the stages of the reference driver
(VariantsPca.scala:44-47): getSimilarityMatrix -> accumulate_* / finalize, computePca -> compute.
"""
import ctypes

import numpy as np

from . import _lib as L


class PcoaError(RuntimeError):
    def __init__(self, code, message):
        RuntimeError.__init__(self, "pcoa error %d: %s" % (code, message))
        self.code = code


class IndexRangeError(PcoaError, IndexError):
    """A callset index outside [0, N): the reference throws NoSuchElementException /
    IndexOutOfBounds here (VariantsPca.scala:59, :188)."""


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def pcrelate_hat(basis):
    """hat = (basis basis^T)^-1 basis for the covariates `basis` [n_cov, N] of a PC-Relate fit, by pcoa_pcrelate_hat: host
    arithmetic in the library (no engine, no device), so that every host holds the same bits; variants_pca.pcrelate_hat_rule is
    the numpy statement.  PcoaError (PCOA_ERR_INVALID_ARG) for n_cov outside [1, 9], N < n_cov, a non-finite entry or collinear
    covariates."""
    b = np.ascontiguousarray(basis, dtype=np.float64)
    if b.ndim != 2:
        raise ValueError("basis must be [n_cov, N], not %s" % (b.shape,))
    out = np.zeros(b.shape, dtype=np.float64)
    lib = L.load()
    rc = lib.pcoa_pcrelate_hat(int(b.shape[0]), int(b.shape[1]), _ptr(b) if b.size else None, _ptr(out) if out.size else None)
    if rc != 0:
        raise PcoaError(rc, (lib.pcoa_last_error(None) or b"").decode())
    return out


_BITS_ROWS = (np.uint32, "int32", "bits must be 2-D [variants][words]")
_BED_ROWS = (np.uint8, "uint8", "rows must be [variants][row_bytes]")


def _rows_arg(rows, np_dtype, torch_dtype, what, pinned=False):
    """The rows of a bitset / .bed boundary as (pointer, n_rows, row_stride, is_device, keepalive).  A torch CUDA tensor (dtype
    torch.<torch_dtype>, unit inner stride) is read in place: the engine runs on its own stream, so whatever torch queued to
    produce it is waited for.  pinned: a page-locked CPU tensor, taken as it lies (the queued form of the .bed boundaries).
    Anything else goes through numpy; `what` is the ValueError of an array that is not 2-D.  keepalive owns the memory."""
    if pinned or (hasattr(rows, "data_ptr") and getattr(rows, "is_cuda", False)):
        import torch  # plumbing only: memory handles
        assert rows.dtype == getattr(torch, torch_dtype) and rows.dim() == 2 and rows.stride(1) == 1
        if pinned:
            assert rows.is_pinned()
        else:
            torch.cuda.current_stream(rows.device).synchronize()
        is_device = not pinned          # a page-locked tensor is host memory
        return ctypes.c_void_p(rows.data_ptr()), int(rows.shape[0]), int(rows.stride(0)), is_device, rows
    a = np.ascontiguousarray(rows, dtype=np_dtype)
    if a.ndim != 2:
        raise ValueError(what)
    return _ptr(a), a.shape[0], a.shape[1], False, a


class PcoaEngine(object):
    def __init__(self, n_samples, device=0, flags=L.PCOA_FLAG_DEFAULT, gram_kernel=None, eig=None, strip=None,
                 pipeline=True, operand=None, operator=False, grm=False, grm_study=False):
        """gram_kernel: None/"auto" (MX-FP4 MFMA for binary tiles, int8 MFMA for multiplicities; both exact),
        "fp4", "i8" (force one of them) or "f32" (fp32-MFMA path).
        eig: None/"auto" (Lanczos with verified residual -- single vector, then the band iteration --, Householder fallback),
        "householder", "lanczos" (no dense fallback), "band" (Lanczos as the band iteration from the start, PCOA_FLAG_EIG_BAND).
        strip: None, or (col0, cols): a strip owner holding S[:, col0:col0+cols] (pcoa_create_strip; see strips.py).
        pipeline=False: PCOA_FLAG_NO_PIPELINE (fp32 pre-pass and contraction strictly serial; measurements).
        operand: None/"bits" (binary tiles are re-laid out to 1 bit per genotype and expanded to MX-FP4 inside the
        contraction) or "fp4" (PCOA_FLAG_OPERAND_FP4: the operand is stored as MX-FP4, 4 bits per genotype).
        operator=True: the implicit similarity operator (pcoa_create_operator): the engine keeps the carrier bitsets it is fed
        (accumulate_bits / accumulate_plink_bed) and no N x N matrix; compute() runs over the products S v = X^T (X v).
        grm=True: the standardised-genotype operator (pcoa_create_grm): the engine keeps the 2-bit genotypes of the .bed rows it is
        fed (accumulate_plink_bed only) and compute() decomposes K = A^T diag(d) A / M', the genetic relationship matrix of
        smartpca / plink --pca / GCTA / flashpca, through the products K x.
        grm_study=True: a GRM store of study samples (pcoa_create_grm_study, any n_samples >= 1): it is fed like a GRM engine and
        has no weights of its own; a GRM engine's grm_project(study, ...) places its samples on that engine's axes."""
        if not pipeline:
            flags |= L.PCOA_FLAG_NO_PIPELINE
        if operand == "fp4":
            flags |= L.PCOA_FLAG_OPERAND_FP4
        elif operand not in (None, "bits"):
            raise ValueError("operand must be 'bits' or 'fp4'")
        if eig == "householder":
            flags |= L.PCOA_FLAG_EIG_HOUSEHOLDER
        elif eig == "lanczos":
            flags |= L.PCOA_FLAG_EIG_LANCZOS
        elif eig == "band":   # Lanczos only, as the band iteration from the start (eigenvalues of exact multiplicity > 1)
            flags |= L.PCOA_FLAG_EIG_LANCZOS | L.PCOA_FLAG_EIG_BAND
        elif eig not in (None, "auto"):
            raise ValueError("eig must be 'auto', 'householder', 'lanczos' or 'band'")
        if gram_kernel == "f32":
            flags |= L.PCOA_FLAG_GRAM_F32_MFMA
        elif gram_kernel == "i8":
            flags |= L.PCOA_FLAG_GRAM_I8_MFMA
        elif gram_kernel == "fp4":
            flags |= L.PCOA_FLAG_GRAM_FP4_MFMA
        elif gram_kernel not in (None, "auto"):
            raise ValueError("gram_kernel must be 'auto', 'fp4', 'i8' or 'f32'")
        self._lib = L.load()
        self._ctx = ctypes.c_void_p()
        self.strip = None if strip is None else (int(strip[0]), int(strip[1]))
        self.operator = bool(operator)
        self.grm_study = bool(grm_study)
        self.grm = bool(grm) or self.grm_study
        if self.operator and self.strip is not None:
            raise ValueError("operator=True and strip= exclude each other")
        if self.grm and (self.operator or self.strip is not None):
            raise ValueError("grm=True excludes operator=True and strip=")
        if self.grm_study:
            rc = self._lib.pcoa_create_grm_study(ctypes.byref(self._ctx), int(n_samples), int(device), int(flags))
        elif self.grm:
            rc = self._lib.pcoa_create_grm(ctypes.byref(self._ctx), int(n_samples), int(device), int(flags))
        elif self.operator:
            rc = self._lib.pcoa_create_operator(ctypes.byref(self._ctx), int(n_samples), int(device), int(flags))
        elif self.strip is None:
            rc = self._lib.pcoa_create(ctypes.byref(self._ctx), int(n_samples), int(device), int(flags))
        else:
            rc = self._lib.pcoa_create_strip(ctypes.byref(self._ctx), int(n_samples), self.strip[0], self.strip[1],
                                             int(device), int(flags))
        if rc != L.PCOA_OK:
            msg = self._lib.pcoa_last_error(None)
            self._ctx = None
            raise PcoaError(rc, msg.decode() if msg else "pcoa_create failed")
        self.n = int(n_samples)
        self.cols = self.n if self.strip is None else self.strip[1]   # columns of S this ctx holds
        self.device = int(device)
        self._keepalive = []

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != L.PCOA_OK:
            msg = self._lib.pcoa_last_error(self._ctx)
            msg = msg.decode() if msg else ""
            if rc == L.PCOA_ERR_INDEX_RANGE:
                raise IndexRangeError(rc, msg)
            raise PcoaError(rc, msg)

    def close(self):
        if getattr(self, "_ctx", None):
            if not getattr(self, "_borrowed", False):   # (a view of a companion the library owns is not destroyed here)
                self._lib.pcoa_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        self._check(self._lib.pcoa_sync(self._ctx))
        self._keepalive = []

    def reset(self):
        self._check(self._lib.pcoa_reset(self._ctx))

    def reserve(self, variants_per_call=0, num_pc=0):
        """Allocate now what the first accumulate / compute calls would allocate lazily (pcoa_reserve)."""
        self._check(self._lib.pcoa_reserve(self._ctx, int(variants_per_call), int(num_pc)))

    def set_stream(self, hip_stream_ptr):
        self._check(self._lib.pcoa_set_stream(self._ctx, ctypes.c_void_p(hip_stream_ptr or 0)))

    def device_info(self):
        buf = ctypes.create_string_buffer(256)
        cu = ctypes.c_int32(0)
        self._check(self._lib.pcoa_device_info(self._ctx, buf, 256, ctypes.byref(cu)))
        return buf.value.decode(), int(cu.value)

    # ------------------------------------------------------------------ getSimilarityMatrix
    def accumulate_calls(self, sample_idx, row_offsets):
        """CSR carrier lists: exactly what RDD[Seq[Int]] carries (VariantsPca.scala:153-168)."""
        idx = np.ascontiguousarray(sample_idx, dtype=np.int32)
        offs = np.ascontiguousarray(row_offsets, dtype=np.int64)
        if offs.ndim != 1 or offs.size < 1:
            raise ValueError("row_offsets must have n_variants + 1 entries")
        # the C side walks sample_idx[row_offsets[0] .. row_offsets[n]) through raw pointers: inconsistent arrays
        # must fail here, not as an out-of-bounds read
        if idx.ndim != 1:
            raise ValueError("sample_idx must be one-dimensional")
        if offs[0] < 0 or offs[-1] > idx.size or (offs.size > 1 and np.any(np.diff(offs) < 0)):
            raise ValueError("row_offsets must be non-decreasing, start at >= 0 and end at <= len(sample_idx) = %d"
                             % idx.size)
        if idx.size == 0:
            idx = np.zeros(1, dtype=np.int32)
        self._check(self._lib.pcoa_accumulate_calls(self._ctx, _ptr(idx), _ptr(offs), offs.size - 1))

    def accumulate_calls_tensors(self, sample_idx, row_offsets, asynchronous=False):
        """The same boundary for torch tensors (plumbing: memory handles only) -- pcoa_accumulate_calls_ex:
        CUDA tensors are read in place (PCOA_CALLS_DEVICE_PTR), pinned CPU tensors by the DMA engine (PCOA_CALLS_HOST_PINNED),
        other CPU tensors like numpy arrays.  asynchronous=True (PCOA_CALLS_ASYNC): return when the work is queued; the tensors
        are kept alive (and must stay unmodified) until the next synchronising call."""
        import torch
        assert sample_idx.dtype == torch.int32 and row_offsets.dtype == torch.int64
        assert sample_idx.dim() == 1 and row_offsets.dim() == 1 and sample_idx.is_contiguous() and row_offsets.is_contiguous()
        assert sample_idx.device == row_offsets.device
        if sample_idx.numel() == 0:
            return   # only empty lists: they add nothing (filtered at VariantsPca.scala:166); an empty tensor has no address
        flags = 0
        if sample_idx.is_cuda:
            flags |= L.PCOA_CALLS_DEVICE_PTR
            torch.cuda.current_stream(sample_idx.device).synchronize()   # the engine runs on its own stream
        elif sample_idx.is_pinned() and row_offsets.is_pinned():
            flags |= L.PCOA_CALLS_HOST_PINNED
        if asynchronous and not sample_idx.is_cuda:
            flags |= L.PCOA_CALLS_ASYNC
        if flags & (L.PCOA_CALLS_DEVICE_PTR | L.PCOA_CALLS_ASYNC):
            self._keepalive.append((sample_idx, row_offsets))
        self._check(self._lib.pcoa_accumulate_calls_ex(self._ctx, ctypes.c_void_p(sample_idx.data_ptr()),
                                                       ctypes.c_void_p(row_offsets.data_ptr()), int(row_offsets.shape[0]) - 1, flags))

    def accumulate_callsets(self, callsets):
        """Convenience: list of per-variant index lists."""
        offs = np.zeros(len(callsets) + 1, dtype=np.int64)
        for v, c in enumerate(callsets):
            offs[v + 1] = offs[v] + len(c)
        idx = np.fromiter((i for c in callsets for i in c), dtype=np.int32, count=int(offs[-1]))
        self.accumulate_calls(idx, offs)

    def accumulate_dense(self, x, n_variants=None, ld=None):
        """Dense variants x samples fp32 tile.  `x` is a numpy array (host) or any object with
        data_ptr()/is_cuda (a torch CUDA tensor: read in place, kept alive until sync())."""
        if hasattr(x, "data_ptr") and getattr(x, "is_cuda", False):
            import torch  # plumbing only: device memory handle
            assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
            nv = int(x.shape[0]) if n_variants is None else int(n_variants)
            ldv = int(x.stride(0)) if ld is None else int(ld)
            self._keepalive.append(x)
            # the engine runs on its own stream: whatever torch queued to produce x must have finished
            torch.cuda.current_stream(x.device).synchronize()
            self._check(self._lib.pcoa_accumulate_dense_f32(self._ctx, ctypes.c_void_p(x.data_ptr()), nv, ldv, 1))
            return
        a = np.ascontiguousarray(x, dtype=np.float32)
        if a.ndim != 2:
            raise ValueError("x must be 2-D [variants][samples]")
        nv = a.shape[0] if n_variants is None else int(n_variants)
        ldv = a.shape[1] if ld is None else int(ld)
        self._check(self._lib.pcoa_accumulate_dense_f32(self._ctx, _ptr(a), nv, ldv, 0))

    def accumulate_dense_u8(self, x, n_variants=None, ld=None):
        """Dense variants x samples tile with one byte per genotype (0..127): numpy uint8 array (host) or a
        torch uint8 CUDA tensor (read in place)."""
        if hasattr(x, "data_ptr") and getattr(x, "is_cuda", False):
            import torch  # plumbing only
            assert x.dtype == torch.uint8 and x.dim() == 2 and x.stride(1) == 1
            nv = int(x.shape[0]) if n_variants is None else int(n_variants)
            ldv = int(x.stride(0)) if ld is None else int(ld)
            self._keepalive.append(x)
            torch.cuda.current_stream(x.device).synchronize()  # see accumulate_dense
            self._check(self._lib.pcoa_accumulate_dense_u8(self._ctx, ctypes.c_void_p(x.data_ptr()), nv, ldv, 1))
            return
        a = np.ascontiguousarray(x, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("x must be 2-D [variants][samples]")
        nv = a.shape[0] if n_variants is None else int(n_variants)
        ldv = a.shape[1] if ld is None else int(ld)
        self._check(self._lib.pcoa_accumulate_dense_u8(self._ctx, _ptr(a), nv, ldv, 0))

    def accumulate_bits(self, bits, n_variants=None, ld_words=None):
        """Bit-packed tile: row v = carrier bitset of variant v, sample i = bit (i & 31) of word i >> 5
        (`ingest.pack_bits` builds it).  numpy uint32 [V][W] (host) or a torch int32 CUDA tensor (read in place)."""
        ptr, nv, ldv, dev, keep = _rows_arg(bits, *_BITS_ROWS)
        if dev:
            self._keepalive.append(keep)
        self._check(self._lib.pcoa_accumulate_bits(self._ctx, ptr, nv if n_variants is None else int(n_variants),
                                                   ldv if ld_words is None else int(ld_words), int(dev)))

    def accumulate_plink_bed(self, rows, ref_is_a1=False, asynchronous=False):
        """Raw variant-major PLINK .bed rows, numpy uint8 [V][row_bytes] (host) or a torch uint8 CUDA tensor: decoded on the
        device (pcoa_accumulate_plink_bed).  asynchronous=True: a PINNED torch uint8 CPU tensor that is only queued
        (PCOA_BED_HOST_ASYNC): it must stay unmodified until the second later call has returned, or the next sync()."""
        ptr, nv, stride, source = self._bed_arg(rows, asynchronous)
        self._check(self._lib.pcoa_accumulate_plink_bed(self._ctx, ptr, nv, stride, int(bool(ref_is_a1)), source))

    def _bed_arg(self, rows, asynchronous):
        """(pointer, rows, row_bytes, is_device_ptr) of the two accumulate_plink_bed* calls; a device tensor is kept alive."""
        ptr, nv, stride, dev, keep = _rows_arg(rows, *_BED_ROWS, pinned=asynchronous)
        if dev:
            self._keepalive.append(keep)
        return ptr, nv, stride, L.PCOA_BED_HOST_ASYNC if asynchronous else int(dev)

    def accumulate_plink_bed_calls(self, rows, companion, ref_is_a1=False, asynchronous=False):
        """accumulate_plink_bed feeding two engines from one read of the rows (pcoa_accumulate_plink_bed_calls): the carrier
        bitsets into this engine, the missing-call bitsets (code 01) into `companion`, an ordinary full engine with this one's
        N on this one's device.  The same three forms of `rows`, the same lifetime rules."""
        ptr, nv, stride, source = self._bed_arg(rows, asynchronous)
        self._check(self._lib.pcoa_accumulate_plink_bed_calls(self._ctx, companion._ctx, ptr, nv, stride, int(bool(ref_is_a1)), source))

    def accumulate_dense_device_ptr(self, ptr, n_variants, ld):
        self._check(self._lib.pcoa_accumulate_dense_f32(self._ctx, ctypes.c_void_p(int(ptr)), int(n_variants),
                                                        int(ld), 1))

    def _synth_params(self, seed, pop_offsets, thresholds):
        po = np.ascontiguousarray(pop_offsets, dtype=np.int32)
        th = np.ascontiguousarray(thresholds, dtype=np.uint32)
        p = L.PcoaSynthParams()
        p.seed = int(seed)
        p.n_pops = int(po.size - 1)
        p.pop_offsets = po.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        p.thresholds = th.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        return p, (po, th)

    def accumulate_synthetic(self, seed, pop_offsets, thresholds, first_variant):
        th = np.asarray(thresholds)
        p, keep = self._synth_params(seed, pop_offsets, th)
        self._check(self._lib.pcoa_accumulate_synthetic(self._ctx, ctypes.byref(p), int(first_variant),
                                                        int(th.shape[0])))
        del keep

    def synth_fill(self, seed, pop_offsets, thresholds, first_variant, x_dev_ptr, ld):
        th = np.asarray(thresholds)
        p, keep = self._synth_params(seed, pop_offsets, th)
        self._check(self._lib.pcoa_synth_fill_f32(self._ctx, ctypes.byref(p), int(first_variant), int(th.shape[0]),
                                                  ctypes.c_void_p(int(x_dev_ptr)), int(ld)))
        del keep

    def finalize(self):
        self._check(self._lib.pcoa_gram_finalize(self._ctx))

    def gram(self):
        """All N^2 entries of S as int64 (zeros included, as matrix.iterator emits them, :189)."""
        out = np.zeros((self.n, self.cols), dtype=np.int64)   # a strip owner holds N x cols
        self._check(self._lib.pcoa_gram_read_i64(self._ctx, _ptr(out)))
        return out

    def gram_block(self, row0, col0, rows, cols):
        """The block S[row0:row0+rows, col0:col0+cols] as int64 (no N x N staging)."""
        out = np.zeros((int(rows), int(cols)), dtype=np.int64)
        self._check(self._lib.pcoa_gram_read_block_i64(self._ctx, int(row0), int(col0), int(rows), int(cols), _ptr(out)))
        return out

    def load_gram(self, s):
        a = np.ascontiguousarray(s, dtype=np.int64)
        if a.shape != (self.n, self.cols):
            raise ValueError("expected an %d x %d matrix" % (self.n, self.cols))
        self._check(self._lib.pcoa_gram_load_i64(self._ctx, _ptr(a)))

    def lanczos(self, matvec, num_pc, max_steps=512, tol=1e-11, first_check=12, trace=None):
        """Top-k eigenpairs of the symmetric operator `matvec` (float64 CUDA tensor of N entries on this engine's GPU -> the
        same) by the ENGINE's Lanczos iteration (pcoa_lanczos_with_matvec): Krylov basis, re-orthogonalisation, the Ritz
        problem and the true-residual acceptance run in the library's kernels; this method only wraps the callback's device
        pointers as tensors.  Returns (components [N][k] sign-normalised unit columns, eigenvalues [k]).  (max_steps / tol /
        first_check are the stand-in's knobs; the engine uses its own: 512, 1e-11, 12.)"""
        import torch  # plumbing only: a tensor view of a device pointer
        n, k = self.n, int(num_pc)
        dev = torch.device("cuda", self.device)

        class _Ptr(object):   # __cuda_array_interface__: N float64 at a raw device address
            def __init__(self, addr):
                self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (int(addr), False), "version": 2}

        failure = []

        def call(_user, v_ptr, y_ptr):
            try:
                v = torch.as_tensor(_Ptr(v_ptr), device=dev)
                y = torch.as_tensor(_Ptr(y_ptr), device=dev)
                y.copy_(matvec(v))
                torch.cuda.current_stream(dev).synchronize()   # the engine reads y on its own stream next
                return 0
            except BaseException as exc:   # never unwind through the C frames
                failure.append(exc)
                return 1

        cb = L.MATVEC_FN(call)
        comps = np.zeros((k, n), dtype=np.float64)
        lam = np.zeros(k, dtype=np.float64)
        steps = ctypes.c_int32(0)
        rc = self._lib.pcoa_lanczos_with_matvec(self._ctx, k, cb, None, _ptr(comps), _ptr(lam), ctypes.byref(steps))
        if failure:
            raise failure[0]
        if trace is not None:
            trace.append((int(steps.value), lam.copy(), None))
        if rc == L.PCOA_ERR_NOT_CONVERGED:
            raise RuntimeError("Lanczos over strips did not reach a verified residual in %d steps (tiny spectral gaps?); there "
                               "is no dense fallback for a matrix tiled across GPUs" % int(steps.value))
        self._check(rc)
        return np.ascontiguousarray(comps.T), lam

    def debug_centred_matvec(self, x, form):
        """One y = B x of the centred matrix of the current S (test hook of the mat-vec forms of the eigensolver, numbered as
        timings()["matvec_form"]): 0 = one wave per row, S centred on the fly; 1 = upper-triangular tiles (N % 4 == 0, no
        int64 part); 2 = one wave per row over the materialised B."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros(self.n, dtype=np.float64)
        self._check(self._lib.pcoa_debug_centred_matvec(self._ctx, _ptr(x), _ptr(y), int(form)))
        return y

    def reduce_from(self, other):
        """self.S += other.S (two engines of this process; pcoa_gram_reduce_from: peer copy + int64 add, no collective)."""
        self._check(self._lib.pcoa_gram_reduce_from(self._ctx, other._ctx))

    def subset(self, keep):
        """A new PcoaEngine over the samples `keep` (strictly increasing indices into this engine's samples) whose S is
        S[keep][:, keep] of this one, gathered on the device (pcoa_create_subset): the similarity matrix of the reduced cohort
        without feeding a variant again.  This engine is unchanged; the peak is both matrices resident."""
        idx = np.ascontiguousarray(keep, dtype=np.int32)
        if idx.ndim != 1:
            raise ValueError("keep must be one-dimensional")
        ctx = ctypes.c_void_p()
        self._check(self._lib.pcoa_create_subset(ctypes.byref(ctx), self._ctx, _ptr(idx) if idx.size else None, int(idx.size)))
        sub = object.__new__(PcoaEngine)
        sub._lib, sub._ctx = self._lib, ctx
        sub.strip, sub.operator = None, False
        sub.n = sub.cols = int(idx.size)
        sub.device = self.device
        sub._keepalive = []
        return sub

    PAIR_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("shared", np.int64)])   # pcoa_pair

    def similar_pairs(self, min_jaccard, capacity=1 << 20):
        """The screen for duplicate and related sample pairs (pcoa_similar_pairs): with d = diag(S), the pairs i < j with
        U = d_i + d_j - S(i, j) > 0 and S(i, j) >= min_jaccard * U, found on the device in one pass over the upper triangle.
        Returns (pairs, n_found, diag): `pairs` a structured array (fields i, j, shared) of the first min(n_found, capacity)
        pairs in increasing (i, j) order, `n_found` the full count whatever the capacity, `diag` int64 [N]."""
        cap = int(capacity)
        pairs = np.zeros(max(cap, 0), dtype=self.PAIR_DTYPE)
        diag = np.zeros(self.n, dtype=np.int64)
        found = ctypes.c_int64(0)
        self._check(self._lib.pcoa_similar_pairs(self._ctx, float(min_jaccard), _ptr(pairs) if cap > 0 else None, cap,
                                                 ctypes.byref(found), _ptr(diag)))
        n_found = int(found.value)
        return pairs[:min(n_found, cap)], n_found, diag

    # ------------------------------------------------------------------ KING-robust kinship over five planes
    KING_PAIR_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("hethet", np.int64), ("ibs0", np.int64),
                                ("het_sum", np.int64)])   # pcoa_king_pair

    @staticmethod
    def _king_planes(planes):
        """(the library, planes[0] or None, the ctx array) of a sequence of five engines; an entry may be None (the library
        refuses it).  Errors are reported on planes[0], or on the thread where there is none."""
        planes = list(planes) if planes is not None else None
        if planes is not None and len(planes) != L.PCOA_KING_PLANES:
            raise ValueError("planes must be %d engines (het, missing, het_or_missing, hom_a1, hom_a2)" % L.PCOA_KING_PLANES)
        lib = L.load()
        if planes is None:
            return lib, None, None
        arr = (ctypes.c_void_p * L.PCOA_KING_PLANES)(*[p._ctx if p is not None else None for p in planes])
        return lib, planes[0], arr

    @staticmethod
    def _king_check(lib, first, rc):
        if rc != L.PCOA_OK:
            msg = lib.pcoa_last_error(first._ctx if first is not None else None)
            raise PcoaError(rc, msg.decode() if msg else "")

    @staticmethod
    def accumulate_plink_bed_king(planes, rows, asynchronous=False):
        """accumulate_plink_bed feeding the five genotype-class planes from one read of the rows
        (pcoa_accumulate_plink_bed_king): `planes` are five ordinary engines of one N on one device, in the order het, missing,
        het_or_missing, hom_a1, hom_a2 (variants_pca.king_planes is the decode).  The same three forms of `rows`, the same
        lifetime rules; the staging and the keep-alive are planes[0]'s."""
        lib, first, arr = PcoaEngine._king_planes(planes)
        if first is not None:
            ptr, nv, stride, source = first._bed_arg(rows, asynchronous)
        else:
            a = np.ascontiguousarray(rows, dtype=np.uint8)
            ptr, nv, stride, source = _ptr(a), a.shape[0], a.shape[1], 0
        PcoaEngine._king_check(lib, first, lib.pcoa_accumulate_plink_bed_king(arr, ptr, nv, stride, source))

    @staticmethod
    def king_pairs(planes, min_kinship, capacity=1 << 20):
        """The KING-robust kinship screen (pcoa_king_pairs) over the five planes' matrices: the pairs i < j with het_sum > 0
        and hethet - 2 ibs0 >= min_kinship * het_sum (variants_pca.king_counts / king_pairs_rule are the rule), found on the
        device in one pass over the upper triangles.  Returns (pairs, n_found, n_variants, het): `pairs` a structured array
        (fields i, j, hethet, ibs0, het_sum) of the first min(n_found, capacity) pairs in increasing (i, j) order, `n_found` the
        full count whatever the capacity, n_variants = V, `het` int64 [N] the heterozygous calls of each sample."""
        lib, first, arr = PcoaEngine._king_planes(planes)
        cap = int(capacity)
        pairs = np.zeros(max(cap, 0), dtype=PcoaEngine.KING_PAIR_DTYPE)
        n = first.n if first is not None else 0
        het = np.zeros(n, dtype=np.int64)
        found, v = ctypes.c_int64(0), ctypes.c_int64(0)
        PcoaEngine._king_check(lib, first, lib.pcoa_king_pairs(arr, float(min_kinship), _ptr(pairs) if cap > 0 else None, cap,
                                                                ctypes.byref(found), ctypes.byref(v), _ptr(het) if n else None))
        n_found = int(found.value)
        return pairs[:min(n_found, cap)], n_found, int(v.value), het

    def king_stats(self):
        """pcoa_get_king_stats of this engine as planes[0]: king_seconds / king_bytes / king_calls."""
        k = L.PcoaKingStats()
        self._check(self._lib.pcoa_get_king_stats(self._ctx, ctypes.byref(k), ctypes.sizeof(k)))
        return dict((f[0], getattr(k, f[0])) for f in L.PcoaKingStats._fields_)

    SIMILARITY_KINDS = {"shared": 0, "jaccard": 1, "cosine": 2}   # PCOA_SIMILARITY_*

    def set_similarity(self, kind):
        """What compute() decomposes from now on (pcoa_set_similarity): "shared" (the counts S, the default), "jaccard"
        (S_ij / (d_i + d_j - S_ij)) or "cosine" (S_ij / sqrt(d_i d_j)), d = diag(S), evaluated on the fly from the integer S;
        variants_pca.similarity_measure is the rule.  Survives reset(); subset() inherits it.  The number of a kind is
        accepted as well (an unknown one is the library's error)."""
        if isinstance(kind, str):
            if kind not in self.SIMILARITY_KINDS:
                raise ValueError("similarity kind must be one of shared, jaccard, cosine, not %r" % (kind,))
            kind = self.SIMILARITY_KINDS[kind]
        self._check(self._lib.pcoa_set_similarity(self._ctx, int(kind)))

    def get_similarity(self):
        """The name of the measure set (pcoa_get_similarity)."""
        kind = ctypes.c_int32(-1)
        self._check(self._lib.pcoa_get_similarity(self._ctx, ctypes.byref(kind)))
        return dict((v, k) for k, v in self.SIMILARITY_KINDS.items())[int(kind.value)]

    def set_call_companion(self, other, n_variants=0):
        """The pairwise-complete similarity (pcoa_set_call_companion): `other` is an ordinary engine fed the bitsets of the
        MISSING calls, n_variants the number of variants fed.  From now on compute(), center() and debug_centred_matvec() use
        K(i, j) = S(i, j) / M(i, j), M = the variants at which both samples were called; variants_pca.call_complete_measure is
        the rule.  other=None unbinds.  Survives reset(); subset() of a bound engine gets a companion of its own.  The caller
        keeps `other` alive while it is bound."""
        self._check(self._lib.pcoa_set_call_companion(self._ctx, other._ctx if other is not None else None, int(n_variants)))
        self._companion = other

    def get_call_companion(self):
        """(companion, n_variants) as bound (pcoa_get_call_companion), (None, 0) where none is.  The companion is the engine
        given to set_call_companion; for the result of subset() it is a view of the companion the library owns (closing the
        view does nothing, closing the subset destroys it)."""
        ctx, v = ctypes.c_void_p(), ctypes.c_int64(0)
        self._check(self._lib.pcoa_get_call_companion(self._ctx, ctypes.byref(ctx), ctypes.byref(v)))
        if not ctx.value:
            return None, 0
        mine = getattr(self, "_companion", None)
        if mine is not None and mine._ctx is not None and mine._ctx.value == ctx.value:
            return mine, int(v.value)
        view = object.__new__(PcoaEngine)
        view._lib, view._ctx, view._borrowed = self._lib, ctx, True
        view.strip, view.operator = None, False
        view.n = view.cols = self.n
        view.device = self.device
        view._keepalive = []
        return view, int(v.value)

    def export_device(self, dst_ptr):
        self._check(self._lib.pcoa_gram_export_device_i64(self._ctx, ctypes.c_void_p(int(dst_ptr))))

    def import_device(self, src_ptr):
        self._check(self._lib.pcoa_gram_import_device_i64(self._ctx, ctypes.c_void_p(int(src_ptr))))

    # ------------------------------------------------------------------ native RCCL
    def comm_unique_id(self):
        buf = (ctypes.c_uint8 * 128)()
        self._check(self._lib.pcoa_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)))
        return bytes(buf)

    def comm_init(self, unique_id, rank, n_ranks):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)
        comm = ctypes.c_void_p()
        self._check(self._lib.pcoa_comm_init(self._ctx, ctypes.cast(buf, ctypes.c_void_p), int(rank), int(n_ranks),
                                             ctypes.byref(comm)))
        return comm

    def comm_runtime(self):
        """(path, version code) of the RCCL image the library's communicator calls are bound to."""
        buf = ctypes.create_string_buffer(1024)
        ver = ctypes.c_int32(0)
        self._check(self._lib.pcoa_comm_runtime(buf, 1024, ctypes.byref(ver)))
        return buf.value.decode(), int(ver.value)

    def comm_destroy(self, comm):
        self._check(self._lib.pcoa_comm_destroy(comm))

    def comm_count(self, comm):
        n = ctypes.c_int32(0)
        self._check(self._lib.pcoa_comm_count(comm, ctypes.byref(n)))
        return int(n.value)

    def allreduce_rccl(self, comm):
        self._check(self._lib.pcoa_gram_allreduce_rccl(self._ctx, comm))

    # ------------------------------------------------------------------ strip owner
    def strip_col_sums(self):
        """rowSums (VariantsPca.scala:206) of the strip's samples: column sums of the held N x cols block."""
        out = np.zeros(self.cols, dtype=np.float64)
        self._check(self._lib.pcoa_strip_col_sums(self._ctx, _ptr(out)))
        return out

    def strip_matvec(self, v, means, matrix_mean):
        """(B v)[col0:col0+cols] with B evaluated on the fly from the strip (VariantsPca.scala:216-221 order)."""
        v = np.ascontiguousarray(v, dtype=np.float64)
        means = np.ascontiguousarray(means, dtype=np.float64)
        if v.shape != (self.n,) or means.shape != (self.n,):
            raise ValueError("v and means must have N = %d entries" % self.n)
        out = np.zeros(self.cols, dtype=np.float64)
        self._check(self._lib.pcoa_strip_matvec(self._ctx, _ptr(v), _ptr(means), float(matrix_mean), _ptr(out)))
        return out

    def strip_set_centering(self, means, matrix_mean):
        """Row means and matrix mean of the current S, resident on the device for strip_matvec_device."""
        means = np.ascontiguousarray(means, dtype=np.float64)
        if means.shape != (self.n,):
            raise ValueError("means must have N = %d entries" % self.n)
        self._check(self._lib.pcoa_strip_set_centering(self._ctx, _ptr(means), float(matrix_mean)))

    def strip_matvec_device(self, v_dev):
        """(B v)[col0:col0+cols] for a float64 torch tensor v on this engine's GPU; returns a device tensor (no PCIe traffic)."""
        import torch  # plumbing only: device memory handles
        assert v_dev.is_cuda and v_dev.dtype == torch.float64 and v_dev.dim() == 1 and v_dev.shape[0] == self.n
        if v_dev.device.index != self.device:   # the ctx dereferences the pointer on ITS device
            raise ValueError("v lives on cuda:%d, this strip owner on cuda:%d" % (v_dev.device.index, self.device))
        v_dev = v_dev.contiguous()
        y = torch.empty(self.cols, dtype=torch.float64, device=v_dev.device)
        torch.cuda.current_stream(v_dev.device).synchronize()   # the engine runs on its own stream
        self._check(self._lib.pcoa_strip_matvec_device(self._ctx, ctypes.c_void_p(v_dev.data_ptr()), ctypes.c_void_p(y.data_ptr())))
        return y

    # ------------------------------------------------------------------ implicit similarity operator
    def operator_info(self):
        """(variants in the bit store, bytes of HBM its segments hold), or None on an engine that is not an operator."""
        nv, nb = ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self._lib.pcoa_operator_info(self._ctx, ctypes.byref(nv), ctypes.byref(nb))
        if rc < 0:
            self._check(rc)
        return (int(nv.value), int(nb.value)) if rc == 1 else None

    def operator_row_sums(self):
        """rowSums of S (VariantsPca.scala:206) as exact int64, from the bit store."""
        out = np.zeros(self.n, dtype=np.int64)
        self._check(self._lib.pcoa_operator_row_sums(self._ctx, _ptr(out)))
        return out

    def operator_matvec_device(self, v_dev, centred):
        """y = S v (centred false) or y = B v (centred true) for a float64 torch tensor v of N entries on this engine's GPU;
        returns a device tensor."""
        import torch  # plumbing only: device memory handles
        assert v_dev.is_cuda and v_dev.dtype == torch.float64 and v_dev.dim() == 1 and v_dev.shape[0] == self.n
        if v_dev.device.index != self.device:
            raise ValueError("v lives on cuda:%d, this engine on cuda:%d" % (v_dev.device.index, self.device))
        v_dev = v_dev.contiguous()
        y = torch.empty(self.n, dtype=torch.float64, device=v_dev.device)
        torch.cuda.current_stream(v_dev.device).synchronize()   # the engine runs on its own stream
        self._check(self._lib.pcoa_operator_matvec_device(self._ctx, ctypes.c_void_p(v_dev.data_ptr()),
                                                          ctypes.c_void_p(y.data_ptr()), int(bool(centred))))
        return y

    # ------------------------------------------------------------------ standardised genotypes (GRM)
    def grm_info(self):
        """(variants in the genotype store, variants used under the current min MAF, bytes of HBM the store's segments hold), or
        None on an engine that is not a GRM engine."""
        nv, nu, nb = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self._lib.pcoa_grm_info(self._ctx, ctypes.byref(nv), ctypes.byref(nu), ctypes.byref(nb))
        if rc < 0:
            self._check(rc)
        return (int(nv.value), int(nu.value), int(nb.value)) if rc == 1 else None

    def grm_set_min_maf(self, maf):
        """A variant is used only if its minor-allele frequency among the called samples is at least maf (0 <= maf < 0.5)."""
        self._check(self._lib.pcoa_grm_set_min_maf(self._ctx, float(maf)))

    def grm_counts(self, first_variant=0, n_variants=None):
        """[n, 3] int32: called, heterozygous and homozygous non-reference samples of the store's rows."""
        if n_variants is None:
            n_variants = self.grm_info()[0] - int(first_variant)
        out = np.zeros((max(int(n_variants), 0), 3), dtype=np.int32)
        self._check(self._lib.pcoa_grm_counts(self._ctx, int(first_variant), int(n_variants), _ptr(out)))
        return out

    def grm_matvec_device(self, x_dev):
        """y = K x for a float64 torch tensor x of N entries on this engine's GPU; returns a device tensor."""
        import torch  # plumbing only: device memory handles
        assert x_dev.is_cuda and x_dev.dtype == torch.float64 and x_dev.dim() == 1 and x_dev.shape[0] == self.n
        if x_dev.device.index != self.device:
            raise ValueError("x lives on cuda:%d, this engine on cuda:%d" % (x_dev.device.index, self.device))
        x_dev = x_dev.contiguous()
        y = torch.empty(self.n, dtype=torch.float64, device=x_dev.device)
        torch.cuda.current_stream(x_dev.device).synchronize()   # the engine runs on its own stream
        self._check(self._lib.pcoa_grm_matvec_device(self._ctx, ctypes.c_void_p(x_dev.data_ptr()), ctypes.c_void_p(y.data_ptr())))
        return y

    def _grm_axes(self, components, eigenvalues):
        """components [N, k] and eigenvalues [k] as compute(k) returned them -> ([k][N] contiguous, [k], k)."""
        comps = np.asarray(components, dtype=np.float64)
        if comps.ndim == 1:
            comps = comps[:, None]
        lam = np.ascontiguousarray(np.asarray(eigenvalues, dtype=np.float64).reshape(-1))
        if comps.ndim != 2 or comps.shape[0] != self.n or comps.shape[1] != lam.shape[0]:
            raise ValueError("components must be [N = %d, k] and eigenvalues [k], not %s and %s" % (self.n, comps.shape, lam.shape))
        return np.ascontiguousarray(comps.T), lam, int(lam.shape[0])

    def grm_weights(self, components, eigenvalues, scaled=True, first_variant=0, n_variants=None):
        """[n_variants, k] float64: the SNP weights of the axes compute(k) returned (pcoa_grm_weights).  scaled=True: the left
        singular vectors w_c = sqrt(d) (A u_c) / sqrt(M' lambda_c), orthonormal over the used variants and 0.0 at an unused one;
        scaled=False: t_c = d (A u_c), the vector the projection uses."""
        u, lam, k = self._grm_axes(components, eigenvalues)
        if n_variants is None:
            info = self.grm_info()   # (None: not a GRM engine -- the call itself says so)
            n_variants = info[0] - int(first_variant) if info else 0
        out = np.zeros((max(int(n_variants), 0), k), dtype=np.float64)
        self._check(self._lib.pcoa_grm_weights(self._ctx, k, _ptr(u), _ptr(lam), int(bool(scaled)), int(first_variant),
                                               int(n_variants), _ptr(out)))
        return out

    def grm_project(self, study, components, eigenvalues):
        """(coords [N_study, k] float64, called [N_study] int32): the samples of `study` -- a grm_study=True engine, or a GRM
        engine, fed the same variants in the same order -- on the axes compute(k) returned for this engine (pcoa_grm_project);
        called[q]: this engine's used variants at which sample q is called."""
        u, lam, k = self._grm_axes(components, eigenvalues)
        coords = np.zeros((k, study.n), dtype=np.float64)
        called = np.zeros(study.n, dtype=np.int32)
        self._check(self._lib.pcoa_grm_project(self._ctx, study._ctx, k, _ptr(u), _ptr(lam), _ptr(coords), _ptr(called)))
        return np.ascontiguousarray(coords.T), called

    def grm_project_lsq(self, study, components, normal=False):
        """(coords [N_study, k] float64, called [N_study] int32, determined [N_study] bool[, normal]): the samples of `study` on
        the axes `components` [N, k] of this engine, each by least squares over the used variants IT is called at
        (pcoa_grm_project_lsq; 1 <= k <= 16, no eigenvalues).  An undetermined sample -- called at fewer than k used variants,
        or with normal equations that are singular to 2^-40 -- has NaN coordinates and determined False.  normal=True: also
        [k (k + 1) / 2 + k, N_study], the packed H_q (entry c (c + 1) / 2 + c') and then P_q of every sample."""
        comps = np.asarray(components, dtype=np.float64)
        if comps.ndim == 1:
            comps = comps[:, None]
        if comps.ndim != 2 or comps.shape[0] != self.n:
            raise ValueError("components must be [N = %d, k], not %s" % (self.n, comps.shape))
        u, k = np.ascontiguousarray(comps.T), int(comps.shape[1])
        coords = np.zeros((k, study.n), dtype=np.float64)
        called = np.zeros(study.n, dtype=np.int32)
        determined = np.zeros(study.n, dtype=np.int32)
        nrm = np.zeros((k * (k + 1) // 2 + k, study.n), dtype=np.float64) if normal else None
        self._check(self._lib.pcoa_grm_project_lsq(self._ctx, study._ctx, k, _ptr(u), _ptr(coords), _ptr(called), _ptr(determined),
                                                   _ptr(nrm) if normal else None))
        out = (np.ascontiguousarray(coords.T), called, determined.astype(bool))
        return out + (nrm,) if normal else out

    def grm_lsq_stats(self):
        """pcoa_get_grm_lsq_stats: calls, pair vectors, seconds of the pair pass and of the solve, and the undetermined samples of
        the last grm_project_lsq call with this engine as the panel."""
        q = L.PcoaGrmLsqStats()
        self._check(self._lib.pcoa_get_grm_lsq_stats(self._ctx, ctypes.byref(q), ctypes.sizeof(q)))
        return dict((f[0], getattr(q, f[0])) for f in L.PcoaGrmLsqStats._fields_)

    GRM_DIVISORS = {"used": L.PCOA_GRM_DIVISOR_USED, "pairwise": L.PCOA_GRM_DIVISOR_PAIRWISE}

    def _grm_divisor(self, divisor):
        if isinstance(divisor, str):
            if divisor not in self.GRM_DIVISORS:
                raise ValueError("divisor must be one of used, pairwise, not %r" % (divisor,))
            return self.GRM_DIVISORS[divisor]
        return int(divisor)   # (an unknown number is the library's error)

    def grm_block(self, row0, rows, col0, cols, divisor="used", pairs=False, device=False):
        """K[row0 : row0 + rows, col0 : col0 + cols] of the matrix compute() decomposes (pcoa_grm_block), float64.  divisor:
        "used" (num / M') or "pairwise" (num / n(i, j), 0 where n is 0); variants_pca.grm_dense_rule is the rule.  pairs=True:
        returns (K, n) with n the int32 counts of jointly called used variants.  device=True: torch tensors on this engine's
        GPU, written by the kernels directly; otherwise numpy arrays."""
        div = self._grm_divisor(divisor)
        shape = (max(int(rows), 0), max(int(cols), 0))
        if device:
            import torch  # plumbing only: device memory handles
            dev = torch.device("cuda", self.device)
            k = torch.empty(shape, dtype=torch.float64, device=dev)
            n = torch.empty(shape, dtype=torch.int32, device=dev) if pairs else None
            torch.cuda.current_stream(dev).synchronize()   # the engine runs on its own stream
            kp = ctypes.c_void_p(k.data_ptr()) if k.numel() else None
            npp = ctypes.c_void_p(n.data_ptr()) if pairs and n.numel() else None
        else:
            k = np.zeros(shape, dtype=np.float64)
            n = np.zeros(shape, dtype=np.int32) if pairs else None
            kp = _ptr(k) if k.size else None
            npp = _ptr(n) if pairs and n.size else None
        self._check(self._lib.pcoa_grm_block(self._ctx, int(row0), int(rows), int(col0), int(cols), div, kp, npp, int(bool(device))))
        return (k, n) if pairs else k

    def grm_pairs_block(self, row0, rows, col0, cols):
        """n[row0 : row0 + rows, col0 : col0 + cols] alone (int32 numpy): only the counting pass runs."""
        n = np.zeros((max(int(rows), 0), max(int(cols), 0)), dtype=np.int32)
        self._check(self._lib.pcoa_grm_block(self._ctx, int(row0), int(rows), int(col0), int(cols), L.PCOA_GRM_DIVISOR_USED, None,
                                             _ptr(n) if n.size else None, 0))
        return n

    def grm_dense(self, divisor="used", block=4096):
        """The whole N x N matrix as float64 numpy, assembled from blocks of the lower triangle and mirrored (the entries above
        the diagonal are the same bits as their mirror images, so nothing is lost)."""
        block = max(int(block), 1)
        out = np.zeros((self.n, self.n), dtype=np.float64)
        for r0 in range(0, self.n, block):
            r = min(block, self.n - r0)
            for c0 in range(0, r0 + 1, block):
                c = min(block, self.n - c0)
                out[r0:r0 + r, c0:c0 + c] = self.grm_block(r0, r, c0, c, divisor)
        low = np.tril(out, -1)
        return np.tril(out) + low.T

    def grm_block_stats(self):
        """pcoa_get_grm_block_stats: grm_block_seconds / grm_block_calls / grm_block_flops."""
        q = L.PcoaGrmBlockStats()
        self._check(self._lib.pcoa_get_grm_block_stats(self._ctx, ctypes.byref(q), ctypes.sizeof(q)))
        return dict((f[0], getattr(q, f[0])) for f in L.PcoaGrmBlockStats._fields_)

    # ------------------------------------------------------------------ the relatedness cut-off on K
    GRM_PAIR_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("k", np.float64), ("n", np.int64)])   # pcoa_grm_pair

    def grm_pairs(self, cutoff, divisor="used", band_rows=0, capacity=1 << 20, diag=False):
        """The relatedness screen of the matrix compute() decomposes (pcoa_grm_pairs): the pairs i < j with K(i, j) >= cutoff,
        K(i, j) the bits grm_block returns under `divisor`, found on the device a band of `band_rows` rows (0: 1,024; a multiple
        of 64) at a time; variants_pca.grm_pairs_rule is the rule.  Returns (pairs, n_found), or (pairs, n_found, diag) with
        diag=True: `pairs` a structured array (fields i, j, k, n) of the first min(n_found, capacity) pairs in increasing (i, j)
        order, n = n(i, j) under "pairwise" and M' under "used"; `n_found` the full count whatever the capacity; `diag` K(i, i),
        float64 [N]."""
        div = self._grm_divisor(divisor)
        cap = int(capacity)
        pairs = np.zeros(max(cap, 0), dtype=self.GRM_PAIR_DTYPE)
        d = np.zeros(self.n, dtype=np.float64) if diag else None
        found = ctypes.c_int64(0)
        self._check(self._lib.pcoa_grm_pairs(self._ctx, float(cutoff), div, int(band_rows), _ptr(pairs) if cap > 0 else None, cap,
                                             ctypes.byref(found), _ptr(d) if diag else None))
        n_found = int(found.value)
        return (pairs[:min(n_found, cap)], n_found, d) if diag else (pairs[:min(n_found, cap)], n_found)

    def grm_pairs_stats(self):
        """pcoa_get_grm_pairs_stats: grm_pairs_seconds / grm_pairs_screen_seconds / grm_pairs_calls / grm_pairs_bands /
        grm_pairs_flops / grm_pairs_bytes."""
        q = L.PcoaGrmPairsStats()
        self._check(self._lib.pcoa_get_grm_pairs_stats(self._ctx, ctypes.byref(q), ctypes.sizeof(q)))
        return dict((f[0], getattr(q, f[0])) for f in L.PcoaGrmPairsStats._fields_)

    # ------------------------------------------------------------------ the KING-robust screen on the 2-bit store
    GRM_ROWS = {"all": L.PCOA_GRM_ROWS_ALL, "used": L.PCOA_GRM_ROWS_USED}

    def _grm_rows_kind(self, rows):
        if isinstance(rows, str):
            if rows not in self.GRM_ROWS:
                raise ValueError("rows must be one of all, used, not %r" % (rows,))
            return self.GRM_ROWS[rows]
        return int(rows)   # (an unknown number is the library's error)

    def grm_king_block(self, row0, rows, col0, cols, rows_kind="all", hethet=True, ibs0=True, het_sum=True, device=False):
        """The rectangle [row0, row0 + rows) x [col0, col0 + cols) of the three KING counts over the store's counted rows
        (pcoa_grm_king_block; variants_pca.grm_king_rule is the rule), int32.  rows_kind: "all" (every row of the store) or
        "used" (used_v under the min MAF, the filters and an installed LD mask).  Returns (hethet, ibs0, het_sum); an output
        switched off comes back as None and is not computed into.  device=True: torch tensors on this engine's GPU, written by
        the kernel directly; otherwise numpy arrays."""
        kind = self._grm_rows_kind(rows_kind)
        shape = (max(int(rows), 0), max(int(cols), 0))
        want = (bool(hethet), bool(ibs0), bool(het_sum))
        if device:
            import torch  # plumbing only: device memory handles
            dev = torch.device("cuda", self.device)
            outs = [torch.empty(shape, dtype=torch.int32, device=dev) if w else None for w in want]
            torch.cuda.current_stream(dev).synchronize()   # the engine runs on its own stream
            ptrs = [ctypes.c_void_p(o.data_ptr()) if o is not None and o.numel() else None for o in outs]
        else:
            outs = [np.zeros(shape, dtype=np.int32) if w else None for w in want]
            ptrs = [_ptr(o) if o is not None and o.size else None for o in outs]
        self._check(self._lib.pcoa_grm_king_block(self._ctx, kind, int(row0), int(rows), int(col0), int(cols), ptrs[0], ptrs[1], ptrs[2],
                                                  int(bool(device))))
        return tuple(outs)

    def grm_king_pairs(self, min_kinship, rows="all", band_rows=0, capacity=1 << 20, het=False):
        """The KING-robust kinship screen on the resident genotype store (pcoa_grm_king_pairs): the pairs i < j with het_sum > 0
        and hethet - 2 ibs0 >= min_kinship * het_sum over the counted rows (rows: "all" or "used"), found on the device a band
        of `band_rows` rows (0: 1,024; a multiple of 64) at a time; variants_pca.grm_king_pairs_rule is the rule.  Returns
        (pairs, n_found, n_rows), or (pairs, n_found, n_rows, h) with het=True: `pairs` a KING_PAIR_DTYPE array of the first
        min(n_found, capacity) pairs in increasing (i, j) order, `n_found` the full count whatever the capacity, `n_rows` the
        counted rows, `h` the heterozygous counted rows of every sample, int64 [N]."""
        kind = self._grm_rows_kind(rows)
        cap = int(capacity)
        pairs = np.zeros(max(cap, 0), dtype=self.KING_PAIR_DTYPE)
        h = np.zeros(self.n, dtype=np.int64) if het else None
        found = ctypes.c_int64(0)
        counted = ctypes.c_int64(0)
        self._check(self._lib.pcoa_grm_king_pairs(self._ctx, kind, float(min_kinship), int(band_rows), _ptr(pairs) if cap > 0 else None,
                                                  cap, ctypes.byref(found), ctypes.byref(counted), _ptr(h) if het else None))
        n_found = int(found.value)
        out = (pairs[:min(n_found, cap)], n_found, int(counted.value))
        return out + (h,) if het else out

    def grm_king_stats(self):
        """pcoa_get_grm_king_stats: grm_king_seconds / grm_king_screen_seconds / grm_king_calls / grm_king_bands / grm_king_macs /
        grm_king_bytes / grm_king_block_calls."""
        q = L.PcoaGrmKingStats()
        self._check(self._lib.pcoa_get_grm_king_stats(self._ctx, ctypes.byref(q), ctypes.sizeof(q)))
        return dict((f[0], getattr(q, f[0])) for f in L.PcoaGrmKingStats._fields_)

    # ------------------------------------------------------------------ PC-Relate kinship on the 2-bit store
    def grm_pcrelate_fit(self, basis, hat=None):
        """Regresses the dosages of every row of the store on the covariates `basis` [n_cov, N] (1 <= n_cov <= 9: a row of ones
        and up to 8 axes) and leaves beta and the basis resident (pcoa_grm_pcrelate_fit).  hat [n_cov, N]: the matrix applied
        to the mean-imputed dosages; None calls pcrelate_hat(basis).  An accumulate call and reset() drop the fit."""
        b = np.ascontiguousarray(basis, dtype=np.float64)
        if b.ndim != 2 or b.shape[1] != self.n:
            raise ValueError("basis must be [n_cov, N = %d], not %s" % (self.n, b.shape))
        h = pcrelate_hat(b) if hat is None else np.ascontiguousarray(hat, dtype=np.float64)
        if h.shape != b.shape:
            raise ValueError("hat must have the shape of basis %s, not %s" % (b.shape, h.shape))
        self._check(self._lib.pcoa_grm_pcrelate_fit(self._ctx, int(b.shape[0]), _ptr(b), _ptr(h)))

    def grm_pcrelate_beta(self, first=0, n=None):
        """beta [n, n_cov] of the rows [first, first + n) of the store under the resident fit (n=None: to the end)."""
        if n is None:
            n = self.grm_info()[0] - int(first)
        k = max(int(self.grm_pcrelate_stats()["grm_pcrelate_n_cov"]), 1)   # the library's own n_cov: the width the call writes
        out = np.zeros((max(int(n), 0), k), dtype=np.float64)
        self._check(self._lib.pcoa_grm_pcrelate_beta(self._ctx, int(first), int(n), _ptr(out) if out.size else out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def grm_pcrelate_isaf(self, first, n):
        """mu_iv [n, N]: the individual-specific allele frequency of every sample at the rows [first, first + n), unmasked."""
        out = np.zeros((max(int(n), 0), self.n), dtype=np.float64)
        self._check(self._lib.pcoa_grm_pcrelate_isaf(self._ctx, int(first), int(n), _ptr(out) if out.size else out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def grm_pcrelate_block(self, row0, rows, col0, cols, maf_threshold=0.01, pairs=False, device=False):
        """phi[row0 : row0 + rows, col0 : col0 + cols] under the resident fit (pcoa_grm_pcrelate_block), float64;
        variants_pca.grm_pcrelate_rule is the rule.  pairs=True: returns (phi, n) with n the int32 counts of variants at which
        both samples pass the mask.  device=True: torch tensors on this engine's GPU; otherwise numpy arrays."""
        shape = (max(int(rows), 0), max(int(cols), 0))
        if device:
            import torch  # plumbing only: device memory handles
            dev = torch.device("cuda", self.device)
            k = torch.empty(shape, dtype=torch.float64, device=dev)
            n = torch.empty(shape, dtype=torch.int32, device=dev) if pairs else None
            torch.cuda.current_stream(dev).synchronize()   # the engine runs on its own stream
            kp = ctypes.c_void_p(k.data_ptr()) if k.numel() else None
            npp = ctypes.c_void_p(n.data_ptr()) if pairs and n.numel() else None
        else:
            k = np.zeros(shape, dtype=np.float64)
            n = np.zeros(shape, dtype=np.int32) if pairs else None
            kp = _ptr(k) if k.size else None
            npp = _ptr(n) if pairs and n.size else None
        self._check(self._lib.pcoa_grm_pcrelate_block(self._ctx, int(row0), int(rows), int(col0), int(cols), float(maf_threshold), kp, npp,
                                                      int(bool(device))))
        return (k, n) if pairs else k

    def grm_pcrelate_dense(self, maf_threshold=0.01, block=4096):
        """The whole N x N phi as float64 numpy, assembled from blocks of the lower triangle and mirrored (an entry above the
        diagonal has the bits of its mirror image)."""
        block = max(int(block), 1)
        out = np.zeros((self.n, self.n), dtype=np.float64)
        for r0 in range(0, self.n, block):
            r = min(block, self.n - r0)
            for c0 in range(0, r0 + 1, block):
                c = min(block, self.n - c0)
                out[r0:r0 + r, c0:c0 + c] = self.grm_pcrelate_block(r0, r, c0, c, maf_threshold)
        low = np.tril(out, -1)
        return np.tril(out) + low.T

    def grm_pcrelate_pairs(self, cutoff, maf_threshold=0.01, band_rows=0, capacity=1 << 20, diag=False):
        """The PC-Relate kinship screen (pcoa_grm_pcrelate_pairs): the pairs i < j with phi(i, j) >= cutoff on the bits
        grm_pcrelate_block returns, found on the device a band of `band_rows` rows (0: 1,024; a multiple of 64) at a time;
        variants_pca.grm_pairs_rule(phi, cutoff, n) is the rule.  Returns (pairs, n_found), or (pairs, n_found, diag) with
        diag=True: `pairs` a GRM_PAIR_DTYPE array (k = phi, n = n(i, j)) of the first min(n_found, capacity) pairs in increasing
        (i, j) order, `diag` phi(i, i), float64 [N]."""
        cap = int(capacity)
        pairs = np.zeros(max(cap, 0), dtype=self.GRM_PAIR_DTYPE)
        d = np.zeros(self.n, dtype=np.float64) if diag else None
        found = ctypes.c_int64(0)
        self._check(self._lib.pcoa_grm_pcrelate_pairs(self._ctx, float(cutoff), float(maf_threshold), int(band_rows),
                                                      _ptr(pairs) if cap > 0 else None, cap, ctypes.byref(found), _ptr(d) if diag else None))
        n_found = int(found.value)
        return (pairs[:min(n_found, cap)], n_found, d) if diag else (pairs[:min(n_found, cap)], n_found)

    def grm_pcrelate_stats(self):
        """pcoa_get_grm_pcrelate_stats: fits, block / pairs calls, bands, the seconds of the fit, the dense launches and the
        screen, issued fp64 flops, bytes the screen read, and (not cumulative) n_cov of the resident fit, 0 without one."""
        q = L.PcoaGrmPcrelateStats()
        self._check(self._lib.pcoa_get_grm_pcrelate_stats(self._ctx, ctypes.byref(q), ctypes.sizeof(q)))
        return dict((f[0], getattr(q, f[0])) for f in L.PcoaGrmPcrelateStats._fields_)

    # ------------------------------------------------------------------ LD pruning of the GRM store
    def grm_ld_prune(self, window, r2_max, breaks=()):
        """LD-prunes the resident genotype store by the r^2 of the dosages over the jointly called samples (pcoa_grm_ld_prune;
        include/pcoa.h states the rule, tests/grm_ld_cohort.py is its numpy form): forward and greedy over the store's rows, a candidate (a variant used under the
        current min MAF) is removed when a KEPT row among the `window` rows before it, behind the last break, exceeds r2_max.
        breaks: strictly increasing row indices, a break lies in front of row b.  Installs the keep mask -- compute, grm_weights,
        grm_project, grm_block and grm_info see the pruned store until an append, reset, another min MAF or grm_ld_clear --
        and returns (candidates, kept)."""
        br = np.ascontiguousarray(np.asarray(list(breaks), dtype=np.int64).reshape(-1))
        cand, kept = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._lib.pcoa_grm_ld_prune(self._ctx, int(window), float(r2_max), _ptr(br) if br.size else None, int(br.size),
                                                ctypes.byref(cand), ctypes.byref(kept)))
        return int(cand.value), int(kept.value)

    def grm_ld_mask(self, first=0, n=None):
        """bool [n]: True for a row the installed prune kept, False for a removed one (non-candidates included)."""
        if n is None:
            info = self.grm_info()   # (None: not a GRM engine -- the call itself says so)
            n = info[0] - int(first) if info else 0
        out = np.zeros(max(int(n), 0), dtype=np.uint8)
        self._check(self._lib.pcoa_grm_ld_mask(self._ctx, int(first), int(n), _ptr(out) if out.size else None))
        return out.astype(bool)

    def grm_ld_clear(self):
        """Drops the keep mask: the store counts unpruned again."""
        self._check(self._lib.pcoa_grm_ld_clear(self._ctx))

    def grm_ld_stats(self):
        """pcoa_get_grm_ld_stats: rows / candidates / kept / in-window pairs of the last prune, seconds of band / resolve / scan."""
        q = L.PcoaGrmLdStats()
        self._check(self._lib.pcoa_get_grm_ld_stats(self._ctx, ctypes.byref(q), ctypes.sizeof(q)))
        return dict((f[0], getattr(q, f[0])) for f in L.PcoaGrmLdStats._fields_)

    # ------------------------------------------------------------------ sample subsets of the GRM store
    def grm_subset(self, keep, study=False):
        """A new GRM PcoaEngine over the samples `keep` (strictly increasing indices into this engine's samples) whose store is
        this one's rows with the other samples' columns taken out, gathered on the device (pcoa_create_grm_subset): the engine
        of the reduced cohort without feeding a variant again.  study=False: as from grm=True (32 samples or more), with this
        engine's min MAF; study=True: as from grm_study=True (1 sample or more), to be placed by grm_project.  Its counts and
        weights are its own samples'; an LD mask is not inherited.  This engine is unchanged; the peak is both stores resident."""
        idx = np.ascontiguousarray(keep, dtype=np.int32)
        if idx.ndim != 1:
            raise ValueError("keep must be one-dimensional")
        ctx = ctypes.c_void_p()
        kind = L.PCOA_GRM_SUBSET_STUDY if study else L.PCOA_GRM_SUBSET_PANEL
        self._check(self._lib.pcoa_create_grm_subset(ctypes.byref(ctx), self._ctx, _ptr(idx) if idx.size else None, int(idx.size),
                                                     int(kind)))
        sub = object.__new__(PcoaEngine)
        sub._lib, sub._ctx = self._lib, ctx
        sub.strip, sub.operator = None, False
        sub.grm, sub.grm_study = True, bool(study)
        sub.n = sub.cols = int(idx.size)
        sub.device = self.device
        sub._keepalive = []
        return sub

    def grm_rows(self, first=0, n=None):
        """uint8 [n, ceil(N / 4)]: the store's rows as .bed rows in the store's coding, which is ref_is_a1=True (pcoa_grm_rows);
        the unused slots of a row's last byte are 00.  Fed to a fresh engine with ref_is_a1=True they reproduce the store."""
        if n is None:
            info = self.grm_info()   # (None: not a GRM engine -- the call itself says so)
            n = info[0] - int(first) if info else 0
        out = np.zeros((max(int(n), 0), (self.n + 3) // 4), dtype=np.uint8)
        self._check(self._lib.pcoa_grm_rows(self._ctx, int(first), int(n), _ptr(out) if out.size else _ptr(np.zeros(1, np.uint8))))
        return out

    def grm_subset_stats(self):
        """pcoa_get_grm_subset_stats of the SOURCE engine: grm_subset_seconds / grm_subset_calls / grm_subset_bytes."""
        q = L.PcoaGrmSubsetStats()
        self._check(self._lib.pcoa_get_grm_subset_stats(self._ctx, ctypes.byref(q), ctypes.sizeof(q)))
        return dict((f[0], getattr(q, f[0])) for f in L.PcoaGrmSubsetStats._fields_)

    # ------------------------------------------------------------------ variant and sample QC on the GRM store
    def grm_set_variant_filters(self, max_missing=1.0, hwe_min_p=0.0):
        """The two variant filters beside the min MAF (pcoa_grm_set_variant_filters): a variant is used only if its missing
        share is at most max_missing (plink --geno; 1 = off) and its Hardy-Weinberg exact-test p-value is at least hwe_min_p
        (plink --hwe; 0 = off).  Properties of the engine like the min MAF: they survive reset() and a grm_subset inherits
        them; other values drop an installed LD mask."""
        self._check(self._lib.pcoa_grm_set_variant_filters(self._ctx, float(max_missing), float(hwe_min_p)))

    def grm_variant_filters(self):
        """(max_missing, hwe_min_p) as set (pcoa_grm_get_variant_filters)."""
        a, b = ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._check(self._lib.pcoa_grm_get_variant_filters(self._ctx, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def grm_hwe(self, first_variant=0, n_variants=None):
        """float64 [n]: the Hardy-Weinberg exact-test p-values of the store's rows (pcoa_grm_hwe; include/pcoa.h states the rule)."""
        if n_variants is None:
            info = self.grm_info()   # (None: not a GRM engine -- the call itself says so)
            n_variants = (info[0] if info else 0) - int(first_variant)
        out = np.zeros(max(int(n_variants), 0), dtype=np.float64)
        self._check(self._lib.pcoa_grm_hwe(self._ctx, int(first_variant), int(n_variants), _ptr(out) if out.size else None))
        return out

    def grm_sample_counts(self, used=False):
        """int64 [N, 3]: the rows of the store at which each sample is called, heterozygous, homozygous non-reference
        (pcoa_grm_sample_counts); used=True: over the rows used under the min MAF, the filters and an installed LD mask."""
        out = np.zeros((self.n, 3), dtype=np.int64)
        self._check(self._lib.pcoa_grm_sample_counts(self._ctx, L.PCOA_GRM_ROWS_USED if used else L.PCOA_GRM_ROWS_ALL, _ptr(out)))
        return out

    def grm_qc_stats(self):
        """pcoa_get_grm_qc_stats: seconds and calls of the HWE kernel and the sample-count launches, and the variants failing
        the MAF, missing and HWE test under the current settings."""
        q = L.PcoaGrmQcStats()
        self._check(self._lib.pcoa_get_grm_qc_stats(self._ctx, ctypes.byref(q), ctypes.sizeof(q)))
        return dict((f[0], getattr(q, f[0])) for f in L.PcoaGrmQcStats._fields_)

    # ------------------------------------------------------------------ per-variant loadings
    def loadings(self, components, eigenvalues=None, centre=True, unit=True):
        """Per-variant loadings of the principal coordinates (pcoa_loadings_begin): `components` [N, k] and `eigenvalues` [k] are
        what compute(k) returned.  centre: use u_c - mean(u_c); unit: divide by sqrt(eigenvalues[c]) -- both on, the rows are
        w_c = X (J u_c) / sqrt(lambda_c), the left singular vectors of X J.  Returns a Loadings object whose .bits / .plink_bed /
        .operator stream rows past the resident vectors; .close() releases them."""
        return Loadings(self, components, eigenvalues, centre, unit)

    # ------------------------------------------------------------------ LD pruning
    def ld_pruner(self, window, r2_max, accumulate=True):
        """LD pruning in front of the accumulation (pcoa_ld_begin): forward and greedy in feed order, a variant is removed when it
        is monomorphic or when a KEPT variant among the `window` fed before it has r^2 of the carrier indicators above r2_max.
        Returns an LdPruner (a context manager) whose .bits / .plink_bed take rows and return their keep mask; with accumulate
        the kept rows also go into this engine's S (or store), without it the pass is a dry run."""
        return LdPruner(self, window, r2_max, accumulate)

    # ------------------------------------------------------------------ computePca
    def center(self, want_matrix=True):
        """Row sums + double-centring (VariantsPca.scala:206-223).  Returns (B, row_sums, nonzero_rows, mean)."""
        b = np.zeros((self.n, self.n), dtype=np.float64) if want_matrix else None
        rs = np.zeros(self.n, dtype=np.float64)
        nz = ctypes.c_int32(0)
        mm = ctypes.c_double(0.0)
        self._check(self._lib.pcoa_center_read_f64(self._ctx, _ptr(b) if want_matrix else None, _ptr(rs),
                                                   ctypes.byref(nz), ctypes.byref(mm)))
        return b, rs, int(nz.value), float(mm.value)

    def compute(self, num_pc=2):
        """computePca (VariantsPca.scala:198-231).  Returns (components [N, k], eigenvalues [k], nonzero_rows)."""
        k = int(num_pc)
        comps = np.zeros((max(k, 1), self.n), dtype=np.float64)  # column-major N x k == row-major k x N
        lam = np.zeros(max(k, 1), dtype=np.float64)
        nz = ctypes.c_int32(0)
        self._check(self._lib.pcoa_compute(self._ctx, k, _ptr(comps), _ptr(lam), ctypes.byref(nz)))
        return np.ascontiguousarray(comps[:k].T), lam[:k].copy(), int(nz.value)

    def project(self, cross, components, eigenvalues):
        """Places the columns of the strip owner `cross` onto this engine's principal coordinates (pcoa_project): `components`
        [N, k] and `eigenvalues` [k] are what compute(k) returned, cross's rows [0, N) are this engine's samples in order.
        Returns the coordinates [cross.cols, k] (the layout of compute's components)."""
        comps = np.asarray(components, dtype=np.float64)
        lam = np.ascontiguousarray(eigenvalues, dtype=np.float64)
        if comps.ndim != 2 or comps.shape[0] != self.n or lam.shape != (comps.shape[1],):
            raise ValueError("components must be [N = %d, k] and eigenvalues [k]" % self.n)
        if not isinstance(cross, PcoaEngine):
            raise TypeError("cross must be a PcoaEngine")
        k = comps.shape[1]
        u = np.ascontiguousarray(comps.T)   # [k][N]: the column-major layout pcoa_compute writes
        out = np.zeros((max(k, 1), cross.cols), dtype=np.float64)
        self._check(self._lib.pcoa_project(self._ctx, cross._ctx, k, _ptr(u), _ptr(lam), _ptr(out)))
        return np.ascontiguousarray(out[:k].T)

    # ------------------------------------------------------------------ instrumentation
    def timings(self):
        t = L.PcoaTimings()
        self._check(self._lib.pcoa_get_timings_sized(self._ctx, ctypes.byref(t), ctypes.sizeof(t)))
        out = dict((f[0], getattr(t, f[0])) for f in L.PcoaTimings._fields_ if not f[0].startswith("reserved"))
        r = L.PcoaReducePeersStats()   # reduce_peers_calls / _seconds / _bytes_in: a struct of their own in pcoa.h
        self._check(self._lib.pcoa_get_reduce_peers_stats(self._ctx, ctypes.byref(r), ctypes.sizeof(r)))
        out.update((f[0], getattr(r, f[0])) for f in L.PcoaReducePeersStats._fields_)
        q = L.PcoaPairsStats()         # pairs_seconds / _bytes / _calls: likewise
        self._check(self._lib.pcoa_get_pairs_stats(self._ctx, ctypes.byref(q), ctypes.sizeof(q)))
        out.update((f[0], getattr(q, f[0])) for f in L.PcoaPairsStats._fields_)
        return out

    def reset_timings(self):
        self._check(self._lib.pcoa_reset_timings(self._ctx))


class Loadings(object):
    """The vectors of one pcoa_loadings_begin, resident on the engine's GPU until close().  Every method returns the loadings
    of its rows as [rows, k]: a numpy array, or with device_out=True a float64 torch tensor on the engine's GPU (complete when
    the method returns)."""

    def __init__(self, engine, components, eigenvalues=None, centre=True, unit=True):
        comps = np.asarray(components, dtype=np.float64)
        if comps.ndim != 2 or comps.shape[0] != engine.n:
            raise ValueError("components must be [N = %d, k]" % engine.n)
        self.k = int(comps.shape[1])
        lam = None
        if eigenvalues is not None:
            lam = np.ascontiguousarray(eigenvalues, dtype=np.float64)
            if lam.shape != (self.k,):
                raise ValueError("eigenvalues must be [k = %d]" % self.k)
        flags = (L.PCOA_LOADINGS_CENTRE if centre else 0) | (L.PCOA_LOADINGS_UNIT if unit else 0)
        u = np.ascontiguousarray(comps.T)   # [k][N]: the column-major layout pcoa_compute writes
        self._eng = engine
        self._open = False
        engine._check(engine._lib.pcoa_loadings_begin(engine._ctx, self.k, _ptr(u), None if lam is None else _ptr(lam), flags))
        self._open = True

    def _out(self, rows, device_out):
        if not device_out:
            out = np.zeros((rows, self.k), dtype=np.float64)
            return out, _ptr(out)
        import torch  # plumbing only: device memory handles
        out = torch.zeros((rows, self.k), dtype=torch.float64, device="cuda:%d" % self._eng.device)
        torch.cuda.current_stream(out.device).synchronize()   # the engine runs on its own stream
        return out, ctypes.c_void_p(out.data_ptr())

    def _done(self, device_in_or_out):
        if device_in_or_out:   # queued work: the tensors are complete / no longer read when sync returns
            self._eng._check(self._eng._lib.pcoa_sync(self._eng._ctx))

    def bits(self, bits, n_variants=None, ld_words=None, device_out=False):
        """Rows of carrier bitsets in accumulate_bits' layout: numpy uint32 [V][W] (host) or a torch int32 CUDA tensor."""
        e = self._eng
        ptr, nv, ldv, dev, _keep = _rows_arg(bits, *_BITS_ROWS)
        nv, ldv = nv if n_variants is None else int(n_variants), ldv if ld_words is None else int(ld_words)
        out, optr = self._out(nv, device_out)
        e._check(e._lib.pcoa_loadings_bits(e._ctx, ptr, nv, ldv, int(dev), optr, int(bool(device_out))))
        self._done(dev or device_out)
        return out

    def plink_bed(self, rows, ref_is_a1=False, device_out=False):
        """Raw variant-major PLINK .bed rows: numpy uint8 [V][row_bytes] (host) or a torch uint8 CUDA tensor."""
        e = self._eng
        ptr, nv, stride, dev, _keep = _rows_arg(rows, *_BED_ROWS)
        out, optr = self._out(nv, device_out)
        e._check(e._lib.pcoa_loadings_plink_bed(e._ctx, ptr, nv, stride, int(bool(ref_is_a1)), int(dev), optr, int(bool(device_out))))
        self._done(dev or device_out)
        return out

    def operator(self, first=0, n=None, device_out=False):
        """Rows [first, first + n) of an operator engine's resident store (n=None: to its end)."""
        e = self._eng
        if n is None:
            info = e.operator_info()
            n = (info[0] if info else 0) - int(first)
        out, optr = self._out(max(int(n), 0), device_out)
        e._check(e._lib.pcoa_loadings_operator(e._ctx, int(first), int(n), optr, int(bool(device_out))))
        self._done(device_out)
        return out

    def stats(self):
        """pcoa_loadings_stats of the engine: loadings_variants, loadings_bytes, loadings_seconds."""
        q = L.PcoaLoadingsStats()
        self._eng._check(self._eng._lib.pcoa_get_loadings_stats(self._eng._ctx, ctypes.byref(q), ctypes.sizeof(q)))
        return dict((f[0], getattr(q, f[0])) for f in L.PcoaLoadingsStats._fields_)

    def close(self):
        if self._open and getattr(self._eng, "_ctx", None):
            self._open = False
            self._eng._check(self._eng._lib.pcoa_loadings_end(self._eng._ctx))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class LdPruner(object):
    """The pruner of one pcoa_ld_begin: the last `window` rows stay on the engine's GPU between calls, so rows may be fed in calls
    of any size.  .bits / .plink_bed return the keep mask of their rows as a numpy bool array."""

    def __init__(self, engine, window, r2_max, accumulate=True):
        self._eng = engine
        self._open = False
        self.window, self.r2_max, self.accumulate = int(window), float(r2_max), bool(accumulate)
        engine._check(engine._lib.pcoa_ld_begin(engine._ctx, self.window, self.r2_max, L.PCOA_LD_ACCUMULATE if accumulate else 0))
        self._open = True

    def _mask(self, rows):
        keep = np.zeros(max(int(rows), 0), dtype=np.uint8)
        return keep, (_ptr(keep) if keep.size else None), ctypes.c_int64(0)

    def bits(self, bits, n_variants=None, ld_words=None):
        """Rows of carrier bitsets in accumulate_bits' layout: numpy uint32 [V][W] (host) or a torch int32 CUDA tensor."""
        e = self._eng
        ptr, nv, ldv, dev, _keep = _rows_arg(bits, *_BITS_ROWS)
        nv, ldv = nv if n_variants is None else int(n_variants), ldv if ld_words is None else int(ld_words)
        keep, kptr, kept = self._mask(nv)
        e._check(e._lib.pcoa_ld_bits(e._ctx, ptr, nv, ldv, int(dev), kptr, ctypes.byref(kept)))
        self.last_kept = int(kept.value)
        return keep.astype(bool)

    def plink_bed(self, rows, ref_is_a1=False):
        """Raw variant-major PLINK .bed rows: numpy uint8 [V][row_bytes] (host) or a torch uint8 CUDA tensor."""
        e = self._eng
        ptr, nv, stride, dev, _keep = _rows_arg(rows, *_BED_ROWS)
        keep, kptr, kept = self._mask(nv)
        e._check(e._lib.pcoa_ld_plink_bed(e._ctx, ptr, nv, stride, int(bool(ref_is_a1)), int(dev), kptr, ctypes.byref(kept)))
        self.last_kept = int(kept.value)
        return keep.astype(bool)

    def break_contig(self):
        """A contig boundary: the next row starts a new window (pcoa_ld_break)."""
        self._eng._check(self._eng._lib.pcoa_ld_break(self._eng._ctx))

    def stats(self):
        """pcoa_ld_stats of the engine: ld_variants, ld_kept, ld_monomorphic, ld_pairs and the seconds of each kernel."""
        q = L.PcoaLdStats()
        self._eng._check(self._eng._lib.pcoa_get_ld_stats(self._eng._ctx, ctypes.byref(q), ctypes.sizeof(q)))
        return dict((f[0], getattr(q, f[0])) for f in L.PcoaLdStats._fields_)

    def close(self):
        if self._open and getattr(self._eng, "_ctx", None):
            self._open = False
            self._eng._check(self._eng._lib.pcoa_ld_end(self._eng._ctx))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---------------------------------------------------------------------------------------------- layout of S (pcoa.h)
LAYOUTS = {"auto": L.PCOA_LAYOUT_AUTO, "full": L.PCOA_LAYOUT_FULL, "strips": L.PCOA_LAYOUT_STRIPS}


def plan_layout(n_samples, n_engines, free_bytes=None, request="auto"):
    """pcoa_plan_layout (no GPU): ("full", None) or ("strips", [(col0, cols), ..] per engine).  free_bytes: the bytes each
    engine may use (engines sharing a device split it, see engine_free_bytes); needed for "auto" only."""
    lib = L.load()
    if request not in LAYOUTS:
        raise ValueError("layout must be auto, full or strips")
    k = int(n_engines)
    fb = None
    if free_bytes is not None:
        fb = np.ascontiguousarray(free_bytes, dtype=np.int64)
        if fb.shape != (k,):
            raise ValueError("free_bytes needs one entry per engine")
    col0 = np.zeros(max(k, 1), dtype=np.int32)
    cols = np.zeros(max(k, 1), dtype=np.int32)
    out = ctypes.c_int32(0)
    rc = lib.pcoa_plan_layout(int(n_samples), k, _ptr(fb) if fb is not None else None, LAYOUTS[request], ctypes.byref(out),
                              _ptr(col0), _ptr(cols))
    if rc != L.PCOA_OK:
        raise PcoaError(rc, lib.pcoa_last_error(None).decode(errors="replace"))
    if out.value == L.PCOA_LAYOUT_FULL:
        return "full", None
    return "strips", [(int(a), int(b)) for a, b in zip(col0[:k], cols[:k])]


def device_memory(device):
    """(free, total) bytes of a device (pcoa_device_memory: hipMemGetInfo)."""
    lib = L.load()
    fr, tot = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = lib.pcoa_device_memory(int(device), ctypes.byref(fr), ctypes.byref(tot))
    if rc != L.PCOA_OK:
        raise PcoaError(rc, lib.pcoa_last_error(None).decode(errors="replace"))
    return int(fr.value), int(tot.value)


def engine_free_bytes(device_of_engine, free_of_device):
    """The free_bytes of plan_layout: engine g gets the free bytes of its device divided by the engines on that device."""
    devs = [int(d) for d in device_of_engine]
    return [int(free_of_device(d)) // devs.count(d) for d in devs]


def compute_strips(owners, num_pc=2):
    """computePca over the strip owners of this process (pcoa_compute_strips): `owners` are PcoaEngine(strip=...) whose ranges
    tile [0, N) in list order; they may share a device.  Returns (components [N, k], eigenvalues [k], nonzero_rows) as
    PcoaEngine.compute does."""
    if not owners:
        raise ValueError("no strip owners")
    lead = owners[0]
    n, k = lead.n, int(num_pc)
    arr = (ctypes.c_void_p * len(owners))(*[o._ctx.value for o in owners])
    comps = np.zeros((max(k, 1), n), dtype=np.float64)
    lam = np.zeros(max(k, 1), dtype=np.float64)
    nz = ctypes.c_int32(0)
    lead._check(lead._lib.pcoa_compute_strips(arr, len(owners), k, _ptr(comps), _ptr(lam), ctypes.byref(nz)))
    return np.ascontiguousarray(comps[:k].T), lam[:k].copy(), int(nz.value)


def reduce_peers(engines, root_only=False):
    """S of every engine := the sum over `engines` (pcoa_gram_reduce_peers): a reduce-scatter + all-gather over the engines'
    own matrices, nothing staged.  The engines are full engines of this process over the same samples; they may share a device.
    root_only: engines[0] holds the total and every other engine comes back reset.  Errors are raised from engines[0]."""
    lib = L.load()
    engines = list(engines)
    if not engines:
        raise ValueError("no engines")
    arr = (ctypes.c_void_p * len(engines))(*[e._ctx.value if e._ctx else None for e in engines])
    rc = lib.pcoa_gram_reduce_peers(arr, len(engines), int(bool(root_only)))
    if rc != L.PCOA_OK:
        lead = engines[0]
        msg = lib.pcoa_last_error(lead._ctx if lead._ctx else None)
        raise PcoaError(rc, msg.decode(errors="replace") if msg else "")
