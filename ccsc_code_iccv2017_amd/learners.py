"""Python mirror of the reference learners' interface over the libccsc C-ABI.

Same names, argument order, argument meaning and return tuples as the MATLAB
functions they replace (what a MEX wrapper would expose):

  d_res, z_res, DZ, iterations = admm_learn_conv2D_large_dParallel(
      b, kernel_size, lambda_residual, lambda_prior, max_it, tol, verbose, init)
                                   # 2D/admm_learn_conv2D_large_dParallel.m:1-4
  d_res, z_res, DZ, iterations = admm_learn_conv2D_large_dzParallel(...)
                                   # 2D/admm_learn_conv2D_large_dzParallel.m:1-4
  d_res, z_res, DZ, obj_val, iterations = admm_learn_conv3D_large(...)      # 3D/...:1-4
  d_res, z_res, DZ, obj_val, iterations = admm_learn_conv4D_lightfield(...) # 4D/...:1-4
  d_res, z_res, Dz, obj_val = admm_learn(b, kernel_size, lambda_residual, lambda_prior,
      max_it, tol, verbose, init, smooth_init)   # 2-3D/DictionaryLearning/admm_learn.m:1-4

Arrays carry the MATLAB shapes (b: [x, y, n]; kernel_size = [psf, psf, K];
d_res: [psf, psf, K]; z_res: [X, Y, K, n]; DZ: [X, Y, 1, n]) and are exchanged
column-major, so a Fortran-ordered NumPy array is bit-for-bit an mxArray.

``init`` (ignored by the reference, Q11) is honoured: ``{'d': [psf,psf,K],
'z': size_z}`` (dZ: ``size_z_crop`` = [X, Y, K, ni], replicated per block).
With ``init=None`` the engine draws d0/z0 on the device from ``seed``.

The five learners take ``sparse_z=eps``: the z_res position of the return then holds the
compressed sparse column tuple ``(jc, ir, pr, (M, n))`` of ``Session.codes_sparse(eps)``
-- the entries with ``not (abs(z) <= eps)``, thresholded on the GPU -- and the dense z
(97 GB at 10^4 patches) is never allocated.  This runs through a ``Session``, so a
device-list context raises ``CCSCError`` (sessions run on a one-device context).
``synthesize(d_res, codes, grid)`` reconstructs ``sum_k d_k (*) z_k`` from such a tuple on
the GPU and ``densify(codes)`` expands it; ``sparsify`` makes one from any dense matrix.
``threshold_sweep(d_res, codes, b, eps_list, grid)`` (``Session.threshold_sweep``) returns,
per candidate threshold and patch, the surviving entries, their l1 mass and the squared error
of the reconstruction against ``b`` in one pass; ``pick_eps`` chooses among them.

Errors are raised as ``CCSCError`` (the MATLAB reference raises on bad shapes
too; ``n % ni != 0`` is an error here rather than a silent floor, Q13).
"""
from __future__ import annotations

import ctypes as C
import os
import math

import numpy as np

from . import _lib as L


class Context:
    """One GPU (one rank).  ``uid`` (128 bytes from ``unique_id()`` on rank 0)
    is needed when ``nranks > 1``; the consensus then runs over RCCL.

    ``host_comm(op, array) -> None`` instead selects the host-staged transport
    (op 0: in-place sum all-reduce, op 1: in-place broadcast from rank 0), e.g.
    torch.distributed over gloo: used by the multi-rank GPU tests, which share
    one GPU between ranks."""

    def __init__(self, device: int = 0, rank: int = 0, nranks: int = 1, uid: bytes | None = None,
                 host_comm=None):
        self._lib = L.lib()
        eb = L.errbuf()
        if host_comm is not None:
            def _fn(user, op, buf, count):
                try:
                    arr = np.ctypeslib.as_array(buf, shape=(count,))
                    host_comm(op, arr)
                    return 0
                except Exception:  # noqa: BLE001 -- reported to the engine as a status
                    return 1
            self._cfn = L.COMM_FN(_fn)   # keep the trampoline alive
            self.ptr = self._lib.ccsc_create_hostcomm(device, rank, nranks, self._cfn, None, eb,
                                                      len(eb))
        else:
            self.ptr = self._lib.ccsc_create(device, rank, nranks, uid, eb, len(eb))
        if not self.ptr:
            raise L.CCSCError(L.CCSC_E_HIP, eb.value.decode(errors="replace"))
        self.device, self.rank, self.nranks = device, rank, nranks

    @classmethod
    def multi(cls, devices):
        """Single-process multi-device context (ccsc_create_multi): the learners then take
        the WHOLE problem and run rank i on devices[i] in its own host thread -- the
        drop-in path of one MATLAB call over a node's GPUs.  A repeated device ({0, 0})
        exchanges through host memory (one-GPU testing); distinct devices use RCCL."""
        self = cls.__new__(cls)
        self._lib = L.lib()
        eb = L.errbuf()
        devs = (C.c_int32 * len(devices))(*devices)
        self.ptr = self._lib.ccsc_create_multi(devs, len(devices), eb, len(eb))
        if not self.ptr:
            raise L.CCSCError(L.CCSC_E_HIP, eb.value.decode(errors="replace"))
        self.device, self.rank, self.nranks = devices[0], 0, 1
        self.devices = list(devices)
        # ccsc_create_multi builds a rank group for several devices, and for one under the
        # test hook CCSC_TEST_RCCL_SELF=1 (a 1-rank RCCL communicator); such a context
        # serves ccsc_learn only, not sessions
        selftest = os.environ.get("CCSC_TEST_RCCL_SELF", "0").strip()
        self._group = len(devices) > 1 or (selftest.isdigit() and int(selftest) != 0)
        return self

    @property
    def group(self):
        return getattr(self, "_group", False)

    def comm_ranks(self):
        """(ranks, transport) of the context's communicator (ccsc_comm_ranks): RCCL
        reports ncclCommCount, "host" the host-staged transport, "none" one rank."""
        eb = L.errbuf()
        n, t = C.c_int32(0), C.c_int32(0)
        L.check(self._lib.ccsc_comm_ranks(self.ptr, C.byref(n), C.byref(t), eb, len(eb)), eb)
        return n.value, L.TRANSPORT[t.value]

    def close(self):
        if self.ptr:
            self._lib.ccsc_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def unique_id() -> bytes:
    eb = L.errbuf()
    buf = C.create_string_buffer(128)
    L.check(L.lib().ccsc_get_unique_id(buf, eb, len(eb)), eb)
    return buf.raw


_VARIANT_FOR = {
    "dParallel": L.CCSC_DPAR,
    "dzParallel": L.CCSC_DZPAR,
}


def make_problem(variant, b_shape, kernel_size, lambda_residual, lambda_prior, max_it, tol,
                 verbose, *, ni=None, max_it_d=None, max_it_z=None, rho_d=None, rho_z=None,
                 theta_div=None, trace_objective=False, seed=0, precision="fp64",
                 dfactor="auto"):
    p = L.Problem()
    p.variant = variant
    p.ndim = 3 if variant == L.CCSC_L3D else 2
    p.sb[0], p.sb[1] = int(b_shape[0]), int(b_shape[1])
    if variant == L.CCSC_L3D:
        p.sb[2] = int(b_shape[2])
    p.views[0] = p.views[1] = 1
    if variant == L.CCSC_L4D and len(kernel_size) == 5:   # b: [x, y, U, V, n]; kernel [s, s, U, V, K]
        p.views[0], p.views[1] = int(kernel_size[2]), int(kernel_size[3])
    if variant == L.CCSC_HS23:                            # b: [x, y, W, n]; kernel [s, s, W, K]
        p.views[0] = int(kernel_size[2])
    p.n = int(b_shape[-1])
    p.K = int(kernel_size[-1])
    p.psf = int(kernel_size[0])
    p.lambda_residual = float(lambda_residual)
    p.lambda_prior = float(lambda_prior)
    p.max_it = int(max_it)
    p.tol = float(tol)
    if verbose not in L.VERBOSE:
        raise ValueError(f"verbose must be one of {sorted(L.VERBOSE)}")
    p.verbose = L.VERBOSE[verbose]
    p.ni = int(ni or 0)
    p.max_it_d = int(max_it_d or 0)
    p.max_it_z = int(max_it_z or 0)
    p.rho_d = float(rho_d or 0)
    p.rho_z = float(rho_z or 0)
    p.theta_div = float(theta_div or 0)
    if precision != "fp64":
        raise ValueError("precision must be 'fp64' (the reference computes in double)")
    p.precision = L.CCSC_FP64
    p.trace_objective = 1 if trace_objective else 0
    p.seed = int(seed)
    if dfactor not in L.DFACTOR:
        raise ValueError(f"dfactor must be one of {sorted(L.DFACTOR)}")
    p.dfactor = L.DFACTOR[dfactor]
    return p


def resolve(p: L.Problem) -> L.Problem:
    """Fill the variant defaults and validate; host only."""
    q = L.Problem.from_buffer_copy(p)
    eb = L.errbuf()
    L.check(L.lib().ccsc_resolve(C.byref(q), eb, len(eb)), eb)
    return q


def shard(p: L.Problem, rank: int, nranks: int):
    eb = L.errbuf()
    b0, nb = C.c_int64(), C.c_int64()
    L.check(L.lib().ccsc_shard(C.byref(p), rank, nranks, C.byref(b0), C.byref(nb), eb, len(eb)), eb)
    return b0.value, nb.value


def plan_bytes(p: L.Problem, rank: int = 0, nranks: int = 1) -> int:
    eb = L.errbuf()
    out = C.c_uint64()
    L.check(L.lib().ccsc_plan_bytes(C.byref(p), rank, nranks, C.byref(out), eb, len(eb)), eb)
    return out.value


def _f64(a):
    return None if a is None else np.asfortranarray(np.asarray(a, dtype=np.float64))


class Session:
    """Stateful learner (warm restart, bench): create -> step(k) -> results.
    The 2-3D learner (variant CCSC_HS23) also takes ``smooth_init``."""

    def __init__(self, ctx: Context, p: L.Problem, b, d0=None, z0=None, smooth_init=None):
        self.ctx = ctx
        self.p = resolve(p)
        eb = L.errbuf()
        L.check(L.lib().ccsc_supported(C.byref(self.p), eb, len(eb)), eb)   # CCSC_E_UNSUPPORTED
        self._b = _f64(b)
        self._d0 = _f64(d0)
        self._z0 = _f64(z0)
        eb = L.errbuf()
        if self.p.variant == L.CCSC_HS23:
            if smooth_init is None:
                raise ValueError("the 2-3D learner needs smooth_init (admm_learn.m:4)")
            self._sm = _f64(smooth_init)
            if self._sm.shape != self._b.shape:
                raise ValueError("smooth_init must have the shape of b")
            self.ptr = L.lib().ccsc_session_create_hs23(
                ctx.ptr, C.byref(self.p), L.dptr(self._b), L.dptr(self._sm), L.dptr(self._d0),
                L.dptr(self._z0), eb, len(eb))
        else:
            self.ptr = L.lib().ccsc_session_create(ctx.ptr, C.byref(self.p), L.dptr(self._b),
                                                   L.dptr(self._d0), L.dptr(self._z0), eb,
                                                   len(eb))
        if not self.ptr:
            raise L.CCSCError(L.CCSC_E_INVALID, eb.value.decode(errors="replace"))
        b0, nb = shard(self.p, ctx.rank, ctx.nranks)
        self.block_begin, self.nblocks = b0, nb
        # (the 2-3D learner's shards are runs of images: ccsc_shard counts images for it)
        self.n_local = nb if self.p.variant == L.CCSC_HS23 else nb * self.p.ni
        self.outer = 0

    def step(self, n_outer: int = 1) -> bool:
        eb = L.errbuf()
        done = C.c_int32(0)
        L.check(L.lib().ccsc_session_step(self.ptr, n_outer, C.byref(done), eb, len(eb)), eb)
        self.outer += n_outer
        return bool(done.value)

    def objective(self) -> float:
        eb = L.errbuf()
        v = C.c_double()
        L.check(L.lib().ccsc_session_objective(self.ptr, C.byref(v), eb, len(eb)), eb)
        return v.value

    def set_profiling(self, on: bool):
        L.check(L.lib().ccsc_session_set_profiling(self.ptr, 1 if on else 0), L.errbuf())

    def kernel_stats(self, kernel_id: int):
        eb = L.errbuf()
        n = C.c_int64()
        ms = C.c_double()
        by = C.c_double()
        L.check(L.lib().ccsc_session_kernel_stats(self.ptr, kernel_id, C.byref(n), C.byref(ms),
                                                  C.byref(by), eb, len(eb)), eb)
        return n.value, ms.value, by.value

    def grid(self):
        r = self.p.psf // 2
        g = (self.p.sb[0] + 2 * r, self.p.sb[1] + 2 * r)
        if self.p.variant == L.CCSC_L3D:
            g += (self.p.sb[2] + 2 * r,)
        return g

    def results(self, want_z=True, want_DZ=True, want_obj=False):
        p = self.p
        if p.variant == L.CCSC_L3D:
            X, Y, T = self.grid()
            d_res = np.zeros((p.psf, p.psf, p.psf, p.K), order="F")
            z_res = np.zeros((X, Y, T, p.K, self.n_local), order="F") if want_z else None
            DZ = np.zeros((X, Y, T, self.n_local), order="F") if want_DZ else None
            obj = np.zeros(1) if want_obj else None
            out = L.Outputs(L.dptr(d_res), L.dptr(z_res), L.dptr(DZ), L.dptr(obj))
            eb = L.errbuf()
            L.check(L.lib().ccsc_session_results(self.ptr, C.byref(out), eb, len(eb)), eb)
            return d_res, z_res, DZ, (float(obj[0]) if want_obj else None)
        X, Y = self.grid()
        if p.variant == L.CCSC_HS23:
            W = p.views[0]
            d_res = np.zeros((p.psf, p.psf, W, p.K), order="F")
            z_res = np.zeros((X, Y, p.K, self.n_local), order="F") if want_z else None
            DZ = np.zeros((X, Y, W, self.n_local), order="F") if want_DZ else None
        elif p.variant == L.CCSC_L4D:
            U, V = p.views[0], p.views[1]
            d_res = np.zeros((p.psf, p.psf, U, V, p.K), order="F")
            z_res = np.zeros((X, Y, 1, 1, p.K, self.n_local), order="F") if want_z else None
            DZ = (np.zeros((p.sb[0], p.sb[1], U, V, self.n_local), order="F")
                  if want_DZ else None)
        else:
            d_res = np.zeros((p.psf, p.psf, p.K), order="F")
            z_res = np.zeros((X, Y, p.K, self.n_local), order="F") if want_z else None
            DZ = np.zeros((X, Y, 1, self.n_local), order="F") if want_DZ else None
        obj = np.zeros(1) if want_obj else None
        out = L.Outputs(L.dptr(d_res), L.dptr(z_res), L.dptr(DZ), L.dptr(obj))
        eb = L.errbuf()
        L.check(L.lib().ccsc_session_results(self.ptr, C.byref(out), eb, len(eb)), eb)
        return d_res, z_res, DZ, (float(obj[0]) if want_obj else None)

    def codes_sparse(self, eps, as_scipy=False):
        """The codes as a compressed sparse column matrix, thresholded on the GPU: one column
        per local patch (2-3D: image) with M = X Y (T) K rows, the row index being the
        column-major index into that patch's slice of ``results()``'s z_res; an entry is kept
        iff ``not (abs(z) <= eps)`` (a NaN is kept).  Returns ``(jc, ir, pr, (M, n_local))``,
        int64 / int64 / float64, 0-based, or with ``as_scipy`` a scipy.sparse.csc_matrix
        (SciPy is imported here, not by the package).  The dense array is never formed on
        the host; the session is left as ``results(want_z=True)`` leaves it."""
        eps = float(eps)
        lib = L.lib()
        eb = L.errbuf()
        jc = np.zeros(self.n_local + 1, dtype=np.int64)
        M, n = C.c_int64(0), C.c_int64(0)
        L.check(lib.ccsc_session_codes_count(self.ptr, eps, L.lptr(jc), C.byref(M), C.byref(n),
                                             eb, len(eb)), eb)
        nnz = int(jc[-1])
        ir = np.empty(nnz, dtype=np.int64)
        pr = np.empty(nnz, dtype=np.float64)
        eb = L.errbuf()
        L.check(lib.ccsc_session_codes_fill(self.ptr, eps, L.lptr(ir), L.dptr(pr), nnz, eb,
                                            len(eb)), eb)
        shape = (M.value, n.value)
        if as_scipy:
            from scipy.sparse import csc_matrix
            return csc_matrix((pr, ir, jc), shape=shape)
        return jc, ir, pr, shape

    def data(self):
        """The local patches' data as the objective compares it with Dz: the interior-cropped
        ``b`` of this rank's columns (2-3D: ``b - smooth_init``), Fortran-ordered."""
        j0 = self.block_begin * (1 if self.p.variant == L.CCSC_HS23 else self.p.ni)
        sl = (Ellipsis, slice(j0, j0 + self.n_local))
        b = self._b[sl] - self._sm[sl] if self.p.variant == L.CCSC_HS23 else self._b[sl]
        return np.asfortranarray(b)

    def threshold_sweep(self, eps):
        """``threshold_sweep`` of the session's own filters, codes and data: ``results()``'s
        d_res, ``codes_sparse(min(eps))`` (so every threshold is >= 0) and ``data()``, the
        views of the 4D learner and the bands of the 2-3D learner as channels.  Returns the
        dict of ``learners.threshold_sweep`` with ``[E, n_local]`` NumPy arrays; the session
        is left as ``results(want_z=True)`` leaves it."""
        ev = np.atleast_1d(np.asarray(eps, dtype=np.float64))
        if ev.ndim != 1 or ev.size < 1:
            raise ValueError("eps is one threshold or a non-empty vector of them")
        if np.isnan(ev).any():
            raise ValueError("a threshold is NaN")
        d_res = self.results(want_z=False, want_DZ=False)[0]
        codes = self.codes_sparse(float(ev.min()))
        grid = self.grid()
        return threshold_sweep(d_res, codes, self.data(), ev, grid, spatial_dims=len(grid),
                               ctx=self.ctx)

    def iterlog(self, capacity=None):
        p = self.p
        cap = capacity or (self.outer + 1)
        a = {k: np.full(cap, np.nan) for k in ("obj_vals_d", "obj_vals_z", "tim_vals")}
        tr = {
            "obj_d": np.full(cap * p.max_it_d, np.nan),
            "obj_z": np.full(cap * p.max_it_z, np.nan),
            "d_diff": np.full(cap * p.max_it_d, np.nan),
            "z_diff": np.full(cap * p.max_it_z, np.nan),
        }
        nd = np.zeros(cap, dtype=np.int32)
        nz = np.zeros(cap, dtype=np.int32)
        fl = np.zeros(cap, dtype=np.int32)
        lg = L.IterLog(cap, 0, L.dptr(a["obj_vals_d"]), L.dptr(a["obj_vals_z"]),
                       L.dptr(a["tim_vals"]), L.dptr(tr["obj_d"]), L.dptr(tr["obj_z"]),
                       L.dptr(tr["d_diff"]), L.dptr(tr["z_diff"]), L.iptr(nd), L.iptr(nz),
                       L.iptr(fl))
        eb = L.errbuf()
        L.check(L.lib().ccsc_session_iterlog(self.ptr, C.byref(lg), eb, len(eb)), eb)
        cnt = lg.count
        it = {k: v[:cnt].copy() for k, v in a.items()}
        nout = max(cnt - 1, 0)
        it["trace"] = {
            "obj_d": tr["obj_d"][: nout * p.max_it_d].reshape(nout, p.max_it_d),
            "obj_z": tr["obj_z"][: nout * p.max_it_z].reshape(nout, p.max_it_z),
            "d_diff": tr["d_diff"][: nout * p.max_it_d].reshape(nout, p.max_it_d),
            "z_diff": tr["z_diff"][: nout * p.max_it_z].reshape(nout, p.max_it_z),
            "n_d": nd[:nout].copy(),
            "n_z": nz[:nout].copy(),
            "flags": fl[:nout].copy(),
        }
        return it

    def close(self):
        if self.ptr:
            L.lib().ccsc_session_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sparsify(a, eps, ctx=None):
    """Threshold-and-compact a dense matrix on the GPU (csrc/codes.hip): the entries with
    ``not (abs(a) <= eps)`` of the 2-D float64 ``a`` as the compressed sparse column triple
    ``(jc, ir, pr, a.shape)`` -- int64 / int64 / float64, 0-based, rows ascending inside a
    column, values bit for bit (what scipy.sparse.csc_matrix((pr, ir, jc), shape) takes).  A
    NumPy array goes through ccsc_sparsify_count / _fill and NumPy arrays come back; a CUDA
    tensor goes through the _dev forms and everything stays on its device.  ``ctx``: a
    one-device Context (default: a temporary one on the tensor's / the current device)."""
    eps = float(eps)
    lib = L.lib()
    if a.ndim != 2:
        raise ValueError("sparsify takes a 2-D matrix [M, n]")
    M, n = int(a.shape[0]), int(a.shape[1])
    if hasattr(a, "is_cuda"):
        import torch
        if not a.is_cuda:
            raise ValueError("sparsify takes a NumPy array or a CUDA tensor")
        x = a.to(torch.float64).t().contiguous()        # [n, M] row-major = [M, n] column-major
        dev = a.device.index if a.device.index is not None else torch.cuda.current_device()
        jc = torch.empty(n + 1, dtype=torch.int64, device=a.device)
        own = ctx is None
        if own:
            ctx = Context(dev)
        try:
            torch.cuda.synchronize(a.device)
            eb = L.errbuf()
            L.check(lib.ccsc_sparsify_count_dev(ctx.ptr, x.data_ptr(), M, n, eps, jc.data_ptr(),
                                                eb, len(eb)), eb)
            nnz = int(jc[-1].item())
            ir = torch.empty(nnz, dtype=torch.int64, device=a.device)
            pr = torch.empty(nnz, dtype=torch.float64, device=a.device)
            eb = L.errbuf()
            L.check(lib.ccsc_sparsify_fill_dev(ctx.ptr, x.data_ptr(), M, n, eps, ir.data_ptr(),
                                               pr.data_ptr(), nnz, eb, len(eb)), eb)
        finally:
            if own:
                ctx.close()
        return jc, ir, pr, (M, n)
    x = np.asfortranarray(a, dtype=np.float64)
    jc = np.zeros(n + 1, dtype=np.int64)
    own = ctx is None
    if own:
        import torch
        ctx = Context(torch.cuda.current_device())
    try:
        eb = L.errbuf()
        L.check(lib.ccsc_sparsify_count(ctx.ptr, L.dptr(x), M, n, eps, L.lptr(jc), eb, len(eb)), eb)
        nnz = int(jc[-1])
        ir = np.empty(nnz, dtype=np.int64)
        pr = np.empty(nnz, dtype=np.float64)
        eb = L.errbuf()
        L.check(lib.ccsc_sparsify_fill(ctx.ptr, L.dptr(x), M, n, eps, L.lptr(ir), L.dptr(pr), nnz,
                                       eb, len(eb)), eb)
    finally:
        if own:
            ctx.close()
    return jc, ir, pr, (M, n)


def _codes_triple(codes):
    """``(jc, ir, pr, (M, n), on_device)`` of the 4-tuple of ``codes_sparse`` / ``sparsify``
    or of a scipy.sparse matrix (SciPy is imported only for the latter)."""
    if isinstance(codes, (tuple, list)):
        if len(codes) != 4:
            raise ValueError("codes is the tuple (jc, ir, pr, (M, n)) or a scipy.sparse matrix")
        jc, ir, pr, shape = codes
    else:
        from scipy.sparse import csc_matrix
        m = csc_matrix(codes)
        jc, ir, pr, shape = m.indptr, m.indices, m.data, m.shape
    M, n = int(shape[0]), int(shape[1])
    dev = [hasattr(a, "is_cuda") for a in (jc, ir, pr)]
    if any(dev):
        import torch
        if not all(dev) or not all(a.is_cuda for a in (jc, ir, pr)):
            raise ValueError("jc, ir and pr are all NumPy arrays or all CUDA tensors")
        jc, ir = jc.to(torch.int64).contiguous(), ir.to(torch.int64).contiguous()
        pr = pr.to(torch.float64).contiguous()
    else:
        jc = np.ascontiguousarray(jc, dtype=np.int64)
        ir = np.ascontiguousarray(ir, dtype=np.int64)
        pr = np.ascontiguousarray(pr, dtype=np.float64)
    if jc.ndim != 1 or jc.shape[0] != n + 1 or ir.ndim != 1 or ir.shape != pr.shape:
        raise ValueError("jc has n + 1 entries; ir and pr are vectors of one length")
    return jc, ir, pr, (M, n), any(dev)


def synthesize(d, codes, grid, spatial_dims=2, crop=False, ctx=None):
    """Reconstructions from sparse codes on the GPU (csrc/synth_codes.hip): the circular
    convolutions ``sum_k d_k (*) z_k`` of every column of ``codes``, with the filters embedded
    as the learners embed them (``circshift(padarray(d), -r)``).

    ``d``: the learners' ``d_res``, ``[s, s, (s), channels..., K]``; ``codes``: the tuple
    ``(jc, ir, pr, (M, n))`` of ``Session.codes_sparse`` / ``sparsify`` or a
    scipy.sparse.csc_matrix, ``M = prod(grid) * K``; ``grid``: the ``spatial_dims`` (2 or 3)
    extents the codes live on (``Session.grid()``).  Returns ``grid + d.shape[spatial_dims:-1]
    + (n,)``; ``crop=True`` returns the interior ``[r : g - r]`` of every spatial axis -- the
    4D learner's DZ, every objective's Dz.  NumPy codes go through ccsc_synthesize and a
    Fortran-ordered NumPy array comes back; CUDA tensors go through ccsc_synthesize_dev and
    everything stays on the device.  Each output element is one fma per contributing entry in
    storage order: the result is bitwise reproducible and independent of the other columns.
    ``ctx``: a one-device Context (default: a temporary one)."""
    lib = L.lib()
    jc, ir, pr, (M, n), on_dev = _codes_triple(codes)
    if spatial_dims not in (2, 3) or len(grid) != spatial_dims:
        raise ValueError("grid has spatial_dims (2 or 3) extents")
    if d.ndim < spatial_dims + 1:
        raise ValueError("d is [s, s, (s), channels..., K]")
    dshape = tuple(int(v) for v in d.shape)
    sp, chan, K = dshape[:spatial_dims], dshape[spatial_dims:-1], dshape[-1]
    Cn = int(np.prod(chan, dtype=np.int64)) if chan else 1
    g3 = tuple(int(v) for v in grid) + (1,) * (3 - spatial_dims)
    ks3 = sp + (1,) * (3 - spatial_dims)
    if M != g3[0] * g3[1] * g3[2] * K:
        raise ValueError(f"codes have {M} rows; grid {tuple(grid)} with K = {K} has "
                         f"{g3[0] * g3[1] * g3[2] * K}")
    g_c, ks_c = (C.c_int32 * 3)(*g3), (C.c_int32 * 3)(*ks3)
    nnz = int(ir.shape[0])
    oshape = tuple(int(v) for v in grid) + chan + (n,)
    own = ctx is None
    eb = L.errbuf()
    if on_dev:
        import torch
        device = pr.device
        dt = d if hasattr(d, "is_cuda") else torch.from_numpy(np.asarray(d, dtype=np.float64))
        dt = dt.to(device=device, dtype=torch.float64)
        dcol = dt.permute(*reversed(range(dt.ndim))).contiguous()    # column-major memory
        out = torch.empty(tuple(reversed(oshape)), dtype=torch.float64, device=device)
        if own:
            ctx = Context(device.index if device.index is not None
                          else torch.cuda.current_device())
        try:
            torch.cuda.synchronize(device)
            L.check(lib.ccsc_synthesize_dev(ctx.ptr, dcol.data_ptr(), ks_c, Cn, K, g_c,
                                            jc.data_ptr(), ir.data_ptr(), pr.data_ptr(), n, nnz,
                                            out.data_ptr(), eb, len(eb)), eb)
        finally:
            if own:
                ctx.close()
        out = out.permute(*reversed(range(out.ndim)))
    else:
        dh = np.asfortranarray(d, dtype=np.float64)
        out = np.zeros(oshape, order="F")
        if own:
            import torch
            ctx = Context(torch.cuda.current_device())
        try:
            L.check(lib.ccsc_synthesize(ctx.ptr, L.dptr(dh), ks_c, Cn, K, g_c, L.lptr(jc),
                                        L.lptr(ir), L.dptr(pr), n, nnz, L.dptr(out), eb, len(eb)),
                    eb)
        finally:
            if own:
                ctx.close()
    if crop:
        out = out[tuple(slice(s // 2, gg - s // 2) for s, gg in zip(sp, grid))]
    return out


def threshold_sweep(d, codes, b, eps, grid, spatial_dims=2, ctx=None):
    """Sweep candidate thresholds over sparse codes against the data in one pass on the GPU
    (csrc/sweep_codes.hip): for every ``eps[e]`` and column ``j``, the number of entries with
    ``not (abs(v) <= eps[e])``, their l1 mass, and ``sum (b - R_e)**2`` where ``R_e`` is what
    ``synthesize`` gives for those entries alone (never stored).

    ``d``, ``codes``, ``grid``, ``spatial_dims``: as for ``synthesize``.  ``b``: the data,
    ``grid + channels + (n,)`` (everything is compared) or the interior
    ``[g - 2 r ...] + channels + (n,)`` (what ``synthesize(crop=True)`` returns; the learners'
    ``b``); any other shape is a ``ValueError``.  ``eps``: one or more thresholds, any order.
    Returns ``{"eps", "nnz", "l1", "sse"}``: ``eps`` as given (float64, NumPy), the others
    ``[E, n]`` (int64, float64, float64).  NumPy codes go through ccsc_threshold_sweep and NumPy
    arrays come back; CUDA tensors go through ccsc_threshold_sweep_dev and the three arrays
    stay on the device.  Every result is bitwise reproducible and independent of the other
    columns and thresholds of the call.  ``ctx``: a one-device Context (default: a temporary
    one)."""
    lib = L.lib()
    jc, ir, pr, (M, n), on_dev = _codes_triple(codes)
    if spatial_dims not in (2, 3) or len(grid) != spatial_dims:
        raise ValueError("grid has spatial_dims (2 or 3) extents")
    if d.ndim < spatial_dims + 1:
        raise ValueError("d is [s, s, (s), channels..., K]")
    dshape = tuple(int(v) for v in d.shape)
    sp, chan, K = dshape[:spatial_dims], dshape[spatial_dims:-1], dshape[-1]
    Cn = int(np.prod(chan, dtype=np.int64)) if chan else 1
    grid = tuple(int(v) for v in grid)
    g3 = grid + (1,) * (3 - spatial_dims)
    ks3 = sp + (1,) * (3 - spatial_dims)
    if M != g3[0] * g3[1] * g3[2] * K:
        raise ValueError(f"codes have {M} rows; grid {grid} with K = {K} has "
                         f"{g3[0] * g3[1] * g3[2] * K}")
    full = grid + chan + (n,)
    inner = tuple(gg - 2 * (s // 2) for s, gg in zip(sp, grid)) + chan + (n,)
    bshape = tuple(int(v) for v in b.shape)
    if bshape == full:          # (the same region when every ks is 1)
        crop = 0
    elif bshape == inner:
        crop = 1
    else:
        raise ValueError(f"b has shape {bshape}; the grid with its channels and columns is "
                         f"{full}, its interior {inner}")
    ev = np.ascontiguousarray(np.atleast_1d(np.asarray(eps, dtype=np.float64)))
    if ev.ndim != 1 or ev.size < 1:
        raise ValueError("eps is one threshold or a non-empty vector of them")
    E = int(ev.size)
    g_c, ks_c = (C.c_int32 * 3)(*g3), (C.c_int32 * 3)(*ks3)
    nnz = int(ir.shape[0])
    own = ctx is None
    eb = L.errbuf()
    if on_dev:
        import torch
        device = pr.device
        dt = d if hasattr(d, "is_cuda") else torch.from_numpy(np.asarray(d, dtype=np.float64))
        dt = dt.to(device=device, dtype=torch.float64)
        dcol = dt.permute(*reversed(range(dt.ndim))).contiguous()    # column-major memory
        bt = b if hasattr(b, "is_cuda") else torch.from_numpy(np.asarray(b, dtype=np.float64))
        bt = bt.to(device=device, dtype=torch.float64)
        bcol = bt.permute(*reversed(range(bt.ndim))).contiguous()
        cnt = torch.zeros((n, E), dtype=torch.int64, device=device)   # [E, n], e fastest
        l1 = torch.zeros((n, E), dtype=torch.float64, device=device)
        sse = torch.zeros((n, E), dtype=torch.float64, device=device)
        if own:
            ctx = Context(device.index if device.index is not None
                          else torch.cuda.current_device())
        try:
            torch.cuda.synchronize(device)
            L.check(lib.ccsc_threshold_sweep_dev(
                ctx.ptr, dcol.data_ptr(), ks_c, Cn, K, g_c, jc.data_ptr(), ir.data_ptr(),
                pr.data_ptr(), n, nnz, bcol.data_ptr(), crop, L.dptr(ev), E, cnt.data_ptr(),
                l1.data_ptr(), sse.data_ptr(), eb, len(eb)), eb)
        finally:
            if own:
                ctx.close()
        return {"eps": ev, "nnz": cnt.t(), "l1": l1.t(), "sse": sse.t()}
    dh = np.asfortranarray(d, dtype=np.float64)
    bh = np.asfortranarray(b.cpu().numpy() if hasattr(b, "is_cuda") else b, dtype=np.float64)
    cnt = np.zeros((E, n), dtype=np.int64, order="F")
    l1 = np.zeros((E, n), order="F")
    sse = np.zeros((E, n), order="F")
    if own:
        import torch
        ctx = Context(torch.cuda.current_device())
    try:
        L.check(lib.ccsc_threshold_sweep(
            ctx.ptr, L.dptr(dh), ks_c, Cn, K, g_c, L.lptr(jc), L.lptr(ir), L.dptr(pr), n, nnz,
            L.dptr(bh), crop, L.dptr(ev), E, L.lptr(cnt), L.dptr(l1), L.dptr(sse), eb, len(eb)),
            eb)
    finally:
        if own:
            ctx.close()
    return {"eps": ev, "nnz": cnt, "l1": l1, "sse": sse}


def pick_eps(sweep, rel):
    """The threshold to keep from a ``threshold_sweep`` result: the largest ``eps`` whose
    squared error, summed over the columns, is at most ``(1 + rel)`` times the total at the
    smallest threshold of the sweep; the smallest threshold when no other qualifies (or when
    that total is NaN).  Pure NumPy."""
    eps = np.asarray(sweep["eps"], dtype=np.float64).reshape(-1)
    sse = sweep["sse"]
    sse = np.asarray(sse.cpu().numpy() if hasattr(sse, "is_cuda") else sse, dtype=np.float64)
    if eps.size < 1 or sse.shape[0] != eps.size:
        raise ValueError("sweep['sse'] has one row per threshold of sweep['eps']")
    if not rel >= 0:
        raise ValueError("rel must be >= 0")
    total = sse.reshape(eps.size, -1).sum(axis=1)
    base = int(np.argmin(eps))
    ok = total <= (1.0 + rel) * total[base]
    ok[base] = True
    return float(eps[ok].max())


def densify(codes, ctx=None):
    """The inverse of ``sparsify`` on the GPU: the dense ``[M, n]`` float64 matrix of the
    tuple ``(jc, ir, pr, (M, n))`` or scipy.sparse matrix ``codes``, every entry bit for bit,
    zeros elsewhere.  Rows must be strictly ascending inside a column (``CCSCError`` with
    CCSC_E_INVALID otherwise).  NumPy in, Fortran-ordered NumPy out (ccsc_densify); CUDA
    tensors in, a CUDA tensor out (ccsc_densify_dev)."""
    lib = L.lib()
    jc, ir, pr, (M, n), on_dev = _codes_triple(codes)
    nnz = int(ir.shape[0])
    own = ctx is None
    eb = L.errbuf()
    if on_dev:
        import torch
        device = pr.device
        out = torch.empty((n, M), dtype=torch.float64, device=device)
        if own:
            ctx = Context(device.index if device.index is not None
                          else torch.cuda.current_device())
        try:
            torch.cuda.synchronize(device)
            L.check(lib.ccsc_densify_dev(ctx.ptr, jc.data_ptr(), ir.data_ptr(), pr.data_ptr(), M,
                                         n, nnz, out.data_ptr(), eb, len(eb)), eb)
        finally:
            if own:
                ctx.close()
        return out.t()
    out = np.zeros((M, n), order="F")
    if own:
        import torch
        ctx = Context(torch.cuda.current_device())
    try:
        L.check(lib.ccsc_densify(ctx.ptr, L.lptr(jc), L.lptr(ir), L.dptr(pr), M, n, nnz,
                                 L.dptr(out), eb, len(eb)), eb)
    finally:
        if own:
            ctx.close()
    return out


def _learn_2d(variant, b, kernel_size, lambda_residual, lambda_prior, max_it, tol, verbose, init,
              ctx=None, device=0, want_z=True, want_DZ=True, sparse_z=None, **kw):
    b = np.asarray(b, dtype=np.float64)
    if b.ndim == 2:
        b = b[:, :, None]
    if b.ndim != 3:
        raise ValueError("b must be [x, y, n]")
    own = ctx is None
    if own:
        ctx = Context(device)
    try:
        p = make_problem(variant, b.shape, kernel_size, lambda_residual, lambda_prior, max_it, tol,
                         verbose, **kw)
        d0 = z0 = None
        if init is not None and len(init) > 0:
            d0 = init.get("d")
            z0 = init.get("z")
        if ctx.group and sparse_z is None:
            return learn_once(ctx, p, b, d0, z0, want_z=want_z, want_DZ=want_DZ)
        s = Session(ctx, p, b, d0, z0)   # sparse_z on a device list: "one-device context"
        try:
            done = False
            while s.outer < s.p.max_it and not done:
                done = s.step(1)
            d_res, z_res, DZ, _ = s.results(want_z=want_z and sparse_z is None, want_DZ=want_DZ)
            if sparse_z is not None:
                z_res = s.codes_sparse(sparse_z)
            iterations = s.iterlog()
        finally:
            s.close()
    finally:
        if own:
            ctx.close()
    return d_res, z_res, DZ, iterations


def learn_once(ctx, p, b, d0=None, z0=None, want_z=True, want_DZ=True, want_obj=False):
    """One ccsc_learn call over the whole problem (the MEX path): on a multi-device
    context the engine shards it over the devices.  The consensus learners (2D, 3D, 4D),
    with the output shapes of Session.results over all n patches; returns
    (d_res, z_res, DZ, iterations) like the session path, iterations['obj_val'] being the
    final objective (the 3D / 4D learners' obj_val) when ``want_obj``."""
    p = resolve(p)
    if p.variant == L.CCSC_HS23:
        raise ValueError("the 2-3D learner takes smooth_init: use a Session")
    psf, K = p.psf, p.K
    r = psf // 2
    X, Y = p.sb[0] + 2 * r, p.sb[1] + 2 * r
    b = np.asfortranarray(b, dtype=np.float64)
    d0 = None if d0 is None else np.asfortranarray(d0, dtype=np.float64)
    z0 = None if z0 is None else np.asfortranarray(z0, dtype=np.float64)
    if p.variant == L.CCSC_L3D:
        T = p.sb[2] + 2 * r
        sd, sz, sx = (psf, psf, psf, K), (X, Y, T, K, p.n), (X, Y, T, p.n)
    elif p.variant == L.CCSC_L4D:
        U, V = p.views[0], p.views[1]
        sd, sz, sx = (psf, psf, U, V, K), (X, Y, 1, 1, K, p.n), (p.sb[0], p.sb[1], U, V, p.n)
    else:
        sd, sz, sx = (psf, psf, K), (X, Y, K, p.n), (X, Y, 1, p.n)
    d_res = np.zeros(sd, order="F")
    z_res = np.zeros(sz, order="F") if want_z else None
    DZ = np.zeros(sx, order="F") if want_DZ else None
    obj = np.zeros(1) if want_obj else None
    out = L.Outputs(L.dptr(d_res), L.dptr(z_res), L.dptr(DZ), L.dptr(obj))
    cap = p.max_it + 1
    a = {k: np.full(cap, np.nan) for k in ("obj_vals_d", "obj_vals_z", "tim_vals")}
    tr = {"d_diff": np.full(cap * p.max_it_d, np.nan), "z_diff": np.full(cap * p.max_it_z, np.nan)}
    nd = np.zeros(cap, dtype=np.int32)
    nz = np.zeros(cap, dtype=np.int32)
    lg = L.IterLog(cap, 0, L.dptr(a["obj_vals_d"]), L.dptr(a["obj_vals_z"]),
                   L.dptr(a["tim_vals"]), L.dptr(None), L.dptr(None), L.dptr(tr["d_diff"]),
                   L.dptr(tr["z_diff"]), L.iptr(nd), L.iptr(nz), L.iptr(None))
    eb = L.errbuf()
    L.check(L.lib().ccsc_learn(ctx.ptr, C.byref(p), L.dptr(b), L.dptr(d0), L.dptr(z0),
                               C.byref(out), C.byref(lg), L.CB(), None, eb, len(eb)), eb)
    cnt = lg.count
    it = {k: v[:cnt].copy() for k, v in a.items()}
    nout = max(cnt - 1, 0)
    it["trace"] = {"d_diff": tr["d_diff"][: nout * p.max_it_d].reshape(nout, p.max_it_d),
                   "z_diff": tr["z_diff"][: nout * p.max_it_z].reshape(nout, p.max_it_z),
                   "n_d": nd[:nout].copy(), "n_z": nz[:nout].copy()}
    if want_obj:
        it["obj_val"] = float(obj[0])
    return d_res, z_res, DZ, it


def admm_learn_conv2D_large_dParallel(b, kernel_size, lambda_residual, lambda_prior, max_it, tol,
                                      verbose, init=None, **kw):
    """Drop-in for 2D/admm_learn_conv2D_large_dParallel.m:1-199."""
    return _learn_2d(L.CCSC_DPAR, b, kernel_size, lambda_residual, lambda_prior, max_it, tol,
                     verbose, init, **kw)


def admm_learn_conv2D_large_dzParallel(b, kernel_size, lambda_residual, lambda_prior, max_it, tol,
                                       verbose, init=None, **kw):
    """Drop-in for 2D/admm_learn_conv2D_large_dzParallel.m:1-206."""
    return _learn_2d(L.CCSC_DZPAR, b, kernel_size, lambda_residual, lambda_prior, max_it, tol,
                     verbose, init, **kw)


def _learn_nd(ctx, p, b, d0, z0, want_z, want_DZ, sparse_z=None):
    """The 3D / 4D learners' run: a session stepped to the end on one device, one
    ccsc_learn over the whole problem on a multi-device context (as _learn_2d)."""
    if ctx.group and sparse_z is None:
        d_res, z_res, DZ, log = learn_once(ctx, p, b, d0, z0, want_z=want_z, want_DZ=want_DZ,
                                           want_obj=True)
        return d_res, z_res, DZ, log["obj_val"], log
    s = Session(ctx, p, b, d0, z0)
    try:
        done = False
        while s.outer < s.p.max_it and not done:
            done = s.step(1)
        d_res, z_res, DZ, obj = s.results(want_z=want_z and sparse_z is None, want_DZ=want_DZ,
                                          want_obj=True)
        if sparse_z is not None:
            z_res = s.codes_sparse(sparse_z)
        log = s.iterlog()
    finally:
        s.close()
    return d_res, z_res, DZ, obj, log


def admm_learn_conv4D_lightfield(b, kernel_size, lambda_residual, lambda_prior, max_it, tol,
                                 verbose, init=None, ctx=None, device=0, want_z=True,
                                 want_DZ=True, sparse_z=None, **kw):
    """Drop-in for 4D/admm_learn_conv4D_lightfield.m:1-212.

    b: [x, y, U, V, n] (single in the reference driver, Q15: widened to double);
    kernel_size = [psf, psf, U, V, K].  Returns (d_res [psf,psf,U,V,K],
    z_res [X,Y,1,1,K,n] complex (real part computed, Q8), DZ [x,y,U,V,n],
    obj_val, iterations) -- iterations carries empty fields like the reference
    (L4:64-72) plus the engine's 'trace'.
    """
    b = np.asarray(b, dtype=np.float64)
    if b.ndim == 4:
        b = b[..., None]
    if b.ndim != 5:
        raise ValueError("b must be [x, y, U, V, n]")
    own = ctx is None
    if own:
        ctx = Context(device)
    try:
        p = make_problem(L.CCSC_L4D, b.shape, kernel_size, lambda_residual, lambda_prior,
                         max_it, tol, verbose, **kw)
        d0 = z0 = None
        if init is not None and len(init) > 0:
            d0 = init.get("d")
            z0 = init.get("z")
            if z0 is not None:
                z0 = np.real(np.asarray(z0))
        d_res, z_res, DZ, obj, log = _learn_nd(ctx, p, b, d0, z0, want_z, want_DZ, sparse_z)
    finally:
        if own:
            ctx.close()
    iterations = {"obj_vals_d": [], "obj_vals_z": [], "tim_vals": [], "it_vals": [],
                  "trace": log["trace"], "engine_tim_vals": log["tim_vals"]}
    if z_res is not None and sparse_z is None:
        z_res = z_res.astype(np.complex128)
    return d_res, z_res, DZ, obj, iterations


def admm_learn_conv3D_large(b, kernel_size, lambda_residual, lambda_prior, max_it, tol, verbose,
                            init=None, ctx=None, device=0, want_z=True, want_DZ=True,
                            sparse_z=None, **kw):
    """Drop-in for 3D/admm_learn_conv3D_large.m:1-230 (function admm_learn_convND_large).

    b: [x, y, t, n]; kernel_size = [psf, psf, psf, K].  Returns (d_res [psf,psf,psf,K],
    z_res [X,Y,T,K,n], DZ [X,Y,T,n] (uncropped, L3:218-224), obj_val, iterations) --
    iterations carries the reference's empty fields (L3:72-75) plus the engine's 'trace'.
    """
    b = np.asarray(b, dtype=np.float64)
    if b.ndim == 3:
        b = b[..., None]
    if b.ndim != 4:
        raise ValueError("b must be [x, y, t, n]")
    own = ctx is None
    if own:
        ctx = Context(device)
    try:
        p = make_problem(L.CCSC_L3D, b.shape, kernel_size, lambda_residual, lambda_prior,
                         max_it, tol, verbose, **kw)
        d0 = z0 = None
        if init is not None and len(init) > 0:
            d0 = init.get("d")
            z0 = init.get("z")
        d_res, z_res, DZ, obj, log = _learn_nd(ctx, p, b, d0, z0, want_z, want_DZ, sparse_z)
    finally:
        if own:
            ctx.close()
    iterations = {"obj_vals_d": [], "obj_vals_z": [], "tim_vals": [], "it_vals": [],
                  "trace": log["trace"], "engine_tim_vals": log["tim_vals"]}
    return d_res, z_res, DZ, obj, iterations


def admm_learn(b, kernel_size, lambda_residual, lambda_prior, max_it, tol, verbose, init=None,
               smooth_init=None, ctx=None, device=0, want_z=True, want_DZ=True, return_log=False,
               sparse_z=None, **kw):
    """Drop-in for 2-3D/DictionaryLearning/admm_learn.m:1-237 (hyperspectral learner).

    b, smooth_init: [x, y, W, n] (learn_hyperspectral.m:16-17 passes the 13x13 Gaussian
    low-pass of b); kernel_size = [psf, psf, W, K].  ``init = {'d': [psf,psf,K],
    'z': [X,Y,K,n]}`` (the reference's own draw: one filter replicated over W, L23:54-56;
    its init branch, L23:50-52, cannot run).  Returns (d_res [psf,psf,W,K], z_res [X,Y,K,n],
    Dz [X,Y,W,n] incl. smoothinit, obj_val) like the reference; ``return_log=True`` appends
    the engine's log (per-iteration objectives, 'rolled_back' for L23:204-213).
    """
    b = np.asarray(b, dtype=np.float64)
    if b.ndim == 3:
        b = b[..., None]
    if b.ndim != 4:
        raise ValueError("b must be [x, y, W, n]")
    if len(kernel_size) != 4 or int(kernel_size[2]) != b.shape[2]:
        raise ValueError("kernel_size must be [psf, psf, W, K] with W = size(b, 3)")
    if smooth_init is None:
        raise ValueError("smooth_init is required (admm_learn.m:4)")
    sm = np.asarray(smooth_init, dtype=np.float64).reshape(b.shape, order="F")
    own = ctx is None
    if own:
        ctx = Context(device)
    try:
        p = make_problem(L.CCSC_HS23, b.shape, kernel_size, lambda_residual, lambda_prior,
                         max_it, tol, verbose, **kw)
        d0 = z0 = None
        if init is not None and len(init) > 0:
            d0 = init.get("d")
            z0 = init.get("z")
        s = Session(ctx, p, b, d0, z0, smooth_init=sm)
        try:
            done = False
            while s.outer < s.p.max_it and not done:
                done = s.step(1)
            d_res, z_res, DZ, obj = s.results(want_z=want_z and sparse_z is None,
                                              want_DZ=want_DZ, want_obj=True)
            if sparse_z is not None:
                z_res = s.codes_sparse(sparse_z)
            log = s.iterlog()
        finally:
            s.close()
    finally:
        if own:
            ctx.close()
    if not return_log:
        return d_res, z_res, DZ, obj
    log["rolled_back"] = bool(np.any(log["trace"]["flags"] & 1))
    log["outer"] = len(log["trace"]["flags"])
    return d_res, z_res, DZ, obj, log


def fft2d_test(ctx: Context, slices):
    """Kernel-level check: R2C half spectra + C2R round trip of [X, Y, count] slices."""
    a = np.asfortranarray(np.asarray(slices, dtype=np.float64))
    X, Y, cnt = a.shape
    Xh = X // 2 + 1
    hs = np.zeros(2 * Xh * Y * cnt)
    rt = np.zeros_like(a, order="F")
    eb = L.errbuf()
    L.check(L.lib().ccsc_test_fft2d(ctx.ptr, X, Y, cnt, L.dptr(a), L.dptr(hs), L.dptr(rt), eb,
                                    len(eb)), eb)
    h = hs.view(np.complex128).reshape(cnt, Y, Xh)          # [slice][y][x']
    return np.transpose(h, (2, 1, 0)), rt                     # [x', y, slice]


def fft_plan(family, X, Y=1, T=1):
    """Host only: the transform plan the sessions would run (ccsc_test_fft_plan).  ``family``
    is L.FFT_SLICE2D (grid X x Y), L.FFT_TTILE (X = Xh lines, T = Tn), L.FFT_LINE2D or
    L.FFT_LINE3D.  Returns {'x' | 'y' | 't': direction dict, 'inst': name, 'inst_mask': int}
    with the directions the family has; raises CCSCError (CCSC_E_UNSUPPORTED) with the
    planner's message when there is no plan."""
    out = L.FftPlan()
    eb = L.errbuf()
    L.check(L.lib().ccsc_test_fft_plan(int(family), int(X), int(Y), int(T), out, eb, len(eb)), eb)
    res = {"inst": L.FFT_INST[out.inst], "inst_mask": int(out.inst_mask)}
    for name, d in zip("xyt", out.dir):
        if d.n == 0:
            continue
        np_ = int(d.npass)
        res[name] = {"n": int(d.n), "npass": np_, "rad": list(d.rad[:np_]),
                     "twoff": list(d.twoff[:np_]), "pfa": bool(d.pfa), "lines": int(d.lines),
                     "groups": int(d.groups), "ntw": int(d.ntw), "lds_bytes": int(d.lds_bytes),
                     "threads": int(d.threads), "cap": list(d.cap[:np_]), "mask": int(d.mask),
                     "tw_global": bool(d.tw_global)}
    return res


def gfft_test(ctx: Context, vols):
    """Kernel-level check of the global line passes: [X, Y, count] (2D plan) or
    [X, Y, T, count] real slices -> (half spectra [x', y, (t,) slice], round trip)."""
    a = np.asfortranarray(np.asarray(vols, dtype=np.float64))
    if a.ndim == 3:
        X, Y, cnt = a.shape
        T = 1
    else:
        X, Y, T, cnt = a.shape
    Xh = X // 2 + 1
    hs = np.zeros(2 * Xh * Y * T * cnt)
    rt = np.zeros_like(a, order="F")
    eb = L.errbuf()
    L.check(L.lib().ccsc_test_gfft(ctx.ptr, X, Y, T, cnt, L.dptr(a), L.dptr(hs), L.dptr(rt), eb,
                                   len(eb)), eb)
    h = hs.view(np.complex128).reshape(cnt, T, Y, Xh)        # [slice][t][y][x']
    h = np.transpose(h, (3, 2, 1, 0))
    return (h[:, :, 0, :] if a.ndim == 3 else h), rt


def tfft_test(ctx: Context, tiles):
    """Kernel-level check of the 3D learner's t-tile transform: complex [Xh, Yn, Tn, count]
    (x' fastest) -> (forward transform along t, forward then inverse).  The inverse is
    unnormalised: the round trip returns Tn times the input."""
    a = np.asfortranarray(np.asarray(tiles, dtype=np.complex128))
    Xh, Yn, Tn, cnt = a.shape
    out = np.zeros_like(a, order="F")
    rt = np.zeros_like(a, order="F")
    eb = L.errbuf()
    f64 = lambda z: z.ctypes.data_as(L._dp)      # (re, im) pairs
    L.check(L.lib().ccsc_test_tfft(ctx.ptr, Tn, Xh, Yn, cnt, f64(a), f64(out), f64(rt), eb,
                                   len(eb)), eb)
    return out, rt
