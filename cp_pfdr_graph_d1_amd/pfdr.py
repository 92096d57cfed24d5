"""Python host side of the MI355X PFDR solvers (ctypes over libpfdr_mi355x.so).

Two layers, both calling the C ABI of ``include/pfdr_mi355x.h``:

* ``Lib`` — one method per C entry point, same argument order as the
  reference C++ templates (include/PFDR_graph_quadratic_d1_l1.hpp:36-42 and
  friends) minus the outputs, numpy in / numpy out.
* MEX-style front-ends mirroring the reference's Octave wrappers
  (octave/mex/PFDR_*_mex.cpp): ``PFDR_graph_quadratic_d1_l1``,
  ``PFDR_graph_l22_d1_l1``, ``PFDR_graph_quadratic_d1_l1_AtA`` and the bounds
  and simplex counterparts, returning ``(X, it, Obj, Dif)`` like
  ``[X, it, Obj, Dif] = PFDR_..._mex(...)``.

There is no CPU fallback: if the shared library is missing, or the HIP device
is unusable, every call raises ``PFDRError``.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libpfdr_mi355x.so")

PFDR_F32, PFDR_F64 = 0, 1
PFDR_MEM_HOST, PFDR_MEM_DEVICE = 0, 1
PFDR_KIND_L1, PFDR_KIND_BOUNDS, PFDR_KIND_SIMPLEX = 0, 1, 2
SCAL, DIAG = 0, 1
PFDR_REDUCED_DENSE, PFDR_REDUCED_SPARSE, PFDR_REDUCED_SPARSE_ALL = 0, 1, 2
REORDER_AUTO, REORDER_ON, REORDER_OFF = 0, 1, 2
# iterate-evolution statistic (include/pfdr_mi355x.h PFDR_EVOLUTION_*)
EVOLUTION_AUTO, EVOLUTION_SEQUENTIAL, EVOLUTION_TREE = 0, 1, 2
# speculative decisions (PFDR_SPEC_*): own stream / split communicator,
# serial on the session stream over one communicator, or none
SPEC_AUTO, SPEC_SERIAL, SPEC_OFF = 0, 1, 2
# which arcs of an edge r_cap[E] gives pfdr_cpgraph_mincut (PFDR_ARCS_*)
ARCS_BOTH, ARCS_FORWARD = 0, 1
ABI_VERSION = 4  # pfdr_abi_version() of the matching library

# every C entry point of include/pfdr_mi355x.h
EXPORTED = (
    "pfdr_last_error", "pfdr_abi_version", "pfdr_device_count",
    "pfdr_quadratic_d1_l1_f32", "pfdr_quadratic_d1_l1_f64",
    "pfdr_quadratic_d1_bounds_f32", "pfdr_quadratic_d1_bounds_f64",
    "pfdr_loss_d1_simplex_f32", "pfdr_loss_d1_simplex_f64",
    "pfdr_proj_simplex_metric_f32", "pfdr_proj_simplex_metric_f64",
    "pfdr_gram_f32", "pfdr_gram_f64", "pfdr_operator_norm_f32", "pfdr_operator_norm_f64",
    "pfdr_operator_norm_csc_f32", "pfdr_operator_norm_csc_f64",
    "pfdr_lipschitz_diag_csc_f32", "pfdr_lipschitz_diag_csc_f64",
    "pfdr_sequential_sum_f32", "pfdr_sequential_sum_f64",
    "pfdr_radix_sort_pairs_u32", "pfdr_radix_sort_pairs_u64",
    "pfdr_cp_reduce_f32", "pfdr_cp_reduce_f64",
    "pfdr_cp_reduce_csc_f32", "pfdr_cp_reduce_csc_f64",
    "pfdr_cp_reduce_csc_sparse_f32", "pfdr_cp_reduce_csc_sparse_f64",
    "pfdr_cpgraph_create", "pfdr_cpgraph_destroy", "pfdr_cpgraph_set_active",
    "pfdr_cpgraph_get_active", "pfdr_cpgraph_set_components", "pfdr_cpgraph_get_components",
    "pfdr_cpgraph_set_values", "pfdr_cpgraph_components", "pfdr_cpgraph_reduced_graph",
    "pfdr_cpgraph_get_reduced", "pfdr_cpgraph_merge", "pfdr_cpgraph_gradient",
    "pfdr_cpgraph_gradient_csc",
    "pfdr_cpgraph_capacities", "pfdr_cpgraph_capacities_bounds", "pfdr_cpgraph_activate",
    "pfdr_cpgraph_simplex_setup", "pfdr_cpgraph_simplex_observations",
    "pfdr_cpgraph_simplex_set_values", "pfdr_cpgraph_simplex_gradient",
    "pfdr_cpgraph_simplex_capacities", "pfdr_cpgraph_simplex_expand",
    "pfdr_cpgraph_simplex_activate", "pfdr_cpgraph_simplex_merge", "pfdr_cpgraph_simplex_labels",
    "pfdr_cpgraph_capacities_duplex", "pfdr_cpgraph_activate_duplex",
    "pfdr_cpgraph_mincut", "pfdr_cpgraph_mincut_relabels", "pfdr_cpgraph_mincut_duplex",
    "pfdr_cp_quadratic_d1_l1_f32", "pfdr_cp_quadratic_d1_l1_f64",
    "pfdr_cp_quadratic_d1_l1_duplex_f32", "pfdr_cp_quadratic_d1_l1_duplex_f64",
    "pfdr_cp_quadratic_d1_l1_duplex_stats",
    "pfdr_cp_loss_d1_simplex_f32", "pfdr_cp_loss_d1_simplex_f64",
    "pfdr_cp_loss_d1_simplex_stats",
    "pfdr_cp_quadratic_d1_bounds_f32", "pfdr_cp_quadratic_d1_bounds_f64",
    "pfdr_cp_quadratic_d1_bounds_stats",
    "pfdr_cp_solver_create", "pfdr_cp_solver_create_sparse", "pfdr_cp_solver_destroy",
    "pfdr_cp_solver_run",
    "pfdr_cp_solver_get_state", "pfdr_cp_solver_set_state", "pfdr_cp_solver_set_partition",
    "pfdr_cp_solver_set_penalties", "pfdr_cp_solver_stats",
    "pfdr_cp_solver_set_reduced", "pfdr_cp_solver_reduced_stats",
    "pfdr_cp_solver_premultiplied_stats",
    "pfdr_cpgraph_set_weights", "pfdr_cpgraph_set_active_by_labels",
    "pfdr_session_create", "pfdr_session_run", "pfdr_session_prepare", "pfdr_session_result",
    "pfdr_session_device_x", "pfdr_session_set_profiling", "pfdr_session_profile_filter",
    "pfdr_session_kernel_stats", "pfdr_session_sync",
    "pfdr_session_device_bytes", "pfdr_session_query", "pfdr_session_destroy",
    "pfdr_session_create_sparse", "pfdr_debug_session_csr",
    "pfdr_session_create_reusable", "pfdr_session_reload",
    "pfdr_batch_create", "pfdr_batch_run", "pfdr_batch_result", "pfdr_batch_reload",
    "pfdr_batch_query", "pfdr_batch_destroy",
    "pfdr_quadratic_d1_l1_csc_f32", "pfdr_quadratic_d1_l1_csc_f64",
    "pfdr_quadratic_d1_bounds_csc_f32", "pfdr_quadratic_d1_bounds_csc_f64",
    "pfdr_comm_unique_id", "pfdr_comm_init", "pfdr_comm_destroy",
    "pfdr_comm_allreduce_max_f64", "pfdr_loopback_create", "pfdr_loopback_abort",
    "pfdr_loopback_destroy", "pfdr_plan_create", "pfdr_plan_get",
    "pfdr_plan_set_incoming", "pfdr_plan_finish", "pfdr_plan_destroy",
    "pfdr_set_devices", "pfdr_debug_tile_erec", "pfdr_debug_erec_layout",
    "pfdr_debug_device_log",
    "pfdr_gen_knn_jitter_grid", "pfdr_gen_grid_edges",
    "pfdr_gen_piecewise_f32", "pfdr_gen_piecewise_f64",
    "pfdr_gen_uniform_f32", "pfdr_gen_uniform_f64", "pfdr_gen_matvec_f32",
    "pfdr_gen_matvec_f64", "pfdr_gen_symmetric_f32", "pfdr_gen_symmetric_f64",
    "pfdr_locality_order",
)
# the entries named after the reference's preAt, the header's only names with a
# capital letter: declared there and required of the library like the above
EXPORTED_PREAT = ("pfdr_cp_reduce_csc_sparse_preAt_f32", "pfdr_cp_reduce_csc_sparse_preAt_f64")


class PFDRError(RuntimeError):
    pass


class Problem(C.Structure):
    """Mirror of ``pfdr_problem`` (include/pfdr_mi355x.h)."""
    _fields_ = [
        ("kind", C.c_int), ("dtype", C.c_int), ("mem", C.c_int),
        ("V", C.c_int), ("E", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("X", C.c_void_p), ("Y", C.c_void_p), ("A", C.c_void_p),
        ("Eu", C.c_void_p), ("Ev", C.c_void_p),
        ("La_d1", C.c_void_p), ("La_l1", C.c_void_p),
        ("positivity", C.c_int), ("min", C.c_double), ("max", C.c_double),
        ("al", C.c_double), ("Ltype", C.c_int), ("L", C.c_void_p),
        ("rho", C.c_double), ("condMin", C.c_double),
        ("difRcd", C.c_double), ("difTol", C.c_double),
        ("itMax", C.c_int), ("verbose", C.c_int),
        ("record_obj", C.c_int), ("record_dif", C.c_int),
        ("nranks", C.c_int), ("rank", C.c_int), ("comm", C.c_void_p),
        ("comm_kind", C.c_int),
        ("vtx_begin", C.c_int64), ("V_global", C.c_int64),
        ("e_global", C.c_void_p), ("e_offset", C.c_int64),
        ("reorder", C.c_int),
        ("evolution", C.c_int),
        ("vtx_label", C.c_void_p),
        ("spec", C.c_int),
    ]


class CSCStruct(C.Structure):
    """Mirror of ``pfdr_csc`` (include/pfdr_mi355x.h)."""
    _fields_ = [("nnz", C.c_int64), ("colptr", C.c_void_p), ("rowidx", C.c_void_p),
                ("val", C.c_void_p)]


class Reload(C.Structure):
    """Mirror of ``pfdr_reload`` (include/pfdr_mi355x.h)."""
    _fields_ = [
        ("mem", C.c_int),
        ("X", C.c_void_p), ("Y", C.c_void_p), ("La_d1", C.c_void_p), ("La_l1", C.c_void_p),
        ("L", C.c_void_p),
        ("min", C.c_double), ("max", C.c_double),
        ("rho", C.c_double), ("condMin", C.c_double),
        ("difRcd", C.c_double), ("difTol", C.c_double),
        ("itMax", C.c_int),
    ]


class CPProblem(C.Structure):
    """Mirror of ``pfdr_cp_problem`` (include/pfdr_mi355x.h)."""
    _fields_ = [
        ("kind", C.c_int), ("duplex", C.c_int), ("dtype", C.c_int), ("mem", C.c_int),
        ("V", C.c_int), ("E", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("Y", C.c_void_p), ("A", C.c_void_p), ("Eu", C.c_void_p), ("Ev", C.c_void_p),
        ("La_d1", C.c_void_p), ("La_l1", C.c_void_p),
        ("positivity", C.c_int), ("min", C.c_double), ("max", C.c_double), ("al", C.c_double),
    ]


class CPParams(C.Structure):
    """Mirror of ``pfdr_cp_params`` (include/pfdr_mi355x.h)."""
    _fields_ = [
        ("CP_difTol", C.c_double), ("CP_itMax", C.c_int),
        ("rho", C.c_double), ("condMin", C.c_double), ("difRcd", C.c_double),
        ("difTol", C.c_double), ("itMax", C.c_int), ("verbose", C.c_int),
    ]


_LIB = None


def _solver_argtypes(lib, vp):
    """the resumable solver takes its pointers as integers or ctypes pointers"""
    lib.pfdr_cp_solver_create.argtypes = [C.POINTER(vp), C.POINTER(CPProblem)]
    if hasattr(lib, "pfdr_cp_solver_create_sparse"):
        lib.pfdr_cp_solver_create_sparse.argtypes = [C.POINTER(vp), C.POINTER(CPProblem),
                                                     C.POINTER(CSCStruct)]
    lib.pfdr_cp_solver_destroy.argtypes = [vp]
    lib.pfdr_cp_solver_destroy.restype = None
    lib.pfdr_cp_solver_run.argtypes = [vp, C.POINTER(CPParams), vp, vp, vp, vp]
    lib.pfdr_cp_solver_get_state.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int]
    lib.pfdr_cp_solver_set_state.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int]
    lib.pfdr_cp_solver_set_partition.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    lib.pfdr_cp_solver_set_penalties.argtypes = [vp, vp, vp, C.c_int]
    lib.pfdr_cp_solver_stats.argtypes = [vp, vp, vp, vp]
    if hasattr(lib, "pfdr_cp_solver_set_reduced"):
        lib.pfdr_cp_solver_set_reduced.argtypes = [vp, C.c_int]
        lib.pfdr_cp_solver_reduced_stats.argtypes = [vp, vp, vp, vp]
    if hasattr(lib, "pfdr_cp_solver_premultiplied_stats"):
        lib.pfdr_cp_solver_premultiplied_stats.argtypes = [vp, vp, vp, vp]


def load():
    """Load libpfdr_mi355x.so (built by __graft_entry__.build() / make)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise PFDRError("%s is missing: build it with "
                            "`make -C cp_pfdr_graph_d1_amd/csrc`" % LIB_PATH)
        # torch (when installed) first: its bundled HIP runtime is then the one
        # the library binds to, and torch.cuda keeps working in this process
        # (loaded the other way round, torch finds no GPU: INTEGRATION.md)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        # PFDR_LIB_PATH: A/B of compile-time variants of the same library
        lib = C.CDLL(os.environ.get("PFDR_LIB_PATH") or LIB_PATH)
        lib.pfdr_last_error.restype = C.c_char_p
        lib.pfdr_session_device_x.restype = C.c_void_p
        lib.pfdr_session_device_bytes.restype = C.c_int64
        lib.pfdr_gen_knn_jitter_grid.restype = C.c_int64
        lib.pfdr_gen_grid_edges.restype = C.c_int64
        lib.pfdr_gen_knn_jitter_grid.argtypes = [
            C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_double,
            C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        lib.pfdr_gen_grid_edges.argtypes = [
            C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
            C.c_void_p, C.c_void_p]
        for nm, ct in (("pfdr_gen_piecewise_f32", C.c_float),
                       ("pfdr_gen_piecewise_f64", C.c_double)):
            getattr(lib, nm).argtypes = [C.c_int, C.c_uint64, C.c_double,
                                         C.c_int64, C.c_int64, C.c_void_p]
        lib.pfdr_comm_allreduce_max_f64.argtypes = [C.c_void_p,
                                                    C.POINTER(C.c_double)]
        lib.pfdr_comm_init.argtypes = [C.POINTER(C.c_void_p), C.c_int,
                                       C.c_int, C.c_void_p]
        lib.pfdr_comm_destroy.argtypes = [C.c_void_p]
        vp = C.c_void_p
        for sfx, ct in (("f32", C.c_float), ("f64", C.c_double)):
            if hasattr(lib, "pfdr_operator_norm_csc_" + sfx):  # (as for the solver below)
                getattr(lib, "pfdr_operator_norm_csc_" + sfx).argtypes = [
                    C.c_int, C.c_int, C.POINTER(CSCStruct), C.c_int, ct, C.c_int, C.c_int,
                    C.c_int, C.c_void_p, C.c_void_p]
                getattr(lib, "pfdr_lipschitz_diag_csc_" + sfx).argtypes = [
                    C.c_int, C.c_int, C.POINTER(CSCStruct), C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(lib, "pfdr_cp_solver_create"):  # (absent from an older PFDR_LIB_PATH build)
            _solver_argtypes(lib, vp)
        # (PFDR_LIB_PATH: an A/B against a build of the previous ABI, 3, which
        # reads the problem without its trailing `spec` field)
        old_ok = bool(os.environ.get("PFDR_LIB_PATH")) and lib.pfdr_abi_version() == 3
        if lib.pfdr_abi_version() != ABI_VERSION and not old_ok:
            raise PFDRError("%s has ABI %d, this module expects %d: rebuild it" % (
                LIB_PATH, lib.pfdr_abi_version(), ABI_VERSION))
        _LIB = lib
    return _LIB


def _check(status, what):
    if status != 0:
        raise PFDRError("%s failed (%d): %s" % (
            what, status, load().pfdr_last_error().decode()))


def _real(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return C.c_float, "f32", PFDR_F32
    if dtype == np.float64:
        return C.c_double, "f64", PFDR_F64
    raise TypeError("PFDR supports float32 and float64, got %s" % dtype)


def _arr(a, dtype):
    if a is None:
        return None
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a, ct):
    return None if a is None else a.ctypes.data_as(C.POINTER(ct))


def _is_device(a):
    return hasattr(a, "data_ptr")


def _vp(a):
    """a numpy array, an address or None as a void pointer"""
    if a is None:
        return None
    return C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else int(a))


def _cp_stats(fill, first="n_cuts"):
    """the cut pursuits' seconds[6] / counts[4] record, which ``fill(seconds,
    counts)`` writes -> dict: seconds per phase and counts"""
    sec = np.zeros(6, np.float64)
    cnt = np.zeros(4, np.int64)
    fill(_ptr(sec, C.c_double), _ptr(cnt, C.c_int64))
    out = dict(zip(("gradient", "cuts", "graph", "pfdr", "sums", "total"), sec.tolist()))
    out.update(zip((first, "rounds", "relabels", "pfdr_it"), cnt.tolist()))
    return out


class CSC:
    """A sparse N-by-V observation operator in compressed sparse columns
    (``pfdr_csc``, include/pfdr_mi355x.h): column v holds the entries
    colptr[v] .. colptr[v+1] - 1, rowidx strictly ascending inside a column,
    stored zeros allowed.  The arrays are numpy arrays (colptr int64, rowidx
    int32, val float32 / float64) or torch GPU tensors of those types."""

    def __init__(self, colptr, rowidx, val, N):
        self.device = _is_device(val)
        if self.device:
            if not (_is_device(colptr) and _is_device(rowidx)):
                raise TypeError("CSC: colptr, rowidx and val must all be torch GPU tensors, "
                                "or all host arrays")
            import torch
            if (colptr.dtype != torch.int64 or rowidx.dtype != torch.int32 or
                    val.dtype not in (torch.float32, torch.float64)):
                raise TypeError("CSC: device arrays must be int64 / int32 / float32 or float64")
            self.colptr, self.rowidx, self.val = (colptr.contiguous(), rowidx.contiguous(),
                                                  val.contiguous())
            self.dtype = np.dtype(np.float32 if val.dtype == torch.float32 else np.float64)
        else:
            self.colptr = np.ascontiguousarray(colptr, np.int64)
            self.rowidx = np.ascontiguousarray(rowidx, np.int32)
            val = np.ascontiguousarray(val)
            if val.dtype not in (np.float32, np.float64):
                val = val.astype(np.float64)
            self.val = val
            self.dtype = val.dtype
        self.N = int(N)
        self.V = int(self.colptr.shape[0]) - 1
        self.nnz = int(self.val.shape[0])
        self.shape = (self.N, self.V)

    @classmethod
    def from_dense(cls, A, stored=None):
        """The nonzeros of the N-by-V matrix A, and the entries where the
        boolean N-by-V mask ``stored`` is set whatever their value (stored
        zeros)."""
        A = np.asarray(A)
        if A.ndim != 2:
            raise ValueError("CSC.from_dense: A must be N-by-V")
        keep = A != 0
        if stored is not None:
            keep = keep | np.asarray(stored, bool)
        cols, rows = np.nonzero(keep.T)  # column by column, rows ascending
        colptr = np.zeros(A.shape[1] + 1, np.int64)
        np.cumsum(np.bincount(cols, minlength=A.shape[1]), out=colptr[1:])
        return cls(colptr, rows.astype(np.int32), A[rows, cols], A.shape[0])

    @classmethod
    def from_scipy(cls, m):
        """Any object with ``tocsc()`` giving ``indptr``, ``indices``, ``data``
        and ``shape`` (a scipy.sparse matrix; scipy itself is not imported)."""
        m = m.tocsc()
        if hasattr(m, "sort_indices"):
            m.sort_indices()
        return cls(m.indptr, m.indices, m.data, m.shape[0])

    def astype(self, dtype):
        if self.device:
            import torch
            t = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
            return CSC(self.colptr, self.rowidx, self.val.to(t), self.N)
        return CSC(self.colptr, self.rowidx, self.val.astype(dtype, copy=False), self.N)

    def to_host(self):
        if not self.device:
            return self
        return CSC(self.colptr.cpu().numpy(), self.rowidx.cpu().numpy(), self.val.cpu().numpy(),
                   self.N)

    def to_device(self, device="cuda"):
        if self.device:
            return self
        import torch
        return CSC(torch.from_numpy(self.colptr).to(device), torch.from_numpy(self.rowidx).to(device),
                   torch.from_numpy(self.val).to(device), self.N)

    def to_dense(self):
        """The N-by-V numpy matrix (stored zeros become plain zeros)."""
        h = self.to_host()
        A = np.zeros((h.N, h.V), h.dtype)
        cols = np.repeat(np.arange(h.V), np.diff(h.colptr))
        A[h.rowidx, cols] = h.val
        return A

    def struct(self):
        """The ``pfdr_csc`` of these arrays (which must outlive its use)."""
        if self.device:
            return CSCStruct(self.nnz, self.colptr.data_ptr(), self.rowidx.data_ptr(),
                             self.val.data_ptr())
        return CSCStruct(self.nnz, self.colptr.ctypes.data, self.rowidx.ctypes.data,
                         self.val.ctypes.data)


class Lib:
    """Raw C-ABI calls (host pointers, synchronous)."""

    @staticmethod
    def _csc_args(A, dt):
        """nnz, colptr, rowidx, val of a CSC for the one-call entries (host)"""
        A = A.to_host().astype(dt)
        keep = (A.colptr, A.rowidx, A.val)
        return keep, (C.c_int64(A.nnz), C.c_void_p(A.colptr.ctypes.data),
                      C.c_void_p(A.rowidx.ctypes.data), C.c_void_p(A.val.ctypes.data))

    def __init__(self):
        self.lib = load()

    # batched dense sessions (pfdr_batch_*): raw mirrors, addresses as
    # integers or None, `problem` a Problem and `reload` a Reload
    def batch_create(self, problem, B):
        h = C.c_void_p()
        _check(self.lib.pfdr_batch_create(C.byref(h), None if problem is None else
                                          C.byref(problem), C.c_int(B)), "pfdr_batch_create")
        return h

    def batch_run(self, handle, iters, it=None):
        _check(self.lib.pfdr_batch_run(handle, C.c_int(iters), _vp(it)), "pfdr_batch_run")

    def batch_result(self, handle, X=None, it=None, Obj=None, Dif=None):
        _check(self.lib.pfdr_batch_result(handle, _vp(X), _vp(it), _vp(Obj), _vp(Dif)),
               "pfdr_batch_result")

    def batch_reload(self, handle, reload):
        _check(self.lib.pfdr_batch_reload(handle, None if reload is None else C.byref(reload)),
               "pfdr_batch_reload")

    def batch_query(self, handle, what):
        v = C.c_int64(0)
        _check(self.lib.pfdr_batch_query(handle, None if what is None else what.encode(),
                                         C.byref(v)), "pfdr_batch_query")
        return v.value

    def batch_destroy(self, handle):
        self.lib.pfdr_batch_destroy(handle)

    def quadratic_d1_l1(self, X0, Y, A, N, Eu, Ev, La_d1, La_l1=None,
                        positivity=0, Ltype=SCAL, L=None, rho=1.5,
                        condMin=1e-3, difRcd=0.0, difTol=1e-5, itMax=1000,
                        obj=False, dif=False, verbose=0):
        X = np.array(X0, copy=True)
        ct, sfx, _ = _real(X.dtype)
        dt = X.dtype
        csc = isinstance(A, CSC)
        if csc:  # (A: a CSC in place of the dense matrix, N its row count)
            _keep, aargs = self._csc_args(A, dt)
            sfx = "csc_" + sfx
            A = None
        Y, A, La_d1, La_l1, L = (_arr(a, dt) for a in (Y, A, La_d1, La_l1, L))
        Eu, Ev = _arr(Eu, np.int32), _arr(Ev, np.int32)
        Obj = np.zeros(itMax + 1, dt) if obj else None
        Dif = np.zeros(max(itMax, 1), dt) if dif else None
        it = C.c_int(0)
        fn = getattr(self.lib, "pfdr_quadratic_d1_l1_" + sfx)
        if not csc:
            aargs = (_ptr(A, ct),)
        _check(fn(C.c_int(X.size), C.c_int(Eu.size), C.c_int(N), _ptr(X, ct),
                  _ptr(Y, ct), *aargs, _ptr(Eu, C.c_int),
                  _ptr(Ev, C.c_int), _ptr(La_d1, ct), _ptr(La_l1, ct),
                  C.c_int(positivity), C.c_int(Ltype), _ptr(L, ct), ct(rho),
                  ct(condMin), ct(difRcd), ct(difTol), C.c_int(itMax),
                  C.byref(it), _ptr(Obj, ct), _ptr(Dif, ct),
                  C.c_int(verbose)), "pfdr_quadratic_d1_l1_" + sfx)
        return X, it.value, Obj, Dif

    def _cp_quadratic(self, flavour, V, N, Y, A, Eu, Ev, La_d1, own, CP_difTol, CP_itMax, rho,
                      condMin, difRcd, difTol, itMax, verbose):
        """the quadratic cut-pursuit entries' one call; ``own``, the flavour's
        own arguments: (La_l1, positivity) for "l1" and "duplex", (lo, hi) for
        "bounds" -> (Cv[V] int32, rX[rV], CP_it, Obj[CP_itMax + 1],
        Dif[CP_itMax], Time[CP_itMax + 1])"""
        Y = np.ascontiguousarray(Y)
        ct, sfx, _ = _real(Y.dtype)
        dt = Y.dtype
        A, La_d1 = (_arr(a, dt) for a in (A, La_d1))
        Eu, Ev = _arr(Eu, np.int32), _arr(Ev, np.int32)
        if flavour == "bounds":
            name = "pfdr_cp_quadratic_d1_bounds_" + sfx
            own = (ct(own[0]), ct(own[1]))
        else:
            name = "pfdr_cp_quadratic_d1_l1_" + ("duplex_" if flavour == "duplex" else "") + sfx
            La_l1 = _arr(own[0], dt)
            own = (_ptr(La_l1, ct), C.c_int(int(own[1])))
        V, CP_itMax = int(V), int(CP_itMax)
        Cv = np.zeros(V, np.int32)
        rX = np.zeros(V, dt)
        Obj = np.zeros(CP_itMax + 1, dt)
        Dif = np.zeros(max(CP_itMax, 1), dt)
        Time = np.zeros(CP_itMax + 1, np.float64)
        rV, it = C.c_int(0), C.c_int(0)
        _check(getattr(self.lib, name)(
            C.c_int(V), C.c_int(Eu.size), C.c_int(N), C.byref(rV), _ptr(Cv, C.c_int),
            _ptr(rX, ct), _ptr(Y, ct), _ptr(A, ct), _ptr(Eu, C.c_int), _ptr(Ev, C.c_int),
            _ptr(La_d1, ct), *own, ct(CP_difTol), C.c_int(CP_itMax), C.byref(it), ct(rho),
            ct(condMin), ct(difRcd), ct(difTol), C.c_int(itMax), _ptr(Time, C.c_double),
            _ptr(Obj, ct), _ptr(Dif, ct), C.c_int(verbose)), name)
        return Cv, rX[:rV.value].copy(), it.value, Obj, Dif[:CP_itMax], Time

    def cp_quadratic_d1_l1(self, V, N, Y, A, Eu, Ev, La_d1, La_l1=None, positivity=0,
                           CP_difTol=1e-3, CP_itMax=10, rho=1.0, condMin=1e-3, difRcd=0.0,
                           difTol=1e-4, itMax=10000, verbose=0):
        """pfdr_cp_quadratic_d1_l1: the whole cut pursuit -> (Cv[V] int32,
        rX[rV], CP_it, Obj[CP_itMax + 1], Dif[CP_itMax], Time[CP_itMax + 1])"""
        return self._cp_quadratic("l1", V, N, Y, A, Eu, Ev, La_d1, (La_l1, positivity),
                                  CP_difTol, CP_itMax, rho, condMin, difRcd, difTol, itMax,
                                  verbose)

    def cp_quadratic_d1_l1_duplex(self, V, N, Y, A, Eu, Ev, La_d1, La_l1=None, positivity=0,
                                  CP_difTol=1e-3, CP_itMax=10, rho=1.0, condMin=1e-3,
                                  difRcd=0.0, difTol=1e-4, itMax=10000, verbose=0):
        """pfdr_cp_quadratic_d1_l1_duplex: the duplex driver's whole cut pursuit
        (one two-layer cut per iteration); arguments and returns as
        cp_quadratic_d1_l1"""
        return self._cp_quadratic("duplex", V, N, Y, A, Eu, Ev, La_d1, (La_l1, positivity),
                                  CP_difTol, CP_itMax, rho, condMin, difRcd, difTol, itMax,
                                  verbose)

    def cp_quadratic_d1_l1_duplex_stats(self):
        """pfdr_cp_quadratic_d1_l1_duplex_stats of this thread's last
        cp_quadratic_d1_l1_duplex -> dict: seconds per phase and counts"""
        return _cp_stats(lambda sec, cnt: _check(
            self.lib.pfdr_cp_quadratic_d1_l1_duplex_stats(sec, cnt),
            "pfdr_cp_quadratic_d1_l1_duplex_stats"))

    def cp_quadratic_d1_bounds(self, V, N, Y, A, Eu, Ev, La_d1, lo=-np.inf, hi=np.inf,
                               CP_difTol=1e-3, CP_itMax=10, rho=1.0, condMin=1e-3, difRcd=0.0,
                               difTol=1e-4, itMax=10000, verbose=0):
        """pfdr_cp_quadratic_d1_bounds: the bounds driver's whole cut pursuit for
        the box lo <= x <= hi (+-inf: no bound) -> (Cv[V] int32, rX[rV], CP_it,
        Obj[CP_itMax + 1], Dif[CP_itMax], Time[CP_itMax + 1])"""
        return self._cp_quadratic("bounds", V, N, Y, A, Eu, Ev, La_d1, (lo, hi), CP_difTol,
                                  CP_itMax, rho, condMin, difRcd, difTol, itMax, verbose)

    def cp_quadratic_d1_bounds_stats(self):
        """pfdr_cp_quadratic_d1_bounds_stats of this thread's last
        cp_quadratic_d1_bounds -> dict: seconds per phase and counts"""
        return _cp_stats(lambda sec, cnt: _check(
            self.lib.pfdr_cp_quadratic_d1_bounds_stats(sec, cnt),
            "pfdr_cp_quadratic_d1_bounds_stats"))

    def cp_loss_d1_simplex(self, K, Q, Eu, Ev, La_d1, al=0.1, CP_difTol=1e-3, CP_itMax=10,
                           rho=1.0, condMin=0.1, difRcd=0.0, difTol=1e-4, itMax=1000,
                           verbose=0, time=True, obj=True, dif=True):
        """pfdr_cp_loss_d1_simplex: the simplex driver's whole cut pursuit.  Q[V*K]
        vertex-major (Q[v*K + k]) -> (Cv[V] int32, rP[rV*K] vertex-major, CP_it,
        Obj[CP_itMax + 1], Dif[CP_itMax], Time[CP_itMax + 1]); a record not asked
        for (obj / dif / time False) is passed as NULL and returned as None"""
        Q = np.ascontiguousarray(Q).ravel()
        ct, sfx, _ = _real(Q.dtype)
        dt = Q.dtype
        K, CP_itMax = int(K), int(CP_itMax)
        V = Q.size // K
        La_d1 = _arr(La_d1, dt)
        Eu, Ev = _arr(Eu, np.int32), _arr(Ev, np.int32)
        Cv = np.zeros(V, np.int32)
        rP = np.zeros(V * K, dt)
        Obj = np.zeros(CP_itMax + 1, dt) if obj else None
        Dif = np.zeros(max(CP_itMax, 1), dt) if dif else None
        Time = np.zeros(CP_itMax + 1, np.float64) if time else None
        rV, it = C.c_int(0), C.c_int(0)
        fn = getattr(self.lib, "pfdr_cp_loss_d1_simplex_" + sfx)
        _check(fn(C.c_int(K), C.c_int(V), C.c_int(Eu.size), ct(al), C.byref(rV),
                  _ptr(Cv, C.c_int), _ptr(rP, ct), _ptr(Q, ct), _ptr(Eu, C.c_int),
                  _ptr(Ev, C.c_int), _ptr(La_d1, ct), ct(CP_difTol), C.c_int(CP_itMax),
                  C.byref(it), ct(rho), ct(condMin), ct(difRcd), ct(difTol), C.c_int(itMax),
                  _ptr(Time, C.c_double), _ptr(Obj, ct), _ptr(Dif, ct), C.c_int(verbose)),
               "pfdr_cp_loss_d1_simplex_" + sfx)
        return (Cv, rP[:rV.value * K].copy(), it.value, Obj,
                None if Dif is None else Dif[:CP_itMax], Time)

    # the resumable solver (pfdr_cp_solver_*): thin mirrors, pointers as integers
    # or ctypes pointers; CPSolver below is the array-level face
    def cp_solver_create(self, problem, csc=None):
        """pfdr_cp_solver_create(CPProblem), or pfdr_cp_solver_create_sparse
        with a CSCStruct (or None for its NULL) as well -> handle"""
        h = C.c_void_p()
        if csc is None:
            _check(self.lib.pfdr_cp_solver_create(C.byref(h), C.byref(problem)),
                   "pfdr_cp_solver_create")
        else:
            _check(self.lib.pfdr_cp_solver_create_sparse(C.byref(h), C.byref(problem),
                                                         C.byref(csc)),
                   "pfdr_cp_solver_create_sparse")
        return h

    def cp_solver_destroy(self, handle):
        self.lib.pfdr_cp_solver_destroy(handle)

    def cp_solver_run(self, handle, params, CP_it=None, Time=None, Obj=None, Dif=None):
        """pfdr_cp_solver_run(handle, CPParams, host pointers or None)"""
        _check(self.lib.pfdr_cp_solver_run(handle, C.byref(params), CP_it, Time, Obj, Dif),
               "pfdr_cp_solver_run")

    def cp_solver_get_state(self, handle, rV=None, Cv=None, Vc=None, rVc=None, active=None,
                            rX=None, R=None, mem=PFDR_MEM_HOST):
        _check(self.lib.pfdr_cp_solver_get_state(handle, rV, Cv, Vc, rVc, active, rX, R, mem),
               "pfdr_cp_solver_get_state")

    def cp_solver_set_state(self, handle, rV, Cv, Vc, rVc, active, rX, R=None,
                            mem=PFDR_MEM_HOST):
        _check(self.lib.pfdr_cp_solver_set_state(handle, rV, Cv, Vc, rVc, active, rX, R, mem),
               "pfdr_cp_solver_set_state")

    def cp_solver_set_partition(self, handle, nlabels, label, values, mem=PFDR_MEM_HOST):
        _check(self.lib.pfdr_cp_solver_set_partition(handle, nlabels, label, values, mem),
               "pfdr_cp_solver_set_partition")

    def cp_solver_set_penalties(self, handle, La_d1=None, La_l1=None, mem=PFDR_MEM_HOST):
        _check(self.lib.pfdr_cp_solver_set_penalties(handle, La_d1, La_l1, mem),
               "pfdr_cp_solver_set_penalties")

    def cp_solver_stats(self, handle, seconds=None, counts=None, setup_seconds=None):
        _check(self.lib.pfdr_cp_solver_stats(handle, seconds, counts, setup_seconds),
               "pfdr_cp_solver_stats")

    def cp_solver_set_reduced(self, handle, mode):
        _check(self.lib.pfdr_cp_solver_set_reduced(handle, int(mode)),
               "pfdr_cp_solver_set_reduced")

    def cp_solver_reduced_stats(self, handle):
        """-> (sparse iterations, dense direct iterations, max rnnz) of the last run"""
        out = np.zeros(3, np.int64)
        a = out.ctypes.data
        _check(self.lib.pfdr_cp_solver_reduced_stats(handle, a, a + 8, a + 16),
               "pfdr_cp_solver_reduced_stats")
        return tuple(int(x) for x in out)

    def cp_solver_premultiplied_stats(self, handle):
        """-> (iterations solved from stored entries, iterations that formed a
        dense rA, max rnnz) of the last run's premultiplied iterations, N > 0"""
        out = np.zeros(3, np.int64)
        a = out.ctypes.data
        _check(self.lib.pfdr_cp_solver_premultiplied_stats(handle, a, a + 8, a + 16),
               "pfdr_cp_solver_premultiplied_stats")
        return tuple(int(x) for x in out)

    def cp_loss_d1_simplex_stats(self, n_exp=64):
        """pfdr_cp_loss_d1_simplex_stats of this thread's last cp_loss_d1_simplex
        -> dict: seconds per phase, counts, rounds / relabels per expansion"""
        er, el = np.zeros(n_exp, np.int64), np.zeros(n_exp, np.int64)
        out = _cp_stats(lambda sec, cnt: _check(self.lib.pfdr_cp_loss_d1_simplex_stats(
            sec, cnt, _ptr(er, C.c_int64), _ptr(el, C.c_int64), C.c_int(n_exp)),
            "pfdr_cp_loss_d1_simplex_stats"), first="expansions")
        out["exp_rounds"] = er[er >= 0]
        out["exp_relabels"] = el[el >= 0]
        return out

    def quadratic_d1_bounds(self, X0, Y, A, N, Eu, Ev, La_d1, lo=-np.inf,
                            hi=np.inf, Ltype=SCAL, L=None, rho=1.5,
                            condMin=1e-3, difRcd=0.0, difTol=1e-5,
                            itMax=1000, obj=False, dif=False, verbose=0):
        X = np.array(X0, copy=True)
        ct, sfx, _ = _real(X.dtype)
        dt = X.dtype
        csc = isinstance(A, CSC)
        if csc:  # (as quadratic_d1_l1)
            _keep, aargs = self._csc_args(A, dt)
            sfx = "csc_" + sfx
            A = None
        Y, A, La_d1, L = (_arr(a, dt) for a in (Y, A, La_d1, L))
        Eu, Ev = _arr(Eu, np.int32), _arr(Ev, np.int32)
        Obj = np.zeros(itMax + 1, dt) if obj else None
        Dif = np.zeros(max(itMax, 1), dt) if dif else None
        it = C.c_int(0)
        fn = getattr(self.lib, "pfdr_quadratic_d1_bounds_" + sfx)
        if not csc:
            aargs = (_ptr(A, ct),)
        _check(fn(C.c_int(X.size), C.c_int(Eu.size), C.c_int(N), _ptr(X, ct),
                  _ptr(Y, ct), *aargs, _ptr(Eu, C.c_int),
                  _ptr(Ev, C.c_int), _ptr(La_d1, ct), ct(lo), ct(hi),
                  C.c_int(Ltype), _ptr(L, ct), ct(rho), ct(condMin),
                  ct(difRcd), ct(difTol), C.c_int(itMax), C.byref(it),
                  _ptr(Obj, ct), _ptr(Dif, ct), C.c_int(verbose)),
               "pfdr_quadratic_d1_bounds_" + sfx)
        return X, it.value, Obj, Dif

    def loss_d1_simplex(self, P0, Q, K, Eu, Ev, La_d1, al=0.1, La_f=None,
                        rho=1.0, condMin=0.1, difRcd=0.0, difTol=1e-4,
                        itMax=1000, obj=False, dif=False, verbose=0):
        P = np.array(P0, copy=True)
        ct, sfx, _ = _real(P.dtype)
        dt = P.dtype
        Q, La_d1, La_f = (_arr(a, dt) for a in (Q, La_d1, La_f))
        Eu, Ev = _arr(Eu, np.int32), _arr(Ev, np.int32)
        Obj = np.zeros(itMax + 1, dt) if obj else None
        Dif = np.zeros(max(itMax, 1), dt) if dif else None
        it = C.c_int(0)
        fn = getattr(self.lib, "pfdr_loss_d1_simplex_" + sfx)
        _check(fn(C.c_int(K), C.c_int(P.size // K), C.c_int(Eu.size), ct(al),
                  _ptr(La_f, ct), _ptr(P, ct), _ptr(Q, ct), _ptr(Eu, C.c_int),
                  _ptr(Ev, C.c_int), _ptr(La_d1, ct), ct(rho), ct(condMin),
                  ct(difRcd), ct(difTol), C.c_int(itMax), C.byref(it),
                  _ptr(Obj, ct), _ptr(Dif, ct), C.c_int(verbose)),
               "pfdr_loss_d1_simplex_" + sfx)
        return P, it.value, Obj, Dif

    def proj_simplex_metric(self, X0, M, D, N, nm, A, na):
        X = np.array(X0, copy=True)
        ct, sfx, _ = _real(X.dtype)
        M, A = _arr(M, X.dtype), _arr(A, X.dtype)
        fn = getattr(self.lib, "pfdr_proj_simplex_metric_" + sfx)
        _check(fn(_ptr(X, ct), _ptr(M, ct), C.c_int(D), C.c_int(N),
                  C.c_int(nm), _ptr(A, ct), C.c_int(na)),
               "pfdr_proj_simplex_metric_" + sfx)
        return X


# ------------------------------------------------------ MEX-style API -----
def _edges(Eu, Ev):
    # the Python binding reinterprets uint32 edge arrays as int
    # (reference python/CP_quadratic_l1_py.cpp:228-258); accept any integer
    return (np.ascontiguousarray(Eu).astype(np.int32, copy=False),
            np.ascontiguousarray(Ev).astype(np.int32, copy=False))


def _scal_or_vec(x, n, dt):
    """MEX wrappers pass scalars for 'none' (numel == 1 -> NULL)."""
    if x is None:
        return None
    a = np.asarray(x, dt).ravel()
    return None if a.size <= 1 else a


def PFDR_graph_quadratic_d1_l1(Y, A, Eu, Ev, La_d1, La_l1, positivity, L,
                               rho, condMin, difRcd, difTol, itMax,
                               verbose=0, obj=False, dif=False):
    """[X, it, Obj, Dif] = PFDR_graph_quadratic_d1_l1_mex(Y, A, Eu, Ev, La_d1,
    La_l1, positivity, L, rho, condMin, difRcd, difTol, itMax, verbose)
    (octave/mex/PFDR_graph_quadratic_d1_l1_mex.cpp): A is N-by-V, dense or
    a CSC."""
    sparse = isinstance(A, CSC)
    A = A if sparse else np.asarray(A)
    dt = np.result_type(Y, np.float32)
    N, V = A.shape
    L = np.asarray(L, dt).ravel()
    Ltype = SCAL if L.size == 1 else DIAG
    Eu, Ev = _edges(Eu, Ev)
    return Lib().quadratic_d1_l1(
        np.zeros(V, dt), np.asarray(Y, dt),
        A if sparse else np.asfortranarray(A, dt).ravel(order="F"),
        N, Eu, Ev, np.asarray(La_d1, dt), _scal_or_vec(La_l1, V, dt),
        positivity, Ltype, L, rho, condMin, difRcd, difTol, itMax, obj, dif,
        verbose)


def PFDR_graph_quadratic_d1_l1_AtA(AtY, AtA, Eu, Ev, La_d1, La_l1, positivity,
                                   L, rho, condMin, difRcd, difTol, itMax,
                                   verbose=0, obj=False, dif=False):
    """octave/mex/PFDR_graph_quadratic_d1_l1_AtA_mex.cpp: N = -V."""
    dt = np.result_type(AtY, np.float32)
    V = np.asarray(AtY).size
    L = np.asarray(L, dt).ravel()
    Eu, Ev = _edges(Eu, Ev)
    return Lib().quadratic_d1_l1(
        np.zeros(V, dt), np.asarray(AtY, dt),
        np.asfortranarray(AtA, dt).ravel(order="F"), -V, Eu, Ev,
        np.asarray(La_d1, dt), _scal_or_vec(La_l1, V, dt), positivity,
        SCAL if L.size == 1 else DIAG, L, rho, condMin, difRcd, difTol, itMax,
        obj, dif, verbose)


def _l22_scale(Y, La_l2):
    """the l22 wrappers' convention (octave/mex/PFDR_graph_l22_d1_l1_mex.cpp:54-83
    and its counterparts): Y <- La_l2*Y, N = 0, A = La_l2 (diagonal; a scalar:
    none) -> (dtype, V, La_l2 or None, La_l2*Y)"""
    dt = np.result_type(Y, np.float32)
    La_l2 = _scal_or_vec(La_l2, Y.size, dt)
    return dt, Y.size, La_l2, (La_l2 * Y).astype(dt) if La_l2 is not None else Y.astype(dt)


def _l22_correct(Obj, it, Y, La_l2, dt):
    """... and Obj += 1/2 ||y||^2_La_l2, the constant the scaled problem leaves out"""
    if Obj is not None:
        y = Y.astype(dt)
        w = La_l2 if La_l2 is not None else np.ones(Y.size, dt)
        Obj[: it + 1] += float(np.sum(w.astype(np.float64) * y * y)) / 2.0


def PFDR_graph_l22_d1_l1(Y, La_l2, Eu, Ev, La_d1, La_l1, positivity, rho,
                         condMin, difRcd, difTol, itMax, verbose=0,
                         obj=False, dif=False):
    """octave/mex/PFDR_graph_l22_d1_l1_mex.cpp:54-83: Y <- La_l2*Y, N = 0,
    A = La_l2 (diagonal), Ltype DIAG, L = La_l2; Obj += 1/2 ||y||^2_La_l2."""
    Y = np.asarray(Y)
    dt, V, La_l2, Yw = _l22_scale(Y, La_l2)
    Eu, Ev = _edges(Eu, Ev)
    X, it, Obj, Dif = Lib().quadratic_d1_l1(
        np.zeros(V, dt), Yw, La_l2, 0, Eu, Ev, np.asarray(La_d1, dt),
        _scal_or_vec(La_l1, V, dt), positivity, DIAG, La_l2, rho, condMin,
        difRcd, difTol, itMax, obj, dif, verbose)
    _l22_correct(Obj, it, Y, La_l2, dt)
    return X, it, Obj, Dif


def PFDR_graph_quadratic_d1_bounds(Y, A, Eu, Ev, La_d1, Bnd, L, rho, condMin,
                                   difRcd, difTol, itMax, verbose=0,
                                   obj=False, dif=False):
    """octave/mex/PFDR_graph_quadratic_d1_bounds_mex.cpp (Bnd = [min, max]);
    A dense or a CSC."""
    sparse = isinstance(A, CSC)
    A = A if sparse else np.asarray(A)
    dt = np.result_type(Y, np.float32)
    N, V = A.shape
    L = np.asarray(L, dt).ravel()
    Eu, Ev = _edges(Eu, Ev)
    return Lib().quadratic_d1_bounds(
        np.zeros(V, dt), np.asarray(Y, dt),
        A if sparse else np.asfortranarray(A, dt).ravel(order="F"),
        N, Eu, Ev, np.asarray(La_d1, dt), Bnd[0], Bnd[1],
        SCAL if L.size == 1 else DIAG, L, rho, condMin, difRcd, difTol, itMax,
        obj, dif, verbose)


def PFDR_graph_l22_d1_bounds(Y, La_l2, Eu, Ev, La_d1, Bnd, rho, condMin,
                             difRcd, difTol, itMax, verbose=0, obj=False,
                             dif=False):
    """octave/mex/PFDR_graph_l22_d1_bounds_mex.cpp."""
    Y = np.asarray(Y)
    dt, V, La_l2, Yw = _l22_scale(Y, La_l2)
    Eu, Ev = _edges(Eu, Ev)
    X, it, Obj, Dif = Lib().quadratic_d1_bounds(
        np.zeros(V, dt), Yw, La_l2, 0, Eu, Ev, np.asarray(La_d1, dt), Bnd[0],
        Bnd[1], DIAG, La_l2, rho, condMin, difRcd, difTol, itMax, obj, dif,
        verbose)
    _l22_correct(Obj, it, Y, La_l2, dt)
    return X, it, Obj, Dif


def PFDR_graph_loss_d1_simplex(Q, al, Eu, Ev, La_d1, rho, condMin, difRcd,
                               difTol, itMax, verbose=0, obj=False,
                               dif=False, La_f=None, P0=None):
    """octave/mex/PFDR_graph_loss_d1_simplex_mex.cpp: Q is K-by-V (column v
    = Q[:, v]); P starts at Q (:33) and La_f is NULL (:46) unless given."""
    Q = np.asarray(Q)
    dt = np.result_type(Q, np.float32)
    K = Q.shape[0]
    q = np.asfortranarray(Q, dt).ravel(order="F")
    p0 = q if P0 is None else np.asfortranarray(P0, dt).ravel(order="F")
    Eu, Ev = _edges(Eu, Ev)
    P, it, Obj, Dif = Lib().loss_d1_simplex(
        p0, q, K, Eu, Ev, np.asarray(La_d1, dt), al, La_f, rho, condMin,
        difRcd, difTol, itMax, obj, dif, verbose)
    return P.reshape(Q.shape, order="F"), it, Obj, Dif


def CP_PFDR_graph_loss_d1_simplex(Q, al, Eu, Ev, La_d1, CP_difTol, CP_itMax, PFDR_rho,
                                  PFDR_condMin, PFDR_difRcd, PFDR_difTol, PFDR_itMax, verbose=0,
                                  time=False, obj=False, dif=False):
    """octave/mex/CP_PFDR_graph_loss_d1_simplex_mex.cpp: cut pursuit for the
    loss (al = 0 linear, 1 quadratic, else smoothed Kullback-Leibler) of the
    K-by-V Q (column v = Q[:, v]) plus sum_e La_d1 ||p_u - p_v||_1 over the
    simplex, the whole loop on the GPU (pfdr_cp_loss_d1_simplex).  The dtype
    follows Q (float32 or float64).  Returns (Cv, rP, CP_it, Time, Obj, Dif):
    the component of every vertex (int32[V]), the K-by-rV label vectors of
    the components -- the minimiser is rP[:, Cv] -- and the records asked for
    (Time[CP_itMax + 1], Obj[CP_itMax + 1], Dif[CP_itMax]; None otherwise)."""
    Q = np.asarray(Q)
    dt = np.result_type(Q, np.float32)
    K = Q.shape[0]
    q = np.asfortranarray(Q, dt).ravel(order="F")
    Eu, Ev = _edges(Eu, Ev)
    Cv, rP, it, Obj, Dif, Time = Lib().cp_loss_d1_simplex(
        K, q, Eu, Ev, np.asarray(La_d1, dt), al, CP_difTol, CP_itMax, PFDR_rho, PFDR_condMin,
        PFDR_difRcd, PFDR_difTol, PFDR_itMax, verbose, time, obj, dif)
    return Cv, rP.reshape((K, rP.size // K), order="F"), it, Time, Obj, Dif


def _cp_sparse_run(flavour, V, N, Y, A, Eu, Ev, La_d1, own, CP_difTol, CP_itMax, rho, condMin,
                   difRcd, difTol, itMax, verbose, reduced="dense"):
    """Lib._cp_quadratic for a CSC A: one CPSolver, one run (the solver's first
    run is defined to equal the one-call entry); ``reduced``: CPSolver's"""
    if flavour == "bounds":
        kw = dict(lo=own[0], hi=own[1])
    else:
        kw = dict(La_l1=own[0], positivity=own[1], duplex=flavour == "duplex")
    s = CPSolver("bounds" if flavour == "bounds" else "l1", Y, Eu, Ev, La_d1,
                 A=A.astype(Y.dtype), N=N, reduced=reduced, **kw)
    try:
        return s.run(CP_difTol, CP_itMax, rho, condMin, difRcd, difTol, itMax, verbose)
    finally:
        s.close()


def _cp_front(flavour, V, N, Y, A, Eu, Ev, La_d1, own, CP_difTol, CP_itMax, rho, condMin, difRcd,
              difTol, itMax, verbose, time, obj, dif, reduced="dense"):
    """the bounds ("bounds", own = Bnd) and duplex ("duplex", own = (La_l1,
    positivity)) front-ends' common call -> (Cv, rX, CP_it, Time, Obj, Dif), the
    records not asked for None"""
    Eu, Ev = _edges(Eu, Ev)
    if flavour == "duplex":
        own = (_scal_or_vec(own[0], V, Y.dtype), own[1])
    call, kw = Lib()._cp_quadratic, {}
    if isinstance(A, CSC):
        call, kw = _cp_sparse_run, dict(reduced=reduced)
    elif _reduced_mode(reduced) != PFDR_REDUCED_DENSE:
        raise ValueError('reduced="%s" needs A as a CSC' % (reduced,))
    Cv, rX, it, Obj, Dif, Time = call(
        flavour, V, N, Y, A, Eu, Ev, np.asarray(La_d1, Y.dtype), own, CP_difTol, CP_itMax, rho,
        condMin, difRcd, difTol, itMax, verbose, **kw)
    return Cv, rX, it, Time if time else None, Obj if obj else None, Dif if dif else None


def _cp_matrix(A, dt):
    """the N-by-V A of a cut-pursuit front end -> (the CSC as it is, or the
    dense matrix column by column, and its shape)"""
    if isinstance(A, CSC):
        return A, A.shape
    A = np.asarray(A)
    return np.asfortranarray(A, dt).ravel(order="F"), A.shape


def CP_PFDR_graph_quadratic_d1_bounds(Y, A, Eu, Ev, La_d1, Bnd, CP_difTol, CP_itMax, PFDR_rho,
                                      PFDR_condMin, PFDR_difRcd, PFDR_difTol, PFDR_itMax,
                                      verbose=0, time=False, obj=False, dif=False,
                                      reduced="dense"):
    """octave/mex/CP_PFDR_graph_quadratic_d1_bounds_mex.cpp: cut pursuit for
    1/2 ||y - A x||^2 + sum_e La_d1 |x_u - x_v| over Bnd[0] <= x <= Bnd[1]
    (+-inf: no bound), A N-by-V (an array, or a CSC: the same bytes as its
    densified matrix gives), the whole loop on the GPU
    (pfdr_cp_quadratic_d1_bounds).  Returns (Cv, rX, CP_it, Time, Obj, Dif): the
    component of every vertex (int32[V]), the value of every component -- the
    minimiser is rX[Cv] -- and the records asked for (None otherwise).
    reduced="sparse" / "sparse_all" (a CSC A only): CPSolver's sparse reduced
    operator."""
    dt = np.result_type(Y, np.float32)
    A, (N, V) = _cp_matrix(A, dt)
    return _cp_front("bounds", V, N, np.asarray(Y, dt).ravel(), A, Eu, Ev, La_d1, Bnd, CP_difTol,
                     CP_itMax, PFDR_rho, PFDR_condMin, PFDR_difRcd, PFDR_difTol, PFDR_itMax,
                     verbose, time, obj, dif, reduced)


def CP_PFDR_graph_quadratic_d1_bounds_AtA(AtY, AtA, Eu, Ev, La_d1, Bnd, CP_difTol, CP_itMax,
                                          PFDR_rho, PFDR_condMin, PFDR_difRcd, PFDR_difTol,
                                          PFDR_itMax, verbose=0, time=False, obj=False,
                                          dif=False):
    """octave/mex/CP_PFDR_graph_quadratic_d1_bounds_AtA_mex.cpp: the same with
    A^tA (V-by-V) and A^ty given, N = -V; Obj leaves the constant 1/2 ||y||^2 out."""
    dt = np.result_type(AtY, np.float32)
    V = np.asarray(AtY).size
    return _cp_front("bounds", V, -V, np.asarray(AtY, dt).ravel(),
                     np.asfortranarray(AtA, dt).ravel(order="F"), Eu, Ev, La_d1, Bnd, CP_difTol,
                     CP_itMax, PFDR_rho, PFDR_condMin, PFDR_difRcd, PFDR_difTol, PFDR_itMax,
                     verbose, time, obj, dif)


def CP_PFDR_graph_l22_d1_bounds(Y, La_l2, Eu, Ev, La_d1, Bnd, CP_difTol, CP_itMax, PFDR_rho,
                                PFDR_condMin, PFDR_difRcd, PFDR_difTol, PFDR_itMax, verbose=0,
                                time=False, obj=False, dif=False):
    """octave/mex/CP_PFDR_graph_l22_d1_bounds_mex.cpp:62-90: Y <- La_l2*Y, N = 0,
    A = La_l2 (diagonal; a scalar: none); Obj += 1/2 ||y||^2_La_l2."""
    Y = np.asarray(Y).ravel()
    dt, V, La_l2, Yw = _l22_scale(Y, La_l2)
    Cv, rX, it, Time, Obj, Dif = _cp_front(
        "bounds", V, 0, Yw, La_l2, Eu, Ev, La_d1, Bnd, CP_difTol, CP_itMax, PFDR_rho,
        PFDR_condMin, PFDR_difRcd, PFDR_difTol, PFDR_itMax, verbose, time, obj, dif)
    _l22_correct(Obj, it, Y, La_l2, dt)
    return Cv, rX, it, Time, Obj, Dif


def CP_PFDR_graph_quadratic_d1_l1_duplex(Y, A, Eu, Ev, La_d1, La_l1, positivity, CP_difTol,
                                         CP_itMax, PFDR_rho, PFDR_condMin, PFDR_difRcd,
                                         PFDR_difTol, PFDR_itMax, verbose=0, time=False,
                                         obj=False, dif=False, reduced="dense"):
    """octave/mex/CP_PFDR_graph_quadratic_d1_l1_duplex_mex.cpp: cut pursuit for
    1/2 ||y - A x||^2 + sum_e La_d1 |x_u - x_v| + sum_v La_l1 |x_v| (x >= 0 with
    positivity), A N-by-V (an array or a CSC), one two-layer cut per iteration,
    the whole loop on the GPU (pfdr_cp_quadratic_d1_l1_duplex).  La_l1: array,
    scalar or None.  Returns (Cv, rX, CP_it, Time, Obj, Dif): the component of every vertex
    (int32[V]), the value of every component -- the minimiser is rX[Cv] -- and
    the records asked for (None otherwise).  reduced="sparse" / "sparse_all" (a
    CSC A only): CPSolver's sparse reduced operator."""
    dt = np.result_type(Y, np.float32)
    A, (N, V) = _cp_matrix(A, dt)
    return _cp_front("duplex", V, N, np.asarray(Y, dt).ravel(), A, Eu, Ev, La_d1,
                     (La_l1, positivity), CP_difTol, CP_itMax, PFDR_rho, PFDR_condMin,
                     PFDR_difRcd, PFDR_difTol, PFDR_itMax, verbose, time, obj, dif, reduced)


def CP_PFDR_graph_l22_d1_l1_duplex(Y, La_l2, Eu, Ev, La_d1, La_l1, positivity, CP_difTol,
                                   CP_itMax, PFDR_rho, PFDR_condMin, PFDR_difRcd, PFDR_difTol,
                                   PFDR_itMax, verbose=0, time=False, obj=False, dif=False):
    """octave/mex/CP_PFDR_graph_l22_d1_l1_duplex_mex.cpp:66-93: Y <- La_l2*Y,
    N = 0, A = La_l2 (diagonal; a scalar: none); Obj += 1/2 ||y||^2_La_l2."""
    Y = np.asarray(Y).ravel()
    dt, V, La_l2, Yw = _l22_scale(Y, La_l2)
    Cv, rX, it, Time, Obj, Dif = _cp_front(
        "duplex", V, 0, Yw, La_l2, Eu, Ev, La_d1, (La_l1, positivity), CP_difTol, CP_itMax,
        PFDR_rho, PFDR_condMin, PFDR_difRcd, PFDR_difTol, PFDR_itMax, verbose, time, obj, dif)
    _l22_correct(Obj, it, Y, La_l2, dt)
    return Cv, rX, it, Time, Obj, Dif


def _binding_inputs(obs, source, target, edge_weight, A, l1_weight):
    """the input conventions of the reference's Python binding (see
    PFDR_quadratic_l1) -> (dtype, N, V, mode, A, obs, Eu, Ev, edge weights[E],
    l1 weights[V])"""
    obs = np.asarray(obs)
    if obs.dtype not in (np.float32, np.float64):
        raise TypeError("Type unknown, must be float32, float64, f4, or f8.")
    dt = obs.dtype
    sparse = isinstance(A, CSC)
    A = A.astype(dt) if sparse else np.asarray(A, dt)
    N = obs.size
    Eu, Ev = _edges(source, target)
    E = Eu.size
    if sparse:
        if A.N != N:
            raise ValueError("A should be either a scalar, a vector of size N, or a N-by-V matrix ")
        V, mode = A.V, "sparse"
    elif A.ndim == 0 or A.size == 1 and A.ndim <= 1 and N != 1:
        V, mode = N, "identity"
    elif A.ndim == 1:
        if A.size != N:
            raise ValueError("A should be either a scalar, vector of size N, or a N-by-V matrix ")
        V, mode = N, "diagonal"
    elif A.ndim == 2:
        if A.shape[0] != N:
            raise ValueError("A should be either a scalar, a vector of size N, or a N-by-V matrix ")
        V, mode = A.shape[1], "matrix"
    else:
        raise ValueError("A should be either a scalar, a vector of size N, or a N-by-V matrix ")
    ew = np.asarray(edge_weight, dt).ravel()
    ew = np.full(E, ew[0], dt) if ew.size == 1 else ew
    lw = np.asarray(l1_weight, dt).ravel()
    lw = np.full(V, lw[0], dt) if lw.size == 1 else lw
    return dt, N, V, mode, A, obs, Eu, Ev, ew, lw


def PFDR_quadratic_l1(obs, source, target, edge_weight, A, l1_weight, positivity=0,
                      PFDR_rho=1.0, PFDR_condMin=1e-3, PFDR_difRcd=0.0, PFDR_difTol=1e-4,
                      PFDR_itMax=10000, verbose=0, lipschitz="bound"):
    """PFDR front-end with the conventions of the reference's Python binding
    (python/CP_quadratic_l1_py.cpp:7-56, 130-258, which wraps CP; this
    entry solves the same functional F(x) = 1/2 ||A x - obs||^2 + sum_e
    edge_weight |x_u - x_v| + sum_v l1_weight |x_v| directly with PFDR):
      * A scalar -> identity (its value discarded); A of shape (N,) ->
        diagonal, obs and A pre-multiplied (obs*A, A*A) as the binding does
        (:121-132); A of shape (N, V) -> the design matrix; a CSC -> the
        sparse design matrix, its Lipschitz information chosen by
        ``lipschitz`` (read for a CSC only): "bound", the default, the scalar
        ||A||_1 ||A||_inf >= ||A||^2 (largest absolute column sum times
        largest absolute row sum); "power", the scalar operator_norm(csc) at
        the dense path's settings (nTol 1e-3, itMax 100, nbInit 10); "diag",
        the diagonal metric lipschitz_diag(csc)[0];
      * edge_weight / l1_weight: array, or scalar broadcast to every edge /
        vertex (the binding's broadcast loops run to V for both, :134-145,
        an out-of-range write for the edge weights when E > V; here each
        fills its own length);
      * source / target: any integer dtype (the binding reinterprets uint32
        as int32, :228-258);
      * defaults from :64-72 (PFDR_rho 1, condMin 1e-3, difRcd 0, difTol
        1e-4, itMax 1e4).
    Returns (x, iterations)."""
    if lipschitz not in ("bound", "power", "diag"):
        raise ValueError('lipschitz must be "bound", "power" or "diag", got %r' % (lipschitz,))
    dt, N, V, mode, A, obs, Eu, Ev, ew, lw = _binding_inputs(obs, source, target, edge_weight,
                                                             A, l1_weight)
    lib = Lib()
    X0 = np.zeros(V, dt)
    if mode == "identity":
        X, it, _, _ = lib.quadratic_d1_l1(X0, obs, None, 0, Eu, Ev, ew, lw, positivity, SCAL,
                                          None, PFDR_rho, PFDR_condMin, PFDR_difRcd,
                                          PFDR_difTol, PFDR_itMax, verbose=verbose)
    elif mode == "diagonal":
        Yd = (obs * A).astype(dt)
        Ad = (A * A).astype(dt)
        X, it, _, _ = lib.quadratic_d1_l1(X0, Yd, Ad, 0, Eu, Ev, ew, lw, positivity, DIAG, Ad,
                                          PFDR_rho, PFDR_condMin, PFDR_difRcd, PFDR_difTol,
                                          PFDR_itMax, verbose=verbose)
    elif mode == "sparse":
        h = A.to_host()
        Ltype = SCAL
        if lipschitz == "power":
            L = np.array([operator_norm(A)[0]], dt)
        elif lipschitz == "diag":
            L, Ltype = lipschitz_diag(h)[0], DIAG
        else:
            a = np.abs(h.val.astype(np.float64))
            cols = np.repeat(np.arange(h.V), np.diff(h.colptr))
            L = np.array([np.bincount(cols, a, h.V).max() *
                          np.bincount(h.rowidx, a, h.N).max()], dt)
        X, it, _, _ = lib.quadratic_d1_l1(X0, obs, h, N, Eu, Ev, ew, lw, positivity, Ltype, L,
                                          PFDR_rho, PFDR_condMin, PFDR_difRcd, PFDR_difTol,
                                          PFDR_itMax, verbose=verbose)
    else:
        Af = np.asfortranarray(A)
        L = np.array([operator_norm(Af)[0]], dt)
        X, it, _, _ = lib.quadratic_d1_l1(X0, obs, Af.ravel(order="F"), N, Eu, Ev, ew, lw,
                                          positivity, SCAL, L, PFDR_rho, PFDR_condMin,
                                          PFDR_difRcd, PFDR_difTol, PFDR_itMax, verbose=verbose)
    return X, it


def _cp_binding(flavour, reduced, obs, source, target, edge_weight, A, l1_weight, positivity,
                *args):
    """CP_quadratic_l1 and CP_quadratic_l1_duplex after their defaults; ``args``:
    Lib._cp_quadratic's from CP_difTol on"""
    dt, N, V, mode, A, obs, Eu, Ev, ew, lw = _binding_inputs(obs, source, target, edge_weight,
                                                             A, l1_weight)
    if mode == "sparse":
        r = _cp_sparse_run(flavour, V, N, obs.ravel(), A, Eu, Ev, ew, (lw, positivity), *args,
                           reduced=reduced)
        return r[0].astype(np.uint32), r[1]
    if _reduced_mode(reduced) != PFDR_REDUCED_DENSE:
        raise ValueError('reduced="%s" needs A as a CSC' % (reduced,))
    if mode == "identity":
        N, A = 0, None
    elif mode == "diagonal":
        N, obs, A = 0, (obs * A).astype(dt), (A * A).astype(dt)
    else:
        A = np.asfortranarray(A).ravel(order="F")
    r = Lib()._cp_quadratic(flavour, V, N, obs, A, Eu, Ev, ew, (lw, positivity), *args)
    return r[0].astype(np.uint32), r[1]


def CP_quadratic_l1(obs, source, target, edge_weight, A, l1_weight, positivity=0,
                    PFDR_rho=1.0, PFDR_condMin=1e-3, CP_difTol=1e-3, PFDR_difRcd=0.0,
                    PFDR_difTol=1e-4, CP_itMax=10, PFDR_itMax=10000, verbose=0, reduced="dense"):
    """The reference's Python binding (python/CP_quadratic_l1_py.cpp:68-76,
    188-259): cut pursuit for F(x) = 1/2 ||A x - obs||^2 + sum_e edge_weight
    |x_u - x_v| + sum_v l1_weight |x_v|, same signature, defaults and input
    conventions (those of PFDR_quadratic_l1; a CSC A runs the resumable solver
    once and gives the bytes of its densified matrix), the whole loop on the GPU
    (pfdr_cp_quadratic_d1_l1).  Returns (Cv, rX): the component of every
    vertex (uint32, as the binding) and the value of every component.
    reduced="sparse" (a CSC A only): CPSolver's sparse reduced operator, which
    agrees with the default to the solvers' tolerances, not to the byte;
    reduced="sparse_all": the premultiplied iterations on stored entries too."""
    return _cp_binding("l1", reduced, obs, source, target, edge_weight, A, l1_weight, positivity,
                       CP_difTol, CP_itMax, PFDR_rho, PFDR_condMin, PFDR_difRcd, PFDR_difTol,
                       PFDR_itMax, verbose)


def CP_quadratic_l1_duplex(obs, source, target, edge_weight, A, l1_weight, positivity=0,
                           PFDR_rho=1.0, PFDR_condMin=1e-3, CP_difTol=1e-3, PFDR_difRcd=0.0,
                           PFDR_difTol=1e-4, CP_itMax=10, PFDR_itMax=10000, verbose=0,
                           reduced="dense"):
    """CP_quadratic_l1 through the duplex driver (one two-layer cut per
    iteration, pfdr_cp_quadratic_d1_l1_duplex): same signature, defaults, input
    conventions and returns."""
    return _cp_binding("duplex", reduced, obs, source, target, edge_weight, A, l1_weight, positivity,
                       CP_difTol, CP_itMax, PFDR_rho, PFDR_condMin, PFDR_difRcd, PFDR_difTol,
                       PFDR_itMax, verbose)


def proj_simplex_metric(X, M, A):
    """Column-wise metric simplex projection of the D-by-N array X
    (include/proj_simplex.hpp:33-35); M is D-by-nm, A has na entries."""
    X = np.asarray(X)
    dt = np.result_type(X, np.float32)
    D = X.shape[0]
    N = X.shape[1] if X.ndim > 1 else 1
    M = np.asarray(M, dt)
    nm = M.shape[1] if M.ndim > 1 else 1
    A = np.atleast_1d(np.asarray(A, dt))
    out = Lib().proj_simplex_metric(np.asfortranarray(X, dt).ravel(order="F"),
                                    np.asfortranarray(M, dt).ravel(order="F"),
                                    D, N, nm, A, A.size)
    return out.reshape(X.shape, order="F")


def _producers_done():
    """Device inputs are read on the library's own stream, which does not
    wait for torch's: finish the kernels torch has queued (the producers of
    the tensors handed over) before the library reads them
    (include/pfdr_mi355x.h, PFDR_MEM_DEVICE)."""
    import torch
    torch.cuda.current_stream().synchronize()


# ------------------------------------------------------------- sessions ---
class Session:
    """Device-resident solve: setup once, iterate in steps (benchmarks,
    repeated solves).  Arrays may be numpy (host) or torch CUDA tensors
    (device pointers, mem = PFDR_MEM_DEVICE)."""

    def __init__(self, kind, dtype, V, E, Eu, Ev, La_d1, X0, Y, N=0, A=None,
                 La_l1=None, positivity=0, lo=-np.inf, hi=np.inf, K=0,
                 al=0.0, Ltype=SCAL, L=None, rho=1.5, condMin=1e-3,
                 difRcd=0.0, difTol=0.0, itMax=1000, record_obj=False,
                 record_dif=False, verbose=0, device=False, nranks=0, rank=0,
                 comm=None, comm_kind=0, vtx_begin=0, V_global=0, e_global=None,
                 e_offset=0, reorder=REORDER_AUTO, evolution=EVOLUTION_AUTO,
                 vtx_label=None, spec=SPEC_AUTO, reusable=False):
        self.lib = load()
        ct, _, dcode = _real(dtype)
        self._keep = []
        self.device, self.reusable = bool(device), bool(reusable)
        if device:
            _producers_done()

        def addr(a, is_int=False):
            if a is None:
                return None
            if device:
                return C.c_void_p(a.data_ptr())
            a = np.ascontiguousarray(a, np.int32 if is_int else dtype)
            self._keep.append(a)
            return C.c_void_p(a.ctypes.data)

        # a CSC for A: pfdr_session_create_sparse, its arrays where the
        # session's other arrays are (N defaults to the CSC's row count)
        csc = None
        if isinstance(A, CSC):
            csc = (A.to_device() if device else A.to_host()).astype(dtype)
            self._keep.append(csc)
            N = N or csc.N
            A = None

        p = Problem()
        p.kind, p.dtype = kind, dcode
        p.mem = PFDR_MEM_DEVICE if device else PFDR_MEM_HOST
        p.V, p.E, p.N, p.K = V, E, N, K
        p.X, p.Y, p.A = addr(X0), addr(Y), addr(A)
        p.Eu, p.Ev = addr(Eu, True), addr(Ev, True)
        p.La_d1, p.La_l1, p.L = addr(La_d1), addr(La_l1), addr(L)
        p.positivity, p.min, p.max, p.al = positivity, lo, hi, al
        p.Ltype = Ltype
        p.rho, p.condMin, p.difRcd, p.difTol = rho, condMin, difRcd, difTol
        p.itMax, p.verbose = itMax, verbose
        p.record_obj, p.record_dif = int(record_obj), int(record_dif)
        # 1-D vertex-range partition (see partition.py)
        p.nranks, p.rank = nranks, rank
        p.comm = comm
        p.comm_kind = comm_kind
        p.vtx_begin, p.V_global, p.e_offset = vtx_begin, V_global, e_offset
        p.reorder = reorder
        p.evolution = evolution
        p.spec = spec
        if vtx_label is not None:
            vl = np.ascontiguousarray(vtx_label, np.int64)
            self._keep.append(vl)
            p.vtx_label = C.c_void_p(vl.ctypes.data)
        if e_global is not None:
            eg = np.ascontiguousarray(e_global, np.int64)
            self._keep.append(eg)
            p.e_global = C.c_void_p(eg.ctypes.data)
        self.problem = p
        self.dtype = np.dtype(dtype)
        self.V, self.K = V, max(K, 1)
        self.itMax = itMax
        self.record_obj, self.record_dif = record_obj, record_dif
        h = C.c_void_p()
        if csc is not None:
            self.csc = csc
            if device:
                _producers_done()  # (the conversions above may have queued copies)
            cs = csc.struct()
        if reusable:
            _check(self.lib.pfdr_session_create_reusable(
                C.byref(h), C.byref(p), None if csc is None else C.byref(cs)),
                "pfdr_session_create_reusable")
        elif csc is not None:
            _check(self.lib.pfdr_session_create_sparse(C.byref(h), C.byref(p), C.byref(cs)),
                   "pfdr_session_create_sparse")
        else:
            _check(self.lib.pfdr_session_create(C.byref(h), C.byref(p)),
                   "pfdr_session_create")
        self.h = h

    def sparse_csr(self):
        """(rowptr, colidx, rval): the CSR view a sparse session built
        (pfdr_debug_session_csr)"""
        rp = np.zeros(self.problem.N + 1, np.int64)
        ci = np.zeros(self.csc.nnz, np.int32)
        rv = np.zeros(self.csc.nnz, self.dtype)
        _check(self.lib.pfdr_debug_session_csr(self.h, C.c_void_p(rp.ctypes.data),
                                               C.c_void_p(ci.ctypes.data),
                                               C.c_void_p(rv.ctypes.data)),
               "pfdr_debug_session_csr")
        return rp, ci, rv

    def run(self, iters):
        it = C.c_int(0)
        _check(self.lib.pfdr_session_run(self.h, C.c_int(iters), C.byref(it)),
               "pfdr_session_run")
        return it.value

    def sync(self):
        _check(self.lib.pfdr_session_sync(self.h), "pfdr_session_sync")

    def prepare(self, iters):
        """capture the hipGraphs run(iters) will replay (no iteration runs)"""
        _check(self.lib.pfdr_session_prepare(self.h, C.c_int(int(iters))), "pfdr_session_prepare")

    def reload(self, Y=None, La_d1=None, La_l1=None, X0=None, L=None, lo=None, hi=None,
               rho=None, condMin=None, difRcd=None, difTol=None, itMax=None):
        """New values on the kept graph and matrix, back to iteration 0
        (pfdr_session_reload; the session was created with reusable=True).
        None keeps the current value; for X0 that is the current iterate (a
        warm start).  Arrays as at creation: numpy, or torch GPU tensors when
        the session was created with device=True."""
        p = self.problem
        keep = []
        if self.device:
            _producers_done()

        def addr(a):
            if a is None:
                return None
            if self.device:
                keep.append(a)
                return C.c_void_p(a.data_ptr())
            a = np.ascontiguousarray(a, self.dtype)
            keep.append(a)
            return C.c_void_p(a.ctypes.data)

        def scalar(new, cur):
            return cur if new is None else new

        r = Reload()
        r.mem = p.mem
        r.X, r.Y, r.La_d1, r.La_l1, r.L = addr(X0), addr(Y), addr(La_d1), addr(La_l1), addr(L)
        r.min, r.max = scalar(lo, p.min), scalar(hi, p.max)
        r.rho, r.condMin = scalar(rho, p.rho), scalar(condMin, p.condMin)
        r.difRcd, r.difTol = scalar(difRcd, p.difRcd), scalar(difTol, p.difTol)
        r.itMax = scalar(itMax, p.itMax)
        _check(self.lib.pfdr_session_reload(self.h, C.byref(r)), "pfdr_session_reload")
        # (the call has copied every array; the scalars are the session's now)
        p.min, p.max, p.rho, p.condMin = r.min, r.max, r.rho, r.condMin
        p.difRcd, p.difTol, p.itMax = r.difRcd, r.difTol, r.itMax

    def profile(self, on=True, period=1, only=None):
        """time kernels with HIP events: every `period`-th launch, of the
        kernels named in `only` (all when None)"""
        _check(self.lib.pfdr_session_profile_filter(
            self.h, None if not only else ",".join(only).encode()), "pfdr_session_profile_filter")
        _check(self.lib.pfdr_session_set_profiling(
            self.h, C.c_int(0 if not on else max(int(period), 1))), "pfdr_session_set_profiling")

    def kernel_stats(self, name):
        n, ms = C.c_int(0), C.c_double(0.0)
        _check(self.lib.pfdr_session_kernel_stats(
            self.h, name.encode(), C.byref(n), C.byref(ms)),
            "pfdr_session_kernel_stats")
        return n.value, ms.value

    def query(self, what):
        v = C.c_int64(0)
        _check(self.lib.pfdr_session_query(self.h, what.encode(), C.byref(v)),
               "pfdr_session_query")
        return v.value

    def device_bytes(self):
        return int(self.lib.pfdr_session_device_bytes(self.h))

    def result(self):
        X = np.zeros(self.V * self.K, self.dtype)
        it = C.c_int(0)
        Obj = np.zeros(self.itMax + 1, self.dtype) if self.record_obj else None
        Dif = np.zeros(max(self.itMax, 1), self.dtype) if self.record_dif else None
        _check(self.lib.pfdr_session_result(
            self.h, C.c_void_p(X.ctypes.data), C.byref(it),
            None if Obj is None else C.c_void_p(Obj.ctypes.data),
            None if Dif is None else C.c_void_p(Dif.ctypes.data)),
            "pfdr_session_result")
        return X, it.value, Obj, Dif

    def close(self):
        if getattr(self, "h", None):
            self.lib.pfdr_session_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchSession:
    """B dense-A problems (kind l1 or bounds; direct, N > 0, or A^tA, N = -V)
    that share A, the graph, the penalties and every scalar and differ in the
    observation and the iterate, iterated in lock step: one pass over A serves
    a group of channels (pfdr_batch_*, include/pfdr_mi355x.h).  ``X0`` is
    (B, V) and ``Y`` is (B, len), len = N or V; ``B`` defaults to
    ``Y.shape[0]``; the other keywords are Session's.  Channel b gives the
    bytes of a Session on (X0[b], Y[b]).  Arrays are numpy, or torch GPU
    tensors with ``device=True``."""

    def __init__(self, kind, dtype, V, E, Eu, Ev, La_d1, X0, Y, N=0, A=None, B=None,
                 La_l1=None, positivity=0, lo=-np.inf, hi=np.inf, Ltype=SCAL, L=None, rho=1.5,
                 condMin=1e-3, difRcd=0.0, difTol=0.0, itMax=1000, record_obj=False,
                 record_dif=False, verbose=0, device=False, reorder=REORDER_AUTO,
                 evolution=EVOLUTION_AUTO, spec=SPEC_AUTO):
        ct, _, dcode = _real(dtype)
        self.dtype = np.dtype(dtype)
        self.device = bool(device)
        self._keep = []
        V, E, N = int(V), int(E), int(N)
        self.len = N if N > 0 else V
        if B is None:
            if getattr(Y, "ndim", 0) != 2:
                raise PFDRError("BatchSession: Y must have shape (B, %d)" % self.len)
            B = int(Y.shape[0])
        B = int(B)
        self.B, self.V = B, V
        self._shape("X0", X0, (B, V), False)
        self._shape("Y", Y, (B, self.len), False)
        if A is not None:
            if isinstance(A, CSC):
                raise PFDRError("BatchSession: a sparse A is not offered (dense A only)")
            self._shape("A", A, None, False, size=self.len * V)
        self._shape("La_d1", La_d1, (E,), False)
        self._shape("La_l1", La_l1, (V,), True)
        self.lib = load()
        if device:
            _producers_done()
        p = Problem()
        p.kind, p.dtype = kind, dcode
        p.mem = PFDR_MEM_DEVICE if device else PFDR_MEM_HOST
        p.V, p.E, p.N = V, E, N
        p.X, p.Y, p.A = self._addr(X0), self._addr(Y), self._addr(A)
        p.Eu, p.Ev = self._addr(Eu, np.int32), self._addr(Ev, np.int32)
        p.La_d1, p.La_l1, p.L = self._addr(La_d1), self._addr(La_l1), self._addr(L)
        p.positivity, p.min, p.max = positivity, lo, hi
        p.Ltype = Ltype
        p.rho, p.condMin, p.difRcd, p.difTol = rho, condMin, difRcd, difTol
        p.itMax, p.verbose = itMax, verbose
        p.record_obj, p.record_dif = int(record_obj), int(record_dif)
        p.reorder, p.evolution, p.spec = reorder, evolution, spec
        self.problem = p
        self.itMax = itMax
        self.record_obj, self.record_dif = bool(record_obj), bool(record_dif)
        self.h = None
        self.h = Lib().batch_create(p, B)

    def _shape(self, name, a, shape, optional, size=None):
        """the shape and dtype of an input, before the library is called"""
        if a is None:
            if optional:
                return
            raise PFDRError("BatchSession: %s is required" % name)
        if self.device != _is_device(a):
            raise PFDRError("BatchSession: %s must be a %s (device=%s)" % (
                name, "torch GPU tensor" if self.device else "numpy array", self.device))
        got = tuple(a.shape)
        if shape is not None and got != tuple(shape):
            raise PFDRError("BatchSession: %s has shape %s, expected %s" % (name, got, shape))
        if size is not None and int(np.prod(got)) != size:
            raise PFDRError("BatchSession: %s has %d entries, expected %d" % (
                name, int(np.prod(got)), size))
        if self.device:
            import torch
            want = torch.float32 if self.dtype == np.float32 else torch.float64
            if a.dtype != want or not a.is_contiguous():
                raise PFDRError("BatchSession: %s must be a contiguous %s tensor" % (name, want))
        elif np.asarray(a).dtype != self.dtype:
            raise PFDRError("BatchSession: %s has dtype %s, expected %s" % (
                name, np.asarray(a).dtype, self.dtype))

    def _addr(self, a, dt=None, keep=None):
        if a is None:
            return None
        keep = self._keep if keep is None else keep
        if self.device:
            keep.append(a)
            return C.c_void_p(a.data_ptr())
        # (A: column major, given flat or as an (N, V) Fortran-ordered array)
        a = np.asarray(a)
        if a.ndim == 2 and a.flags.f_contiguous and not a.flags.c_contiguous:
            a = a.T
        a = np.ascontiguousarray(a, dt or self.dtype)
        keep.append(a)
        return C.c_void_p(a.ctypes.data)

    def run(self, iters):
        """up to `iters` more iterations of every channel -> its (B,)"""
        its = np.zeros(self.B, np.int32)
        Lib().batch_run(self.h, int(iters), its)
        return its

    def result(self):
        """-> X (B, V), it (B,), Obj, Dif: lists of per-channel arrays cut to
        the channel's own it (Obj: it + 1 values), or None where not recorded"""
        B, m = self.B, self.itMax
        X = np.zeros((B, self.V), self.dtype)
        its = np.zeros(B, np.int32)
        Obj = np.zeros((B, m + 1), self.dtype) if self.record_obj else None
        Dif = np.zeros(B * max(m, 0) + 1, self.dtype) if self.record_dif else None
        Lib().batch_result(self.h, X, its, Obj, Dif)
        if Obj is not None:
            Obj = [Obj[b, :its[b] + 1].copy() for b in range(B)]
        if Dif is not None:
            Dif = [Dif[b * m:b * m + its[b]].copy() for b in range(B)]
        return X, its, Obj, Dif

    def reload(self, Y=None, X0=None, La_d1=None, La_l1=None, L=None, lo=None, hi=None,
               rho=None, condMin=None, difRcd=None, difTol=None, itMax=None):
        """pfdr_batch_reload: new values for every channel, back to iteration
        0.  Y (B, len) and X0 (B, V) are per channel (None: kept; for X0 a warm
        start of every channel from its own iterate); La_d1, La_l1 and L are
        shared; None keeps a scalar."""
        p = self.problem
        self._shape("Y", Y, (self.B, self.len), True)
        self._shape("X0", X0, (self.B, self.V), True)
        self._shape("La_d1", La_d1, (p.E,), True)
        self._shape("La_l1", La_l1, (self.V,), True)
        if self.device:
            _producers_done()
        keep = []

        def scalar(new, cur):
            return cur if new is None else new

        r = Reload()
        r.mem = p.mem
        r.X, r.Y = self._addr(X0, keep=keep), self._addr(Y, keep=keep)
        r.La_d1, r.La_l1 = self._addr(La_d1, keep=keep), self._addr(La_l1, keep=keep)
        r.L = self._addr(L, keep=keep)
        r.min, r.max = scalar(lo, p.min), scalar(hi, p.max)
        r.rho, r.condMin = scalar(rho, p.rho), scalar(condMin, p.condMin)
        r.difRcd, r.difTol = scalar(difRcd, p.difRcd), scalar(difTol, p.difTol)
        r.itMax = scalar(itMax, p.itMax)
        Lib().batch_reload(self.h, r)
        p.min, p.max, p.rho, p.condMin = r.min, r.max, r.rho, r.condMin
        p.difRcd, p.difTol, p.itMax = r.difRcd, r.difTol, r.itMax

    def query(self, what):
        return Lib().batch_query(self.h, what)

    def close(self):
        if getattr(self, "h", None):
            self.lib.pfdr_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------ device group ----
def set_devices(devices, min_vertices=-1):
    """Partition this process's drop-in calls (Lib, and any CP / C++ caller of
    the library) across `devices` (a list of device ids; [] = one GPU): one
    host thread per device, RCCL over xGMI, bit-identical to one GPU.  Calls
    below min_vertices vertices (< 0: 2^20) stay on one GPU.  A list repeating
    one device runs the ranks as threads on it (loopback; tests)."""
    devs = [int(d) for d in devices]
    arr = (C.c_int * max(len(devs), 1))(*devs)
    lib = load()
    lib.pfdr_set_devices.argtypes = [C.c_int, C.c_void_p, C.c_int64]
    _check(lib.pfdr_set_devices(len(devs), arr if devs else None, int(min_vertices)),
           "pfdr_set_devices")


# ------------------------------------------------------- native inputs ----
def gen_knn_jitter_grid(shape, k=6, seed=6, jitter=0.25, v_range=None):
    """Native twin of graphs.knn_jitter_grid (multi-threaded C++)."""
    nx, ny, nz = shape
    V = nx * ny * nz
    v0, v1 = (0, V) if v_range is None else v_range
    n = (v1 - v0) * k
    Eu = np.empty(n, np.int32)
    Ev = np.empty(n, np.int32)
    got = load().pfdr_gen_knn_jitter_grid(nx, ny, nz, k, seed, jitter, v0, v1,
                                          Eu.ctypes.data, Ev.ctypes.data)
    if got != n:
        raise PFDRError("pfdr_gen_knn_jitter_grid failed")
    return Eu, Ev


def gen_grid_edges(shape, conn, v_range=None):
    nx, ny = shape[0], shape[1]
    nz = shape[2] if len(shape) > 2 else 1
    V = nx * ny * nz
    v0, v1 = (0, V) if v_range is None else v_range
    lib = load()
    n = lib.pfdr_gen_grid_edges(nx, ny, nz, conn, v0, v1, None, None)
    if n < 0:
        raise PFDRError("pfdr_gen_grid_edges: unsupported connectivity")
    Eu = np.empty(n, np.int32)
    Ev = np.empty(n, np.int32)
    lib.pfdr_gen_grid_edges(nx, ny, nz, conn, v0, v1, Eu.ctypes.data,
                            Ev.ctypes.data)
    return Eu, Ev


def gram(A, which=0, device=False):
    """G = A^t A (which = 0) or A A^t (which = 1) on the matrix cores.
    A: (M, N) numpy array (any order; treated as the matrix) or, with
    device=True, a torch CUDA tensor holding the column-major M-by-N matrix
    as a (N, M) contiguous tensor.  Returns (G, kernel_ms)."""
    lib = load()
    ms = C.c_double(0.0)
    if device:
        import torch
        _producers_done()
        N, M = A.shape
        P = N if which == 0 else M
        G = torch.empty((P, P), dtype=A.dtype, device=A.device)
        fn = lib.pfdr_gram_f32 if A.dtype == torch.float32 else lib.pfdr_gram_f64
        _check(fn(which, M, N, C.c_void_p(A.data_ptr()), PFDR_MEM_DEVICE,
                  C.c_void_p(G.data_ptr()), C.byref(ms)), "pfdr_gram")
        return G, ms.value
    A = np.asarray(A)
    M, N = A.shape
    Af = np.asfortranarray(A)
    ct, sfx, _ = _real(Af.dtype)
    P = N if which == 0 else M
    G = np.empty((P, P), Af.dtype, order="F")
    _check(getattr(lib, "pfdr_gram_" + sfx)(which, M, N, C.c_void_p(Af.ctypes.data),
                                             PFDR_MEM_HOST, C.c_void_p(G.ctypes.data),
                                             C.byref(ms)), "pfdr_gram")
    return np.ascontiguousarray(G), ms.value


def sequential_sum(a, seed=0.0, method=0):
    """seed + a[0] + ... + a[n-1] rounded as the one-thread loop, for
    nonnegative terms (the preconditioner's amplitude sum).  method 0: the
    workgroup binade scan the solvers use, 1: one lane.  Returns (sum, ms)."""
    lib = load()
    a = np.ascontiguousarray(a)
    ct, sfx, _ = _real(a.dtype)
    fn = getattr(lib, "pfdr_sequential_sum_" + sfx)
    fn.argtypes = [C.c_int64, C.c_void_p, C.c_int, ct, C.c_int, C.c_void_p, C.c_void_p]
    out, ms = ct(0), C.c_double(0.0)
    _check(fn(a.size, C.c_void_p(a.ctypes.data) if a.size else None, PFDR_MEM_HOST, ct(seed),
              method, C.byref(out), C.byref(ms)), "pfdr_sequential_sum")
    return a.dtype.type(out.value), ms.value


def operator_norm(A, nTol=1e-3, itMax=100, nbInit=10, symmetric=False, device=False,
                  M=None, N=None, verbose=0):
    """||A||^2 (reference operator_norm_matrix).  symmetric=True: A is the
    S-by-S A^tA / AA^t itself (the reference's M or N = 0).  device=True: A
    is a torch CUDA tensor, column-major M-by-N stored as (N, M).  Returns
    (norm2, gram_ms).  A CSC (host arrays or torch GPU tensors) goes through
    pfdr_operator_norm_csc_*, the power method on the stored entries, and
    returns (norm2, ms_power); symmetric, device, M and N do not apply."""
    lib = load()
    if isinstance(A, CSC):
        ct, sfx, _ = _real(A.dtype)
        if A.device:
            _producers_done()
        csc, out, ms = A.struct(), ct(0), (C.c_double * 2)()
        _check(getattr(lib, "pfdr_operator_norm_csc_" + sfx)(
            A.N, A.V, C.byref(csc), PFDR_MEM_DEVICE if A.device else PFDR_MEM_HOST, ct(nTol),
            itMax, nbInit, verbose, C.byref(out), ms), "pfdr_operator_norm_csc")
        return out.value, ms[1]
    gms = C.c_double(0.0)
    if device:
        import torch
        _producers_done()
        Nn, Mm = A.shape
        if symmetric:
            Mm, Nn = 0, Nn
        ct = C.c_float if A.dtype == torch.float32 else C.c_double
        fn = lib.pfdr_operator_norm_f32 if A.dtype == torch.float32 else lib.pfdr_operator_norm_f64
        out = ct(0)
        _check(fn(Mm, Nn, C.c_void_p(A.data_ptr()), PFDR_MEM_DEVICE, ct(nTol), itMax, nbInit,
                  verbose, C.byref(out), C.byref(gms)), "pfdr_operator_norm")
        return out.value, gms.value
    A = np.asarray(A)
    Af = np.asfortranarray(A)
    ct, sfx, _ = _real(Af.dtype)
    Mm, Nn = (0, A.shape[0]) if symmetric else A.shape
    out = ct(0)
    _check(getattr(lib, "pfdr_operator_norm_" + sfx)(Mm, Nn, C.c_void_p(Af.ctypes.data),
                                                      PFDR_MEM_HOST, ct(nTol), itMax, nbInit,
                                                      verbose, C.byref(out), C.byref(gms)),
           "pfdr_operator_norm")
    return out.value, gms.value


def lipschitz_diag(csc):
    """The diagonal Lipschitz majorant of a CSC (pfdr_lipschitz_diag_csc_*):
    L[v] = sum_i |A_iv| sum_j |A_ij|, valid ``Ltype = DIAG`` input, and the
    scalar bound ||A||_1 ||A||_inf >= max L.  Returns (L, bound): L a numpy
    array, or a torch tensor beside a device CSC's arrays."""
    if not isinstance(csc, CSC):
        raise TypeError("lipschitz_diag takes a pfdr.CSC")
    lib = load()
    ct, sfx, _ = _real(csc.dtype)
    st, bound = csc.struct(), ct(0)
    if csc.device:
        import torch
        _producers_done()
        L = torch.empty(max(csc.V, 0), dtype=csc.val.dtype, device=csc.val.device)
        ptr, mem = L.data_ptr(), PFDR_MEM_DEVICE
    else:
        L = np.empty(max(csc.V, 0), csc.dtype)
        ptr, mem = L.ctypes.data, PFDR_MEM_HOST
    _check(getattr(lib, "pfdr_lipschitz_diag_csc_" + sfx)(
        csc.N, csc.V, C.byref(st), mem, C.c_void_p(ptr), C.byref(bound)),
        "pfdr_lipschitz_diag_csc")
    return L, csc.dtype.type(bound.value)


def _reduced_mode(reduced):
    """"dense" / "sparse" / "sparse_all" -> PFDR_REDUCED_*; an integer as it is
    (the library refuses the ones it does not know)"""
    modes = {"dense": PFDR_REDUCED_DENSE, "sparse": PFDR_REDUCED_SPARSE,
             "sparse_all": PFDR_REDUCED_SPARSE_ALL}
    if isinstance(reduced, str):
        if reduced not in modes:
            raise ValueError('reduced must be "dense", "sparse" or "sparse_all", got %r' % (
                reduced,))
        return modes[reduced]
    return int(reduced)


def cp_reduce(N, A, Y, comp_ptr, comp_vertices, preAt=True, normTol=1e-3, normItMax=100,
              normNbInit=10, reduced="dense"):
    """CP reduced-problem builder (pfdr_cp_reduce_*): A is (N, V) for
    N > 0 (or (V, V) A^tA for N < 0, length-V diagonal / None for N = 0),
    comp_ptr (rV + 1) and comp_vertices (V) the components; a CSC A (N > 0)
    goes through pfdr_cp_reduce_csc_* and gives the bytes of its densified
    matrix.  Returns dict rA, rAA, rY, L, Leq (None where not formed).
    reduced="sparse" (a CSC A, preAt=False): pfdr_cp_reduce_csc_sparse_*, "rA"
    is a host CSC (N-by-rV) that is never densified, rAA and rY are None.
    reduced="sparse_all" (a CSC A): the same for preAt=False, and for
    preAt=True pfdr_cp_reduce_csc_sparse_preAt_*: "rA" is that CSC (not
    scaled), rAA and rY are summed over its stored entries."""
    Y = np.asarray(Y)
    dt = Y.dtype
    ct, sfx, _ = _real(dt)
    ptr = np.ascontiguousarray(comp_ptr, np.int32)
    Vc = np.ascontiguousarray(comp_vertices, np.int32)
    rV, V = ptr.size - 1, Vc.size
    Af = None
    sparse = isinstance(A, CSC)
    mode = _reduced_mode(reduced)
    if mode not in (PFDR_REDUCED_DENSE, PFDR_REDUCED_SPARSE, PFDR_REDUCED_SPARSE_ALL):
        raise ValueError('cp_reduce: reduced must be "dense", "sparse" or "sparse_all", got %r'
                         % (reduced,))
    if mode != PFDR_REDUCED_DENSE:
        if not sparse:
            raise ValueError('cp_reduce: reduced="%s" needs A as a CSC' % (reduced,))
        if preAt and mode == PFDR_REDUCED_SPARSE:
            raise ValueError('cp_reduce: reduced="sparse" is the direct branch, preAt=False')
        A = A.to_host().astype(dt)
        csc = A.struct()
        Yc = np.ascontiguousarray(Y)
        rnnz = C.c_int64(0)
        rcolptr = np.zeros(rV + 1, np.int64)
        rrowidx, rval = np.zeros(A.nnz, np.int32), np.zeros(A.nnz, dt)
        L, Leq = np.zeros(rV, dt), np.zeros(rV, dt)
        rAA = rY = None
        p = lambda a: C.c_void_p(a.ctypes.data)
        head = (C.c_int(N), C.c_int(V), C.byref(csc), p(Yc), C.c_int(rV), p(ptr), p(Vc),
                PFDR_MEM_HOST, ct(normTol), C.c_int(normItMax), C.c_int(normNbInit))
        kept = (C.byref(rnnz), p(rcolptr), p(rrowidx), p(rval))
        if preAt:
            rAA, rY = np.zeros((rV, rV), dt), np.zeros(rV, dt)
            _check(getattr(load(), "pfdr_cp_reduce_csc_sparse_preAt_" + sfx)(
                *head, p(rAA), p(rY), p(L), p(Leq), *kept), "pfdr_cp_reduce_csc_sparse_preAt")
        else:
            _check(getattr(load(), "pfdr_cp_reduce_csc_sparse_" + sfx)(
                *head, *kept, p(L), p(Leq)), "pfdr_cp_reduce_csc_sparse")
        n = rnnz.value
        return {"rA": CSC(rcolptr, rrowidx[:n].copy(), rval[:n].copy(), N), "rAA": rAA,
                "rY": rY, "L": L, "Leq": Leq}
    if sparse:
        A = A.to_host().astype(dt)
        csc = A.struct()
    elif A is not None:
        Af = np.asfortranarray(np.asarray(A, dt)) if np.ndim(A) == 2 else np.ascontiguousarray(A, dt)
    if N <= 0:
        preAt = True
    rA = np.zeros((rV, N), dt) if N > 0 else None        # column rv = rA[rv]
    rAA = (np.zeros(rV, dt) if N == 0 else np.zeros((rV, rV), dt)) if preAt else None
    rY = np.zeros(rV, dt) if preAt else None
    L = np.zeros(rV, dt)
    Leq = np.zeros(rV, dt) if N != 0 else None
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    _check(getattr(load(), "pfdr_cp_reduce_" + ("csc_" if sparse else "") + sfx)(
        C.c_int(N), C.c_int(V), C.byref(csc) if sparse else p(Af), p(np.ascontiguousarray(Y)), C.c_int(rV), p(ptr), p(Vc),
        C.c_int(int(preAt)), PFDR_MEM_HOST, ct(normTol), C.c_int(normItMax),
        C.c_int(normNbInit), p(rA), p(rAA), p(rY), p(L), p(Leq)), "pfdr_cp_reduce")
    return {"rA": None if rA is None else rA.T, "rAA": rAA, "rY": rY, "L": L, "Leq": Leq}


class CPGraph:
    """Device-resident cut-pursuit graph (pfdr_cpgraph_*, SURVEY.md §8(f)
    ranks 2-3): the full-graph steps of every CP iteration of
    src/CP_PFDR_graph_quadratic_d1_l1.cpp with the reference's results and
    orders.  Arrays in and out are numpy (host); the cut between
    ``capacities`` and ``activate`` is ``mincut`` (or the caller's own)."""

    def __init__(self, V, Eu, Ev, La_d1, La_l1=None):
        La_d1 = np.asarray(La_d1)
        self.dtype = La_d1.dtype
        self.ct, _, code = _real(self.dtype)
        self.V = int(V)
        Eu, Ev = _edges(Eu, Ev)
        self.E = Eu.size
        La_d1 = _arr(La_d1, self.dtype)
        La_l1 = _arr(La_l1, self.dtype)
        self._keep = (Eu, Ev, La_d1, La_l1)
        self.h = C.c_void_p()
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        _check(load().pfdr_cpgraph_create(C.byref(self.h), code, C.c_int(self.V),
                                          C.c_int(self.E), p(Eu), p(Ev), p(La_d1), p(La_l1),
                                          PFDR_MEM_HOST), "pfdr_cpgraph_create")
        self.has_l1 = La_l1 is not None
        self.rV = 1

    @staticmethod
    def _p(a):
        return None if a is None else C.c_void_p(a.ctypes.data)

    def _call(self, name, *args):
        _check(getattr(load(), name)(self.h, *args), name)

    def set_active(self, active):
        a = np.ascontiguousarray(active, np.uint8)
        self._call("pfdr_cpgraph_set_active", self._p(a), PFDR_MEM_HOST)

    def active(self):
        a = np.empty(self.E, np.uint8)
        self._call("pfdr_cpgraph_get_active", self._p(a), PFDR_MEM_HOST)
        return a

    def set_components(self, Cv, Vc, rVc):
        Cv, Vc, rVc = (np.ascontiguousarray(x, np.int32) for x in (Cv, Vc, rVc))
        self.rV = rVc.size - 1
        self._call("pfdr_cpgraph_set_components", C.c_int(self.rV), self._p(Cv), self._p(Vc),
                   self._p(rVc), PFDR_MEM_HOST)

    def components(self):
        """:566-597 -> (Cv, Vc, rVc)"""
        rV = C.c_int()
        self._call("pfdr_cpgraph_components", C.byref(rV))
        self.rV = rV.value
        Cv = np.empty(self.V, np.int32)
        Vc = np.empty(self.V, np.int32)
        rVc = np.empty(self.rV + 1, np.int32)
        self._call("pfdr_cpgraph_get_components", None, self._p(Cv), self._p(Vc), self._p(rVc),
                   PFDR_MEM_HOST)
        return Cv, Vc, rVc

    def set_values(self, rX):
        x = np.ascontiguousarray(rX, self.dtype)
        self._call("pfdr_cpgraph_set_values", self._p(x), PFDR_MEM_HOST)

    def reduced_graph(self, eps):
        """:599-661 -> (rEu, rEv, rLa_d1, rLa_l1 or None)"""
        rE = C.c_int()
        self._call("pfdr_cpgraph_reduced_graph", C.c_double(eps), C.byref(rE))
        n = rE.value
        rEu = np.empty(n, np.int32)
        rEv = np.empty(n, np.int32)
        rLa = np.empty(n, self.dtype)
        rL1 = np.empty(self.rV, self.dtype) if self.has_l1 else None
        self._call("pfdr_cpgraph_get_reduced", self._p(rEu), self._p(rEv), self._p(rLa),
                   self._p(rL1), PFDR_MEM_HOST)
        return rEu, rEv, rLa, rL1

    def merge(self, eps, difTol):
        """:863-886 -> number of deactivated edges"""
        n = C.c_int()
        self._call("pfdr_cpgraph_merge", C.c_double(eps), C.c_double(difTol), C.byref(n))
        return n.value

    def gradient(self, N=0, A=None, Y=None, R=None):
        """:339-413 -> DfS[V]; a CSC A (N > 0): pfdr_cpgraph_gradient_csc"""
        if isinstance(A, CSC):
            A = A.to_host().astype(self.dtype)
            R = _arr(R, self.dtype)
            DfS = np.empty(self.V, self.dtype)
            csc = A.struct()
            self._call("pfdr_cpgraph_gradient_csc", C.c_int(N), C.byref(csc), self._p(R),
                       PFDR_MEM_HOST, self._p(DfS))
            return DfS
        Af = None
        if A is not None:
            Af = (np.asfortranarray(np.asarray(A, self.dtype)) if np.ndim(A) == 2
                  else np.ascontiguousarray(A, self.dtype))
        Y = _arr(Y, self.dtype)
        R = _arr(R, self.dtype)
        DfS = np.empty(self.V, self.dtype)
        self._call("pfdr_cpgraph_gradient", C.c_int(N), self._p(Af), self._p(Y), self._p(R),
                   PFDR_MEM_HOST, self._p(DfS))
        return DfS

    def capacities(self, cut, positivity=0):
        """:402-535 -> (tr_cap[V], r_cap[E]) of cut 0 (differentiable), 1 or 2"""
        tr = np.empty(self.V, self.dtype)
        rc = np.empty(self.E, self.dtype)
        self._call("pfdr_cpgraph_capacities", C.c_int(cut), C.c_int(int(positivity)),
                   self._p(tr), self._p(rc), PFDR_MEM_HOST)
        return tr, rc

    def capacities_bounds(self, cut, lo=-np.inf, hi=np.inf):
        """bounds driver (src/CP_PFDR_graph_quadratic_d1_bounds.cpp:386-534)
        -> (tr_cap[V], r_cap[E]) of cut 0 (no bound), 1 or 2"""
        tr = np.empty(self.V, self.dtype)
        rc = np.empty(self.E, self.dtype)
        self._call("pfdr_cpgraph_capacities_bounds", C.c_int(cut), C.c_double(lo),
                   C.c_double(hi), self._p(tr), self._p(rc), PFDR_MEM_HOST)
        return tr, rc

    def activate(self, segment):
        """activate the inactive edges the cut separates -> how many"""
        seg = np.ascontiguousarray(segment, np.uint8)
        n = C.c_int()
        self._call("pfdr_cpgraph_activate", self._p(seg), PFDR_MEM_HOST, C.byref(n))
        return n.value

    def mincut(self, tr_cap, r_cap, arcs=ARCS_BOTH):
        """minimum cut of the capacities ``capacities`` / ``capacities_bounds``
        (ARCS_BOTH) or ``simplex_capacities`` (ARCS_FORWARD) give -> (segment[V]
        uint8: 0 = reachable from the source in the residual graph, the
        reference's maxflow labels; cut value; push/relabel rounds)"""
        tr = np.ascontiguousarray(tr_cap, self.dtype)
        rc = np.ascontiguousarray(r_cap, self.dtype)
        if tr.size != self.V or rc.size != self.E:
            raise ValueError("mincut: tr_cap must have V and r_cap E entries")
        seg = np.empty(self.V, np.uint8)
        flow = C.c_double()
        rounds = C.c_int64()
        self._call("pfdr_cpgraph_mincut", C.c_int(int(arcs)), self._p(tr),
                   self._p(rc) if self.E else None, PFDR_MEM_HOST, self._p(seg),
                   C.byref(flow), C.byref(rounds))
        return seg, flow.value, rounds.value

    def mincut_duplex(self, tr_cap, r_link, r_cap):
        """minimum cut of the two-layer network ``capacities_duplex`` gives
        (node v and node V + v per vertex) -> (segment[2V] uint8: 0 = reachable
        from the source in the residual graph, the reference's maxflow labels;
        cut value; push/relabel rounds)"""
        tr = np.ascontiguousarray(tr_cap, self.dtype)
        ln = np.ascontiguousarray(r_link, self.dtype)
        rc = np.ascontiguousarray(r_cap, self.dtype)
        if tr.size != 2 * self.V or ln.size != self.V or rc.size != self.E:
            raise ValueError("mincut_duplex: tr_cap must have 2V, r_link V and r_cap E entries")
        seg = np.empty(2 * self.V, np.uint8)
        flow = C.c_double()
        rounds = C.c_int64()
        self._call("pfdr_cpgraph_mincut_duplex", self._p(tr), self._p(ln),
                   self._p(rc) if self.E else None, PFDR_MEM_HOST, self._p(seg),
                   C.byref(flow), C.byref(rounds))
        return seg, flow.value, rounds.value

    def mincut_relabels(self):
        """global relabels of the last ``mincut`` or ``mincut_duplex``"""
        n = C.c_int64()
        self._call("pfdr_cpgraph_mincut_relabels", C.byref(n))
        return n.value

    # ---- the duplex driver's two-layer cut (src/CP_PFDR_graph_quadratic_d1_l1_duplex.cpp)
    def capacities_duplex(self, positivity=0):
        """:469-527 -> (tr_cap[2V]: v1 then v2 nodes, r_link[V], r_cap[E])"""
        tr = np.empty(2 * self.V, self.dtype)
        link = np.empty(self.V, self.dtype)
        rc = np.empty(self.E, self.dtype)
        self._call("pfdr_cpgraph_capacities_duplex", C.c_int(int(positivity)), self._p(tr),
                   self._p(link), self._p(rc), PFDR_MEM_HOST)
        return tr, link, rc

    def activate_duplex(self, segment):
        """:531-545, segment[2V] -> how many edges were activated"""
        seg = np.ascontiguousarray(segment, np.uint8)
        if seg.size != 2 * self.V:
            raise ValueError("segment must hold 2V entries")
        n = C.c_int()
        self._call("pfdr_cpgraph_activate_duplex", self._p(seg), PFDR_MEM_HOST, C.byref(n))
        return n.value

    # ---- the simplex driver (src/CP_PFDR_graph_loss_d1_simplex.cpp); P
    # layouts vertex-major [v*K + k]
    def simplex_setup(self, K, al, Q):
        """K labels, loss al (0 linear, 1 quadratic, else smoothed KL), Q[V*K]"""
        self.K = int(K)
        self.al = float(al)
        self._Q = np.ascontiguousarray(Q, self.dtype).reshape(-1)
        if self._Q.size != self.V * self.K:
            raise ValueError("Q must hold V*K values")
        self._call("pfdr_cpgraph_simplex_setup", C.c_int(self.K), C.c_double(self.al),
                   self._p(self._Q), PFDR_MEM_HOST)

    def simplex_observations(self):
        """:733-766 -> (rP[rV*K], rQ[rV*K], rLa_f[rV] or None when al == 0);
        rP becomes the component values"""
        n = self.rV * self.K
        rP = np.empty(n, self.dtype)
        rQ = np.empty(n, self.dtype)
        rLa_f = np.empty(self.rV, self.dtype) if self.al != 0 else None
        self._call("pfdr_cpgraph_simplex_observations", self._p(rP), self._p(rQ),
                   self._p(rLa_f), PFDR_MEM_HOST)
        return rP, rQ, rLa_f

    def simplex_set_values(self, rP):
        x = np.ascontiguousarray(rP, self.dtype).reshape(-1)
        if x.size != self.rV * self.K:
            raise ValueError("rP must hold rV*K values")
        self._call("pfdr_cpgraph_simplex_set_values", self._p(x), PFDR_MEM_HOST)

    def simplex_gradient(self, eps):
        """:327-376, :525-536 -> (DfS[V*K], rDi[rV])"""
        DfS = np.empty(self.V * self.K, self.dtype)
        rDi = np.empty(self.rV, np.int32)
        self._call("pfdr_cpgraph_simplex_gradient", C.c_double(eps), self._p(DfS),
                   rDi.ctypes.data_as(C.POINTER(C.c_int)), PFDR_MEM_HOST)
        return DfS, rDi

    def simplex_capacities(self, n):
        """:542-595 -> (tr_cap[V], r_cap[E] of arc 2e; arc 2e + 1 has none)"""
        tr = np.empty(self.V, self.dtype)
        rc = np.empty(self.E, self.dtype)
        self._call("pfdr_cpgraph_simplex_capacities", C.c_int(n), self._p(tr), self._p(rc),
                   PFDR_MEM_HOST)
        return tr, rc

    def simplex_expand(self, n, segment):
        seg = np.ascontiguousarray(segment, np.uint8)
        self._call("pfdr_cpgraph_simplex_expand", C.c_int(n), self._p(seg), PFDR_MEM_HOST)

    def simplex_labels(self):
        D = np.empty(self.V, np.int32)
        self._call("pfdr_cpgraph_simplex_labels", D.ctypes.data_as(C.POINTER(C.c_int)),
                   PFDR_MEM_HOST)
        return D

    def simplex_activate(self):
        n = C.c_int()
        self._call("pfdr_cpgraph_simplex_activate", C.byref(n))
        return n.value

    def simplex_merge(self, eps):
        n = C.c_int()
        self._call("pfdr_cpgraph_simplex_merge", C.c_double(eps), C.byref(n))
        return n.value

    def close(self):
        if self.h:
            load().pfdr_cpgraph_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _CPSolverType(type):
    """CPSolver(..., reduced="dense" | "sparse" | "sparse_all"): the keyword is no argument of
    the constructor proper but a set_reduced() on the finished solver, which
    the library refuses (PFDRError) unless A came as a CSC"""

    def __call__(cls, *args, reduced="dense", **kw):
        mode = _reduced_mode(reduced)
        s = super().__call__(*args, **kw)
        if mode != PFDR_REDUCED_DENSE:
            try:
                s.set_reduced(mode)
            except Exception:
                s.close()
                raise
        return s


class CPSolver(metaclass=_CPSolverType):
    """The resumable cut pursuit (pfdr_cp_solver_*): the problem, its graph and
    the cut-pursuit state stay on the device between calls.

    kind: "l1", "bounds" or "simplex" (or PFDR_KIND_*); duplex=True with "l1" is
    the duplex driver.  Y_or_Q, A, N as the one-call entries (Q[V*K] vertex-major
    with K for the simplex).  Every array is a numpy array (host) or a torch
    tensor on the GPU (device pointers; copied by the library, except A, which
    is borrowed and kept alive here).  A may be a CSC ("l1" and "bounds", N > 0
    or taken from it; host, or to_device() with the other arrays on the GPU):
    it is copied, V is its column count, and every call gives the bytes of the
    solver on the densified matrix (pfdr_cp_solver_create_sparse).  With a CSC,
    reduced="sparse" (or set_reduced) keeps the reduced operator of a direct
    iteration sparse as well (pfdr_cp_solver_set_reduced): the dense N-by-rV
    array is never allocated there, and a run then agrees with the default to the
    solvers' tolerances; reduced="sparse_all" also sums the normal equations of
    a premultiplied iteration over the stored entries of a sparse rA, with the
    default's bytes (premultiplied_stats() counts them).  The first run() equals the matching
    Lib.cp_* call byte for byte; every later one is the reference's warm restart
    from the state the handle holds."""

    KINDS = {"l1": PFDR_KIND_L1, "bounds": PFDR_KIND_BOUNDS, "simplex": PFDR_KIND_SIMPLEX}

    def __init__(self, kind, Y_or_Q, Eu, Ev, La_d1, A=None, N=0, La_l1=None, positivity=0,
                 lo=-np.inf, hi=np.inf, K=0, al=0.1, duplex=False):
        self._L = Lib()
        self.kind = self.KINDS.get(kind, kind)
        self._h = None
        dev = _is_device(Y_or_Q)
        if dev:
            import torch
            self.dtype = np.dtype(str(Y_or_Q.dtype).replace("torch.", ""))
            _producers_done()
            size = lambda a: int(a.numel())
            ints = lambda a: a.to(torch.int32).contiguous()
            reals = lambda a: a.contiguous()
        else:
            Y_or_Q = np.ascontiguousarray(Y_or_Q)
            self.dtype = Y_or_Q.dtype
            size = lambda a: int(a.size)
            ints = lambda a: np.ascontiguousarray(a, np.int32)
            reals = lambda a: np.ascontiguousarray(a, self.dtype).ravel()
        self._ct, _, dcode = _real(self.dtype)
        self.device = dev
        simplex = self.kind == PFDR_KIND_SIMPLEX
        self.K = int(K) if simplex else 1
        self.N = 0 if simplex else int(N)
        csc = None
        if isinstance(A, CSC):
            if A.device != dev:
                raise TypeError("CPSolver: a CSC on the GPU goes with arrays on the GPU, a host "
                                "CSC with host arrays")
            csc, A = A.astype(self.dtype), None
            self.N = self.N or csc.N
        arrs = [None if a is None else reals(a) for a in (Y_or_Q, A, La_d1, La_l1)]
        Eu, Ev = ints(Eu), ints(Ev)
        if csc is not None:
            self.V = csc.V
        elif self.N > 0 and arrs[1] is not None:
            self.V = size(arrs[1]) // self.N
        else:
            self.V = size(arrs[0]) // max(self.K, 1)
        self.E = size(Eu)
        self._keep = arrs + [Eu, Ev]  # A is borrowed for the solver's lifetime
        p = CPProblem()
        p.kind, p.duplex, p.dtype = self.kind, int(bool(duplex)), dcode
        p.mem = PFDR_MEM_DEVICE if dev else PFDR_MEM_HOST
        p.V, p.E, p.N, p.K = self.V, self.E, self.N, int(K) if simplex else 0
        p.Y, p.A, p.La_d1, p.La_l1 = (self._addr(a) for a in arrs)
        p.Eu, p.Ev = self._addr(Eu), self._addr(Ev)
        p.positivity, p.min, p.max, p.al = int(positivity), lo, hi, al
        self.has_l1 = La_l1 is not None
        self._h = self._L.cp_solver_create(p, None if csc is None else csc.struct())
        if not dev:
            self._keep = []

    @staticmethod
    def _addr(a):
        if a is None:
            return None
        return a.data_ptr() if _is_device(a) else a.ctypes.data

    def run(self, CP_difTol=1e-3, CP_itMax=10, rho=1.0, condMin=1e-3, difRcd=0.0, difTol=1e-4,
            itMax=10000, verbose=0, obj=True, dif=True, time=True):
        """-> (Cv[V] int32, rX[rV] (rP[rV*K]), CP_it, Obj[CP_itMax + 1], Dif[CP_itMax],
        Time[CP_itMax + 1]); a record not asked for is passed as NULL and None"""
        CP_itMax = int(CP_itMax)
        q = CPParams(CP_difTol, CP_itMax, rho, condMin, difRcd, difTol, int(itMax), int(verbose))
        Obj = np.zeros(CP_itMax + 1, self.dtype) if obj else None
        Dif = np.zeros(max(CP_itMax, 1), self.dtype) if dif else None
        Time = np.zeros(CP_itMax + 1, np.float64) if time else None
        it = C.c_int(0)
        self._L.cp_solver_run(self._h, q, C.addressof(it), self._addr(Time), self._addr(Obj),
                              self._addr(Dif))
        Cv = np.zeros(self.V, np.int32)
        rX = np.zeros(self.V * self.K, self.dtype)
        rV = C.c_int(0)
        self._L.cp_solver_get_state(self._h, rV=C.addressof(rV), Cv=Cv.ctypes.data,
                                    rX=rX.ctypes.data)
        return (Cv, rX[:rV.value * self.K].copy(), it.value, Obj,
                None if Dif is None else Dif[:CP_itMax], Time)

    def state(self, device=False):
        """-> dict: active[E] uint8, Cv[V], Vc[V], rVc[rV + 1] int32, rX[rV]
        (rP[rV*K]) and, for N > 0, R[N]; numpy arrays, or torch tensors on the GPU"""
        V, E, K = self.V, self.E, self.K
        rV = C.c_int(0)
        if device:
            import torch
            td = getattr(torch, self.dtype.name)
            new = lambda n, t: torch.empty(max(n, 1), dtype=t, device="cuda")
            i32, u8 = torch.int32, torch.uint8
        else:
            td, i32, u8 = self.dtype, np.int32, np.uint8
            new = lambda n, t: np.zeros(max(n, 1), t)
        st = dict(active=new(E, u8), Cv=new(V, i32), Vc=new(V, i32), rVc=new(V + 1, i32),
                  rX=new(V * K, td))
        if self.N > 0:
            st["R"] = new(self.N, td)
        self._L.cp_solver_get_state(
            self._h, C.addressof(rV), self._addr(st["Cv"]), self._addr(st["Vc"]),
            self._addr(st["rVc"]), self._addr(st["active"]), self._addr(st["rX"]),
            self._addr(st.get("R")), PFDR_MEM_DEVICE if device else PFDR_MEM_HOST)
        r = rV.value
        st["active"] = st["active"][:E]
        st["rVc"] = st["rVc"][:r + 1]
        st["rX"] = st["rX"][:r * K]
        return st

    def set_state(self, state, R="given"):
        """Replace the state (a dict as state() returns; torch tensors on the GPU
        are read in place).  R=None: the residual is recomputed on the device;
        by default state["R"] is used when present."""
        dev = _is_device(state["Cv"])
        if dev:
            _producers_done()
            cvt = lambda a, t: a.contiguous()
            rV = int(state["rVc"].numel()) - 1
        else:
            cvt = lambda a, t: np.ascontiguousarray(a, t)
            rV = int(np.size(state["rVc"])) - 1
        Cv, Vc, rVc = (cvt(state[k], np.int32) for k in ("Cv", "Vc", "rVc"))
        act = cvt(state["active"], np.uint8)
        rX = cvt(state["rX"], self.dtype)
        Rv = state.get("R") if isinstance(R, str) else R
        Rv = None if Rv is None or self.N <= 0 else cvt(Rv, self.dtype)
        self._L.cp_solver_set_state(
            self._h, rV, self._addr(Cv), self._addr(Vc), self._addr(rVc),
            self._addr(act) if self.E > 0 else None, self._addr(rX), self._addr(Rv),
            PFDR_MEM_DEVICE if dev else PFDR_MEM_HOST)

    def set_partition(self, label, values):
        """A state from a label per vertex and a value per label (what the
        drivers return): edges between labels become active, the components are
        those of that activity, each takes its label's value"""
        dev = _is_device(label)
        if dev:
            _producers_done()
            label, values = label.contiguous(), values.contiguous()
            n = int(values.numel()) // self.K
        else:
            label = np.ascontiguousarray(label, np.int32)
            values = np.ascontiguousarray(values, self.dtype).ravel()
            n = values.size // self.K
        self._L.cp_solver_set_partition(self._h, n, self._addr(label), self._addr(values),
                                        PFDR_MEM_DEVICE if dev else PFDR_MEM_HOST)

    def set_penalties(self, La_d1=None, La_l1=None):
        """Overwrite La_d1[E] and / or La_l1[V]; the state is kept"""
        dev = _is_device(La_d1) or _is_device(La_l1)
        if dev:
            _producers_done()
            cvt = lambda a: None if a is None else a.contiguous()
        else:
            cvt = lambda a: None if a is None else np.ascontiguousarray(a, self.dtype).ravel()
        La_d1, La_l1 = cvt(La_d1), cvt(La_l1)
        self._L.cp_solver_set_penalties(self._h, self._addr(La_d1), self._addr(La_l1),
                                        PFDR_MEM_DEVICE if dev else PFDR_MEM_HOST)

    def set_reduced(self, reduced):
        """"dense", "sparse" or "sparse_all" (pfdr_cp_solver_set_reduced): how
        the reduced operator of a direct iteration ("sparse") and of a
        premultiplied one as well ("sparse_all") is kept; a solver with a CSC A
        only.  The state is kept."""
        self._L.cp_solver_set_reduced(self._h, _reduced_mode(reduced))

    def reduced_stats(self):
        """-> (direct iterations solved on a sparse rA, direct iterations solved
        on a dense one, the most entries a sparse rA held) of the last run"""
        return self._L.cp_solver_reduced_stats(self._h)

    def premultiplied_stats(self):
        """-> (premultiplied iterations, N > 0, solved from the stored entries
        of a sparse rA, those that formed a dense rA, the most entries such a
        sparse rA held) of the last run"""
        return self._L.cp_solver_premultiplied_stats(self._h)

    def stats(self):
        """-> dict: seconds per phase and counts of the last run, and the seconds
        the constructor's setup took"""
        setup = C.c_double(0)
        out = _cp_stats(lambda sec, cnt: self._L.cp_solver_stats(self._h, sec, cnt,
                                                                 C.addressof(setup)))
        out["setup"] = setup.value
        return out

    def close(self):
        if self._h is not None:
            self._L.cp_solver_destroy(self._h)
            self._h = None
            self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grid_edge_count(shape, conn, v_end):
    """Edges gen_grid_edges emits for the vertices [0, v_end) (the global id
    of a slab's first edge)."""
    nx, ny = shape[0], shape[1]
    nz = shape[2] if len(shape) > 2 else 1
    n = load().pfdr_gen_grid_edges(nx, ny, nz, conn, 0, v_end, None, None)
    if n < 0:
        raise PFDRError("pfdr_gen_grid_edges: unsupported connectivity")
    return int(n)


def gen_piecewise(nx, V, seed, dtype=np.float32, noise=0.2, v_range=None):
    v0, v1 = (0, V) if v_range is None else v_range
    Y = np.empty(v1 - v0, dtype)
    fn = (load().pfdr_gen_piecewise_f32 if np.dtype(dtype) == np.float32
          else load().pfdr_gen_piecewise_f64)
    fn(nx, seed, noise, v0, v1, Y.ctypes.data)
    return Y


def _gen_fn(name, dtype):
    _, sfx, _ = _real(dtype)
    return getattr(load(), "pfdr_gen_%s_%s" % (name, sfx))


def gen_uniform(seed, n, lo, hi, dtype=np.float32, i0=0, out=None):
    """out[i] = lo + (hi - lo) U(seed, i0 + i) (native, multi-threaded)."""
    out = np.empty(n, dtype) if out is None else out
    fn = _gen_fn("uniform", out.dtype)
    fn.argtypes = [C.c_uint64, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_void_p]
    _check(fn(seed, i0, n, lo, hi, out.ctypes.data), "pfdr_gen_uniform")
    return out


def gen_matvec(A_cm, N, V, x):
    """y = A x for the column-major N-by-V matrix held in A_cm (length N V),
    each row summed in double in increasing column order (deterministic)."""
    y = np.empty(N, A_cm.dtype)
    x = np.ascontiguousarray(x, A_cm.dtype)
    fn = _gen_fn("matvec", A_cm.dtype)
    fn.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(fn(N, V, A_cm.ctypes.data, x.ctypes.data, y.ctypes.data), "pfdr_gen_matvec")
    return y


def gen_symmetric(V, seed, s, d, dtype=np.float32):
    """Symmetric diagonally dominant V-by-V matrix (flat, column-major)."""
    G = np.empty(V * V, dtype)
    fn = _gen_fn("symmetric", dtype)
    fn.argtypes = [C.c_int64, C.c_uint64, C.c_double, C.c_double, C.c_void_p]
    _check(fn(V, seed, s, d, G.ctypes.data), "pfdr_gen_symmetric")
    return G
