"""CPU: the sparse-A (CSC) entries are declared, exported and listed; the
ABI is still 4; pfdr.CSC builds from dense matrices; the new compute entries
fail loudly without a GPU."""
import os
import re

import numpy as np
import pytest

from cp_pfdr_graph_d1_amd import pfdr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "pfdr_mi355x.h")

NEW_ENTRIES = [
    "pfdr_session_create_sparse",
    "pfdr_quadratic_d1_l1_csc_f32", "pfdr_quadratic_d1_l1_csc_f64",
    "pfdr_quadratic_d1_bounds_csc_f32", "pfdr_quadratic_d1_bounds_csc_f64",
]


def test_header_declares_the_sparse_entries_and_abi_4():
    txt = open(HEADER).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    assert re.search(r"typedef\s+struct\s+pfdr_csc\s*\{[^}]*int64_t\s+nnz;[^}]*"
                     r"const\s+int64_t\s*\*colptr;[^}]*const\s+int32_t\s*\*rowidx;[^}]*"
                     r"const\s+void\s*\*val;[^}]*\}\s*pfdr_csc;", txt)
    assert re.search(r"int\s+pfdr_abi_version\(void\);\s*/\*\s*4\b", txt)


def test_library_exports_the_sparse_entries():
    lib = pfdr.load()
    assert lib.pfdr_abi_version() == pfdr.ABI_VERSION == 4
    for name in NEW_ENTRIES:
        assert name in pfdr.EXPORTED, name
        assert hasattr(lib, name), name


def test_csc_from_dense_round_trips():
    rng = np.random.default_rng(3)
    for dt in (np.float32, np.float64):
        A = (rng.standard_normal((13, 9)) * (rng.random((13, 9)) < 0.3)).astype(dt)
        A[:, 4] = 0  # an empty column
        c = pfdr.CSC.from_dense(A)
        assert c.shape == (13, 9) and c.N == 13 and c.V == 9 and c.dtype == dt
        assert c.colptr.dtype == np.int64 and c.rowidx.dtype == np.int32 and c.val.dtype == dt
        assert c.nnz == int((A != 0).sum()) == c.colptr[-1] and c.colptr[0] == 0
        assert c.colptr[4] == c.colptr[5]
        for v in range(9):
            r = c.rowidx[c.colptr[v]:c.colptr[v + 1]]
            assert np.all(np.diff(r) > 0)
            assert np.array_equal(r, np.nonzero(A[:, v])[0])
        assert np.array_equal(c.to_dense(), A)


def test_csc_from_dense_keeps_a_stored_zero():
    A = np.array([[1.0, 0.0], [0.0, 2.0], [3.0, 0.0]], np.float32)
    stored = np.zeros(A.shape, bool)
    stored[1, 0] = True
    c = pfdr.CSC.from_dense(A, stored)
    assert c.nnz == 4
    assert c.colptr.tolist() == [0, 3, 4]
    assert c.rowidx.tolist() == [0, 1, 2, 1]
    assert c.val.tolist() == [1.0, 0.0, 3.0, 2.0]
    assert np.array_equal(c.to_dense(), A)
    assert pfdr.CSC.from_dense(A).nnz == 3


def test_csc_from_scipy_is_duck_typed():
    class Fake:  # what scipy.sparse matrices offer
        shape = (3, 2)
        indptr = np.array([0, 2, 3], np.int32)
        indices = np.array([0, 2, 1], np.int64)
        data = np.array([1.0, 3.0, 2.0])

        def tocsc(self):
            return self

    c = pfdr.CSC.from_scipy(Fake())
    assert c.colptr.dtype == np.int64 and c.rowidx.dtype == np.int32
    assert np.array_equal(c.to_dense(), [[1.0, 0.0], [0.0, 2.0], [3.0, 0.0]])


def _tiny(dt=np.float32):
    A = np.array([[1.0, 0.0, 0.5, 0.0], [0.0, 2.0, 0.0, 1.0]], dt)
    return (pfdr.CSC.from_dense(A), np.ones(2, dt), np.array([0, 1, 2], np.int32),
            np.array([1, 2, 3], np.int32), np.ones(3, dt))


def test_sparse_entries_fail_loudly_without_gpu():
    lib = pfdr.load()
    if lib.pfdr_device_count() > 0:
        pytest.skip("a GPU is visible")
    for dt in (np.float32, np.float64):
        csc, Y, Eu, Ev, La = _tiny(dt)
        with pytest.raises(pfdr.PFDRError):
            pfdr.Lib().quadratic_d1_l1(np.zeros(4, dt), Y, csc, 2, Eu, Ev, La)
        with pytest.raises(pfdr.PFDRError):
            pfdr.Lib().quadratic_d1_bounds(np.zeros(4, dt), Y, csc, 2, Eu, Ev, La, lo=0.0, hi=1.0)
        with pytest.raises(pfdr.PFDRError):
            pfdr.Session(pfdr.PFDR_KIND_L1, dt, 4, 3, Eu, Ev, La, np.zeros(4, dt), Y, A=csc)
