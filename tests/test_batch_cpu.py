"""CPU: the batched dense sessions (pfdr_batch_*, include/pfdr_mi355x.h) refuse
what they do not offer with the offence named, before any device work -- so
without a device --, a NULL handle is refused by every entry, and the Python
front end checks shapes and dtypes before the library is called."""
import ctypes as C

import numpy as np
import pytest

from cp_pfdr_graph_d1_amd import pfdr

V, N, E, B = 6, 4, 5, 3
DT = np.float32


def _arrays(n=N):
    ln = n if n > 0 else V
    return dict(X=np.zeros((B, V), DT), Y=np.ones((B, ln), DT), A=np.ones(ln * V, DT),
                Eu=np.arange(E, dtype=np.int32), Ev=np.arange(1, E + 1, dtype=np.int32),
                La_d1=np.full(E, 0.1, DT))


def _problem(keep, n=N, kind=pfdr.PFDR_KIND_L1, **over):
    a = _arrays(n)
    keep.append(a)
    p = pfdr.Problem()
    p.kind, p.dtype, p.mem = kind, pfdr.PFDR_F32, pfdr.PFDR_MEM_HOST
    p.V, p.E, p.N = V, E, n
    for k in ("X", "Y", "A", "Eu", "Ev", "La_d1"):
        setattr(p, k, C.c_void_p(a[k].ctypes.data))
    p.rho, p.condMin, p.itMax = 1.5, 1e-3, 10
    p.min, p.max = -1.0, 1.0
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _refused(p, b, *words):
    with pytest.raises(pfdr.PFDRError) as e:
        h = pfdr.Lib().batch_create(p, b)
        pfdr.Lib().batch_destroy(h)  # (not reached)
    msg = str(e.value)
    assert "pfdr_batch_create" in msg, msg
    for w in words:
        assert w in msg, (w, msg)
    return msg


@pytest.mark.parametrize("b", [0, -1, 65, 1000])
def test_channel_count_outside_1_64(b):
    keep = []
    _refused(_problem(keep), b, "B must be in [1, 64]", str(b))


def test_identity_and_diagonal_matrices_name_the_reusable_session():
    keep = []
    msg = _refused(_problem(keep, n=0), B, "N == 0", "pfdr_session_create_reusable")
    assert "pfdr_session_reload" in msg
    _refused(_problem(keep, n=0, A=None), B, "N == 0")


def test_simplex_kind():
    keep = []
    _refused(_problem(keep, kind=pfdr.PFDR_KIND_SIMPLEX), B, "simplex")
    _refused(_problem(keep, kind=7), B, "unknown problem kind")


@pytest.mark.parametrize("n", [N, -V])
def test_matrix_required(n):
    keep = []
    _refused(_problem(keep, n=n, A=None), B, "A == NULL")


def test_partitions_and_communicators():
    keep = []
    _refused(_problem(keep, nranks=2), B, "one GPU", "device group")
    hub = np.zeros(8, np.int64)
    _refused(_problem(keep, comm=C.c_void_p(hub.ctypes.data)), B, "communicator")


def test_what_a_session_refuses_for_one_channel():
    keep = []
    _refused(_problem(keep, Y=None), B, "Y")
    _refused(_problem(keep, La_d1=None), B, "La_d1")
    _refused(_problem(keep, V=0), B, "V must be > 0")
    _refused(_problem(keep, n=-(V + 1)), B, "N = -V")
    _refused(_problem(keep, dtype=5), B, "dtype")
    _refused(_problem(keep, kind=pfdr.PFDR_KIND_BOUNDS, min=2.0, max=1.0), B, "min > max")


def test_null_arguments():
    lib = pfdr.load()
    h = C.c_void_p()
    assert lib.pfdr_batch_create(C.byref(h), None, C.c_int(2)) != 0
    assert b"null" in lib.pfdr_last_error()
    keep = []
    p = _problem(keep)
    assert lib.pfdr_batch_create(None, C.byref(p), C.c_int(2)) != 0


def test_null_handle_refused_by_every_entry():
    L = pfdr.Lib()
    its = np.zeros(B, np.int32)
    for call in (lambda: L.batch_run(None, 1, its),
                 lambda: L.batch_result(None, None, its, None, None),
                 lambda: L.batch_reload(None, pfdr.Reload()),
                 lambda: L.batch_query(None, "channels")):
        with pytest.raises(pfdr.PFDRError) as e:
            call()
        assert "null batch" in str(e.value)
    L.batch_destroy(None)  # a no-op


def test_no_handle_after_a_refusal():
    lib = pfdr.load()
    keep = []
    p = _problem(keep, n=0)
    h = C.c_void_p(1)
    assert lib.pfdr_batch_create(C.byref(h), C.byref(p), C.c_int(B)) != 0
    assert h.value is None


def _front(**over):
    a = _arrays()
    kw = dict(kind=pfdr.PFDR_KIND_L1, dtype=DT, V=V, E=E, Eu=a["Eu"], Ev=a["Ev"],
              La_d1=a["La_d1"], X0=a["X"], Y=a["Y"], N=N, A=a["A"])
    kw.update(over)
    return kw


@pytest.mark.parametrize("over,word", [
    (dict(X0=np.zeros((B, V + 1), DT)), "X0 has shape"),
    (dict(X0=np.zeros(B * V, DT)), "X0 has shape"),
    (dict(Y=np.ones((B + 1, N), DT)), "X0 has shape"),   # B follows Y: X0 no longer fits
    (dict(Y=np.ones((B, N + 1), DT)), "Y has shape"),
    (dict(Y=np.ones(B * N, DT)), "Y must have shape"),
    (dict(Y=np.ones((B, N), np.float64)), "Y has dtype"),
    (dict(X0=np.zeros((B, V), np.float64)), "X0 has dtype"),
    (dict(A=np.ones(N * V + 1, DT)), "A has"),
    (dict(A=np.ones(N * V, np.float64)), "A has dtype"),
    (dict(La_d1=np.ones(E + 1, DT)), "La_d1 has shape"),
    (dict(La_l1=np.ones(V + 2, DT)), "La_l1 has shape"),
    (dict(B=2), "X0 has shape"),
    (dict(Y=None, B=B), "Y is required"),
])
def test_python_checks_before_the_library(monkeypatch, over, word):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(pfdr, "load", no_library)
    with pytest.raises(pfdr.PFDRError) as e:
        pfdr.BatchSession(**_front(**over))
    assert word in str(e.value), str(e.value)


def test_python_front_end_signatures():
    import inspect
    names = list(inspect.signature(pfdr.BatchSession.__init__).parameters)
    assert names[1:13] == ["kind", "dtype", "V", "E", "Eu", "Ev", "La_d1", "X0", "Y", "N", "A", "B"]
    assert list(inspect.signature(pfdr.BatchSession.reload).parameters)[1:4] == ["Y", "X0", "La_d1"]
    for m in ("run", "result", "reload", "query", "close"):
        assert callable(getattr(pfdr.BatchSession, m))
    for m in ("create", "run", "result", "reload", "query", "destroy"):
        assert callable(getattr(pfdr.Lib, "batch_" + m))
