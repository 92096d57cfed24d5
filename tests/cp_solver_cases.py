"""Shared by tests/test_cp_solver_*.py: problems as cp_problems dicts for the
four drivers, the resumable solver and the matching one-call entry over one
dict, and the twins restarted from a solver's state."""
import numpy as np
import pytest

pytest.register_assert_rewrite("cp_entry")  # its asserts report their values

import cp_entry as E
import cp_problems as P
import cp_simplex_twin as ST
import cp_twin as T
from cp_fixtures import BNAMES, DNAMES, NAMES, SNAMES, iteration_state, load_case
from cp_pfdr_graph_d1_amd import pfdr

F32, F64 = np.float32, np.float64
same_bytes, STEP = E.same_bytes, E.STEP
STEP_SIMPLEX = dict(rho=1.5, condMin=1e-3, difRcd=0.0, difTol=1e-3, itMax=1000)
FIXTURES = [("l1", n) for n in NAMES] + [("bounds", n) for n in BNAMES] + \
           [("simplex", n) for n in SNAMES] + [("duplex", n) for n in DNAMES]


def fixture_problem(kind, name):
    """-> (problem dict, the fixture's npz) of an iteration fixture"""
    c, d = load_case(name)
    st = STEP_SIMPLEX if kind == "simplex" else STEP
    p = dict(kind=kind, N=0, K=0, CP_itMax=6, PFDR_itMax=st["itMax"], positivity=0,
             CP_difTol=c["CP_difTol"], PFDR_difTol=st["difTol"], rho=st["rho"],
             condMin=st["condMin"], difRcd=st["difRcd"], lo=-np.inf, hi=np.inf, al=0.0,
             A=None, La_l1=None, Eu=c["Eu"], Ev=c["Ev"], La_d1=c["La_d1"], E=c["Eu"].size)
    if kind == "simplex":
        p.update(K=c["K"], al=c["al"], Y=c["Q"], V=c["Q"].size // c["K"])
    else:
        p.update(Y=c["Y"], A=c["A"], V=c["Y"].size)
        if kind == "bounds":
            p.update(lo=c["lo"], hi=c["hi"])
        else:
            p.update(La_l1=c["La_l1"], positivity=c["positivity"])
    p["dtype"] = p["Y"].dtype.type
    return p, d


def small(kind, dt, V):
    """V vertices without an edge"""
    z = np.zeros(0, np.int32)
    p = dict(kind=kind, V=V, E=0, N=0, K=0, dtype=dt, CP_itMax=3, PFDR_itMax=2000,
             positivity=0, CP_difTol=1e-4, PFDR_difTol=1e-5, rho=1.5, condMin=1e-3, difRcd=0.0,
             lo=-np.inf, hi=np.inf, al=0.0, Y=(np.arange(V) % 3 - 0.75).astype(dt), A=None,
             Eu=z, Ev=z, La_d1=np.zeros(0, dt), La_l1=None)
    if kind == "simplex":
        K = 3
        Q = np.full((V, K), 0.1, dt)
        Q[np.arange(V), np.arange(V) % K] = 0.8
        p.update(K=K, al=0.1, Y=Q.ravel(), condMin=0.1, rho=1.0)
    return p


def run_params(p, **over):
    q = dict(CP_difTol=p["CP_difTol"], CP_itMax=p["CP_itMax"], rho=p["rho"],
             condMin=p["condMin"], difRcd=p["difRcd"], difTol=p["PFDR_difTol"],
             itMax=p["PFDR_itMax"])
    q.update(over)
    return q


def solver(p, device=False, **over):
    """the resumable solver of a problem dict; device: torch tensors on the GPU"""
    q = dict(p)
    q.update(over)
    arrs = {k: q[k] for k in ("Y", "Eu", "Ev", "La_d1", "A", "La_l1")}
    if device:
        import torch
        arrs = {k: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
                for k, a in arrs.items()}
    kind = "l1" if q["kind"] == "duplex" else q["kind"]
    return pfdr.CPSolver(kind, arrs["Y"], arrs["Eu"], arrs["Ev"], arrs["La_d1"], A=arrs["A"],
                         N=q["N"], La_l1=arrs["La_l1"], positivity=q["positivity"], lo=q["lo"],
                         hi=q["hi"], K=q["K"], al=q["al"], duplex=q["kind"] == "duplex")


def entry(p, **over):
    """the matching one-call entry -> (Cv, rX, CP_it, Obj, Dif, Time)"""
    q = dict(p)
    q.update(over)
    if q["kind"] != "simplex":
        return E.entry(q["kind"], q)
    return pfdr.Lib().cp_loss_d1_simplex(
        q["K"], q["Y"], q["Eu"], q["Ev"], q["La_d1"], al=q["al"], CP_difTol=q["CP_difTol"],
        CP_itMax=q["CP_itMax"], rho=q["rho"], condMin=q["condMin"], difRcd=q["difRcd"],
        difTol=q["PFDR_difTol"], itMax=q["PFDR_itMax"])


def twin(p, **over):
    """the twin over the library's steps (cp_twin.py, cp_simplex_twin.py) for a problem dict"""
    return (ST if p["kind"] == "simplex" else T).gpu_twin(p, **over)


def twin_restart(t, p, state):
    """restart a fresh twin from a solver's state() (host arrays)"""
    st = dict(state)
    if p["kind"] == "simplex":
        st["rP"] = st["rX"]
        t.restart(st)
    else:
        t.restart(st, state.get("R"))


def fixture_state(d, k, io):
    st = iteration_state(d, k, io)
    if "rP" in st:
        st["rX"] = st.pop("rP").ravel()
    return st


def state_equal(a, b, keys=("active", "Cv", "Vc", "rVc", "rX")):
    return [k for k in keys if not same_bytes(np.asarray(a[k]).ravel(), np.asarray(b[k]).ravel())]


def host(st):
    """a state dict of torch tensors as numpy arrays"""
    return {k: v.cpu().numpy() if hasattr(v, "cpu") else v for k, v in st.items()}


def union_find(V, Eu, Ev, keep):
    """component label of every vertex over the edges with keep[e], plain Python"""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for u, v, k in zip(Eu.tolist(), Ev.tolist(), keep.tolist()):
        if k:
            a, b = find(u), find(v)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(v) for v in range(V)], np.int64)
