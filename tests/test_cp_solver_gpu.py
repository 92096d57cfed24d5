"""The resumable cut-pursuit solver (pfdr_cp_solver_*, pfdr.CPSolver) on the GPU.

1. the reference's restart, byte for byte: every recorded step of the N = 0
   iteration fixtures of the four drivers, k_in -> one iteration -> k_out;
2. the first run is the one-call entry;
3. a split run is the uninterrupted one (N = 0, N = -V), Obj and Dif included;
4. dense restarts against the twin, one of them flipping preAt; R recomputed;
5. a state exported and imported (host and device arrays) continues alike;
   a dense A given as device arrays runs as the host arrays do;
6. a change of penalties is a restart of a solver created with them;
7. the partition import against the step API, a union-find and the twin;
8. rejected states leave the solver unchanged;
9. repeatability, optional outputs, stats.
"""
import numpy as np
import pytest

import cp_run_cases as RC
import cp_bounds_run_cases as BRC
import cp_duplex_run_cases as DRC
import cp_problems as P
import cp_solver_cases as SC
import cp_twin as T
from cp_fixtures import TIES
from cp_pfdr_graph_d1_amd import pfdr
from cp_solver_cases import F32, F64, same_bytes

pytestmark = pytest.mark.gpu

DTS = (F32, F64)
_dn = lambda dt: "f32" if dt is F32 else "f64"
KINDS = ("l1", "duplex", "bounds", "simplex")


def small_problem(kind, dt, nx=24, ny=20, **over):
    mode = "diag" if kind != "simplex" else None
    return P.problem(kind, mode, dt, nx=nx, ny=ny, **over)


def run(s, p, **over):
    return s.run(**SC.run_params(p, **over))


def out_equal(a, b, what=("Cv", "rX", "it", "Obj", "Dif")):
    names = ("Cv", "rX", "it", "Obj", "Dif")
    bad = []
    for n, x, y in zip(names, a, b):
        if n in what and not (x == y if n == "it" else same_bytes(x, y)):
            bad.append(n)
    return bad


# ------------------------------------------- 1. the reference's restart --
@pytest.mark.parametrize("kind,name", SC.FIXTURES, ids=[n for _, n in SC.FIXTURES])
def test_restart_is_the_references(gpu_lib, kind, name):
    """set_state(k_in), one iteration with the recorder's parameters, state()
    = k_out: the fixtures were recorded through the reference's own CP_restart."""
    p, d = SC.fixture_problem(kind, name)
    s = SC.solver(p)
    for k in range(int(d["meta_steps"])):
        s.set_state(SC.fixture_state(d, k, "in"))
        out = run(s, p, CP_itMax=1)
        assert out[2] == 1, (name, k)
        got = s.state()
        if (name, k) in TIES:  # a tie of the two-layer cut: the twin instead
            print("tie:", name, "k", k)
            t = SC.twin(p)
            SC.twin_restart(t, p, SC.fixture_state(d, k, "in"))
            rec = t.iterate()
            t.b.close()
            assert same_bytes(got["Cv"], rec["Cv"]) and same_bytes(got["rX"], rec["rX"])
            assert same_bytes(got["active"], rec["active"])
            continue
        want = SC.fixture_state(d, k, "out")
        assert SC.state_equal(got, want) == [], (name, k)
        assert same_bytes(out[0], want["Cv"]), (name, k)
    s.close()


# ----------------------------------------- 2. first run = one-call entry --
def first_run_cases():
    for dt in DTS:
        yield "l1_diag", lambda dt=dt: small_problem("l1", dt, CP_itMax=3), dt
        yield "duplex_diag", lambda dt=dt: small_problem("duplex", dt, CP_itMax=3), dt
        yield "bounds_diag", lambda dt=dt: small_problem("bounds", dt, CP_itMax=3), dt
        yield "simplex", lambda dt=dt: small_problem("simplex", dt, CP_itMax=3), dt
    yield "l1_direct12", lambda: dict(RC.problem("direct12", F32), CP_itMax=3), F32
    yield "bounds_direct160", lambda: dict(BRC.problem("direct160", F64), CP_itMax=3), F64
    yield "l1_23x19", lambda: small_problem("l1", F32, nx=23, ny=19, CP_itMax=3), F32
    for kind in KINDS:
        yield kind + "_E0_V5", lambda kind=kind: SC.small(kind, F32, 5), F32
        yield kind + "_E0_V1", lambda kind=kind: SC.small(kind, F64, 1), F64


_first = list(first_run_cases())


@pytest.mark.parametrize("make", [c[1] for c in _first],
                         ids=["%s_%s" % (c[0], _dn(c[2])) for c in _first])
def test_first_run_is_the_entry(gpu_lib, make):
    p = make()
    want = SC.entry(p)
    s = SC.solver(p)
    got = run(s, p)
    s.close()
    assert out_equal(got, want) == []


# ------------------------------------------------------- 3. split runs --
def split_cases():
    for kind in KINDS:
        yield kind, "N0", lambda kind=kind: small_problem(kind, F32, CP_itMax=4)
    yield "l1", "AtA", lambda: dict(RC.problem("AtA", F64), CP_itMax=4)
    yield "bounds", "AtA", lambda: dict(BRC.problem("AtA", F32), CP_itMax=4)
    yield "duplex", "AtA", lambda: dict(DRC.problem("AtA", F32), CP_itMax=4)


_split = list(split_cases())


@pytest.mark.parametrize("make", [c[2] for c in _split], ids=["%s_%s" % c[:2] for c in _split])
def test_split_run_is_the_uninterrupted_one(gpu_lib, make):
    p = make()
    want = SC.entry(p, CP_itMax=4)
    assert want[2] == 4, "the case must not stop before its fourth iteration"
    for k1 in (1, 2, 3):
        k2 = 4 - k1
        s = SC.solver(p)
        a = run(s, p, CP_itMax=k1)
        b = run(s, p, CP_itMax=k2)
        s.close()
        assert a[2] == k1 and b[2] == k2
        assert same_bytes(b[0], want[0]) and same_bytes(b[1], want[1]), k1
        assert same_bytes(b[4][:k2], want[4][k1:4]), k1           # Dif
        assert same_bytes(b[3][1:k2 + 1], want[3][k1 + 1:5]), k1  # Obj
        assert same_bytes(b[3][:1], a[3][k1:k1 + 1]), k1          # Obj[0]: the last one computed
        assert same_bytes(a[3][:k1 + 1], want[3][:k1 + 1]), k1


# ---------------------------------- 4. dense restarts against the twin --
DENSE = [("l1", RC, "direct12", F32), ("l1", RC, "direct160", F64), ("l1", RC, "AtA", F32),
         ("bounds", BRC, "direct12", F64), ("bounds", BRC, "direct160", F32),
         ("bounds", BRC, "AtA", F64),
         ("duplex", DRC, "direct12", F32), ("duplex", DRC, "direct160", F32),
         ("duplex", DRC, "AtA", F64)]


@pytest.mark.parametrize("kind,mod,case,dt", DENSE,
                         ids=["%s_%s_%s" % (k, c, _dn(d)) for k, _, c, d in DENSE])
def test_dense_restart_is_the_twin(gpu_lib, kind, mod, case, dt, first=2, flips=False):
    """R = None recomputes the residual from the component column sums as a
    direct (not premultiplied) iteration leaves them, which is what the loop
    holds after such an iteration: every case here ends on one."""
    p = mod.problem(case, dt)
    s = SC.solver(p)
    run(s, p, CP_itMax=first)
    st = s.state()
    assert ("R" in st) == (p["N"] > 0)
    t = SC.twin(p)
    SC.twin_restart(t, p, st)
    rec = t.iterate()
    t.b.close()
    out = run(s, p, CP_itMax=1)
    got = s.state()
    assert same_bytes(out[0], rec["Cv"]) and same_bytes(out[1], rec["rX"])
    assert same_bytes(got["active"], rec["active"])
    if p["N"] > 0:
        assert same_bytes(got["R"], t.R)
    if p["N"] > 0 and not flips:
        # R = None: recomputed on the device, the bytes of the exported one
        s.set_state(st, R=None)
        assert same_bytes(s.state()["R"], st["R"])
        again = run(s, p, CP_itMax=1)
        assert out_equal(again, out, what=("Cv", "rX", "it", "Dif")) == []
        assert same_bytes(again[3][1:], out[3][1:])
    if flips:
        u = SC.twin(p)
        _, recs = u.run(first + 1)
        u.b.close()
        print("preAt uninterrupted", [r["preAt"] for r in recs], "resumed", rec["preAt"],
              "rV", [r["rV"] for r in recs], "pfdr_it", [r["pfdr_it"] for r in recs])
        assert recs[first]["preAt"] != rec["preAt"], "the case no longer flips preAt"
    s.close()


def test_dense_restart_flips_preAt(gpu_lib):
    """direct160 (N = 160) after one iteration: the first PFDR stops after some
    60 iterations, so the uninterrupted run's second iteration (109 components)
    works on rA directly (109 >= 2 N it / (N + it) = 88), while the resumed one
    decides with PFDR_itMax = 2000 (bound 296) and premultiplies, as the
    reference's restart does.  The handle follows the twin restarted there.
    (The first iteration premultiplied, so R = None is not compared here: the
    equilibration of a direct iteration scales rA and scales it back.)"""
    test_dense_restart_is_the_twin(gpu_lib, "l1", RC, "direct160", F32, first=1, flips=True)


# ------------------------------------------------------- 5. round trip --
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_state_round_trip(gpu_lib, kind, device):
    p = small_problem(kind, F32, nx=23, ny=19, CP_itMax=2)
    a, b = SC.solver(p, device=device), SC.solver(p, device=device)
    first = run(a, p)
    st = a.state(device=device)
    b.set_state(st)
    assert SC.state_equal(SC.host(b.state(device=device)), a.state()) == []
    ra, rb = run(a, p), run(b, p)
    assert out_equal(ra, rb, what=("Cv", "rX", "it", "Dif")) == []
    assert same_bytes(ra[3][1:], rb[3][1:]) and np.isnan(rb[3][0])
    assert same_bytes(ra[3][:1], first[3][first[2]:first[2] + 1])
    a.close(), b.close()
    if device:  # host and device inputs: the same bytes
        h = SC.solver(p)
        assert out_equal(run(h, p), first) == []
        h.close()


@pytest.mark.parametrize("kind,mod", [("l1", RC), ("duplex", DRC), ("bounds", BRC)],
                         ids=("l1", "duplex", "bounds"))
def test_dense_device_arrays_are_the_host_ones(gpu_lib, kind, mod):
    """a dense A (direct12, N = 12) given as device arrays: the bytes of the
    host-array solver, Obj[0] (the sums of initialize()) and R included"""
    p = mod.problem("direct12", F32)
    assert p["kind"] == kind and p["N"] == 12
    outs = []
    for device in (True, False):
        s = SC.solver(p, device=device)
        out = run(s, p, CP_itMax=3)
        outs.append((out, s.state()["R"]))
        s.close()
    (dev, dev_R), (host, host_R) = outs
    assert dev[3] is not None and dev[4] is not None
    assert out_equal(dev, host) == []
    assert same_bytes(dev_R, host_R)


# ----------------------------------------------------- 6. penalty path --
@pytest.mark.parametrize("kind,with_l1", [("l1", False), ("l1", True), ("duplex", True),
                                          ("bounds", False), ("simplex", False)])
def test_penalty_path(gpu_lib, kind, with_l1):
    p = small_problem(kind, F64, CP_itMax=2)
    half = (0.5 * p["La_d1"]).astype(p["La_d1"].dtype)
    l1 = (2 * p["La_l1"]).astype(p["La_l1"].dtype) if with_l1 else None
    a = SC.solver(p)
    run(a, p)  # the duplex builds its two-layer CSR here
    st = a.state()
    a.set_penalties(half, l1)
    assert SC.state_equal(a.state(), st) == []
    ra = run(a, p)
    b = SC.solver(p, La_d1=half, **({"La_l1": l1} if with_l1 else {}))
    b.set_state(st)
    rb = run(b, p)
    assert out_equal(ra, rb, what=("Cv", "rX", "it", "Dif")) == []
    assert np.isnan(ra[3][0]) and same_bytes(ra[3][1:], rb[3][1:])
    assert SC.state_equal(a.state(), b.state()) == []
    for bad in (-half, np.where(np.arange(half.size) == 3, np.nan, half)):
        with pytest.raises(pfdr.PFDRError):
            a.set_penalties(bad)
    if p["La_l1"] is None:
        with pytest.raises(pfdr.PFDRError):
            a.set_penalties(None, np.zeros(p["V"], F64))
    a.close(), b.close()


# -------------------------------------------------- 7. partition import --
def composed(p, Cv, values):
    """the state the step API composes from a label per vertex and its values"""
    K = max(p["K"], 1)
    g = pfdr.CPGraph(p["V"], p["Eu"], p["Ev"], p["La_d1"], p["La_l1"])
    act = (Cv[p["Eu"]] != Cv[p["Ev"]]).astype(np.uint8)
    g.set_active(act)
    c, Vc, rVc = g.components()
    g.close()
    first = Vc[rVc[:-1]]
    rX = np.asarray(values).reshape(-1, K)[Cv[first]].ravel()
    return dict(active=act, Cv=c, Vc=Vc, rVc=rVc, rX=rX)


@pytest.mark.parametrize("kind", KINDS)
def test_partition_import(gpu_lib, kind):
    p = small_problem(kind, F32, CP_itMax=3)
    Cv, rX = SC.entry(p)[:2]
    s = SC.solver(p)
    s.set_partition(Cv, rX)
    got = s.state()
    want = composed(p, Cv, rX)
    assert SC.state_equal(got, want) == []
    uf = SC.union_find(p["V"], p["Eu"], p["Ev"], Cv[p["Eu"]] == Cv[p["Ev"]])
    assert np.array_equal(T.canonical(got["Cv"]), T.canonical(uf))
    t = SC.twin(p)
    SC.twin_restart(t, p, got)
    rec = t.iterate()
    t.b.close()
    out = run(s, p, CP_itMax=1)
    vals = rec["rP"] if kind == "simplex" else rec["rX"]
    assert same_bytes(out[0], rec["Cv"]) and same_bytes(out[1], np.ravel(vals))
    with pytest.raises(pfdr.PFDRError):
        s.set_partition(np.where(np.arange(p["V"]) == 7, Cv.max() + 1, Cv), rX)
    s.close()


def test_partition_two_blobs_one_label(gpu_lib):
    """a label class made of two disconnected blobs: two components, one value"""
    p = small_problem("l1", F64, nx=24, ny=20)
    x = np.arange(p["V"]) % 24
    label = ((x >= 8) & (x < 16)).astype(np.int32)  # label 0: the left and the right band
    values = np.array([0.25, -1.5], F64)
    s = SC.solver(p)
    s.set_partition(label, values)
    st = s.state()
    assert st["rVc"].size - 1 == 3
    assert sorted(st["rX"].tolist()) == [-1.5, 0.25, 0.25]
    assert np.array_equal(st["rX"][st["Cv"]], values[label])
    s.close()


def test_partition_import_dense_recomputes_R(gpu_lib):
    p = dict(RC.problem("direct160", F64), CP_itMax=2)
    s = SC.solver(p)
    out = run(s, p)
    st = s.state()
    s.set_partition(out[0], out[1])
    # the merge may have joined components: compare through the values
    got = s.state()
    assert np.array_equal(got["rX"][got["Cv"]], st["rX"][st["Cv"]])
    A = T.matrix(p["N"], p["V"], p["A"], np.dtype(F64))
    R = p["Y"] - A @ got["rX"][got["Cv"]]
    assert np.allclose(got["R"], R, rtol=0, atol=1e-12 * np.abs(p["Y"]).max() * p["V"])
    s.close()


# ---------------------------------------------------- 8. rejected states --
def _bad_states(st, V):
    def mod(key, f):
        b = {k: np.array(v) for k, v in st.items()}
        f(b[key])
        return b
    rV = st["rVc"].size - 1
    assert rV >= 3
    yield "Vc repeated", mod("Vc", lambda a: a.__setitem__(5, a[6]))
    yield "Vc out of range", mod("Vc", lambda a: a.__setitem__(5, V))
    yield "rVc not increasing", mod("rVc", lambda a: a.__setitem__(2, a[1]))
    yield "rVc wrong end", mod("rVc", lambda a: a.__setitem__(rV, V - 1))
    yield "rVc wrong start", mod("rVc", lambda a: a.__setitem__(0, 1))
    yield "Cv disagrees", mod("Cv", lambda a: a.__setitem__(9, (a[9] + 1) % rV))
    yield "active 2", mod("active", lambda a: a.__setitem__(a.size - 1, 2))
    yield "NaN in rX", mod("rX", lambda a: a.__setitem__(rV - 1, np.nan))
    b = {k: np.array(v) for k, v in st.items()}
    b["rVc"] = b["rVc"][:1]  # rV = 0
    yield "rV = 0", b


@pytest.mark.parametrize("kind", ("l1", "bounds", "simplex"))
def test_rejected_states_change_nothing(gpu_lib, kind):
    p = small_problem(kind, F32, nx=23, ny=19, CP_itMax=2)
    ref = SC.solver(p)
    run(ref, p)
    want = run(ref, p, CP_itMax=1)
    ref.close()
    s = SC.solver(p)
    run(s, p)
    st = s.state()
    bad = list(_bad_states(st, p["V"]))
    if kind == "bounds":
        b = {k: np.array(v) for k, v in st.items()}
        b["rX"][0] = p["hi"] + 1
        bad.append(("outside the box", b))
    for what, b in bad:
        with pytest.raises(pfdr.PFDRError) as e:
            s.set_state(b)
        assert "(1)" in str(e.value), what  # PFDR_ERR_ARG
        assert SC.state_equal(s.state(), st) == [], what
    with pytest.raises(pfdr.PFDRError):
        s.set_partition(np.full(p["V"], -1, np.int32), st["rX"])
    assert SC.state_equal(s.state(), st) == []
    got = run(s, p, CP_itMax=1)
    assert out_equal(got, want, what=("Cv", "rX", "it", "Dif")) == []
    assert same_bytes(got[3], want[3])  # Obj[0] too: nothing was invalidated
    s.close()


@pytest.mark.parametrize("kind", ("l1", "duplex", "bounds"))
def test_hand_made_states(gpu_lib, kind):
    """rV = 1 and rV = V (every edge active), against the twin restarted there"""
    p = small_problem(kind, F64, nx=23, ny=19)
    V, E = p["V"], p["E"]
    one = dict(active=np.zeros(E, np.uint8), Cv=np.zeros(V, np.int32),
               Vc=np.arange(V, dtype=np.int32), rVc=np.array([0, V], np.int32),
               rX=np.array([0.125], F64))
    every = dict(active=np.ones(E, np.uint8), Cv=np.arange(V, dtype=np.int32),
                 Vc=np.arange(V, dtype=np.int32), rVc=np.arange(V + 1, dtype=np.int32),
                 rX=np.clip(p["Y"], 0.0, 0.5).astype(F64))
    s = SC.solver(p)
    for st in (one, every):
        s.set_state(st)
        assert SC.state_equal(s.state(), st) == []
        out = run(s, p, CP_itMax=1)
        t = SC.twin(p)
        SC.twin_restart(t, p, st)
        rec = t.iterate()
        t.b.close()
        assert same_bytes(out[0], rec["Cv"]) and same_bytes(out[1], rec["rX"])
        assert same_bytes(s.state()["active"], rec["active"])
    s.close()


# ------------------------------- 9. repeatability, optional outputs, stats --
@pytest.mark.parametrize("kind", KINDS)
def test_repeatable_optional_outputs_and_stats(gpu_lib, kind):
    p = small_problem(kind, F32, CP_itMax=2)
    outs = []
    for _ in range(2):
        s = SC.solver(p)
        a = run(s, p)
        st = s.state()
        b = run(s, p)
        outs.append((a, b))
        stats = s.stats()
        # NULL Time / Obj / Dif / CP_it
        q = pfdr.CPParams(p["CP_difTol"], 1, p["rho"], p["condMin"], p["difRcd"],
                          p["PFDR_difTol"], p["PFDR_itMax"], 0)
        s.set_state(st)
        pfdr.Lib().cp_solver_run(s._h, q)
        bare = s.state()
        s.set_state(st)
        full = run(s, p, CP_itMax=1)
        assert SC.state_equal(bare, s.state()) == []
        assert np.isnan(full[3][0]) and not np.isnan(full[3][1])
        s.close()
    for x, y in zip(outs[0], outs[1]):
        assert out_equal(x, y) == []
    assert stats["n_cuts"] > 0 and stats["rounds"] >= 0 and stats["setup"] > 0
    assert stats["total"] >= stats["pfdr"] >= 0
    # PFDR iterations: the sum over the reduced problems of the second run
    t = SC.twin(p)
    SC.twin_restart(t, p, st)
    pit = 0
    for _ in range(outs[0][1][2]):
        rec = t.iterate()
        pit += rec["pfdr_it"] or 0
    t.b.close()
    assert stats["pfdr_it"] == pit


def test_argument_errors(gpu_lib):
    p = small_problem("l1", F32)
    with pytest.raises(pfdr.PFDRError):
        pfdr.CPSolver("l1", p["Y"], p["Eu"], p["Ev"], p["La_d1"], A=None, N=5)
    with pytest.raises(pfdr.PFDRError):
        pfdr.CPSolver("bounds", p["Y"], p["Eu"], p["Ev"], p["La_d1"], lo=1.0, hi=0.0)
    with pytest.raises(pfdr.PFDRError):
        pfdr.CPSolver("simplex", p["Y"], p["Eu"], p["Ev"], p["La_d1"], K=4, al=1.5)
    s = SC.solver(p)
    with pytest.raises(pfdr.PFDRError):
        run(s, p, CP_itMax=-1)
    s.close()
