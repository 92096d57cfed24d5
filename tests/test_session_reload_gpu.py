"""GPU: reusable quadratic sessions (pfdr_session_create_reusable /
pfdr_session_reload, include/pfdr_mi355x.h).

One criterion, no tolerance: a session created on problem P0, run, reloaded
with P1 and run again gives the bytes of a fresh plain Session on P1 -- X,
it, Dif and Obj where recorded, and the path queries QUERIES; in the graph
modes (identity / diagonal A) also the bytes of the restatement of the
reference (oracle_port): X and it on every path, Dif where the session sums
the evolution sequentially (the tiny and fused paths sum it in a tree by
design; see _dif_matches).  The shapes are the smallest 4-connected grids that
reach each loop variant (kBlock 256; tiny <= 8 blocks in f32, 5 in f64;
kFuseBlocks 1024; kSeqDifMin 2^17):
  16 x 16     one-workgroup loop (tiny)
  64 x 64     16 blocks: decision fused into the edge sweep, per-block lists
  513 x 512   262,656 vertices, just past kFuseBlocks * kBlock: tile order,
              sequential evolution, speculative decisions, ratio edge sweep
  24 x 25     dense direct (N = 16), A^tA and the same A as a CSC
"""
import functools

import numpy as np
import pytest

from cp_pfdr_graph_d1_amd import pfdr
from cp_pfdr_graph_d1_amd.graphs import piecewise_observation, uniform

pytestmark = pytest.mark.gpu

DTS = [np.float32, np.float64]
QUERIES = ("la_uniform", "edge_ratio", "tiny", "fused", "padded", "seqdif", "speculative")
TINY, FUSED, TILED, DENSE = (16, 16), (64, 64), (513, 512), (24, 25)
LA = 0.1  # the uniform La_d1


@functools.lru_cache(maxsize=None)
def _grid(shape):
    Eu, Ev = pfdr.gen_grid_edges(shape, 4)
    return int(np.prod(shape)), Eu, Ev


def _rand(seed, n, lo, hi, dt):
    return (lo + (hi - lo) * uniform(seed, np.arange(n, dtype=np.int64))).astype(dt)


def _problem(shape, dt, seed=3, la="uniform", l1="uniform", kind=pfdr.PFDR_KIND_L1, **kw):
    """a problem as the keyword arguments of pfdr.Session (graph-mode l1 by default)"""
    V, Eu, Ev = _grid(shape)
    E = Eu.size
    P = dict(kind=kind, dtype=dt, V=V, E=E, Eu=Eu, Ev=Ev, X0=np.zeros(V, dt),
             Y=piecewise_observation(shape, seed, dt), rho=1.5, condMin=1e-3, difRcd=0.0,
             difTol=0.0, itMax=40)
    P["La_d1"] = np.full(E, LA, dt) if la == "uniform" else _rand(seed + 50, E, 0.5 * LA, 1.5 * LA, dt)
    if kind == pfdr.PFDR_KIND_L1 and l1 is not None:
        P["La_l1"] = np.full(V, 0.01, dt) if l1 == "uniform" else _rand(seed + 60, V, 0.005, 0.02, dt)
    P.update(kw)
    return P


def _run(s, P, prepare=False):
    q = {k: s.query(k) for k in QUERIES}
    if prepare:
        s.prepare(P["itMax"])
    s.run(P["itMax"])
    X, it, Obj, Dif = s.result()
    return dict(X=X, it=it, Obj=None if Obj is None else Obj[:it + 1],
                Dif=None if Dif is None else Dif[:it], q=q)


def _fresh(P, **kw):
    s = pfdr.Session(**P)
    try:
        return _run(s, P, **kw)
    finally:
        s.close()


def _same(a, b, what):
    assert a["it"] == b["it"], (what, a["it"], b["it"])
    assert a["q"] == b["q"], (what, a["q"], b["q"])
    for k in ("X", "Obj", "Dif"):
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert a[k].tobytes() == b[k].tobytes(), (what, k)


ARRAYS = dict(Y="Y", La_d1="La_d1", La_l1="La_l1", X0="X0", L="L")
SCALARS = ("lo", "hi", "rho", "condMin", "difRcd", "difTol", "itMax")


def _reload(s, old, new):
    """the arrays of `new` that are not `old`'s own objects, X0 always (None
    would be a warm start), every scalar that differs"""
    kw = {k: new[k] for k in ARRAYS if k in new and (k == "X0" or new[k] is not old.get(k))}
    kw.update({k: new[k] for k in SCALARS if k in new and new[k] != old.get(k)})
    s.reload(**kw)


def _oracle(oracle_port, P):
    common = dict(rho=P["rho"], condMin=P["condMin"], difRcd=P["difRcd"], difTol=P["difTol"],
                  itMax=P["itMax"], dif=bool(P.get("record_dif")))
    Lt, L = P.get("Ltype", pfdr.SCAL), P.get("L")
    if P["kind"] == pfdr.PFDR_KIND_L1:
        return oracle_port.quadratic_d1_l1(P["X0"], P["Y"], P.get("A"), 0, P["Eu"], P["Ev"],
                                           P["La_d1"], P.get("La_l1"), 0, Lt, L, **common)
    return oracle_port.quadratic_d1_bounds(P["X0"], P["Y"], P.get("A"), 0, P["Eu"], P["Ev"],
                                           P["La_d1"], P.get("lo", -np.inf), P.get("hi", np.inf),
                                           Lt, L, **common)


def _dif_matches(got, Do, what):
    """Dif against the restatement: its bytes where the session sums the
    evolution sequentially (seqdif = 1).  The small-graph paths (tiny, fused)
    sum in a fixed tree by design (PFDR_EVOLUTION_AUTO, include/pfdr_mi355x.h),
    so their Dif -- a plain session's too, before reusable sessions existed --
    is held to the tree / sequential bound of tests/test_fused_gpu.py; X and
    it are the restatement's bytes on every path."""
    D = got["Dif"]
    if got["q"]["seqdif"]:
        assert D.tobytes() == Do.tobytes(), what
    else:
        a, b = D.astype(np.float64), Do.astype(np.float64)
        rel = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
        print("Dif against the restatement, tree sums: rel l2 %.3g" % rel)
        assert rel <= (1e-4 if D.dtype == np.float32 else 1e-9), (what, rel)


def _cycle(problems, oracle_port=None, prepare=False, expect=None):
    """problems[0] created reusable and run, then each later one reloaded and
    run: every run equals a fresh plain session on its problem (and the
    restatement); a problem listed twice must give the same bytes twice"""
    fresh = {}
    s = pfdr.Session(reusable=True, **problems[0])
    try:
        assert s.query("reusable") == 1
        for i, P in enumerate(problems):
            if i:
                _reload(s, problems[i - 1], P)
            got = _run(s, P, prepare=prepare)
            if id(P) not in fresh:
                fresh[id(P)] = _fresh(P, prepare=prepare)
            _same(got, fresh[id(P)], "run %d against a fresh session" % i)
            if expect and i < len(expect):
                for k, v in expect[i].items():
                    assert got["q"][k] == v, (i, k, got["q"])
            if oracle_port is not None:
                Xo, ito, _, Do = _oracle(oracle_port, P)
                assert got["it"] == ito, (i, got["it"], ito)
                assert got["X"].tobytes() == Xo.tobytes(), i
                if Do is not None:
                    _dif_matches(got, Do[:ito], i)
    finally:
        s.close()


# ------------------------------------------------------------ 1: tiny ----
@pytest.mark.parametrize("dt", DTS)
def test_tiny(gpu_lib, oracle_port, dt):
    kw = dict(difTol=1e-4, itMax=300, record_dif=True)
    P0 = _problem(TINY, dt, seed=3, **kw)
    P1 = _problem(TINY, dt, seed=4, la="random", **kw)
    _cycle([P0, P1, P0], oracle_port, expect=[dict(tiny=1, la_uniform=1), dict(tiny=1, la_uniform=0)])


# ------------------------------------------------ 2: fused and padded ----
@pytest.mark.parametrize("dt", DTS)
def test_fused_padded(gpu_lib, oracle_port, dt):
    kw = dict(difTol=1e-4, itMax=300, record_dif=True)
    P0 = _problem(FUSED, dt, seed=3, **kw)
    P1 = _problem(FUSED, dt, seed=4, **kw)
    _cycle([P0, P1], oracle_port, expect=[dict(fused=1, padded=1)] * 2)


# ---------------------------------------------------- 3: multi-launch ----
@pytest.mark.parametrize("dt", DTS)
def test_multi_launch_prepared(gpu_lib, oracle_port, dt):
    """untracked, itMax 70: two replayed chunks of 32 and a tail of 6, the
    graphs captured again by the prepare() after the reload"""
    P0 = _problem(FUSED, dt, seed=3, itMax=70)
    P1 = _problem(FUSED, dt, seed=4, la="random", itMax=70)
    _cycle([P0, P1], oracle_port, prepare=True, expect=[dict(fused=0, tiny=0)] * 2)


# ----------------------------------------------------------- 4: tiled ----
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant", ["fixed", "tracked", "spec_off"])
def test_tiled(gpu_lib, oracle_port, dt, variant):
    kw = dict(itMax=40) if variant == "fixed" else dict(difTol=1e-4, itMax=200, record_dif=True)
    if variant == "spec_off":
        kw["spec"] = pfdr.SPEC_OFF
    P0 = _problem(TILED, dt, seed=3, **kw)
    P1 = _problem(TILED, dt, seed=4, **kw)
    P1["La_d1"] = np.full(P1["E"], 0.07, dt)
    want = dict(fixed=dict(edge_ratio=1, seqdif=0), tracked=dict(seqdif=1, speculative=1),
                spec_off=dict(seqdif=1, speculative=0, edge_ratio=1))[variant]
    _cycle([P0, P1, P0] if variant == "fixed" else [P0, P1], oracle_port, expect=[want] * 2)


# ------------------------------------------------- 5: uniformity flip ----
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [FUSED, TILED])
def test_uniformity_flip(gpu_lib, oracle_port, dt, shape):
    """La_d1 uniform -> per-edge in [0.5, 1.5] La -> uniform, La_l1 uniform ->
    varying -> uniform: la_uniform, the Z-direct and ratio sweeps follow"""
    kw = dict(difTol=1e-4, itMax=60, record_dif=True, spec=pfdr.SPEC_OFF)
    P0 = _problem(shape, dt, seed=3, **kw)
    P1 = dict(P0, La_d1=_rand(53, P0["E"], 0.5 * LA, 1.5 * LA, dt))
    P2 = dict(P1, La_d1=P0["La_d1"], La_l1=_rand(63, P0["V"], 0.005, 0.02, dt))
    tiled = int(shape == TILED)
    _cycle([P0, P1, P2, P0], oracle_port,
           expect=[dict(la_uniform=1, edge_ratio=tiled), dict(la_uniform=0, edge_ratio=0),
                   dict(la_uniform=1, edge_ratio=tiled), dict(la_uniform=1, edge_ratio=tiled)])


# ------------------------------------------------------ 6: relabelled ----
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("tracked", [False, True])
def test_relabelled(gpu_lib, oracle_port, dt, tracked):
    """the tiled grid with randomly permuted labels, relabelled internally:
    Y, La_l1 and a diagonal L go through the kept order"""
    V, Eu, Ev = _grid(TILED)
    perm = np.argsort(uniform(71, np.arange(V, dtype=np.int64)), kind="stable").astype(np.int32)
    kw = dict(difTol=1e-4, itMax=60, record_dif=True) if tracked else dict(itMax=30)
    P0 = _problem(TILED, dt, seed=3, reorder=pfdr.REORDER_ON, Ltype=pfdr.DIAG,
                  L=np.ones(V, dt), **kw)
    P0["Eu"], P0["Ev"] = perm[Eu], perm[Ev]
    Y0 = P0["Y"].copy()
    P0["Y"][perm] = Y0
    P1 = dict(P0, Y=_rand(81, V, -1.0, 1.0, dt), La_l1=_rand(82, V, 0.005, 0.02, dt),
              L=_rand(83, V, 1.0, 2.0, dt))
    s = pfdr.Session(reusable=True, **P0)
    try:
        assert s.query("reordered") == 1
    finally:
        s.close()
    _cycle([P0, P1], oracle_port)


# ---------------------------------------------- 7: dense and sparse A ----
@functools.lru_cache(maxsize=None)
def _dense(dt, which):
    N, (nx, ny) = 16, DENSE
    V = nx * ny
    A = 2.0 * uniform(91, np.arange(N * V, dtype=np.int64)).reshape(N, V) - 1.0
    A[uniform(92, np.arange(N * V, dtype=np.int64)).reshape(N, V) < 0.6] = 0.0
    A[np.arange(V) % N, np.arange(V)] = 1.0  # (no empty column)
    L = np.array([np.linalg.norm(A, 2) ** 2], dt)

    def obs(seed):
        x = piecewise_observation(DENSE, seed, np.float64)
        return A @ x + 0.05 * (2.0 * uniform(seed + 7, np.arange(N, dtype=np.int64)) - 1.0)

    kw = dict(record_obj=True, record_dif=True, difTol=1e-5, itMax=80, Ltype=pfdr.SCAL, L=L)
    Ps = []
    for seed, la in ((3, "uniform"), (4, "random")):
        y = obs(seed)
        if which == "ata":
            P = _problem(DENSE, dt, seed, la=la, N=-V, A=np.asfortranarray(A.T @ A).astype(dt).ravel("F"),
                         **kw)
            P["Y"] = (A.T @ y).astype(dt)
        else:
            mat = (pfdr.CSC.from_dense(A) if which == "csc"
                   else np.asfortranarray(A).astype(dt).ravel("F"))
            P = _problem(DENSE, dt, seed, la=la, N=N, A=mat, **kw)
            P["Y"] = y.astype(dt)
        Ps.append(P)
    Ps[1]["A"] = Ps[0]["A"]
    return Ps


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("which", ["direct", "ata", "csc"])
def test_dense_and_sparse(gpu_lib, dt, which):
    """equality with the fresh session (Obj recorded); A is kept by the reload"""
    P0, P1 = _dense(dt, which)
    s = pfdr.Session(reusable=True, **P0)
    try:
        assert s.query("dense_exact") == int(which != "csc")
        assert s.query("sparse_exact") == int(which == "csc")
    finally:
        s.close()
    _cycle([P0, P1, P0])


# ---------------------------------------------------------- 8: bounds ----
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [FUSED, TILED])
def test_bounds(gpu_lib, oracle_port, dt, shape):
    """other boxes, one side infinite (another prox variant)"""
    kw = dict(kind=pfdr.PFDR_KIND_BOUNDS, difTol=1e-4, itMax=60, record_dif=True)
    P0 = _problem(shape, dt, seed=3, lo=-0.25, hi=0.75, **kw)
    P1 = dict(P0, lo=-np.inf, hi=0.5)
    P2 = dict(P0, lo=0.0, hi=np.inf, Y=piecewise_observation(shape, 5, dt))
    _cycle([P0, P1, P2, P0], oracle_port)


# -------------------------------------------------- 9: reconditioning ----
@pytest.mark.parametrize("dt", DTS)
def test_after_reconditioning(gpu_lib, oracle_port, dt):
    """the settings of tests/test_tiled_gpu.py (difTol 1e-6, difRcd 1e-3, itMax
    400): the first run reconditions (its weights leave cw La_d1, the ratio
    sweep is dropped); the reload is back at a fresh session's state"""
    kw = dict(difTol=1e-6, difRcd=1e-3, itMax=400, record_dif=True)
    P0 = _problem(TILED, dt, seed=3, **kw)
    P1 = _problem(TILED, dt, seed=4, **kw)
    f1 = _fresh(P1)
    s = pfdr.Session(reusable=True, **P0)
    try:
        before = s.query("edge_ratio")
        r0 = _run(s, P0)
        n = s.query("reconditionings")
        print("reconditionings", n, "it", r0["it"], "edge_ratio", before, "->", s.query("edge_ratio"))
        assert n >= 1
        assert before == 1 and s.query("edge_ratio") == 0
        _reload(s, P0, P1)
        assert s.query("reconditionings") == 0 and s.query("edge_ratio") == 1
        r1 = _run(s, P1)
        _same(r1, f1, "reload after a reconditioning")
        assert s.query("reconditionings") >= 1
    finally:
        s.close()
    Xo, ito, _, Do = _oracle(oracle_port, P1)
    assert r1["it"] == ito and r1["X"].tobytes() == Xo.tobytes()
    _dif_matches(r1, Do[:ito], "reload after a reconditioning")


# ------------------------------------------------------ 10: warm start ----
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [TINY, FUSED, TILED])
def test_warm_start(gpu_lib, dt, shape):
    """reload(difTol=...) without X0 after a converged run = a fresh session
    started from the downloaded iterate"""
    P0 = _problem(shape, dt, seed=3, difTol=1e-3, itMax=200, record_dif=True)
    s = pfdr.Session(reusable=True, **P0)
    try:
        r0 = _run(s, P0)
        assert 0 < r0["it"] < P0["itMax"]
        P1 = dict(P0, difTol=1e-4, X0=r0["X"])
        s.reload(difTol=1e-4)
        r1 = _run(s, P1)
    finally:
        s.close()
    assert r1["it"] > 0
    _same(r1, _fresh(P1), "warm start")


def test_device_arrays(gpu_lib):
    """torch GPU tensors in, as at creation"""
    torch = pytest.importorskip("torch")
    dt = np.float32
    P0 = _problem(TILED, dt, seed=3, itMax=20)
    P1 = _problem(TILED, dt, seed=4, la="random", itMax=20)

    def dev(P):
        return {k: torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v
                for k, v in P.items()}

    D0, D1 = dev(P0), dev(P1)
    s = pfdr.Session(reusable=True, device=True, **D0)
    try:
        r0 = _run(s, P0)
        s.reload(Y=D1["Y"], La_d1=D1["La_d1"], X0=D1["X0"])
        assert s.query("staging_bytes") == 0
        r1 = _run(s, P1)
    finally:
        s.close()
    _same(r0, _fresh(P0), "device arrays, first run")
    _same(r1, _fresh(P1), "device arrays, reloaded")


# -------------------------------------------------------- 11: refusals ----
def _raises(msg, fn, *a, **kw):
    with pytest.raises(pfdr.PFDRError) as e:
        fn(*a, **kw)
    assert msg in str(e.value), str(e.value)


def test_refusals(gpu_lib):
    dt = np.float32
    P0 = _problem(FUSED, dt, seed=3, difTol=1e-4, itMax=100, record_dif=True)
    V, E = P0["V"], P0["E"]
    f0 = _fresh(P0)
    plain = pfdr.Session(**P0)
    try:
        assert plain.query("reusable") == 0
        _raises("not created reusable", plain.reload, Y=P0["Y"])
    finally:
        plain.close()
    K = 3
    sx = pfdr.Session(pfdr.PFDR_KIND_SIMPLEX, dt, V, E, P0["Eu"], P0["Ev"], P0["La_d1"],
                      np.full(V * K, 1.0 / K, dt), np.full(V * K, 1.0 / K, dt), K=K, al=0.1,
                      itMax=10)
    try:
        _raises("simplex", sx.reload, difTol=0.0)
    finally:
        sx.close()
    _raises("simplex", pfdr.Session, pfdr.PFDR_KIND_SIMPLEX, dt, V, E, P0["Eu"], P0["Ev"],
            P0["La_d1"], np.full(V * K, 1.0 / K, dt), np.full(V * K, 1.0 / K, dt), K=K, al=0.1,
            itMax=10, reusable=True)
    _raises("one GPU", pfdr.Session, reusable=True, nranks=2, rank=0, V_global=2 * V, **P0)

    s = pfdr.Session(reusable=True, **dict(P0, La_l1=None))
    try:
        _raises("La_l1 given", s.reload, La_l1=np.full(V, 0.01, dt))
        _raises("L given", s.reload, L=np.ones(1, dt))
    finally:
        s.close()

    s = pfdr.Session(reusable=True, **P0)
    try:
        r0 = _run(s, P0)
        _same(r0, f0, "first run")
        _raises("itMax above", s.reload, itMax=101)
        _raises("zero and non-zero", s.reload, difRcd=1e-3)
        s.reload(X0=P0["X0"])  # the session still runs, on the problem it holds
        _same(_run(s, P0), f0, "after the refusals")
    finally:
        s.close()

    Pu = _problem(FUSED, dt, seed=3, itMax=40)
    s = pfdr.Session(reusable=True, **Pu)
    try:
        ru = _run(s, Pu)
        _raises("tracking", s.reload, difTol=1e-4)
        _raises("tracking", s.reload, difRcd=1e-3)
        _raises("itMax above", s.reload, itMax=41)
        s.reload(X0=Pu["X0"])  # the session still runs, on the problem it holds
        _same(_run(s, Pu), ru, "after the refusals")
    finally:
        s.close()

    Pt = _problem(TILED, dt, seed=3, difTol=1e-4, itMax=30)
    s = pfdr.Session(reusable=True, **Pt)
    try:
        assert s.query("speculative") == 1
        rt = _run(s, Pt)
        _raises("zero and non-zero", s.reload, difRcd=1e-3)
        _raises("tracking", s.reload, difTol=0.0)
        s.reload(X0=Pt["X0"])
        _same(_run(s, Pt), rt, "after the refusals")
    finally:
        s.close()
    # difRcd 1e-30 is non-zero but its square is 0 in f32: the session is a
    # speculative one, which a difRcd with a non-zero square would not be
    s = pfdr.Session(reusable=True, **dict(Pt, difRcd=1e-30))
    try:
        assert s.query("speculative") == 1
        _raises("loop variant", s.reload, difRcd=1e-3)
    finally:
        s.close()

    Pb = _problem(FUSED, dt, seed=3, kind=pfdr.PFDR_KIND_BOUNDS, lo=0.0, hi=1.0, itMax=40)
    s = pfdr.Session(reusable=True, **Pb)
    try:
        rb = _run(s, Pb)
        _raises("min > max", s.reload, lo=1.0, hi=0.0)
        _raises("min > max", s.reload, lo=float("nan"))
        s.reload(X0=Pb["X0"])
        _same(_run(s, Pb), rb, "after the refusals")
    finally:
        s.close()


# ----------------------------------------- 12: plain sessions unchanged ----
# device_bytes() of the plain session of _problem(shape, dt, seed=3, itMax=40)
# with the library of commit 93f2cab (the parent of the change that added
# reusable sessions)
PARENT_BYTES = {
    (FUSED, "float32"): 552232,
    (FUSED, "float64"): 893960,
    (TILED, "float32"): 35699574,
    (TILED, "float64"): 58899418,
}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [FUSED, TILED])
def test_plain_device_bytes_unchanged(gpu_lib, dt, shape):
    """A plain session holds what it held before.  A reusable one reports
    more by exactly: 4 E for the kept edge map when the session has an
    internal edge order (tile-ordered or relabelled; 64 x 64 has none), 4 V
    for the kept relabelling when relabelled (unless the sequential evolution
    keeps it anyway), and the staging of the host arrays that go through
    either map ("staging_bytes": here the E reals of La_d1 on the tiled
    shape, nothing on 64 x 64, whose host arrays are copied straight into the
    session's own buffers, plus the V reals of X0, which is staged on its way
    into the (X, P) pairs)."""
    P = _problem(shape, dt, seed=3, itMax=40)
    V, E, w = P["V"], P["E"], np.dtype(dt).itemsize
    s = pfdr.Session(**P)
    try:
        plain = s.device_bytes()
        assert s.query("staging_bytes") == 0
    finally:
        s.close()
    print(shape, np.dtype(dt).name, "plain device_bytes", plain)
    assert plain == PARENT_BYTES[(shape, np.dtype(dt).name)]
    s = pfdr.Session(reusable=True, **P)
    try:
        staging = s.query("staging_bytes")
        assert staging == w * (V + (E if shape == TILED else 0))
        assert s.device_bytes() == plain + (4 * E if shape == TILED else 0) + staging
        s.reload(Y=P["Y"], La_d1=P["La_d1"], X0=P["X0"])
        assert s.query("staging_bytes") == staging  # (kept, not grown)
        assert s.device_bytes() == plain + (4 * E if shape == TILED else 0) + staging
    finally:
        s.close()
    # relabelled: + 4 V
    Pr = dict(P, reorder=pfdr.REORDER_ON)
    if shape == TILED:
        got = []
        for reusable in (False, True):
            s = pfdr.Session(reusable=reusable, **Pr)
            try:
                assert s.query("reordered") == 1
                got.append((s.device_bytes(), s.query("staging_bytes")))
            finally:
                s.close()
        assert got[1][1] == w * (E + 3 * V)  # La_d1; Y, La_l1 and X0
        assert got[1][0] == got[0][0] + 4 * E + 4 * V + got[1][1]
