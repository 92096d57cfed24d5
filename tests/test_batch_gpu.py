"""GPU: batched dense-A sessions (pfdr.BatchSession, pfdr_batch_*).

One criterion, no tolerance: channel b of a batch gives the bytes (X, it, Obj,
Dif) of a scalar pfdr.Session on (X0[b], Y[b]) and the shared rest, after the
same sequence of run() calls; on the shapes whose products run in the
reference's order (dense_exact) also the bytes of the restatement of the
reference (oracle_port).  The evolution statistic is summed sequentially
(EVOLUTION_SEQUENTIAL) wherever it is tracked, so that Dif and the stopping
iterations are the restatement's.

Shapes: 48 x 36 and 12 x 40 (sequential-order products); 24 x 8203 and 22 x
8203 (column dots and row partials: max(N, V) > 8192; the last column block of
the row partials holds 11 columns, two groups of 4 and a tail of 3; N = 22 is
off the f32 vector); V = 8320, 8452, 8450 in A^tA mode (whole and ragged
symmetric tiles, column dots off the vector or for an asymmetric matrix)."""
import functools

import numpy as np
import pytest

from cp_pfdr_graph_d1_amd import pfdr

pytestmark = pytest.mark.gpu

DTS = [np.float32, np.float64]
AMP = [1.0, 0.05, 4.0, 0.0]
SHAPE1 = (48, 36, 6, 7)  # N, V, nx, seed


@functools.lru_cache(maxsize=None)
def _direct(N, V, nx, seed, dtname, B):
    """the shared matrix (column major), graph and L, and B observations"""
    dt = np.dtype(dtname).type
    rng = np.random.default_rng(seed)
    A = np.asfortranarray((rng.standard_normal((N, V)) / np.sqrt(N)).astype(dt))
    A64 = A.astype(np.float64)
    Eu, Ev = pfdr.gen_grid_edges((nx, V // nx), 4)
    x0 = np.where(np.arange(V) % nx < nx // 2, 1.0, -0.5)
    Y64 = np.stack([A64 @ (x0 * (1 + b) + AMP[b % 4] * rng.standard_normal(V))
                    for b in range(B)])
    L = np.array([np.linalg.norm(A64, 2) ** 2], dt)
    return A, A64, Eu.astype(np.int32), Ev.astype(np.int32), Y64, L


def _problem(N, V, nx, seed, dt, B, kind="l1", ata=False, **kw):
    """the keyword arguments of pfdr.BatchSession; a scalar session takes
    them with X0[b], Y[b] (see _channel)"""
    A, A64, Eu, Ev, Y64, L = _direct(N, V, nx, seed, np.dtype(dt).name, B)
    if ata:  # G = A^tA formed in float64 and symmetrised, observations A^t Y_b
        G = A64.T @ A64
        G = (G + G.T) * 0.5
        Af, Y, n = np.asfortranarray(G.astype(dt)).ravel(order="F"), (Y64 @ A64).astype(dt), -V
    else:
        Af, Y, n = A.ravel(order="F"), Y64.astype(dt), N
    P = dict(kind=pfdr.PFDR_KIND_BOUNDS if kind == "bounds" else pfdr.PFDR_KIND_L1, dtype=dt, V=V,
             E=Eu.size, Eu=Eu, Ev=Ev, La_d1=np.full(Eu.size, 0.05, dt), X0=np.zeros((B, V), dt),
             Y=np.ascontiguousarray(Y), N=n, A=Af, L=L, rho=1.5, condMin=1e-3, difRcd=0.0,
             difTol=0.0, itMax=12, evolution=pfdr.EVOLUTION_SEQUENTIAL)
    if kind == "bounds":
        P.update(lo=-1.0, hi=3.0)
    else:
        P["La_l1"] = np.full(V, 0.01, dt)
    P.update(kw)
    return P


def _cut(X, its, Obj, Dif, b):
    return dict(X=X[b], it=int(its[b]), Obj=None if Obj is None else Obj[b],
                Dif=None if Dif is None else Dif[b])


def _batch(P, runs=None, facts=()):
    """every channel's result after the run() calls `runs` (default: one run to itMax)"""
    s = pfdr.BatchSession(**P)
    try:
        q = {k: s.query(k) for k in facts}
        for n in runs or [P["itMax"]]:
            its = s.run(n)
        X, it, Obj, Dif = s.result()
        assert np.array_equal(its, it)
        q.update({k + "_after": s.query(k) for k in ("active", "shared_products")})
    finally:
        s.close()
    return [_cut(X, it, Obj, Dif, b) for b in range(X.shape[0])], q


def _channel(P, b, runs=None, facts=()):
    """the scalar session on channel b"""
    kw = dict(P, X0=P["X0"][b], Y=P["Y"][b])
    s = pfdr.Session(**kw)
    try:
        q = {k: s.query(k) for k in facts}
        for n in runs or [P["itMax"]]:
            s.run(n)
        X, it, Obj, Dif = s.result()
    finally:
        s.close()
    return dict(X=X, it=it, Obj=None if Obj is None else Obj[:it + 1],
                Dif=None if Dif is None else Dif[:it]), q


def _oracle(oracle_port, P, b):
    common = dict(rho=P["rho"], condMin=P["condMin"], difRcd=P["difRcd"], difTol=P["difTol"],
                  itMax=P["itMax"], obj=bool(P.get("record_obj")), dif=bool(P.get("record_dif")))
    a = (P["X0"][b], P["Y"][b], P["A"], P["N"], P["Eu"], P["Ev"], P["La_d1"])
    if P["kind"] == pfdr.PFDR_KIND_L1:
        X, it, Obj, Dif = oracle_port.quadratic_d1_l1(*a, P["La_l1"], 0, pfdr.SCAL, P["L"], **common)
    else:
        X, it, Obj, Dif = oracle_port.quadratic_d1_bounds(*a, P["lo"], P["hi"], pfdr.SCAL, P["L"],
                                                         **common)
    return dict(X=X, it=it, Obj=None if Obj is None else Obj[:it + 1],
                Dif=None if Dif is None else Dif[:it])


def _same(got, ref, what, keys=("X", "Obj", "Dif")):
    assert got["it"] == ref["it"], (what, got["it"], ref["it"])
    for k in keys:
        assert (got[k] is None) == (ref[k] is None), (what, k)
        if got[k] is not None:
            a, r = np.asarray(got[k]), np.asarray(ref[k])
            n = int((a != r).sum()) if a.shape == r.shape else -1
            print("%s %s: %d of %d values differ" % (what, k, n, a.size))
            assert a.dtype == r.dtype and a.tobytes() == r.tobytes(), (what, k, n)


def _against_sessions(P, runs=None, facts=()):
    got, q = _batch(P, runs, facts)
    for b, g in enumerate(got):
        ref, qs = _channel(P, b, runs, [f for f in facts if f in ("symv", "dense_exact")])
        for k, v in qs.items():
            assert q[k] == v, (k, q[k], v)
        _same(g, ref, ("channel %d against its session" % b,))
    return got, q


# ---------------------------------- 1. exact path, own stop and recondition --
@pytest.mark.parametrize("variant", ["l1", "bounds", "ata"])
@pytest.mark.parametrize("dt", DTS)
def test_exact_path_own_stopping_and_reconditioning(gpu_lib, oracle_port, dt, variant):
    P = _problem(*SHAPE1, dt, 4, kind="bounds" if variant == "bounds" else "l1",
                 ata=variant == "ata", difRcd=1e-2, difTol=1e-4, itMax=400, record_obj=True,
                 record_dif=True)
    refs = [_oracle(oracle_port, P, b) for b in range(4)]
    print("restatement iterations:", [r["it"] for r in refs])
    assert len({r["it"] for r in refs}) > 1, "every channel stops at the same iteration"
    assert all(0 < r["it"] < 400 for r in refs)
    got, q = _against_sessions(P, facts=("dense_exact", "channels", "channel_group"))
    assert q["dense_exact"] == 1 and q["channels"] == 4 and q["channel_group"] >= 4
    assert q["active_after"] == 0
    for b in range(4):
        _same(got[b], refs[b], ("channel %d against the restatement" % b, variant))


@pytest.mark.parametrize("dt", DTS)
def test_exact_path_ata_objective_against_the_restatement(gpu_lib, oracle_port, dt):
    """Obj of the A^tA case above against the restatement, byte for byte: a
    premultiplied session on the sequential-order path adds the objective's
    data term x_v (1/2 (A^tA x)_v - (A^tY)_v) with one accumulator over v, as
    the reference does (k_obj_data_seq), and the TV and l1 terms term by term
    (k_obj_terms), like a direct-mode one.  A fixed-tree sum of the data term
    differed in the last places of 57 to 85 of each channel's 89 to 145 Obj
    values (worst relative 3.6e-07 in f32, 8.4e-16 in f64)."""
    P = _problem(*SHAPE1, dt, 4, ata=True, difRcd=1e-2, difTol=1e-4, itMax=400, record_obj=True,
                 record_dif=True)
    got, _ = _batch(P)
    bad = []
    for b in range(4):
        ref = _oracle(oracle_port, P, b)
        assert got[b]["it"] == ref["it"]
        o, oo = got[b]["Obj"], ref["Obj"]
        n = int((o != oo).sum())
        o64, r64 = o.astype(np.float64), oo.astype(np.float64)
        rel = float(np.max(np.abs(o64 - r64) / np.maximum(np.abs(r64), 1e-300)))
        print("channel %d %s: %d of %d Obj values differ, worst relative %.3e" % (
            b, np.dtype(dt).name, n, o.size, rel))
        bad.append(n)
    assert sum(bad) == 0, bad


# ------------------------------------------------------- 2. channel groups --
@pytest.mark.parametrize("shape", [SHAPE1, (12, 40, 8, 7)], ids=["48x36", "12x40"])
@pytest.mark.parametrize("dt", DTS)
def test_channel_groups(gpu_lib, oracle_port, dt, shape):
    s = pfdr.BatchSession(**_problem(*SHAPE1, dt, 1))
    G = s.query("channel_group")
    s.close()
    assert G >= 4
    for B in (1, 2, G, G + 1):  # (G + 1: a ragged last group)
        P = _problem(*shape, dt, B)
        got, _ = _against_sessions(P)
        for b in range(B):
            assert got[b]["it"] == 12
            _same(got[b], _oracle(oracle_port, P, b), ("B = %d channel %d, restatement" % (B, b),))


# ----------------------------------- 3. column dots and row partials (direct) --
@pytest.mark.parametrize("N", [24, 22])
@pytest.mark.parametrize("dt", DTS)
def test_column_dots_and_row_partials(gpu_lib, dt, N):
    P = _problem(N, 8203, 13, 11, dt, 3, itMax=6, record_obj=True, record_dif=True)
    got, q = _against_sessions(P, facts=("dense_exact",))
    assert q["dense_exact"] == 0 and q["shared_products_after"] > 0
    assert all(g["it"] == 6 for g in got)


def test_column_dots_and_row_partials_groups(gpu_lib):
    """every group size of the batched kernels (2, 4, 8) and a ragged tail,
    ungated (nothing tracked or recorded) and stopping"""
    G = 8
    _against_sessions(_problem(24, 8203, 13, 11, np.float32, 2, itMax=3))
    P = _problem(22, 8203, 13, 11, np.float32, G + 3, itMax=40, difTol=3e-2, record_dif=True)
    got, _ = _against_sessions(P)
    print("iterations:", [g["it"] for g in got])
    assert len({g["it"] for g in got}) > 1


# -------------------------------- 4. symmetric tiles and A^tA column dots --
@functools.lru_cache(maxsize=2)
def _gram(V, nx, dtname, asym):
    """the matrices of tests/test_symv_gpu.py, B observations"""
    dt = np.dtype(dtname).type
    rng = np.random.default_rng(V)
    M = 64
    Bm = rng.standard_normal((M, V)) / np.sqrt(M)
    G64 = Bm.T @ Bm
    G64 = (G64 + G64.T) * 0.5  # exactly symmetric
    A = np.asfortranarray(G64.astype(dt))
    if asym:
        A[3, 700] = np.nextafter(A[3, 700], dt(np.inf))
    x0 = np.where(np.arange(V) < V // 2, 1.0, -0.5)
    Y = np.stack([G64 @ (x0 * (1 + b) + AMP[b % 4] * rng.standard_normal(V))
                  for b in range(4)]).astype(dt)
    Eu, Ev = pfdr.gen_grid_edges((nx, V // nx), 4)
    L = np.array([np.linalg.eigvalsh(Bm @ Bm.T)[-1]], dt)  # (the nonzero spectrum of B^t B)
    return A.ravel(order="F"), Y, Eu.astype(np.int32), Ev.astype(np.int32), L


def _gram_problem(V, nx, dt, asym, B, **kw):
    Af, Y, Eu, Ev, L = _gram(V, nx, np.dtype(dt).name, asym)
    P = dict(kind=pfdr.PFDR_KIND_L1, dtype=dt, V=V, E=Eu.size, Eu=Eu, Ev=Ev,
             La_d1=np.full(Eu.size, 0.05, dt), La_l1=np.full(V, 0.01, dt), X0=np.zeros((B, V), dt),
             Y=np.ascontiguousarray(Y[:B]), N=-V, A=Af, L=L, rho=1.5, condMin=1e-3, difRcd=0.0,
             difTol=0.0, itMax=6, record_obj=True, record_dif=True,
             evolution=pfdr.EVOLUTION_SEQUENTIAL)
    P.update(kw)
    return P


SYMV = [(8320, 64, np.float32, False, 1), (8320, 64, np.float64, False, 1),
        (8452, 2, np.float32, False, 1), (8450, 2, np.float32, False, 0),
        (8452, 2, np.float32, True, 0)]


@pytest.mark.parametrize("V,nx,dt,asym,symv", SYMV,
                         ids=["%d-%s%s" % (c[0], np.dtype(c[2]).name, "-asym" if c[3] else "")
                              for c in SYMV])
def test_symmetric_tiles_and_ata_column_dots(gpu_lib, V, nx, dt, asym, symv):
    P = _gram_problem(V, nx, dt, asym, 3)
    got, q = _against_sessions(P, facts=("symv", "dense_exact"))
    assert q["symv"] == symv and q["dense_exact"] == 0 and q["shared_products_after"] > 0
    assert all(g["it"] == 6 for g in got)


# --------------------------------------------------------- 5. run in pieces --
@pytest.mark.parametrize("dt", DTS)
def test_run_in_pieces(gpu_lib, dt):
    P = _problem(*SHAPE1, dt, 4, difRcd=1e-2, difTol=1e-4, itMax=400, record_obj=True,
                 record_dif=True)
    whole, _ = _batch(P)
    pieces, _ = _against_sessions(P, runs=[10, 400])
    for b in range(4):
        _same(pieces[b], whole[b], ("channel %d in pieces" % b,))


# ----------------------------------------------------------------- 6. reload --
def _result(s):
    X, it, Obj, Dif = s.result()
    return [_cut(X, it, Obj, Dif, b) for b in range(X.shape[0])]


@pytest.mark.parametrize("dt", DTS)
def test_reload_equals_a_fresh_batch(gpu_lib, dt):
    kw = dict(difRcd=1e-2, difTol=1e-4, itMax=400, record_obj=True, record_dif=True)
    P0 = _problem(*SHAPE1, dt, 4, **kw)
    Y1 = np.ascontiguousarray(P0["Y"][::-1] * dt(0.75))
    P1 = dict(P0, Y=Y1)
    fresh1, _ = _batch(P1)
    s = pfdr.BatchSession(**P0)
    try:
        s.run(400)
        first = _result(s)
        s.reload(Y=Y1, X0=P0["X0"])
        assert s.query("active") == 4
        s.run(400)
        for b, g in enumerate(_result(s)):
            _same(g, fresh1[b], ("reloaded channel %d" % b,))
        # a warm start: every channel from its own iterate, on the first observations
        Xw = np.stack([g["X"] for g in _result(s)])
        s.reload(Y=P0["Y"])
        s.run(400)
        warm, _ = _batch(dict(P0, X0=Xw))
        for b, g in enumerate(_result(s)):
            _same(g, warm[b], ("warm-started channel %d" % b,))
        # a reload that would change the loop variant is refused; the batch runs on
        with pytest.raises(pfdr.PFDRError) as e:
            s.reload(difRcd=0.0)
        assert "difRcd" in str(e.value)
        s.reload(X0=P0["X0"])
        s.run(400)
        for b, g in enumerate(_result(s)):
            _same(g, first[b], ("channel %d after the refusal" % b,))
    finally:
        s.close()


# ------------------------------------------------------------ 7. A held once --
def test_matrix_held_once(gpu_lib):
    P = _gram_problem(8320, 64, np.float32, False, 4, record_obj=False, record_dif=False)
    s = pfdr.BatchSession(**P)
    try:
        assert s.query("channels") == 4 and s.query("shared_products") == 0
        assert s.query("device_bytes") < 2 * P["A"].nbytes
        assert np.array_equal(s.run(3), [3, 3, 3, 3])
        assert s.query("shared_products") > 0 and s.query("active") == 4
    finally:
        s.close()


# --------------------------------------------------------- 8. device tensors --
@pytest.mark.parametrize("dt", DTS)
def test_device_tensors(gpu_lib, dt):
    import torch
    P = _problem(*SHAPE1, dt, 4, difRcd=1e-2, difTol=1e-4, itMax=400, record_obj=True,
                 record_dif=True)
    host, _ = _batch(P)
    D = dict(P, device=True)
    for k in ("Eu", "Ev", "La_d1", "La_l1", "X0", "Y", "A", "L"):
        D[k] = torch.from_numpy(np.ascontiguousarray(P[k])).cuda()
    dev, _ = _batch(D)
    for b in range(4):
        _same(dev[b], host[b], ("channel %d from device tensors" % b,))
