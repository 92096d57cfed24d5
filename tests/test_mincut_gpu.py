"""pfdr_cpgraph_mincut (csrc/pfdr_mincut.hip) on the GPU: the cut of the
reference's Boykov-Kolmogorov maxflow, the set reachable from the source in
the residual graph of a maximum flow.

1. fixtures from the reference's BK (tests/golden/mincut/*.npz, integer
   capacities): segments byte-equal, cut value exact;
2. larger graphs against the live reference (where it is built): segments
   byte-equal;
3. real capacities against the recorded f64 BK cut (mincut/real_bk.npz):
   the value of the GPU's cut within [1 - 1e-12, 1 + 1e-5] of BK's;
4. the recorded cut-pursuit iterations (l1, bounds, simplex drivers): the
   value of the GPU's cut against the value of the recorded segments on the
   same capacities;
5. determinism: same bytes and bits on every run;
6. argument checks.
"""
import numpy as np
import pytest

import cp_cases as CC
import mincut_cases as MC
from cp_fixtures import (BNAMES, NAMES, SNAMES, expansion_segments, iteration_state,
                                  load_case)
from cp_pfdr_graph_d1_amd import pfdr
from cp_pfdr_graph_d1_amd.graphs import grid_graph, knn_jitter_grid
from oracle import CPStepRef, CPStepRefSimplex

pytestmark = pytest.mark.gpu

REL = 1e-5  # the project's parity bar


def graph(V, Eu, Ev, dtype):
    return pfdr.CPGraph(V, Eu, Ev, np.zeros(Eu.size, dtype))


# ------------------------------------------------------------ 1. golden --
@pytest.mark.parametrize("name", MC.names())
def test_golden_exact(gpu_lib, name):
    f = MC.load(name)
    g = graph(int(f["V"]), f["Eu"], f["Ev"], f["tr_cap"].dtype)
    seg, flow, rounds = g.mincut(f["tr_cap"], f["r_cap"], int(f["arcs"]))
    g.close()
    print(name, "rounds", rounds, "differing bytes", int((seg != f["segment"]).sum()),
          "flow", flow, "stored", float(f["cut"]))
    assert seg.dtype == np.uint8 and np.array_equal(seg, f["segment"])
    assert flow == float(f["cut"])


# ---------------------------------------------------- 2. live reference --
LARGE = {
    "grid3d": lambda: (40 * 36 * 30,) + grid_graph((40, 36, 30), 6),
    "knn": lambda: (30 * 28 * 24,) + knn_jitter_grid((30, 28, 24), k=6),
    "grid2d8": lambda: (300 * 200,) + grid_graph((300, 200), 8),
    "chain": lambda: (6000,) + MC.chain(6000),
}
_large = {}


def large(name):
    if name not in _large:
        _large[name] = LARGE[name]()
    return _large[name]


@pytest.mark.skipif(not (CPStepRef.available() and CPStepRefSimplex.available()),
                    reason="reference harness not built here")
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("arcs", [MC.ARCS_BOTH, MC.ARCS_FORWARD], ids=["both", "fwd"])
@pytest.mark.parametrize("name", list(LARGE))
def test_larger_exact_against_reference(gpu_lib, name, arcs, dt):
    V, Eu, Ev = large(name)
    tr, rc = MC.integer_capacities(V, Eu.size, 7 + arcs, dt)
    ref = CPStepRef() if arcs == MC.ARCS_BOTH else CPStepRefSimplex()
    want = ref.maxflow(Eu, Ev, tr, rc)
    g = graph(V, Eu, Ev, dt)
    seg, flow, rounds = g.mincut(tr, rc, arcs)
    relabels = g.mincut_relabels()
    g.close()
    print(name, "rounds", rounds, "global relabels", relabels, "differing bytes",
          int((seg != want).sum()))
    assert np.array_equal(seg, want)
    assert flow == MC.cut(Eu, Ev, tr, rc, arcs, want)


# --------------------------------------------------- 3. real capacities --
@pytest.fixture(scope="module")
def real_bk():
    with np.load(MC.REAL_PATH) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", MC.real_names())
def test_real_capacities(gpu_lib, real_bk, name, dt):
    c = MC.real_inputs(name)
    V, Eu, Ev = c["V"], c["Eu"], c["Ev"]
    tr, rc = c["tr_cap"].astype(dt), c["r_cap"].astype(dt)
    bk_seg = np.unpackbits(real_bk[name + "_seg"])[:V]
    bk = float(real_bk[name + "_cut"])
    assert bk == MC.cut(Eu, Ev, tr, rc, c["arcs"], bk_seg)
    g = graph(V, Eu, Ev, dt)
    seg, flow, rounds = g.mincut(tr, rc, c["arcs"])
    g.close()
    mine = MC.cut(Eu, Ev, tr, rc, c["arcs"], seg)
    print(name, np.dtype(dt).name, "rounds", rounds, "differing bytes",
          int((seg != bk_seg).sum()), "gap %.3e" % (mine / bk - 1), "flow-cut %.3e" %
          (abs(flow - mine) / mine))
    assert mine >= bk * (1 - 1e-12)  # no cut is below the minimum
    assert mine <= bk * (1 + REL)
    assert abs(flow - mine) <= REL * mine


# --------------------------------------- 4. recorded CP iterations --
def _both_sided(mine, rec):
    assert abs(mine - rec) <= REL * rec, (mine, rec)


@pytest.mark.parametrize("name", NAMES + BNAMES + SNAMES)
def test_recorded_cp_iterations(gpu_lib, oracle_port, name):
    c, d = load_case(name)
    simplex = name in SNAMES
    arcs = MC.ARCS_FORWARD if simplex else MC.ARCS_BOTH
    dt = c["La_d1"].dtype
    V = (c["Q"].size // c["K"]) if simplex else c["Y"].size
    g = graph(V, c["Eu"], c["Ev"], dt)
    step = (CC.cp_graph_iteration_simplex if simplex else
            CC.cp_graph_iteration_bounds if name in BNAMES else CC.cp_graph_iteration)
    ncut = nequal = 0
    for k in range(int(d["meta_steps"])):
        st = iteration_state(d, k, "in")
        if simplex:
            segs = expansion_segments(d, c["K"], k)
        else:
            segs = [d["k%d_seg_first" % k]] if ("k%d_seg_first" % k) in d.files else []
            segs.append(d["k%d_seg_last" % k])
        it = iter(segs)

        def maxflow(tr, rc):
            # the GPU's cut on these capacities; the chain goes on with the
            # recorded segments, so the next capacities are the recorded ones
            nonlocal ncut, nequal
            rec = next(it)
            seg, flow, _ = g.mincut(tr, rc, arcs)
            mine = MC.cut(c["Eu"], c["Ev"], tr, rc, arcs, seg)
            want = MC.cut(c["Eu"], c["Ev"], tr, rc, arcs, rec)
            ncut += 1
            nequal += int(np.array_equal(seg, rec))
            _both_sided(mine, want)
            return rec

        step(oracle_port, maxflow, c, st)
    g.close()
    print(name, "cuts", ncut, "with segments equal to the recorded ones", nequal)
    assert ncut > 0


# ------------------------------------------------------ 5. determinism --
def test_determinism(gpu_lib):
    c = MC.real_inputs("grid3d_blocks_0")
    g = graph(c["V"], c["Eu"], c["Ev"], np.float32)
    a = g.mincut(c["tr_cap"], c["r_cap"])
    b = g.mincut(c["tr_cap"], c["r_cap"])
    g.close()
    g = graph(c["V"], c["Eu"], c["Ev"], np.float32)
    f = g.mincut(c["tr_cap"], c["r_cap"])
    g.close()
    for x in (b, f):
        assert x[0].tobytes() == a[0].tobytes()
        assert np.float64(x[1]).tobytes() == np.float64(a[1]).tobytes()
        assert x[2] == a[2]


# -------------------------------------------------------- 6. arguments --
def test_arguments(gpu_lib):
    f = MC.load("grid2d_both_f32")
    g = graph(int(f["V"]), f["Eu"], f["Ev"], np.float32)
    tr, rc = f["tr_cap"].copy(), f["r_cap"].copy()
    bad = tr.copy()
    bad[5] = np.nan
    with pytest.raises(pfdr.PFDRError, match="mincut.*NaN"):
        g.mincut(bad, rc)
    bad = rc.copy()
    bad[7] = -1
    with pytest.raises(pfdr.PFDRError, match="mincut.*r_cap"):
        g.mincut(tr, bad)
    bad = rc.copy()
    bad[3] = np.nan
    with pytest.raises(pfdr.PFDRError, match="mincut.*r_cap"):
        g.mincut(tr, bad)
    with pytest.raises(pfdr.PFDRError, match="arcs"):
        g.mincut(tr, rc, arcs=2)
    seg, flow, _ = g.mincut(tr, rc)  # the graph stays usable
    g.close()
    assert np.array_equal(seg, f["segment"]) and flow == float(f["cut"])
