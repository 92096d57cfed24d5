"""Inputs of the minimum-cut fixtures and tests (pfdr_cpgraph_mincut).

Integer-valued capacities, so every sum is exact in f32 and f64 and the cut
(the set reachable from the source in the residual graph of a maximum flow)
is one well-defined set of bytes: tr_cap uniform integers in [-6, 6], r_cap
in [0, 3] (zero-capacity arcs and ties are plentiful), 5 % of the terminals
+inf and 5 % -inf.
"""
import os

import numpy as np

from cp_pfdr_graph_d1_amd.graphs import grid_graph, knn_jitter_grid

HERE = os.path.dirname(os.path.abspath(__file__))
ARCS_BOTH, ARCS_FORWARD = 0, 1


def chain(n):
    u = np.arange(n - 1, dtype=np.int32)
    return u, u + 1


GRAPHS = {
    "grid2d": lambda: (12 * 9,) + grid_graph((12, 9), 4),
    "grid3d": lambda: (6 * 5 * 4,) + grid_graph((6, 5, 4), 6),
    "chain": lambda: (300,) + chain(300),
    "knn": lambda: (8 * 7 * 6,) + knn_jitter_grid((8, 7, 6), k=6),  # duplicate edges
}
SPECIAL = ("isolated", "allsource", "allsink")


def integer_capacities(V, E, seed, dtype, inf=0.05):
    rng = np.random.default_rng(seed)
    tr = rng.integers(-6, 7, V).astype(dtype)
    rc = rng.integers(0, 4, E).astype(dtype)
    u = rng.random(V)
    tr[u < inf] = np.inf
    tr[u > 1.0 - inf] = -np.inf
    return tr, rc


def names():
    out = []
    for g in GRAPHS:
        for arcs in ("both", "fwd"):
            for dt in ("f32", "f64"):
                out.append("%s_%s_%s" % (g, arcs, dt))
    return out + ["%s_both_f32" % s for s in SPECIAL]


def inputs(name):
    """-> dict(V, Eu, Ev, tr_cap, r_cap, arcs) of a fixture's case"""
    g, arcs, dt = name.rsplit("_", 2)
    dtype = np.float32 if dt == "f32" else np.float64
    arcs = ARCS_BOTH if arcs == "both" else ARCS_FORWARD
    seed = sum(ord(c) for c in name)
    if g == "isolated":
        V, Eu, Ev = 1000, np.zeros(0, np.int32), np.zeros(0, np.int32)
        tr, rc = integer_capacities(V, 0, seed, dtype)
    elif g in ("allsource", "allsink"):
        V = 12 * 9
        Eu, Ev = grid_graph((12, 9), 4)
        rng = np.random.default_rng(seed)
        tr = rng.integers(0, 7, V).astype(dtype)
        tr[0] = 3
        rc = rng.integers(1, 4, Eu.size).astype(dtype)
        if g == "allsink":
            tr = -tr
    else:
        V, Eu, Ev = GRAPHS[g]()
        tr, rc = integer_capacities(V, Eu.size, seed, dtype)
    return {"V": V, "Eu": Eu, "Ev": Ev, "tr_cap": tr, "r_cap": rc, "arcs": arcs}


# ---- real capacities: tr_cap standard normal, plain or with the means of
# blocks of 97 vertices removed (cut pursuit's near-degenerate case: the
# gradient sums to about zero over each component), r_cap = 0.3 uniform with
# 10 % zeros.  Drawn in f32, so the f32 and f64 runs see the same numbers.
REAL_GRAPHS = {
    "grid3d": lambda: (24 * 20 * 16,) + grid_graph((24, 20, 16), 6),
    "knn": lambda: (20 * 18 * 16,) + knn_jitter_grid((20, 18, 16), k=6),
    "grid2d8": lambda: (120 * 80,) + grid_graph((120, 80), 8),
}
REAL_BLOCK = 97


def real_names():
    return ["%s_%s_%d" % (g, kind, seed) for g in REAL_GRAPHS for kind in ("plain", "blocks")
            for seed in range(4)]


def real_inputs(name):
    g, kind, seed = name.rsplit("_", 2)
    V, Eu, Ev = REAL_GRAPHS[g]()
    rng = np.random.default_rng(1000 + int(seed))
    tr = rng.standard_normal(V)
    if kind == "blocks":
        b = np.arange(V) // REAL_BLOCK
        tr -= (np.bincount(b, tr) / np.bincount(b))[b]
    rc = 0.3 * rng.random(Eu.size)
    rc[rng.random(Eu.size) < 0.1] = 0
    return {"V": V, "Eu": Eu, "Ev": Ev, "tr_cap": tr.astype(np.float32),
            "r_cap": rc.astype(np.float32), "arcs": ARCS_BOTH}


REAL_PATH = os.path.join(HERE, "mincut", "real_bk.npz")


def path(name):
    return os.path.join(HERE, "mincut", "%s.npz" % name)


def load(name):
    with np.load(path(name)) as z:
        return {k: z[k] for k in z.files}


def cut(Eu, Ev, tr_cap, r_cap, arcs, segment):
    """Value, in f64, of the cut ``segment`` (0 = SOURCE, 1 = SINK): the
    terminal arcs and edge arcs that lead from the source side to the sink
    side."""
    tr = np.asarray(tr_cap, np.float64)
    rc = np.asarray(r_cap, np.float64)
    seg = np.asarray(segment).astype(bool)
    val = tr[seg & (tr > 0)].sum() - tr[~seg & (tr < 0)].sum()
    su, sv = seg[Eu], seg[Ev]
    val += rc[~su & sv].sum()
    if arcs == ARCS_BOTH:
        val += rc[su & ~sv].sum()
    return float(val)
