"""Inputs of the two-layer minimum-cut fixtures and tests
(pfdr_cpgraph_mincut_duplex): the duplex driver's network, node v (v1) and
node V + v (v2) per vertex, tr_cap[2V], r_link[V] (arc v1 -> v2 only) and
r_cap[E] (both arcs of edge e in both layers).

Integer-valued capacities, so every sum is exact in f32 and f64 and the cut
(the set reachable from the source in the residual graph of a maximum flow)
is one well-defined set of bytes: tr_cap uniform integers in [-6, 6], r_link
and r_cap in [0, 3] (zero capacities and ties are plentiful).
"""
import os

import numpy as np

from cp_pfdr_graph_d1_amd.graphs import grid_graph, knn_jitter_grid

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "mincut_duplex")
DTYPES = {"f32": np.float32, "f64": np.float64}

_NONE = (np.zeros(0, np.int32), np.zeros(0, np.int32))
GRAPHS = {
    "grid12x9": lambda: (12 * 9,) + grid_graph((12, 9), 4),      # 216 nodes: one workgroup
    "grid24x20": lambda: (24 * 20,) + grid_graph((24, 20), 4),   # 960 nodes: several
    "grid3d": lambda: (6 * 5 * 4,) + grid_graph((6, 5, 4), 6),
    "knn": lambda: (8 * 7 * 6,) + knn_jitter_grid((8, 7, 6), k=6),  # duplicate edges
    "allsource": lambda: (12 * 9,) + grid_graph((12, 9), 4),
    "allsink": lambda: (12 * 9,) + grid_graph((12, 9), 4),
    "links": lambda: (5,) + _NONE,                               # E = 0
    "single": lambda: (1,) + _NONE,                              # V = 1
    "infsource": lambda: (24 * 20,) + grid_graph((24, 20), 4),   # positivity's shape
    "zerocap": lambda: (24 * 20,) + grid_graph((24, 20), 4),     # 10 % zero r_cap
    "nolink": lambda: (12 * 9,) + grid_graph((12, 9), 4),        # the layers decouple
}


def names():
    return ["%s_%s" % (g, d) for g in GRAPHS for d in DTYPES]


def inputs(name):
    """-> dict(V, Eu, Ev, tr_cap[2V], r_link[V], r_cap[E]) of a fixture's case"""
    g, d = name.rsplit("_", 1)
    dtype = DTYPES[d]
    V, Eu, Ev = GRAPHS[g]()
    Eu, Ev = np.asarray(Eu, np.int32), np.asarray(Ev, np.int32)
    E = Eu.size
    rng = np.random.default_rng(sum(ord(c) for c in name))
    tr = rng.integers(-6, 7, 2 * V)
    link = rng.integers(0, 4, V)
    rc = rng.integers(0, 4, E)
    tr = tr.astype(dtype)
    if g == "allsource":
        tr = np.abs(tr)
        tr[0] = 3
        rc = np.maximum(rc, 1)
        link = np.maximum(link, 1)
    elif g == "allsink":
        tr = -np.abs(tr)
        tr[V] = -3
        rc = np.maximum(rc, 1)
    elif g == "infsource":
        # positivity: tr_cap[v1] = +inf on the zero components (k_cp_trcap_duplex)
        tr[:V][rng.random(V) < 0.3] = np.inf
    elif g == "zerocap":
        rc = rng.integers(1, 4, E)
        rc[rng.random(E) < 0.1] = 0
    elif g == "nolink":
        link[:] = 0
    return {"V": V, "Eu": Eu, "Ev": Ev, "tr_cap": tr, "r_link": link.astype(dtype),
            "r_cap": rc.astype(dtype)}


def path(name):
    return os.path.join(DIR, "%s.npz" % name)


def load(name):
    with np.load(path(name)) as z:
        return {k: z[k] for k in z.files}


def cut_duplex(V, Eu, Ev, tr_cap, r_link, r_cap, segment):
    """Value, in f64, of the cut ``segment[2V]`` (0 = SOURCE, 1 = SINK) of the
    two-layer network: the terminal arcs, the edge arcs of either layer and
    the links v1 -> v2 that lead from the source side to the sink side."""
    tr = np.asarray(tr_cap, np.float64)
    ln = np.asarray(r_link, np.float64)
    rc = np.asarray(r_cap, np.float64)
    seg = np.asarray(segment).astype(bool)
    Eu, Ev = np.asarray(Eu, np.int64), np.asarray(Ev, np.int64)
    val = tr[seg & (tr > 0)].sum() - tr[~seg & (tr < 0)].sum()
    for off in (0, V):
        val += rc[seg[off + Eu] != seg[off + Ev]].sum()
    val += ln[~seg[:V] & seg[V:]].sum()
    return float(val)


def forward_network(V, Eu, Ev, r_link, r_cap):
    """The two-layer network as forward arcs over 2V nodes (mincut_model's
    ARCS_FORWARD): (u, v), (v, u), (u + V, v + V), (v + V, u + V) with r_cap
    and (v, v + V) with r_link -> (Eu2, Ev2, cap)"""
    Eu, Ev = np.asarray(Eu, np.int64), np.asarray(Ev, np.int64)
    v = np.arange(V, dtype=np.int64)
    u2 = np.concatenate([Eu, Ev, Eu + V, Ev + V, v])
    v2 = np.concatenate([Ev, Eu, Ev + V, Eu + V, v + V])
    rc = np.asarray(r_cap, np.float64)
    cap = np.concatenate([rc, rc, rc, rc, np.asarray(r_link, np.float64)])
    return u2, v2, cap
