"""The two-layer minimum cut and the duplex entry without a GPU: the
interface's names, the tests' own cut_duplex() helper, and the numpy model of
the device algorithm (tests/mincut_model.py) on the forward-arc form of the
two-layer network, against the fixtures of the reference's Boykov-Kolmogorov
maxflow (tests/golden/mincut_duplex/*.npz) and the 48 recorded cuts of the
duplex driver's iterations (tests/golden/cp_duplex_*.npz)."""
import os
import re

import numpy as np
import pytest

import cp_cases as CC
import mincut_duplex_cases as MD
from cp_fixtures import DNAMES, iteration_state, load_case
from cp_pfdr_graph_d1_amd import pfdr
from mincut_model import FORWARD, mincut_model

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("pfdr_cpgraph_mincut_duplex", "pfdr_cp_quadratic_d1_l1_duplex_f32",
       "pfdr_cp_quadratic_d1_l1_duplex_f64", "pfdr_cp_quadratic_d1_l1_duplex_stats")
# the fixtures of at most 240 nodes
SMALL = [n for n in MD.names() if n.rsplit("_", 1)[0] in
         ("grid12x9", "grid3d", "allsource", "allsink", "links", "single", "nolink")]


def model(V, Eu, Ev, tr, link, rc, period=16):
    """the device algorithm (sink-side preflow) on the two-layer network as
    forward arcs over 2V nodes"""
    u2, v2, cap = MD.forward_network(V, Eu, Ev, link, rc)
    return mincut_model(2 * V, u2, v2, tr, cap, FORWARD, period=period)


# ------------------------------------------------------------- a. names --
def test_names_in_header_and_python():
    hdr = open(os.path.join(ROOT, "include", "pfdr_mi355x.h")).read()
    declared = set(re.findall(r"\b(pfdr_[a-z0-9_]+)\s*\(", hdr))
    for n in NEW:
        assert n in declared, n
        assert n in pfdr.EXPORTED, n
    assert pfdr.ABI_VERSION == 4
    assert callable(getattr(pfdr.CPGraph, "mincut_duplex"))
    for n in ("cp_quadratic_d1_l1_duplex", "cp_quadratic_d1_l1_duplex_stats"):
        assert callable(getattr(pfdr.Lib, n)), n
    for n in ("CP_quadratic_l1_duplex", "CP_PFDR_graph_quadratic_d1_l1_duplex",
              "CP_PFDR_graph_l22_d1_l1_duplex"):
        assert callable(getattr(pfdr, n)), n


def test_fixtures_complete():
    have = sorted(f[:-4] for f in os.listdir(MD.DIR) if f.endswith(".npz"))
    assert have == sorted(MD.names())
    assert len(MD.names()) == 22
    for n in MD.names():
        assert os.path.getsize(MD.path(n)) < 100 * 1024, n
    assert len(SMALL) == 14


# ------------------------------------------------------ c. cut_duplex() --
def test_cut_helper_by_hand():
    # chain 0 -(2)- 1 -(1)- 2 in both layers; links 0: 4, 1: 0, 2: 1;
    # source 3 into node 0 (v1 of vertex 0), node 5 (v2 of vertex 2) to the sink 5
    V, Eu, Ev = 3, np.array([0, 1]), np.array([1, 2])
    tr = np.array([3.0, 0, 0, 0, 0, -5.0])
    link, rc = np.array([4.0, 0.0, 1.0]), np.array([2.0, 1.0])
    cut = lambda seg: MD.cut_duplex(V, Eu, Ev, tr, link, rc, seg)
    assert cut([1, 1, 1, 1, 1, 1]) == 3           # the source arc alone
    assert cut([0, 0, 0, 0, 0, 0]) == 5           # the sink arc alone
    assert cut([0, 0, 0, 1, 1, 1]) == 4 + 0 + 1   # the three links
    assert cut([0, 1, 1, 1, 1, 1]) == 2 + 4       # edge (0, 1) of layer 1, link 0
    assert cut([0, 0, 0, 0, 0, 1]) == 1 + 1       # edge (1, 2) of layer 2, link 2
    assert cut([0, 1, 1, 0, 1, 1]) == 2 + 2       # edge (0, 1) in both layers, no link
    # v2 -> v1 has no arc: node 3 on the source side, node 0 on the sink side
    assert cut([1, 1, 1, 0, 0, 0]) == 3 + 5
    # a real minimum cut by enumeration: the model's answer has that value
    best = min(cut([(m >> i) & 1 for i in range(6)]) for m in range(64))
    seg, _ = model(V, Eu, Ev, tr, link, rc)
    assert cut(seg) == best == 2


@pytest.mark.parametrize("name", MD.names())
def test_cut_helper_reproduces_stored_values(name):
    f = MD.load(name)
    c = MD.inputs(name)  # the stored inputs are the generator's
    for k in ("Eu", "Ev", "tr_cap", "r_link", "r_cap"):
        assert np.array_equal(f[k], c[k]) and f[k].dtype == c[k].dtype, k
    V = int(f["V"])
    assert V == c["V"] and f["segment"].shape == (2 * V,) and f["segment"].dtype == np.uint8
    assert MD.cut_duplex(V, f["Eu"], f["Ev"], f["tr_cap"], f["r_link"], f["r_cap"],
                         f["segment"]) == float(f["cut"])
    g = name.rsplit("_", 1)[0]
    if g == "allsource":
        assert not f["segment"].any() and f["cut"] == 0
    if g == "allsink":
        assert f["segment"].all() and f["cut"] == 0
    if g == "infsource":
        inf = np.isinf(f["tr_cap"])
        assert inf[:V].any() and not inf[V:].any() and not f["segment"][inf].any()
    if g == "zerocap":
        assert 0.05 < np.mean(f["r_cap"] == 0) < 0.15
    if g == "nolink":
        assert not f["r_link"].any()


# ---------------------------------------------------- b. the numpy model --
@pytest.mark.parametrize("name", SMALL)
def test_model_reproduces_reference_segments(name):
    f = MD.load(name)
    a = (int(f["V"]), f["Eu"], f["Ev"], f["tr_cap"], f["r_link"], f["r_cap"])
    seg, _ = model(*a)
    assert np.array_equal(seg, f["segment"])
    seg, _ = model(*a, period=3)  # any global-relabel period gives the same set
    assert np.array_equal(seg, f["segment"])


@pytest.mark.parametrize("name", DNAMES)
def test_model_reproduces_recorded_duplex_cuts(oracle_port, name):
    """the 48 recorded cuts: the capacities the restatement gives in the
    recorded state, the chain continued with the recorded segments"""
    c, d = load_case(name)
    V = c["Y"].size
    steps = int(d["meta_steps"])
    assert steps == 6
    for k in range(steps):
        rec = d["k%d_seg_last" % k]

        def maxflow(tr, link, rc):
            seg, rounds = model(V, c["Eu"], c["Ev"], tr, link, rc)
            assert np.array_equal(seg, rec), (k, int((seg != rec).sum()))
            return rec

        CC.cp_graph_iteration_duplex(oracle_port, maxflow, c, iteration_state(d, k, "in"))


def test_eight_recorded_fixtures():
    assert len(DNAMES) == 8, DNAMES
