"""The minimum cut without a GPU: the interface's names, the tests' own
cut() helper, and a numpy model of the device algorithm
(tests/mincut_model.py) against the fixtures of the reference's
Boykov-Kolmogorov maxflow (tests/golden/mincut/*.npz)."""
import os
import re

import numpy as np
import pytest

import mincut_cases as MC
from cp_pfdr_graph_d1_amd import pfdr
from mincut_model import mincut_model

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("pfdr_cpgraph_mincut", "pfdr_cpgraph_mincut_relabels",
       "pfdr_cp_quadratic_d1_l1_f32", "pfdr_cp_quadratic_d1_l1_f64")
# the three smallest fixtures (108, 108 and 120 vertices) in both arc modes
SMALL = ["grid2d_both_f32", "grid2d_fwd_f64", "grid3d_both_f64", "grid3d_fwd_f32",
         "allsource_both_f32", "allsink_both_f32"]


def test_names_in_header_and_python():
    hdr = open(os.path.join(ROOT, "include", "pfdr_mi355x.h")).read()
    declared = set(re.findall(r"\b(pfdr_[a-z0-9_]+)\s*\(", hdr))
    for n in NEW:
        assert n in declared, n
        assert n in pfdr.EXPORTED, n
    assert re.search(r"#define PFDR_ARCS_BOTH 0\b", hdr)
    assert re.search(r"#define PFDR_ARCS_FORWARD 1\b", hdr)
    assert (pfdr.ARCS_BOTH, pfdr.ARCS_FORWARD) == (0, 1)
    assert hasattr(pfdr.CPGraph, "mincut") and hasattr(pfdr, "CP_quadratic_l1")


def test_fixtures_complete():
    for n in MC.names():
        assert os.path.getsize(MC.path(n)) < 100 * 1024, n
    assert len(MC.names()) == 19
    with np.load(MC.REAL_PATH) as z:
        assert sorted(z.files) == sorted(n + s for n in MC.real_names() for s in ("_seg", "_cut"))


@pytest.mark.parametrize("name", MC.names())
def test_cut_helper_reproduces_stored_values(name):
    f = MC.load(name)
    c = MC.inputs(name)  # the stored inputs are the generator's
    for k in ("Eu", "Ev", "tr_cap", "r_cap"):
        assert np.array_equal(f[k], c[k]) and f[k].dtype == c[k].dtype, k
    assert int(f["arcs"]) == c["arcs"] and int(f["V"]) == c["V"]
    assert MC.cut(f["Eu"], f["Ev"], f["tr_cap"], f["r_cap"], int(f["arcs"]),
                  f["segment"]) == float(f["cut"])
    if name.startswith("allsource"):
        assert not f["segment"].any() and f["cut"] == 0
    if name.startswith("allsink"):
        assert f["segment"].all() and f["cut"] == 0


def test_cut_helper_by_hand():
    # 0 -(2)- 1 -(1)- 2, source 3 into vertex 0, vertex 2 to the sink 5
    Eu, Ev = np.array([0, 1]), np.array([1, 2])
    tr, rc = np.array([3.0, 0, -5.0]), np.array([2.0, 1.0])
    assert MC.cut(Eu, Ev, tr, rc, MC.ARCS_BOTH, [0, 0, 1]) == 1
    assert MC.cut(Eu, Ev, tr, rc, MC.ARCS_BOTH, [0, 1, 1]) == 2
    assert MC.cut(Eu, Ev, tr, rc, MC.ARCS_BOTH, [1, 1, 1]) == 3
    assert MC.cut(Eu, Ev, tr, rc, MC.ARCS_BOTH, [0, 0, 0]) == 5
    # forward arcs only: the arc 1 -> 0 does not exist
    assert MC.cut(Eu, Ev, tr, rc, MC.ARCS_FORWARD, [1, 0, 1]) == 3 + 1


@pytest.mark.parametrize("name", SMALL)
def test_model_reproduces_reference_segments(name):
    f = MC.load(name)
    seg, _ = mincut_model(int(f["V"]), f["Eu"], f["Ev"], f["tr_cap"], f["r_cap"],
                          int(f["arcs"]))
    assert np.array_equal(seg, f["segment"])
    # any global-relabel period gives the same set
    seg, _ = mincut_model(int(f["V"]), f["Eu"], f["Ev"], f["tr_cap"], f["r_cap"],
                          int(f["arcs"]), period=3)
    assert np.array_equal(seg, f["segment"])


def test_forward_preflow_gives_the_other_extreme_cut():
    """run from the source side, the first phase yields the LARGEST source
    side: a minimum cut too, but not the reference's set"""
    differ = 0
    for name in SMALL[:4]:
        f = MC.load(name)
        a = (int(f["V"]), f["Eu"], f["Ev"], f["tr_cap"], f["r_cap"], int(f["arcs"]))
        seg, _ = mincut_model(*a, side="source")
        assert MC.cut(*a[1:], seg) == float(f["cut"])       # still a minimum cut
        assert not (seg.astype(bool) & ~f["segment"].astype(bool)).any()  # a superset
        differ += int(not np.array_equal(seg, f["segment"]))
    assert differ == 4


def test_relabel_must_see_the_residuals_after_the_pushes():
    """a labelling is valid when h(u) <= h(v) + 1 on every residual arc
    u -> v.  Relabelling from the residuals AFTER the round's pushes keeps it
    valid in every round; relabelling from the snapshot misses the reverse
    arc that a simultaneous push v -> u has just opened, and in some of these
    cases the labelling turns invalid (a node may then be retired with
    excess it could still deliver)"""
    rng = np.random.default_rng(5)
    Eu, Ev = MC.grid_graph((9, 9), 4)
    broken = 0
    for _ in range(12):
        tr = rng.integers(-6, 7, 81).astype(np.float64)
        rc = rng.integers(0, 4, Eu.size).astype(np.float64)
        after, snap = [], []
        mincut_model(81, Eu, Ev, tr, rc, MC.ARCS_BOTH, period=1 << 30, invalid=after)
        assert sum(after) == 0
        try:
            mincut_model(81, Eu, Ev, tr, rc, MC.ARCS_BOTH, period=1 << 30,
                         relabel_after_apply=False, max_rounds=3000, invalid=snap)
        except RuntimeError:
            pass
        broken += int(sum(snap) > 0)
    assert broken > 0
