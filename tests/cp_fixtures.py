"""TEST INFRASTRUCTURE -- the recorded cut-pursuit iterations under tests/golden/
(cp_*.npz, made by tests/golden/make_cp_golden.py): their names by driver, the
loader, and the recorded cuts that are ties.
"""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "cp_*.npz")))
_ALL = [os.path.basename(f)[:-4] for f in FILES]
# the l1 driver's iterations; the bounds driver's (cp_bounds_*); the dense
# reduced problems are test_cp_reduce.py's (cp_dense_*)
NAMES = [n for n in _ALL
         if not n.startswith(("cp_bounds_", "cp_dense_", "cp_simplex_", "cp_duplex_"))]
BNAMES = [n for n in _ALL if n.startswith("cp_bounds_")]
# the simplex driver's (src/CP_PFDR_graph_loss_d1_simplex.cpp): K - 1
# alpha-expansions per iteration, label vectors rP
SNAMES = [n for n in _ALL if n.startswith("cp_simplex_")]
# the duplex driver's (src/CP_PFDR_graph_quadratic_d1_l1_duplex.cpp): one
# two-layer cut per iteration, 2V segments
DNAMES = [n for n in _ALL if n.startswith("cp_duplex_")]


def load_case(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    c = {k[3:]: d[k] for k in d.files if k.startswith("in_")}
    for k in ("A", "La_l1"):
        c.setdefault(k, None)
    c["positivity"] = int(c.get("positivity", 0))
    for k in ("K",):
        if k in c:
            c[k] = int(c[k])
    if "al" in c:
        c["al"] = float(c["al"])
    c["CP_difTol"] = float(c["CP_difTol"])
    for k in ("lo", "hi"):
        if k in c:
            c[k] = float(c[k])
    return c, d


def iteration_state(d, k, io):
    vals = "rP" if ("k%d_%s_rP" % (k, io)) in d.files else "rX"
    return {key: d["k%d_%s_%s" % (k, io, key)] for key in ("active", "Cv", "Vc", "rVc", vals)}


def expansion_segments(d, K, k):
    """the segments of the K - 1 alpha-expansions of recorded iteration k"""
    return [d["k%d_seg_exp%d" % (k, n)] for n in range(1, K - 1)] + [d["k%d_seg_last" % k]]


# Recorded cuts exempt from byte-equality: (fixture, iteration).  An entry is a
# genuine tie between minimum cuts: its value in f64 equals the recorded one
# within 1e-12 relative.  At most 4 of the 48.  Measured on an MI355X: 47 of 48
# byte-equal; in this one, 10 nodes change side at a cut value that is the
# recorded one to the last bit of f64 (f32 capacities; the f64 twin fixture and
# the f64 numpy model return the recorded set).
TIES = (("cp_duplex_grid2d_l1_f32", 4),)
assert len(TIES) <= 4
