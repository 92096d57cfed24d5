"""Generate the two-layer minimum-cut fixtures from the REFERENCE's own maxflow.

For every case of mincut_duplex_cases.py, run Boykov-Kolmogorov on the duplex
driver's own two-layer graph (oracle/_ref/libcp_step_duplex_ref.so,
CPStepRefDuplex.maxflow) and store the inputs, the segments of the 2V nodes
and the value of that cut.  Runs only where the reference is built.

Usage:  python tests/golden/make_mincut_duplex_golden.py          (write the files)
        python tests/golden/make_mincut_duplex_golden.py --check  (compare with them)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, HERE)
from oracle import CPStepRefDuplex  # noqa: E402
import mincut_duplex_cases as MD  # noqa: E402


def main():
    if not CPStepRefDuplex.available():
        sys.exit("the reference maxflow is not built (make -C oracle ref)")
    check = "--check" in sys.argv
    os.makedirs(MD.DIR, exist_ok=True)
    ref = CPStepRefDuplex()
    bad = 0
    for name in MD.names():
        c = MD.inputs(name)
        seg = ref.maxflow(c["V"], c["Eu"], c["Ev"], c["tr_cap"], c["r_link"], c["r_cap"])
        val = MD.cut_duplex(c["V"], c["Eu"], c["Ev"], c["tr_cap"], c["r_link"], c["r_cap"], seg)
        assert np.isfinite(val) and val == int(val), (name, val)
        if check:
            g = MD.load(name)
            same = (np.array_equal(g["segment"], seg) and float(g["cut"]) == val
                    and all(g[k].dtype == c[k].dtype and np.array_equal(g[k], c[k])
                            for k in ("Eu", "Ev", "tr_cap", "r_link", "r_cap")))
            print("%-18s %s" % (name, "same" if same else "DIFFERENT"))
            bad += not same
            continue
        np.savez_compressed(MD.path(name), V=np.int32(c["V"]), Eu=c["Eu"], Ev=c["Ev"],
                            tr_cap=c["tr_cap"], r_link=c["r_link"], r_cap=c["r_cap"],
                            segment=seg, cut=np.float64(val))
        print("%-18s V=%5d E=%5d source=%5d of %5d cut=%g  %d bytes" % (
            name, c["V"], c["Eu"].size, int((seg == 0).sum()), 2 * c["V"], val,
            os.path.getsize(MD.path(name))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
