"""Child of tests/test_gram_exact_gpu.py: python tests/gram_child.py in.npz
out.npz.  Loads the matrices "A.<name>" and layouts "w.<name>", calls
pfdr.gram on each and saves "G.<name>".  It is started with
PFDR_GRAM_SPLIT=0, which gram() reads once per process: the f32 cases then
run on the exact-f32 tiles (k_gram_v<float>, k_gram<float>).  Nothing is
checked here; the parent compares."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cp_pfdr_graph_d1_amd import pfdr  # noqa: E402


def main(src, dst):
    out = {}
    with np.load(src) as z:
        for key in z.files:
            if key.startswith("A."):
                name = key[2:]
                out["G." + name], _ = pfdr.gram(z[key], int(z["w." + name]))
    np.savez(dst, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
