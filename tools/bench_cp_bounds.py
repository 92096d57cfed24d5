"""Measure the bounds driver's one-call cut pursuit (pfdr_cp_quadratic_d1_bounds)
on one GPU: wall time of the entry, where it goes (gradient, the cuts, the
other graph steps and the reduction, PFDR, the evolution / objective sums:
pfdr_cp_quadratic_d1_bounds_stats), the push/relabel rounds and global relabels
of its cuts, and -- where oracle/_ref holds them -- the wall time of the
reference's CP code linked against this library's PFDR (cp_bounds_mi355x) and
of the reference itself (cp_bounds_ref) on the same problem, with a byte
comparison of what they return.

Problem: an nx x ny grid (4- or 8-neighbour), a truth of three vertical bands
(1, -0.5, 0.25) observed through uniform noise, identity A, La_d1 constant, the
box [lo, hi] (the default [-0.3, 0.8] binds on two of the three bands).  The
first call is a warm-up (library initialisation, allocator cache); the median
of --reps further calls is reported.  Prints one JSON line.

    python tools/bench_cp_bounds.py [--shape 512 512] [--conn 8] [--lo -0.3] [--hi 0.8]
                                    [--dtype f32] [--CP_itMax 10] [--reps 3] [--ref]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--conn", type=int, default=8)
    ap.add_argument("--lo", type=float, default=-0.3)
    ap.add_argument("--hi", type=float, default=0.8)
    ap.add_argument("--la", type=float, default=0.15)
    ap.add_argument("--noise", type=float, default=0.4)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--CP_difTol", type=float, default=1e-4)
    ap.add_argument("--CP_itMax", type=int, default=10)
    ap.add_argument("--PFDR_difTol", type=float, default=1e-5)
    ap.add_argument("--PFDR_itMax", type=int, default=2000)
    ap.add_argument("--rho", type=float, default=1.5)
    ap.add_argument("--condMin", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref", action="store_true",
                    help="also time oracle/_ref/cp_bounds_mi355x and cp_bounds_ref")
    args = ap.parse_args()
    from cp_pfdr_graph_d1_amd import pfdr
    from cp_pfdr_graph_d1_amd.graphs import uniform
    dt = np.float32 if args.dtype == "f32" else np.float64
    nx, ny = args.shape
    V = nx * ny
    Eu, Ev = pfdr.gen_grid_edges((nx, ny), args.conn)
    E = Eu.size
    x = np.arange(V) % nx
    truth = np.where(x < nx // 3, 1.0, np.where(x < 2 * nx // 3, -0.5, 0.25))
    Y = (truth + args.noise * (2 * uniform(9, np.arange(V)) - 1)).astype(dt)
    La = np.full(E, args.la, dt)
    lib = pfdr.Lib()
    kw = dict(lo=args.lo, hi=args.hi, CP_difTol=args.CP_difTol, CP_itMax=args.CP_itMax,
              rho=args.rho, condMin=args.condMin, difRcd=0.0, difTol=args.PFDR_difTol,
              itMax=args.PFDR_itMax)
    runs = []
    for r in range(args.reps + 1):
        t = time.perf_counter()
        Cv, rX, it, Obj, Dif, Time = lib.cp_quadratic_d1_bounds(V, 0, Y, None, Eu, Ev, La, **kw)
        wall = time.perf_counter() - t
        st = lib.cp_quadratic_d1_bounds_stats()
        st["wall"] = wall
        if r:
            runs.append(st)
    med = lambda key: round(float(np.median([s[key] for s in runs])) * 1e3, 3)
    st = runs[-1]
    out = {
        "what": "pfdr_cp_quadratic_d1_bounds, one MI355X, host arrays in, Cv / rX out",
        "graph": "%dx%d %d-neighbour grid (V=%d, E=%d), box [%g, %g], %s" % (
            nx, ny, args.conn, V, E, args.lo, args.hi, args.dtype),
        "CP_it": it, "rV": int(rX.size),
        "at_lo": int(np.count_nonzero(rX == dt(args.lo))),
        "at_hi": int(np.count_nonzero(rX == dt(args.hi))),
        "Obj": [float(x) for x in Obj[:it + 1]], "Dif": [float(x) for x in Dif[:it]],
        "entry_wall_ms": med("wall"),
        "phase_ms": {k: med(k) for k in ("gradient", "cuts", "graph", "pfdr", "sums", "total")},
        "cuts": st["n_cuts"], "cut_rounds_total": st["rounds"],
        "cut_relabels_total": st["relabels"], "pfdr_iterations_total": st["pfdr_it"],
    }
    if args.ref:
        import cp_problems as P
        p = dict(kind="bounds", V=V, E=E, N=0, K=0, dtype=dt, CP_itMax=args.CP_itMax,
                 PFDR_itMax=args.PFDR_itMax, positivity=0, CP_difTol=args.CP_difTol,
                 PFDR_difTol=args.PFDR_difTol, rho=args.rho, condMin=args.condMin, difRcd=0.0,
                 lo=args.lo, hi=args.hi, al=0.0, Y=Y, A=None, Eu=Eu, Ev=Ev, La_d1=La, La_l1=None)
        ref_dir = os.path.join(ROOT, "oracle", "_ref")
        with tempfile.TemporaryDirectory() as tmp:
            inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            P.write(inp, p)
            for prov in ("mi355x", "ref"):
                drv = P.driver("bounds", prov, ref_dir)
                if not os.path.exists(drv):
                    out["cp_bounds_%s" % prov] = "not built"
                    continue
                t = time.perf_counter()
                r = subprocess.run([drv, inp, outp], capture_output=True, text=True)
                wall = time.perf_counter() - t
                rec = {"process_wall_ms": round(wall * 1e3, 1), "rc": r.returncode}
                for tok in r.stderr.split():
                    if tok.startswith("cp_time_s="):
                        rec["cp_ms"] = round(float(tok[10:]) * 1e3, 1)
                if r.returncode == 0:
                    rV2, it2, Cv2, rX2 = P.read(outp, p)
                    rec.update(CP_it=it2, rV=rV2, same_Cv=bool(np.array_equal(Cv, Cv2)),
                               same_rX=bool(rX2.size == rX.size and np.array_equal(rX, rX2)))
                out["cp_bounds_%s" % prov] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
