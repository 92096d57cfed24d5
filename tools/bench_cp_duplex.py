"""Measure the duplex driver's one-call cut pursuit
(pfdr_cp_quadratic_d1_l1_duplex) on one GPU: wall time of the entry, where it
goes (gradient, the cuts, the other graph steps and the reduction, PFDR, the
evolution / objective sums: pfdr_cp_quadratic_d1_l1_duplex_stats), the
push/relabel rounds and global relabels of its two-layer cuts, the l1 entry
(pfdr_cp_quadratic_d1_l1: two one-layer cuts per iteration) on the same
problem, and -- where oracle/_ref holds them -- the wall time of the
reference's CP code linked against this library's PFDR (cp_duplex_mi355x) and
of the reference itself (cp_duplex_ref), with a byte comparison of what they
return.

Problem: an nx x ny grid (4- or 8-neighbour), a truth of three vertical bands
(1, -0.5, 0.25) observed through uniform noise, identity A, La_d1 and La_l1
constant, positivity optional.  The first call is a warm-up (library
initialisation, allocator cache); the median of --reps further calls is
reported.  Prints one JSON line.

    python tools/bench_cp_duplex.py [--shape 512 512] [--conn 4] [--l1 0.02]
                                    [--positivity 0] [--dtype f32] [--CP_itMax 10]
                                    [--reps 3] [--ref]
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
    ap.add_argument("--conn", type=int, default=4)
    ap.add_argument("--la", type=float, default=0.15)
    ap.add_argument("--l1", type=float, default=0.02)
    ap.add_argument("--positivity", type=int, default=0)
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
                    help="also time oracle/_ref/cp_duplex_mi355x and cp_duplex_ref")
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
    L1 = np.full(V, args.l1, dt)

    def functional(Cv, rX):
        """F in f64 at x = rX[Cv], the premultiplied form the driver's Obj uses"""
        x = np.asarray(rX, np.float64)[Cv]
        return float(np.sum(x * (0.5 * x - Y)) + args.la * np.sum(np.abs(x[Eu] - x[Ev]))
                     + args.l1 * np.sum(np.abs(x)))

    def moved(a, b):
        """vertices outside the component of ``b`` that holds most of their component of ``a``"""
        pair, n = np.unique(a.astype(np.int64) * (int(b.max()) + 1) + b, return_counts=True)
        best = np.zeros(int(a.max()) + 1, np.int64)
        np.maximum.at(best, pair // (int(b.max()) + 1), n)
        return int(a.size - best.sum())

    lib = pfdr.Lib()
    kw = dict(positivity=args.positivity, CP_difTol=args.CP_difTol, CP_itMax=args.CP_itMax,
              rho=args.rho, condMin=args.condMin, difRcd=0.0, difTol=args.PFDR_difTol,
              itMax=args.PFDR_itMax)
    runs, l1_wall = [], []
    for r in range(args.reps + 1):
        t = time.perf_counter()
        Cv, rX, it, Obj, Dif, Time = lib.cp_quadratic_d1_l1_duplex(V, 0, Y, None, Eu, Ev, La, L1,
                                                                   **kw)
        wall = time.perf_counter() - t
        st = lib.cp_quadratic_d1_l1_duplex_stats()
        st["wall"] = wall
        t = time.perf_counter()
        Cv1, rX1, it1, Obj1, _, _ = lib.cp_quadratic_d1_l1(V, 0, Y, None, Eu, Ev, La, L1, **kw)
        if r:
            runs.append(st)
            l1_wall.append(time.perf_counter() - t)
    med = lambda key: round(float(np.median([s[key] for s in runs])) * 1e3, 3)
    st = runs[-1]
    out = {
        "what": "pfdr_cp_quadratic_d1_l1_duplex, one MI355X, host arrays in, Cv / rX out",
        "graph": "%dx%d %d-neighbour grid (V=%d, E=%d), l1 %g, positivity %d, %s" % (
            nx, ny, args.conn, V, E, args.l1, args.positivity, args.dtype),
        "CP_it": it, "rV": int(rX.size), "zeros": int(np.count_nonzero(rX == 0)),
        "Obj": [float(x) for x in Obj[:it + 1]], "Dif": [float(x) for x in Dif[:it]],
        "entry_wall_ms": med("wall"),
        "phase_ms": {k: med(k) for k in ("gradient", "cuts", "graph", "pfdr", "sums", "total")},
        "cuts": st["n_cuts"], "cut_rounds_total": st["rounds"],
        "cut_relabels_total": st["relabels"], "pfdr_iterations_total": st["pfdr_it"],
        "F_f64": functional(Cv, rX),
        "l1_entry": {"wall_ms": round(float(np.median(l1_wall)) * 1e3, 3), "CP_it": it1,
                     "rV": int(rX1.size), "Obj_last": float(Obj1[it1]),
                     "same_Cv": bool(np.array_equal(Cv, Cv1)),
                     "vertices_in_another_component": moved(Cv, Cv1),
                     "F_f64": functional(Cv1, rX1)},
    }
    if args.ref:
        import cp_problems as P
        p = dict(kind="duplex", V=V, E=E, N=0, K=0, dtype=dt, CP_itMax=args.CP_itMax,
                 PFDR_itMax=args.PFDR_itMax, positivity=args.positivity,
                 CP_difTol=args.CP_difTol, PFDR_difTol=args.PFDR_difTol, rho=args.rho,
                 condMin=args.condMin, difRcd=0.0, lo=-np.inf, hi=np.inf, al=0.0, Y=Y, A=None,
                 Eu=Eu, Ev=Ev, La_d1=La, La_l1=L1)
        ref_dir = os.path.join(ROOT, "oracle", "_ref")
        with tempfile.TemporaryDirectory() as tmp:
            inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            P.write(inp, p)
            for prov in ("mi355x", "ref"):
                drv = P.driver("duplex", prov, ref_dir)
                if not os.path.exists(drv):
                    out["cp_duplex_%s" % prov] = "not built"
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
                               same_rX=bool(rX2.size == rX.size and np.array_equal(rX, rX2)),
                               vertices_in_another_component=moved(Cv, Cv2),
                               F_f64=functional(Cv2, rX2))
                out["cp_duplex_%s" % prov] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
