"""Measure the simplex driver's one-call cut pursuit (pfdr_cp_loss_d1_simplex)
on one GPU: wall time of the entry, where it goes (gradient, the K - 1 cuts,
the other graph steps, PFDR, the evolution / objective sums:
pfdr_cp_loss_d1_simplex_stats), the push/relabel rounds and global relabels of
every expansion's cut, and -- where oracle/_ref holds them -- the wall time of
the reference's CP code linked against this library's PFDR (cp_simplex_mi355x)
and of the reference itself (cp_simplex_ref) on the same problem.

Problem: an nx x ny grid (4- or 8-neighbour), K labels in vertical bands
observed through uniform noise, La_d1 constant; loss al (0 linear, 1
quadratic, else smoothed KL).  The first call is a warm-up (library
initialisation, allocator cache); the median of --reps further calls is
reported.  Prints one JSON line.

    python tools/bench_cp_simplex.py [--shape 512 512] [--conn 8] [--K 10] [--al 0.1]
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
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--al", type=float, default=0.1)
    ap.add_argument("--la", type=float, default=0.1)
    ap.add_argument("--noise", type=float, default=0.2)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--CP_difTol", type=float, default=1e-4)
    ap.add_argument("--CP_itMax", type=int, default=10)
    ap.add_argument("--PFDR_difTol", type=float, default=1e-4)
    ap.add_argument("--PFDR_itMax", type=int, default=2000)
    ap.add_argument("--rho", type=float, default=1.0)
    ap.add_argument("--condMin", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref", action="store_true",
                    help="also time oracle/_ref/cp_simplex_mi355x and cp_simplex_ref")
    args = ap.parse_args()
    from cp_pfdr_graph_d1_amd import pfdr
    from cp_pfdr_graph_d1_amd.graphs import uniform
    dt = np.float32 if args.dtype == "f32" else np.float64
    nx, ny = args.shape
    K, V = args.K, nx * ny
    Eu, Ev = pfdr.gen_grid_edges((nx, ny), args.conn)
    E = Eu.size
    v = np.arange(V)
    Q = args.noise * (1 + (2 * uniform(8, np.arange(K * V)) - 1).reshape(V, K))
    Q[v, (v % nx) * K // nx] += 1.0
    Q /= Q.sum(1, keepdims=True)
    Q = Q.astype(dt).ravel()
    La = np.full(E, args.la, dt)
    lib = pfdr.Lib()
    kw = dict(al=args.al, CP_difTol=args.CP_difTol, CP_itMax=args.CP_itMax, rho=args.rho,
              condMin=args.condMin, difRcd=0.0, difTol=args.PFDR_difTol, itMax=args.PFDR_itMax,
              obj=True, dif=True, time=True)
    runs = []
    for r in range(args.reps + 1):
        t = time.perf_counter()
        Cv, rP, it, Obj, Dif, Time = lib.cp_loss_d1_simplex(K, Q, Eu, Ev, La, **kw)
        wall = time.perf_counter() - t
        st = lib.cp_loss_d1_simplex_stats()
        st["wall"] = wall
        if r:
            runs.append(st)
    med = lambda key: round(float(np.median([s[key] for s in runs])) * 1e3, 3)
    st = runs[-1]
    out = {
        "what": "pfdr_cp_loss_d1_simplex, one MI355X, host arrays in, Cv / rP out",
        "graph": "%dx%d %d-neighbour grid (V=%d, E=%d), K=%d, al=%g, %s" % (
            nx, ny, args.conn, V, E, K, args.al, args.dtype),
        "CP_it": it, "rV": int(rP.size // K), "Obj": [float(x) for x in Obj[:it + 1]],
        "Dif": [float(x) for x in Dif[:it]],
        "entry_wall_ms": med("wall"),
        "phase_ms": {k: med(k) for k in ("gradient", "cuts", "graph", "pfdr", "sums", "total")},
        "expansions": st["expansions"], "cut_rounds_total": st["rounds"],
        "cut_relabels_total": st["relabels"], "pfdr_iterations_total": st["pfdr_it"],
        "cut_rounds_per_expansion": st["exp_rounds"].tolist(),
        "cut_relabels_per_expansion": st["exp_relabels"].tolist(),
    }
    if args.ref:
        import cp_problems as P
        p = dict(kind="simplex", V=V, E=E, N=0, K=K, dtype=dt, CP_itMax=args.CP_itMax,
                 PFDR_itMax=args.PFDR_itMax, positivity=0, CP_difTol=args.CP_difTol,
                 PFDR_difTol=args.PFDR_difTol, rho=args.rho, condMin=args.condMin, difRcd=0.0,
                 lo=-np.inf, hi=np.inf, al=args.al, Y=Q, A=None, Eu=Eu, Ev=Ev, La_d1=La,
                 La_l1=None)
        ref_dir = os.path.join(ROOT, "oracle", "_ref")
        with tempfile.TemporaryDirectory() as tmp:
            inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            P.write(inp, p)
            for prov in ("mi355x", "ref"):
                drv = P.driver("simplex", prov, ref_dir)
                if not os.path.exists(drv):
                    out["cp_simplex_%s" % prov] = "not built"
                    continue
                t = time.perf_counter()
                r = subprocess.run([drv, inp, outp], capture_output=True, text=True)
                wall = time.perf_counter() - t
                rec = {"process_wall_ms": round(wall * 1e3, 1), "rc": r.returncode}
                for tok in r.stderr.split():
                    if tok.startswith("cp_time_s="):
                        rec["cp_ms"] = round(float(tok[10:]) * 1e3, 1)
                if r.returncode == 0:
                    rV2, it2, Cv2, rP2 = P.read(outp, p)
                    rec.update(CP_it=it2, rV=rV2, same_Cv=bool(np.array_equal(Cv, Cv2)),
                               same_rP=bool(rP2.size == rP.size and np.array_equal(rP, rP2)))
                out["cp_simplex_%s" % prov] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
