"""Measure cut pursuit with a sparse observation operator
(pfdr_cp_solver_create_sparse) on one GPU against the dense solver on the same
problem: where a run goes (pfdr_cp_solver_stats: gradient, the cuts, the other
graph steps and the reduction, PFDR, the evolution / objective sums), the
seconds create spent, and whether both return the same bytes.

Problem: the 3x3 normalised blur (graphs.blur3x3_csc) on an nx x ny grid, N = V,
a truth of three vertical bands (1, -0.5, 0.25) observed through the blur and
uniform noise, a 4-neighbour graph, La_d1 constant; kind l1 (with La_l1) or
bounds (box [-0.3, 0.8]).  Without --dense only the sparse solver runs (the
dense A holds V^2 reals).  With it, the sparse and the dense solver alternate
in one process.  The first run of each is a warm-up (library initialisation,
allocator cache); --reps further runs of each are reported, every run on a
fresh solver.  Prints one JSON line.

--reduced dense|sparse|sparse_all (one or several) chooses how the sparse solver
keeps the reduced operator (pfdr_cp_solver_set_reduced): of a direct iteration
("sparse"), and of a premultiplied one as well ("sparse_all", whose counts are
"premultiplied_stats", pfdr_cp_solver_premultiplied_stats); with several, the
modes alternate like the solvers above.  A direct iteration needs
rV >= 2 N pit / (N + pit), about twice the previous PFDR iteration count, so
--pfdr-itmax must be small for a run to take one: the line reports, per mode,
how many iterations were solved on a sparse rA and how many direct ones on a
dense rA (pfdr_cp_solver_reduced_stats), the most entries a sparse rA held
beside N rV of the final partition, and the device memory in use after the
mode's runs (hipMemGetInfo through torch; the library's allocator cache keeps
what a run freed, so run one mode per process for that figure).

    python tools/bench_cp_sparse.py --shape 128 128 --kind l1 [--dense] [--dtype f32]
                                    [--CP_itMax 10] [--reps 3]
                                    [--reduced dense sparse] [--pfdr-itmax 2000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("gradient", "cuts", "graph", "pfdr", "sums", "total", "setup")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, default=[128, 128])
    ap.add_argument("--kind", choices=["l1", "bounds"], default="l1")
    ap.add_argument("--dense", action="store_true", help="also run the dense solver")
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--la", type=float, default=0.05)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--CP_difTol", type=float, default=1e-4)
    ap.add_argument("--CP_itMax", type=int, default=10)
    ap.add_argument("--PFDR_difTol", type=float, default=1e-5)
    ap.add_argument("--PFDR_itMax", "--pfdr-itmax", dest="PFDR_itMax", type=int, default=2000)
    ap.add_argument("--reduced", nargs="+", choices=["dense", "sparse", "sparse_all"],
                    default=["dense"],
                    help="the sparse solver's reduced operator: one mode, or several alternating")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from cp_pfdr_graph_d1_amd import pfdr
    from cp_pfdr_graph_d1_amd.graphs import blur3x3_csc, uniform
    dt = np.float32 if args.dtype == "f32" else np.float64
    nx, ny = args.shape
    V = nx * ny
    colptr, rowidx, val = blur3x3_csc(nx, ny)
    csc = pfdr.CSC(colptr, rowidx, val.astype(dt), V)
    cols = np.repeat(np.arange(V), np.diff(colptr))
    x = np.arange(V) % nx
    truth = np.where(x < nx // 3, 1.0, np.where(x < 2 * nx // 3, -0.5, 0.25))
    Y = np.bincount(rowidx, val * truth[cols], V)
    Y = (Y + args.noise * (2 * uniform(9, np.arange(V)) - 1)).astype(dt)
    Eu, Ev = pfdr.gen_grid_edges((nx, ny), 4)
    La = np.full(Eu.size, args.la, dt)
    own = dict(lo=-0.3, hi=0.8) if args.kind == "bounds" else dict(La_l1=np.full(V, 0.02, dt))
    dense = None
    if args.dense:
        dense = np.zeros((V, V), dt, order="F")
        dense[rowidx, cols] = csc.val
        dense = dense.ravel(order="F")
    run = dict(CP_difTol=args.CP_difTol, CP_itMax=args.CP_itMax, rho=1.5, condMin=1e-3,
               difRcd=0.0, difTol=args.PFDR_difTol, itMax=args.PFDR_itMax)

    def device_mb():
        try:
            import torch
            free, total = torch.cuda.mem_get_info()
            return round((total - free) / 2 ** 20, 1)
        except Exception:
            return None

    def once(A, reduced):
        t = time.perf_counter()
        s = pfdr.CPSolver(args.kind, Y, Eu, Ev, La, A=A, N=V, **own)
        if reduced != "dense":
            s.set_reduced(reduced)
        r = s.run(**run)
        st = s.stats()
        if A is csc:
            st["reduced"] = s.reduced_stats()
            st["premultiplied"] = s.premultiplied_stats()
        s.close()
        st["wall"] = time.perf_counter() - t
        st["device_mb"] = device_mb()
        return r, st

    modes = list(dict.fromkeys(args.reduced))
    variants = [("sparse" if len(modes) == 1 else "sparse_A_reduced_" + m, csc, m) for m in modes]
    if args.dense:
        variants.append(("dense", dense, "dense"))
    runs = {name: [] for name, _, _ in variants}
    last = {}
    for rep in range(args.reps + 1):
        for name, A, mode in variants:  # alternating
            r, st = once(A, mode)
            last[name] = r
            if rep:
                runs[name].append(st)
    ms = lambda name, key: [round(s[key] * 1e3, 3) for s in runs[name]]
    first = variants[0][0]
    r = last[first]
    out = {
        "what": "pfdr_cp_solver_create_sparse + run, one MI355X, host arrays in",
        "problem": "3x3 blur on the %dx%d grid (N = V = %d, nnz = %d), kind %s, %s" % (
            nx, ny, V, csc.nnz, args.kind, args.dtype),
        "CP_it": r[2], "rV": int(r[1].size), "Obj": [float(x) for x in r[3][:r[2] + 1]],
        "phase_ms": {name: dict({k: ms(name, k) for k in PHASES}, wall=ms(name, "wall"))
                     for name, _, _ in variants},
        "pfdr_iterations_total": {name: runs[name][-1]["pfdr_it"] for name, _, _ in variants},
        "PFDR_itMax": args.PFDR_itMax,
        "reduced": {name: dict(zip(("sparse_iterations", "dense_direct_iterations", "max_rnnz"),
                                   runs[name][-1]["reduced"]),
                               N_rV_final=V * int(last[name][1].size),
                               CP_it=last[name][2], rV=int(last[name][1].size),
                               device_mb_after=[s["device_mb"] for s in runs[name]])
                    for name, A, _ in variants if A is csc},
        "premultiplied_stats": {name: dict(zip(("sparse_iterations", "dense_iterations",
                                                "max_rnnz"), runs[name][-1]["premultiplied"]))
                                for name, A, _ in variants if A is csc},
    }
    if args.dense:
        d = last["dense"]
        out["same_bytes_as_dense"] = len(modes) == 1 and modes[0] == "dense" and bool(
            r[2] == d[2] and all(a.tobytes() == b.tobytes() for a, b in
                                 ((r[0], d[0]), (r[1], d[1]), (r[3], d[3]), (r[4], d[4]))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
