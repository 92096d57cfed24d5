"""Measure the resumable cut-pursuit solver (pfdr.CPSolver) on one GPU against
the one-call entries, on a regularisation path: four scalings of La_d1 on one
graph.

Block 1: the handle -- seconds of create, then per scaling the seconds of
set_penalties and of run with its phases (gradient, cuts, graph, pfdr, sums:
CPSolver.stats) -- beside the same four problems solved by the one-call entry,
each from the one-component state with its own upload and setup.  The handle's
runs after the first are warm restarts from the previous solution, so the two
sides do not do the same iterations: CP_it and rV are printed for both.
Block 2: the seconds of get_state, set_state (with and without R where N > 0)
and set_partition at the final state.

Problem: tools/bench_cp_bounds.py's -- an nx x ny grid, three vertical bands
observed through uniform noise, identity A -- with an l1 term for l1 / duplex,
the box [-0.3, 0.8] for bounds and K = 4 noisy one-hot observations for the
simplex.  One warm-up pass of both sides first; prints one JSON line.

    python tools/bench_cp_resume.py --shape 512 512 [--kind l1|bounds|simplex|duplex]
                                    [--dtype f32] [--CP_itMax 10] [--scales 1 0.5 0.25 0.125]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--kind", choices=["l1", "bounds", "simplex", "duplex"], default="l1")
    ap.add_argument("--conn", type=int, default=8)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--la", type=float, default=0.15)
    ap.add_argument("--CP_difTol", type=float, default=1e-4)
    ap.add_argument("--CP_itMax", type=int, default=10)
    ap.add_argument("--scales", type=float, nargs="+", default=[1.0, 0.5, 0.25, 0.125])
    args = ap.parse_args()
    from cp_pfdr_graph_d1_amd import pfdr
    from cp_pfdr_graph_d1_amd.graphs import uniform
    dt = np.float32 if args.dtype == "f32" else np.float64
    nx, ny = args.shape
    V = nx * ny
    Eu, Ev = pfdr.gen_grid_edges((nx, ny), args.conn)
    E = Eu.size
    x = np.arange(V) % nx
    kind = args.kind
    lib = pfdr.Lib()
    simplex = kind == "simplex"
    if simplex:
        K = 4
        Q = 0.2 * (2 * uniform(9, np.arange(K * V)).reshape(V, K))
        Q[np.arange(V), x * K // nx] += 1.0
        Y = (Q / Q.sum(1, keepdims=True)).astype(dt).ravel()
        La = np.full(E, 0.1, dt)
        par = dict(CP_difTol=args.CP_difTol, CP_itMax=args.CP_itMax, rho=1.0, condMin=0.1,
                   difRcd=0.0, difTol=1e-4, itMax=1000)
        make = lambda la: pfdr.CPSolver("simplex", Y, Eu, Ev, la, K=K, al=0.1)
        entry = lambda la: lib.cp_loss_d1_simplex(K, Y, Eu, Ev, la, al=0.1, **par)
    else:
        truth = np.where(x < nx // 3, 1.0, np.where(x < 2 * nx // 3, -0.5, 0.25))
        Y = (truth + 0.4 * (2 * uniform(9, np.arange(V)) - 1)).astype(dt)
        La = np.full(E, args.la, dt)
        par = dict(CP_difTol=args.CP_difTol, CP_itMax=args.CP_itMax, rho=1.5, condMin=1e-3,
                   difRcd=0.0, difTol=1e-5, itMax=2000)
        if kind == "bounds":
            make = lambda la: pfdr.CPSolver("bounds", Y, Eu, Ev, la, lo=-0.3, hi=0.8)
            entry = lambda la: lib.cp_quadratic_d1_bounds(V, 0, Y, None, Eu, Ev, la, lo=-0.3,
                                                          hi=0.8, **par)
        else:
            L1 = np.full(V, 0.02, dt)
            make = lambda la: pfdr.CPSolver("l1", Y, Eu, Ev, la, La_l1=L1,
                                            duplex=kind == "duplex")
            fn = lib.cp_quadratic_d1_l1_duplex if kind == "duplex" else lib.cp_quadratic_d1_l1
            entry = lambda la: fn(V, 0, Y, None, Eu, Ev, la, L1, **par)
    las = [(s * La).astype(dt) for s in args.scales]
    ms = lambda t: round(t * 1e3, 3)

    def timed(f, *a, **kw):
        t = time.perf_counter()
        r = f(*a, **kw)
        return r, time.perf_counter() - t

    def handle_path():
        s, t_create = timed(make, las[0])
        rows = []
        for i, la in enumerate(las):
            t_pen = timed(s.set_penalties, la)[1] if i else 0.0
            out, t_run = timed(s.run, **par)
            st = s.stats()
            rows.append(dict(scale=args.scales[i], set_penalties_ms=ms(t_pen), run_wall_ms=ms(t_run),
                             CP_it=out[2], rV=int(out[1].size) // (K if simplex else 1),
                             phase_ms={k: ms(st[k]) for k in ("gradient", "cuts", "graph", "pfdr",
                                                              "sums", "total")}))
        return s, t_create, rows

    def entry_path():
        rows = []
        for i, la in enumerate(las):
            out, t = timed(entry, la)
            rows.append(dict(scale=args.scales[i], wall_ms=ms(t), CP_it=out[2],
                             rV=int(out[1].size) // (K if simplex else 1)))
        return rows

    handle_path()[0].close()  # warm-up: library initialisation, allocator cache
    entry_path()
    s, t_create, hrows = handle_path()
    erows = entry_path()
    st, t_get = timed(s.state)
    t_set = timed(s.set_state, st)[1]
    Cv, rX = st["Cv"], st["rX"]
    t_part = timed(s.set_partition, Cv, rX)[1]
    setup = s.stats()["setup"]
    s.close()
    handle_total = t_create + sum(r["run_wall_ms"] + r["set_penalties_ms"] for r in hrows) / 1e3
    entry_total = sum(r["wall_ms"] for r in erows) / 1e3
    print(json.dumps({
        "what": "pfdr.CPSolver on a path of %d La_d1 scalings beside the one-call entry, one "
                "MI355X, host arrays" % len(las),
        "graph": "%dx%d %d-neighbour grid (V=%d, E=%d), %s, %s" % (nx, ny, args.conn, V, E, kind,
                                                                  args.dtype),
        "path": {"create_wall_ms": ms(t_create), "create_setup_ms": ms(setup), "handle": hrows,
                 "entry": erows, "handle_total_ms": ms(handle_total),
                 "entry_total_ms": ms(entry_total)},
        "state": {"get_state_ms": ms(t_get), "set_state_ms": ms(t_set),
                  "set_partition_ms": ms(t_part)},
    }))


if __name__ == "__main__":
    main()
