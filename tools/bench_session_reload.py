"""Measure the reusable PFDR session (pfdr.Session(reusable=True), reload) on one
GPU against fresh sessions, on a regularisation path: four scalings of La_d1
on one graph.

Block 1 (default): per scaling, the wall seconds of create + prepare + run of a
fresh plain session beside reload + prepare + run of one reusable session
(its first scaling is its create), with the iterations each ran; the two sides
solve the same problems from the same start (X0 = 0), so the iterations are
equal and the final iterates are compared byte for byte.
Block 2 (--measure create | reload): the median of --reps wall times of
create + prepare of a plain session, or of reload + prepare of a reusable one,
on the same inputs, every timing closed by a device synchronise.  `create`
runs with whatever library PFDR_LIB_PATH names, so an older build of the
library can be measured in a process of its own.

Problem: an nx x ny [x nz] grid (4- / 6-connected), piecewise-constant
observation through uniform noise, identity A, l1 + TV; or --workload headline
/ c5 of tools/workloads.py (bench.py's graphs).  Inputs resident on the device
as in bench.py (--host: numpy arrays).  Prints one JSON line.

    python tools/bench_session_reload.py --shape 1024 1024 [--workload headline]
        [--dtype f32] [--steps 100] [--difTol 0] [--scales 1 0.5 0.25 0.125]
        [--measure create|reload] [--reps 5] [--host]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs="+", default=[1024, 1024])
    ap.add_argument("--workload", choices=["headline", "c5"], default=None)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--steps", type=int, default=100, help="itMax of every solve")
    ap.add_argument("--difTol", type=float, default=0.0, help="0: fixed number of steps")
    ap.add_argument("--scales", type=float, nargs="+", default=[1.0, 0.5, 0.25, 0.125])
    ap.add_argument("--measure", choices=["create", "reload"], default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    import torch
    from cp_pfdr_graph_d1_amd import pfdr
    from cp_pfdr_graph_d1_amd.graphs import piecewise_observation

    if args.workload:
        from workloads import WORKLOADS
        wl = WORKLOADS[args.workload]
        inp = wl.inputs(0, 1)
        kind, dt, V, E, kw = wl.kind, wl.dtype, inp["V"], inp["E"], inp["kw"]
        graph = "%s (%s)" % (args.workload, inp["graph"])
    else:
        shape = tuple(args.shape)
        dt = np.float32 if args.dtype == "f32" else np.float64
        Eu, Ev = pfdr.gen_grid_edges(shape, 2 * len(shape))
        V, E, kind = int(np.prod(shape)), Eu.size, pfdr.PFDR_KIND_L1
        kw = dict(Eu=Eu, Ev=Ev, La_d1=np.full(E, 0.1, dt), X0=np.zeros(V, dt),
                  Y=piecewise_observation(shape, 2, dt), La_l1=np.full(V, 0.01, dt), rho=1.5,
                  condMin=1e-3)
        graph = "x".join(map(str, shape)) + " grid"
    las = [(s * np.asarray(kw["La_d1"])).astype(dt) for s in args.scales]
    if not args.host:
        for k, v in list(kw.items()):
            if isinstance(v, np.ndarray):
                kw[k] = torch.from_numpy(np.ascontiguousarray(
                    v, np.int32 if k in ("Eu", "Ev") else dt)).cuda()
        las = [torch.from_numpy(la).cuda() for la in las]
        kw["device"] = True
        torch.cuda.synchronize()
    kw.update(difTol=args.difTol, itMax=args.steps, record_dif=args.difTol > 0)
    ms = lambda t: round(t * 1e3, 3)

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t

    def create(la, reusable=False):
        s = pfdr.Session(kind, dt, V, E, **dict(kw, La_d1=la), reusable=reusable)
        s.prepare(args.steps)
        s.sync()
        return s

    def reload(s, la):
        s.reload(La_d1=la, X0=kw["X0"])
        s.prepare(args.steps)
        s.sync()

    out = {"graph": "%s (V=%d, E=%d), %s, %s arrays" % (graph, V, E, np.dtype(dt).name,
                                                         "host" if args.host else "device"),
           "lib": os.environ.get("PFDR_LIB_PATH") or "libpfdr_mi355x.so"}
    if args.measure == "create":
        create(las[0]).close()  # warm-up: library initialisation, allocator cache
        ts = []
        for i in range(args.reps):
            s, t = timed(lambda: create(las[i % len(las)]))
            s.close()
            ts.append(t)
        out.update(what="create + prepare of a plain session", wall_ms=[ms(t) for t in ts],
                   median_ms=ms(statistics.median(ts)))
    elif args.measure == "reload":
        s = create(las[0], reusable=True)
        reload(s, las[1 % len(las)])  # warm-up: staging
        ts = [timed(lambda: reload(s, las[i % len(las)]))[1] for i in range(args.reps)]
        out.update(what="reload + prepare of a reusable session", wall_ms=[ms(t) for t in ts],
                   median_ms=ms(statistics.median(ts)), device_bytes=s.device_bytes(),
                   staging_bytes=s.query("staging_bytes"))
        s.close()
    else:
        def fresh_path():
            rows = []
            for i, la in enumerate(las):
                s, t_setup = timed(lambda: create(la))
                it, t_run = timed(lambda: s.run(args.steps))
                rows.append(dict(scale=args.scales[i], setup_ms=ms(t_setup), run_ms=ms(t_run),
                                 it=it, X=s.result()[0]))
                s.close()
            return rows

        def reload_path():
            rows, s = [], None
            for i, la in enumerate(las):
                if s is None:
                    s, t_setup = timed(lambda: create(la, reusable=True))
                else:
                    t_setup = timed(lambda: reload(s, la))[1]
                it, t_run = timed(lambda: s.run(args.steps))
                rows.append(dict(scale=args.scales[i], setup_ms=ms(t_setup), run_ms=ms(t_run),
                                 it=it, reconditionings=s.query("reconditionings"),
                                 X=s.result()[0]))
            s.close()
            return rows

        create(las[0]).close()  # warm-up
        f, r = fresh_path(), reload_path()
        same = all(a["it"] == b["it"] and a.pop("X").tobytes() == b.pop("X").tobytes()
                   for a, b in zip(f, r))
        total = lambda rows: ms(sum(x["setup_ms"] + x["run_ms"] for x in rows) / 1e3)
        out.update(what="a path of %d La_d1 scalings: fresh plain sessions (create + prepare, "
                        "run) beside one reusable session (create, then reload + prepare, run)"
                        % len(las),
                   fresh=f, reusable=r, fresh_total_ms=total(f), reusable_total_ms=total(r),
                   identical=same)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
