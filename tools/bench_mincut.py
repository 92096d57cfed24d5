"""Measure the device minimum cut (pfdr_cpgraph_mincut) on cut-pursuit-like
capacities, with the reference's Boykov-Kolmogorov maxflow timed beside it
where oracle/_ref/libcp_step_ref.so exists.

Capacities: tr_cap = the headline piecewise observation minus its means over
alternating blocks of --block^dim vertices (the gradient of a reduced optimum:
it sums to about zero over each component), r_cap = 0.1 with --zeros of the
edges at zero (active edges).  BK runs in a child process started before this
one touches the GPU.  Prints one JSON line.

--duplex measures the two-layer cut (pfdr_cpgraph_mincut_duplex) instead: the
duplex driver's capacities for that gradient with an l1 weight --l1 on every
vertex of a zero component (up / down = gradient +- l1, m = max(0, -up, down),
tr_cap = (-down + m, -(up + m)), r_link = m), its rounds and global relabels,
the one-layer cut on the same graph beside it, and the reference's BK on its
own two-layer graph where oracle/_ref/libcp_step_duplex_ref.so exists.

    python tools/bench_mincut.py [--shape 250 200 200] [--graph grid|knn]
                                 [--dtype f32|f64] [--reps 3] [--no-ref]
                                 [--duplex [--l1 0.05] [--no-one-layer]]
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def problem(args):
    from cp_pfdr_graph_d1_amd import pfdr
    shape = tuple(args.shape)
    V = int(np.prod(shape))
    dt = np.float32 if args.dtype == "f32" else np.float64
    if args.graph == "knn":
        Eu, Ev = pfdr.gen_knn_jitter_grid(shape, 6, 6, 0.25)
    else:
        Eu, Ev = pfdr.gen_grid_edges(shape, 2 * len(shape))
    Y = pfdr.gen_piecewise(shape[0], V, 2, dt, 0.2).astype(np.float64)
    v = np.arange(V, dtype=np.int64)
    blk, stride, mult = np.zeros(V, np.int64), 1, 1
    for n in shape:
        nb = (n + args.block - 1) // args.block
        blk += ((v // stride) % n) // args.block * mult
        stride *= n
        mult *= nb
    tr = Y - (np.bincount(blk, Y) / np.maximum(np.bincount(blk), 1))[blk]
    rng = np.random.default_rng(11)
    rc = np.full(Eu.size, 0.1)
    rc[rng.random(Eu.size) < args.zeros] = 0
    return V, Eu, Ev, tr.astype(dt), rc.astype(dt)


def cut_value(Eu, Ev, tr, rc, seg):
    tr, rc, s = tr.astype(np.float64), rc.astype(np.float64), seg.astype(bool)
    su, sv = s[Eu], s[Ev]
    return float(tr[s & (tr > 0)].sum() - tr[~s & (tr < 0)].sum() + rc[su != sv].sum())


def duplex_capacities(tr, l1):
    """the two-layer terminals and links of gradient ``tr`` (k_cp_trcap_duplex, x = 0)"""
    dt = tr.dtype.type
    up, dn = tr + dt(l1), tr - dt(l1)
    m = np.maximum(dt(0), np.maximum(-up, dn))
    return np.concatenate([-dn + m, -(up + m)]).astype(tr.dtype), m.astype(tr.dtype)


def cut_value_duplex(V, Eu, Ev, tr, link, rc, seg):
    tr, link, rc = (a.astype(np.float64) for a in (tr, link, rc))
    s = seg.astype(bool)
    val = tr[s & (tr > 0)].sum() - tr[~s & (tr < 0)].sum() + link[~s[:V] & s[V:]].sum()
    for off in (0, V):
        val += rc[s[off + Eu] != s[off + Ev]].sum()
    return float(val)


def child(path):
    """the reference's BK on the saved capacities (no GPU in this process)"""
    from oracle import CPStepRef, CPStepRefDuplex
    z = np.load(path + ".npz")
    if "link" in z.files:
        ref = CPStepRefDuplex()
        t = time.perf_counter()
        seg = ref.maxflow(z["link"].size, z["Eu"], z["Ev"], z["tr"], z["link"], z["rc"])
        ms = 1e3 * (time.perf_counter() - t)
        np.save(path + "_seg.npy", seg)
        print(json.dumps({"bk_ms": ms}))
        return
    ref = CPStepRef()
    t = time.perf_counter()
    seg = ref.maxflow(z["Eu"], z["Ev"], z["tr"], z["rc"])
    ms = 1e3 * (time.perf_counter() - t)
    np.save(path + "_seg.npy", seg)
    print(json.dumps({"bk_ms": ms}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs="+", default=(250, 200, 200))
    ap.add_argument("--graph", choices=("grid", "knn"), default="knn")
    ap.add_argument("--dtype", choices=("f32", "f64"), default="f32")
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--zeros", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--duplex", action="store_true", help="the two-layer cut")
    ap.add_argument("--l1", type=float, default=0.05, help="--duplex: the l1 weight")
    ap.add_argument("--no-one-layer", action="store_true",
                    help="--duplex: skip the one-layer cut (to trace the two-layer cut alone)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    V, Eu, Ev, tr, rc = problem(args)
    out = {"graph": args.graph, "shape": list(args.shape), "dtype": args.dtype, "V": V,
           "E": int(Eu.size)}
    from oracle import CPStepRef, CPStepRefDuplex
    bk = None
    tmp = tempfile.mkdtemp(prefix="bench_mincut_")
    path = os.path.join(tmp, "caps")
    if args.duplex:
        tr1 = tr
        tr, link = duplex_capacities(tr1, args.l1)
        out.update(cut="two-layer", nodes=2 * V, arcs=2 * (2 * int(Eu.size) + V), l1=args.l1)
    have_ref = CPStepRefDuplex.available() if args.duplex else CPStepRef.available()
    if not args.no_ref and have_ref:
        if args.duplex:
            np.savez(path, Eu=Eu, Ev=Ev, tr=tr, link=link, rc=rc)
        else:
            np.savez(path, Eu=Eu, Ev=Ev, tr=tr, rc=rc)
        bk = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", path],
                              stdout=subprocess.PIPE, text=True)
    import torch
    from cp_pfdr_graph_d1_amd import pfdr
    torch.cuda.set_device(0)
    g = pfdr.CPGraph(V, Eu, Ev, np.zeros(Eu.size, tr.dtype))
    if args.duplex:
        cut = lambda: g.mincut_duplex(tr, link, rc)
        value = lambda s: cut_value_duplex(V, Eu, Ev, tr, link, rc, s)
    else:
        cut = lambda: g.mincut(tr, rc)
        value = lambda s: cut_value(Eu, Ev, tr, rc, s)
    seg, flow, rounds = cut()  # warm-up: caches (the CSR), allocations
    times = []
    for _ in range(args.reps):
        t = time.perf_counter()
        seg, flow, rounds = cut()
        times.append(1e3 * (time.perf_counter() - t))
    out.update(ms=float(np.median(times)), rounds=int(rounds),
               global_relabels=int(g.mincut_relabels()), flow=flow,
               cut_f64=value(seg), source_side=int((seg == 0).sum()))
    if args.duplex and not args.no_one_layer:  # the one-layer cut of the same gradient, same graph
        g.mincut(tr1, rc)
        times = []
        for _ in range(args.reps):
            t = time.perf_counter()
            _, _, r1 = g.mincut(tr1, rc)
            times.append(1e3 * (time.perf_counter() - t))
        one = {"ms": float(np.median(times)), "rounds": int(r1),
               "global_relabels": int(g.mincut_relabels())}
        out["one_layer"] = one
        if one["rounds"] and out["rounds"]:
            out["ms_per_round_ratio"] = round((out["ms"] / out["rounds"]) /
                                              (one["ms"] / one["rounds"]), 3)
    g.close()
    if bk is not None:
        line = bk.communicate()[0].strip().splitlines()
        if bk.returncode == 0 and line:
            out.update(json.loads(line[-1]))
            bseg = np.load(path + "_seg.npy")
            out.update(segments_equal=bool(np.array_equal(seg, bseg)),
                       differing=int((seg != bseg).sum()),
                       bk_cut_f64=value(bseg))
        else:
            out["bk_error"] = bk.returncode
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
