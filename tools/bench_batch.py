#!/usr/bin/env python
"""Per-iteration time of a batch of B dense-A channels (pfdr.BatchSession)
against B runs of one reusable scalar session (pfdr.Session, reloaded for each
channel), on the dense flagship shapes:

  c3      direct mode, N = 1,024 x V = 2M on a 2000 x 1000 4-NN grid (the shape
          of ``bench.py --workload c3``), A 8.2 GB in f32
  c3_ata  premultiplied, V = 32,768 on a 256 x 128 grid (tools/workloads.py)

    python tools/bench_batch.py --workload c3 --B 1 2 4 8 [--dtype f32|f64]
                                [--iters K] [--lib-path OTHER/libpfdr_mi355x.so]

Both sides run the same protocol, difTol = 0 (nothing tracked: every channel
runs every iteration): reload to X = 0, a warm-up run of K iterations, then
one timed run of K iterations closed by a device synchronise (run() returns
after it).  Five repeats, the median reported, the five values kept.  The
scalar side's time is the sum over the B channels.  With --lib-path the
scalar side runs in a child process that loads that build (PFDR_LIB_PATH), so
a parent commit's library can be the yardstick.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

REPS = 5
AMP = [1.0, 0.05, 4.0, 0.0]


def inputs(workload, dt, Bmax):
    """device tensors: the shared problem and Bmax observations"""
    import torch
    from cp_pfdr_graph_d1_amd import pfdr
    tdt = torch.float32 if dt == np.float32 else torch.float64
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    if workload == "c3":
        N, nx, ny = 1024, 2000, 1000
        V = nx * ny
        h = (3.0 / N) ** 0.5
        A = torch.from_numpy(pfdr.gen_uniform(3, N * V, -h, h, dt)).cuda()  # column major
        op = A.view(V, N).t()  # N x V
        n, ln = N, N
        L = np.array([(1.0 + (V / N) ** 0.5) ** 2], dt)
    else:
        N, nx, ny = 1024, 256, 128
        V = nx * ny
        At = ((torch.rand((V, N), generator=g, device="cuda", dtype=tdt) - 0.5) * (12.0 / N) ** 0.5)
        A, _ = pfdr.gram(At, which=0, device=True)  # V x V, exactly symmetric
        op = A.view(V, V)
        n, ln = -V, V
        n2, _ = pfdr.operator_norm(At, nTol=1e-3, itMax=100, nbInit=10, device=True)
        L = np.array([n2], dt)
        A = A.reshape(-1)
    x0 = torch.zeros(V, device="cuda", dtype=tdt)
    x0[: V // 3] = 1.0
    x0[V // 3: 2 * V // 3] = -0.5
    Y = torch.stack([torch.mv(op, x0 * (1 + b) + AMP[b % 4] * torch.randn(
        V, generator=g, device="cuda", dtype=tdt)) for b in range(Bmax)]).contiguous()
    Eu, Ev = pfdr.gen_grid_edges((nx, ny), 4)
    E = Eu.size
    dev = lambda a, t=tdt: torch.as_tensor(np.ascontiguousarray(a), dtype=t, device="cuda")
    torch.cuda.synchronize()
    return dict(kind=pfdr.PFDR_KIND_L1, dtype=dt, V=V, E=E, Eu=dev(Eu, torch.int32),
                Ev=dev(Ev, torch.int32), La_d1=torch.full((E,), 0.05, device="cuda", dtype=tdt),
                La_l1=torch.full((V,), 0.005, device="cuda", dtype=tdt), N=n, A=A, L=dev(L),
                Ltype=pfdr.SCAL, rho=1.5, condMin=1e-3, difRcd=0.0, difTol=0.0, device=True), Y, ln


def timed(run, K):
    t0 = time.perf_counter()
    run(K)  # (returns after a stream synchronise)
    return (time.perf_counter() - t0) * 1e3 / K


def scalar_side(P, Y, Bs, K):
    """{B: REPS values of sum_b T_scalar(channel b), ms per iteration}"""
    import torch
    from cp_pfdr_graph_d1_amd import pfdr
    V = P["V"]
    X0 = torch.zeros(V, device="cuda", dtype=Y.dtype)
    s = pfdr.Session(X0=X0, Y=Y[0], itMax=2 * K, reusable=True, **P)
    out = {}
    try:
        for B in Bs:
            reps = []
            for _ in range(REPS):
                tot = 0.0
                for b in range(B):
                    s.reload(Y=Y[b], X0=X0)
                    s.run(K)
                    tot += timed(s.run, K)
                reps.append(tot)
            out[B] = reps
        out["graphs"] = s.query("graphs")
    finally:
        s.close()
    return out


def batch_side(P, Y, Bs, K):
    import torch
    from cp_pfdr_graph_d1_amd import pfdr
    out = {}
    for B in Bs:
        X0 = torch.zeros((B, P["V"]), device="cuda", dtype=Y.dtype)
        Yb = Y[:B].contiguous()
        s = pfdr.BatchSession(X0=X0, Y=Yb, B=B, itMax=2 * K, **P)
        try:
            reps = []
            for _ in range(REPS):
                s.reload(Y=Yb, X0=X0)
                s.run(K)
                reps.append(timed(s.run, K))
            out[B] = reps
            out["channel_group"] = s.query("channel_group")
            out["symv"] = s.query("symv")
        finally:
            s.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--workload", choices=("c3", "c3_ata"), required=True)
    ap.add_argument("--B", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--dtype", choices=("f32", "f64"), default="f32")
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--lib-path", default=None,
                    help="the scalar side from this build (a child process, PFDR_LIB_PATH)")
    ap.add_argument("--scalar-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    dt = np.float32 if a.dtype == "f32" else np.float64
    K = max(a.iters, 1)
    scalar = None
    if a.lib_path and not a.scalar_only:
        # (before this process opens the GPU: one process on it at a time)
        env = dict(os.environ, PFDR_LIB_PATH=os.path.abspath(a.lib_path))
        cmd = [sys.executable, os.path.abspath(__file__), "--workload", a.workload, "--dtype",
               a.dtype, "--iters", str(K), "--scalar-only", "--B"] + [str(b) for b in a.B]
        r = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True)
        scalar = {(int(k) if k.isdigit() else k): v
                  for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items()}
    P, Y, _ = inputs(a.workload, dt, max(a.B))
    if a.scalar_only:
        print(json.dumps(scalar_side(P, Y, a.B, K)))
        return
    batch = batch_side(P, Y, a.B, K)
    if scalar is None:
        scalar = scalar_side(P, Y, a.B, K)
    rows = []
    for B in a.B:
        tb, ts = statistics.median(batch[B]), statistics.median(scalar[B])
        rows.append({"B": B, "T_batch_ms": round(tb, 4), "B_T_scalar_ms": round(ts, 4),
                     "ratio": round(tb / ts, 4),
                     "batch_reps_ms": [round(x, 4) for x in batch[B]],
                     "scalar_reps_ms": [round(x, 4) for x in scalar[B]],
                     "batch_spread": round((max(batch[B]) - min(batch[B])) / tb, 4),
                     "scalar_spread": round((max(scalar[B]) - min(scalar[B])) / ts, 4)})
    print(json.dumps({"workload": a.workload, "dtype": a.dtype, "iters": K, "repeats": REPS,
                      "channel_group": batch["channel_group"], "symv": batch["symv"],
                      "scalar_graphs": scalar.get("graphs"),
                      "scalar_lib": a.lib_path or "this build", "unit": "ms per iteration",
                      "results": rows}))


if __name__ == "__main__":
    main()
