"""Measure the sparse operator norm (pfdr_operator_norm_csc_*) and what its
result is worth to a PFDR solve, on one GPU.

The operator, on V = S x S unknowns (a 4-neighbour grid graph for the prior):
  blur    the 3x3 normalised blur, N = V, up to 9 entries per row and column;
  random  N = V / 4 rows (--rows), 8 entries per column (--per-col) at one
          random row in each of 8 equal row bands, values uniform in [-1, 1).

It prints one JSON line with
  csr_build_ms          the CSR build of the standalone entry, beside
  session_csr_build_ms  "sparse_csr_us" of a session on the same matrix;
  ms_per_power_iter     from two calls that never stop early (nTol = -1) at
                        --iters and 3 x --iters iterations, batch B = 16;
  bytes_per_iter        what the kernels of one iteration must read or write:
                        the value and index streams and the offsets of both
                        views once, and the block vectors -- X read and
                        written by the scaling, X gathered and T written by
                        A X, T gathered and Y written by A^t T, Y read by the
                        norms: (5 V + 2 N) B reals;
  fraction_of_peak      bytes_per_iter / ms_per_power_iter against 8 TB/s;
  L_bound / _power / _diag_max and it_bound / _power / _diag: the three
                        choices of PFDR_quadratic_l1(lipschitz=...) and the
                        PFDR iterations each takes to difTol = 1e-4;
  with --dense (sizes whose dense matrix fits): dense_ms and dense_norm2 of
  pfdr_operator_norm_* on the densified matrix at the same settings, beside
  sparse_ms and sparse_norm2.

    python tools/bench_sparse_opnorm.py --shape 2048 2048 [--op blur|random]
        [--dtype f32|f64] [--rows N] [--per-col K] [--iters 20] [--dense] [--no-pfdr]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_csc(N, V, per_col, dt, pfdr):
    """per_col entries per column, one in each of per_col equal row bands"""
    rng = np.random.default_rng(5)
    band = N // per_col
    if band < 1:
        raise SystemExit("--rows must be at least --per-col")
    rows = rng.integers(0, band, (V, per_col)) + band * np.arange(per_col)
    val = 2.0 * rng.random((V, per_col)) - 1.0
    colptr = per_col * np.arange(V + 1, dtype=np.int64)
    return pfdr.CSC(colptr, rows.ravel().astype(np.int32), val.ravel().astype(dt), N)


def matvec(csc, x):
    cols = np.repeat(np.arange(csc.V), np.diff(csc.colptr))
    return np.bincount(csc.rowidx, csc.val.astype(np.float64) * x[cols], csc.N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, default=[2048, 2048])
    ap.add_argument("--op", choices=["blur", "random"], default="blur")
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--rows", type=int, default=0, help="random: N (default V / 4)")
    ap.add_argument("--per-col", type=int, default=8, help="random: entries per column")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--no-pfdr", action="store_true")
    args = ap.parse_args()
    from cp_pfdr_graph_d1_amd import pfdr
    from cp_pfdr_graph_d1_amd.graphs import blur3x3_csc
    dt = np.float32 if args.dtype == "f32" else np.float64
    nx, ny = args.shape
    V = nx * ny
    if args.op == "blur":
        colptr, rowidx, val = blur3x3_csc(nx, ny)
        csc = pfdr.CSC(colptr, rowidx, val.astype(dt), V)
    else:
        csc = random_csc(args.rows or V // 4, V, args.per_col, dt, pfdr)
    N, B, esz = csc.N, 16, np.dtype(dt).itemsize
    out = dict(op=args.op, shape=[nx, ny], dtype=args.dtype, N=N, V=V, nnz=csc.nnz, batch=B)
    dev = csc.to_device()

    # time per power iteration: two runs that never stop early
    pfdr.operator_norm(dev, nTol=-1.0, itMax=2, nbInit=10)  # first launches discarded
    k1, k2 = args.iters, 3 * args.iters
    t1 = pfdr.operator_norm(dev, nTol=-1.0, itMax=k1, nbInit=10)[1]
    t2 = pfdr.operator_norm(dev, nTol=-1.0, itMax=k2, nbInit=10)[1]
    ms = (t2 - t1) / (k2 - k1)
    stream = 2 * csc.nnz * (esz + 4) + (V + 1 + N + 1) * 8 + (5 * V + 2 * N) * B * esz
    out.update(ms_per_power_iter=ms, bytes_per_iter=int(stream),
               fraction_of_peak=stream / (ms * 1e-3) / 8e12)

    # the CSR build, standalone and in a session
    lib = pfdr.load()
    import ctypes as C
    ct, sfx, _ = pfdr._real(dt)
    st, res, two = dev.struct(), ct(0), (C.c_double * 2)()
    for _ in range(2):  # the second call's
        pfdr._check(getattr(lib, "pfdr_operator_norm_csc_" + sfx)(
            N, V, C.byref(st), pfdr.PFDR_MEM_DEVICE, ct(1e-3), 0, 1, 0, C.byref(res), two),
            "pfdr_operator_norm_csc")
    out["csr_build_ms"] = two[0]

    # the three choices of L
    t0 = time.perf_counter()
    Lp, pms = pfdr.operator_norm(dev)
    out.update(L_power=float(Lp), power_ms=pms, power_call_ms=(time.perf_counter() - t0) * 1e3)
    Ld, Lb = pfdr.lipschitz_diag(dev)
    out.update(L_bound=float(Lb), L_diag_max=float(Ld.max()), L_diag_mean=float(Ld.mean()))

    if args.dense:
        import torch
        A = torch.from_numpy(np.ascontiguousarray(csc.to_dense().T)).cuda()  # column-major N x V
        kw = dict(nTol=1e-6, itMax=100, nbInit=10)
        pfdr.operator_norm(A, device=True, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dn = pfdr.operator_norm(A, device=True, **kw)[0]
        out.update(dense_ms=(time.perf_counter() - t0) * 1e3, dense_norm2=float(dn))
        del A
        pfdr.operator_norm(dev, **kw)
        t0 = time.perf_counter()
        sn = pfdr.operator_norm(dev, **kw)[0]
        out.update(sparse_ms=(time.perf_counter() - t0) * 1e3, sparse_norm2=float(sn))

    if not args.no_pfdr:
        Eu, Ev = pfdr.gen_grid_edges((nx, ny), 4)
        Eu, Ev = Eu.astype(np.int32), Ev.astype(np.int32)
        x0 = np.where((np.arange(V) // nx) < ny // 3, 1.0, -0.5)
        rng = np.random.default_rng(7)
        Y = (matvec(csc, x0) + 0.2 * (rng.random(N) - 0.5)).astype(dt)
        s = pfdr.Session(pfdr.PFDR_KIND_L1, dt, V, Eu.size, Eu, Ev, np.full(Eu.size, 0.1, dt),
                         np.zeros(V, dt), Y, N=N, A=csc, La_l1=np.full(V, 0.01, dt),
                         Ltype=pfdr.SCAL, L=np.array([Lb], dt), itMax=8)
        out["session_csr_build_ms"] = s.query("sparse_csr_us") / 1e3
        s.close()
        for choice in ("bound", "power", "diag"):
            t0 = time.perf_counter()
            x, it = pfdr.PFDR_quadratic_l1(Y, Eu, Ev, 0.1, csc, 0.01, lipschitz=choice)
            out["it_" + choice] = int(it)
            out["solve_ms_" + choice] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
