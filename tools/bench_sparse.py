"""Measure a sparse-A (CSC) quadratic l1 session on one GPU: a 3x3 normalised
blur in front of a graph-TV prior on an S x S 4-neighbour grid (N = V, up to 9
entries per row and per column), f32, untracked iterations (difTol = difRcd =
0, no Dif / Obj record).

For PFDR_SPARSE_EXACT = 1 (sequential-order kernels) and = 0 (parallel
kernels) it prints: ms per iteration (the first run() discarded), the mean
time of the four products with A -- gemv_rows (R = Y - A X) and gemv_cols
(-A^t R and the forward step) from a profiled run, diag_cols and pinv_cols
from the session's setup --, the wall time of the session's setup (second
creation; the first is discarded) and the CSR build's share of it, and the
bytes the two per-iteration products stream (12 B per entry for an f32 value
and an int32 index, plus the offsets; gathers not counted).  Beside them: the
identity-A session on the same graph, and at --shape 64 64 only the dense
session on the densified matrix.  One JSON line.

    python tools/bench_sparse.py [--shape 1024 1024] [--iters 200] [--dtype f32]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def blur_csc(nx, ny, dt, pfdr):
    """the 3x3 normalised blur as a CSC, without the dense matrix"""
    V = nx * ny
    ids = np.arange(V, dtype=np.int64).reshape(nx, ny)
    rows, cols = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            rows.append(ids[max(0, -dx):nx - max(0, dx), max(0, -dy):ny - max(0, dy)].ravel())
            cols.append(ids[max(0, dx):nx - max(0, -dx), max(0, dy):ny - max(0, -dy)].ravel())
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    val = (1.0 / np.bincount(rows, minlength=V))[rows]
    o = np.lexsort((rows, cols))
    colptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(cols, minlength=V), out=colptr[1:])
    return pfdr.CSC(colptr, rows[o].astype(np.int32), val[o].astype(dt), V)


def timed(make, iters):
    """(ms per iteration, setup ms, session) of the second session make() gives"""
    s = make()
    s.run(8)
    s.close()
    t0 = time.perf_counter()
    s = make()
    s.sync()
    setup = (time.perf_counter() - t0) * 1e3
    s.run(iters)  # discarded: graph capture, first launches
    t0 = time.perf_counter()
    s.run(2 * iters)
    s.sync()
    return (time.perf_counter() - t0) * 1e3 / (2 * iters), setup, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, default=[1024, 1024])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f32")
    args = ap.parse_args()
    from cp_pfdr_graph_d1_amd import pfdr
    from cp_pfdr_graph_d1_amd.graphs import uniform
    dt = np.float32 if args.dtype == "f32" else np.float64
    nx, ny = args.shape
    V = nx * ny
    Eu, Ev = pfdr.gen_grid_edges((nx, ny), 4)
    Eu, Ev = Eu.astype(np.int32), Ev.astype(np.int32)
    csc = blur_csc(nx, ny, dt, pfdr)
    x0 = np.where((np.arange(V) // ny) < nx // 3, 1.0, -0.5)
    Y = (x0 + 0.2 * (uniform(7, np.arange(V, dtype=np.uint64)) - 0.5)).astype(dt)
    La = np.full(Eu.size, 0.1, dt)
    L1 = np.full(V, 0.01, dt)
    iters = args.iters
    common = dict(La_l1=L1, Ltype=pfdr.SCAL, L=np.array([1.0], dt), rho=1.5, condMin=1e-3,
                  difRcd=0.0, difTol=0.0, itMax=8 * iters + 64)

    def session(A, N):
        return pfdr.Session(pfdr.PFDR_KIND_L1, dt, V, Eu.size, Eu, Ev, La, np.zeros(V, dt), Y,
                            N=N, A=A, **common)

    out = dict(shape=[nx, ny], dtype=args.dtype, V=V, E=int(Eu.size), nnz=csc.nnz, iters=iters)
    esz = np.dtype(dt).itemsize + 4
    out["stream_bytes_per_product"] = int(csc.nnz * esz + (V + 1) * 8)
    for exact in ("1", "0"):
        os.environ["PFDR_SPARSE_EXACT"] = exact
        ms, setup, s = timed(lambda: session(csc, V), iters)
        r = dict(ms_per_iter=ms, setup_ms=setup, csr_build_ms=s.query("sparse_csr_us") / 1e3,
                 sparse_exact=s.query("sparse_exact"), seg_col=s.query("sparse_seg_col"),
                 seg_row=s.query("sparse_seg_row"))
        s.profile(True, period=4, only=["gemv_rows", "gemv_cols"])
        s.run(iters)
        for k in ("gemv_rows", "gemv_cols", "diag_cols", "pinv_cols"):
            n, kms = s.kernel_stats(k)
            r[k + "_ms"] = kms
            r[k + "_launches"] = n
        for k in ("gemv_rows", "gemv_cols"):
            if r[k + "_ms"] > 0:
                r[k + "_GBps"] = out["stream_bytes_per_product"] / r[k + "_ms"] / 1e6
        s.close()
        out["exact_" + exact] = r
    os.environ.pop("PFDR_SPARSE_EXACT")
    ms, setup, s = timed(lambda: session(None, 0), iters)
    s.close()
    out["identity"] = dict(ms_per_iter=ms, setup_ms=setup)
    if (nx, ny) == (64, 64):
        A = np.asfortranarray(csc.to_dense()).ravel(order="F")
        ms, setup, s = timed(lambda: session(A, V), iters)
        out["dense"] = dict(ms_per_iter=ms, setup_ms=setup, dense_exact=s.query("dense_exact"))
        s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
