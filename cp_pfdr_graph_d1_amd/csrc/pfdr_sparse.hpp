// Sparse observation operator of the quadratic PFDR solvers: A (N-by-V) in
// CSC, the sparse twin of the reference's column-major layout, and the CSR
// view of it built at setup.  A session touches A in four products only --
// the diagonal of A^tA (ref src/PFDR_graph_quadratic_d1_l1.cpp:102-110), the
// per-coordinate pseudo-inverse (:126-134), the residual R = Y - A X
// (:356-367) and the gradient / forward step -A^t R (:432-440, :462-464) --
// each a column dot (over the CSC) or a row product (over the CSR) closed by
// col_epilogue's epilogues.
//
// Two kernel families:
//   k_spc_seq / k_spr_seq   one lane per column / row adds the stored
//       entries' products in ascending index order in `real`.  The
//       reference's dense loops add A[i] * w[i] term by term from +0; a term
//       with A[i] = 0 and finite w[i] is +-0, and adding +-0 never changes a
//       running sum that started at +0 (an exact cancellation gives +0 too,
//       round to nearest), so these kernels produce the bytes of the
//       reference's loops on the densified matrix while the iterates are
//       finite.
//   k_spc_dot / k_spr_rows  a segment of G lanes (4 ... 64) per column / row,
//       each lane striding over the entries, products and partial sums in
//       double (dacc), a shuffle reduction inside the segment.
// The value and index streams are read coalesced (consecutive lanes of a
// segment read consecutive entries); w, R and xp are gathered.
//
// Templates and inlines only, on top of pfdr_quadratic_kernels.hpp's gates and
// epilogues (so for pfdr_quadratic.hip); the matrix, its content check and
// its CSR build are DevCsc's (pfdr_spmat.hpp), which any unit may include.
#pragma once
#include <string>

#include "pfdr_quadratic_kernels.hpp"
#include "pfdr_spmat.hpp"

namespace pfdr {

template <typename real>
struct SpArgs {
    const int64_t *ptr;  // colptr (column dots) / rowptr (row products)
    const int *idx;      // rowidx / colidx
    const real *val;
    ColArgs<real> c;     // ncols segments; A and len unused
};

// a column of squared norm 0: the reference divides by it (ref :96, :133)
template <typename real>
__global__ void k_sp_norm_check(int V, const real *__restrict__ diag,
                                unsigned *__restrict__ word) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V && diag[v] == real(0)) atomicOr(word, 1u);
}

// ------------------------------------------------ sequential-order kernels --
// One lane per column: acc += val[e] * w[rowidx[e]] for the column's entries
// in stored (ascending row) order; each product is formed, then added
// (-ffp-contract=off).  U entries' loads in flight ahead of the adds.
template <typename real, int EPI>
__global__ __launch_bounds__(256) void k_spc_seq(SpArgs<real> a) {
    if (gated(a.c.ctrl, a.c.gate)) return;
    const long col = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= a.c.ncols) return;
    int64_t e = a.ptr[col];
    const int64_t e1 = a.ptr[col + 1];
    const real *w = a.c.w;
    constexpr int U = 4;
    real acc = real(0);
    for (; e + U <= e1; e += U) {
        real x[U], y[U];
#pragma unroll
        for (int q = 0; q < U; q++) {
            x[q] = a.val[e + q];
            y[q] = (EPI == EPI_SELF) ? x[q] : w[a.idx[e + q]];
        }
#pragma unroll
        for (int q = 0; q < U; q++) acc += x[q] * y[q];
    }
    for (; e < e1; e++) {
        const real x = a.val[e];
        acc += x * ((EPI == EPI_SELF) ? x : w[a.idx[e]]);
    }
    col_epilogue<real, EPI>(a.c, col, acc);
}

// R[n] = Y[n] - sum of rval[e] * X[colidx[e]] over row n's entries, columns
// ascending (ref :356-367 order), one lane per row
template <typename real>
__global__ __launch_bounds__(256) void k_spr_seq(int N, const int64_t *__restrict__ rowptr,
                                                 const int *__restrict__ colidx,
                                                 const real *__restrict__ rval,
                                                 const R2<real> *__restrict__ xp,
                                                 const real *__restrict__ Y,
                                                 real *__restrict__ R, const Ctrl<real> *ctrl,
                                                 int gate) {
    if (gated(ctrl, gate)) return;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int64_t e = rowptr[n];
    const int64_t e1 = rowptr[n + 1];
    constexpr int U = 4;
    real acc = real(0);
    for (; e + U <= e1; e += U) {
        real c[U], x[U];
#pragma unroll
        for (int q = 0; q < U; q++) {
            c[q] = rval[e + q];
            x[q] = xp[colidx[e + q]].x;
        }
#pragma unroll
        for (int q = 0; q < U; q++) acc += c[q] * x[q];
    }
    for (; e < e1; e++) acc += rval[e] * xp[colidx[e]].x;
    R[n] = Y[n] - acc;
}

// -------------------------------------------------------- parallel kernels --
// sum over the G lanes of a segment (G a power of two <= 64), in every lane
template <int G>
__device__ __forceinline__ double seg_sum(double v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}

// A segment of G lanes per column: lane sl takes entries sl, sl + G, ... of
// the column; products and sums in double (as k_col_dot); lane 0 of the
// segment applies the epilogue.  A wave returns as a whole or not at all, so
// every lane reaches the shuffles.
template <typename real, int EPI, int G>
__global__ __launch_bounds__(256) void k_spc_dot(SpArgs<real> a) {
    if (gated(a.c.ctrl, a.c.gate)) return;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if ((t - (t & (kWave - 1))) / G >= a.c.ncols) return;  // the whole wave is past the last column
    const long col = t / G;
    const int sl = (int)(t & (G - 1));
    const bool live = col < a.c.ncols;
    int64_t e = 0, e1 = 0;
    if (live) { e = a.ptr[col] + sl; e1 = a.ptr[col + 1]; }
    const real *w = a.c.w;
    double acc = 0.0;
    for (; e < e1; e += G) {
        const real x = a.val[e];
        const real y = (EPI == EPI_SELF) ? x : w[a.idx[e]];
        acc = dacc<real>(acc, x, y);
    }
    acc = seg_sum<G>(acc);
    if (live && sl == 0) col_epilogue<real, EPI>(a.c, col, (real)acc);
}

// R[n] = Y[n] - (A X)[n], a segment of G lanes per row, in double and rounded
// once (as k_rows_finish)
template <typename real, int G>
__global__ __launch_bounds__(256) void k_spr_rows(int N, const int64_t *__restrict__ rowptr,
                                                  const int *__restrict__ colidx,
                                                  const real *__restrict__ rval,
                                                  const R2<real> *__restrict__ xp,
                                                  const real *__restrict__ Y,
                                                  real *__restrict__ R, const Ctrl<real> *ctrl,
                                                  int gate) {
    if (gated(ctrl, gate)) return;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if ((t - (t & (kWave - 1))) / G >= N) return;  // the whole wave is past the last row
    const long n = t / G;
    const int sl = (int)(t & (G - 1));
    const bool live = n < N;
    int64_t e = 0, e1 = 0;
    if (live) { e = rowptr[n] + sl; e1 = rowptr[n + 1]; }
    double acc = 0.0;
    for (; e < e1; e += G) acc = dacc<real>(acc, rval[e], xp[colidx[e]].x);
    acc = seg_sum<G>(acc);
    if (live && sl == 0) R[n] = (real)((double)Y[n] - acc);
}

// ------------------------------------------------------------ host side --
// segment width for a mean of `mean` entries: the smallest G of 4 ... 64 with
// mean <= 1.5 G (a segment then strides at most twice on the average, and at
// G = 64 as often as it takes)
inline int sp_segment(double mean) {
    int g = 4;
    while (g < 64 && mean > 1.5 * g) g *= 2;
    return g;
}

// PFDR_SPARSE_EXACT: 1 sequential-order kernels, 0 parallel, unset / auto
inline int sp_exact_env() {
    const char *e = getenv("PFDR_SPARSE_EXACT");
    if (!e || !*e) return -1;
    const std::string v(e);
    if (v == "auto") return -1;
    if (v == "1") return 1;
    if (v == "0") return 0;
    throw std::runtime_error("PFDR_SPARSE_EXACT must be 1, 0 or auto");
}

// A session's operator: the matrix (pfdr_spmat.hpp) and the kernel family
// that walks it.
template <typename real>
struct SparseOp {
    DevCsc<real> m;
    bool exact = false;  // sequential-order kernels
    int gc = 4, gr = 4;  // lanes per column / row of the parallel kernels

    size_t bytes() const {
        return (m.colptr.n + m.rowptr.n) * 8 + (m.rowidx.n + m.colidx.n) * 4 +
               (m.val.n + m.rval.n) * sizeof(real);
    }

    // copy the CSC in, check it, build the CSR view, choose the kernels
    void setup(int V, int N, const pfdr_csc *A, int mem, long exact_chain, hipStream_t s,
               HostPins &pins) {
        m.take(N, V, A, mem, s, pins);
        m.build_csr(s);
        const int forced = sp_exact_env();
        exact = forced < 0 ? (m.maxcol <= exact_chain && m.maxrow <= exact_chain) : forced == 1;
        gc = sp_segment((double)m.nnz / V);
        gr = sp_segment((double)m.nnz / N);
    }

    template <int EPI, int G>
    void cols_g(const SpArgs<real> &a, hipStream_t s) {
        k_spc_dot<real, EPI, G><<<grid_for((long)m.V * G), kBlock, 0, s>>>(a);
    }

    // column dots with epilogue EPI (ca.ncols = V; ca.A and ca.len unused)
    template <int EPI>
    void cols(const ColArgs<real> &ca, hipStream_t s) {
        SpArgs<real> a{m.colptr.p, m.rowidx.p, m.val.p, ca};
        a.c.A = nullptr;
        a.c.ncols = m.V;
        if (exact) {
            k_spc_seq<real, EPI><<<grid_for(m.V), kBlock, 0, s>>>(a);
        } else {
            switch (gc) {
            case 4: cols_g<EPI, 4>(a, s); break;
            case 8: cols_g<EPI, 8>(a, s); break;
            case 16: cols_g<EPI, 16>(a, s); break;
            case 32: cols_g<EPI, 32>(a, s); break;
            default: cols_g<EPI, 64>(a, s); break;
            }
        }
        PFDR_HIP(hipGetLastError());
    }

    template <int G>
    void rows_g(const R2<real> *xp, const real *Y, real *R, const Ctrl<real> *c, int gate,
                hipStream_t s) {
        k_spr_rows<real, G><<<grid_for((long)m.N * G), kBlock, 0, s>>>(
            m.N, m.rowptr.p, m.colidx.p, m.rval.p, xp, Y, R, c, gate);
    }

    // R = Y - A X
    void rows(const R2<real> *xp, const real *Y, real *R, const Ctrl<real> *c, int gate,
              hipStream_t s) {
        if (exact) {
            k_spr_seq<real><<<grid_for(m.N), kBlock, 0, s>>>(m.N, m.rowptr.p, m.colidx.p, m.rval.p,
                                                            xp, Y, R, c, gate);
        } else {
            switch (gr) {
            case 4: rows_g<4>(xp, Y, R, c, gate, s); break;
            case 8: rows_g<8>(xp, Y, R, c, gate, s); break;
            case 16: rows_g<16>(xp, Y, R, c, gate, s); break;
            case 32: rows_g<32>(xp, Y, R, c, gate, s); break;
            default: rows_g<64>(xp, Y, R, c, gate, s); break;
            }
        }
        PFDR_HIP(hipGetLastError());
    }

    // the CSR view into host arrays (debug read-back)
    void read_csr(int64_t *rp, int32_t *ci, void *rv, hipStream_t s) const {
        const auto k = hipMemcpyDeviceToHost;
        if (rp) PFDR_HIP(hipMemcpyAsync(rp, m.rowptr.p, ((size_t)m.N + 1) * 8, k, s));
        if (ci) PFDR_HIP(hipMemcpyAsync(ci, m.colidx.p, (size_t)m.nnz * 4, k, s));
        if (rv) PFDR_HIP(hipMemcpyAsync(rv, m.rval.p, (size_t)m.nnz * sizeof(real), k, s));
        PFDR_HIP(hipStreamSynchronize(s));
    }
};

}  // namespace pfdr
