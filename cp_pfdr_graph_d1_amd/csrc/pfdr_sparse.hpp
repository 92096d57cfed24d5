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
#pragma once
#include <chrono>
#include <string>

#include "pfdr_quadratic_kernels.hpp"
#include "pfdr_sort.hpp"

namespace pfdr {

// content checks of a CSC, folded into one word
enum SpBad : unsigned { SP_BAD_COLPTR = 1u, SP_BAD_ROW = 2u, SP_BAD_ORDER = 4u,
                        SP_BAD_NORM = 8u };

template <typename real>
struct SpArgs {
    const int64_t *ptr;  // colptr (column dots) / rowptr (row products)
    const int *idx;      // rowidx / colidx
    const real *val;
    ColArgs<real> c;     // ncols segments; A and len unused
};

// One pass over colptr (threads 0 .. V) and rowidx (threads 0 .. nnz - 1):
// colptr[0] = 0, colptr[V] = nnz, non-decreasing; every row index in [0, N)
// and above its predecessor in the same column.  ecol[e] = the column of
// entry e (the CSR build's column indices), by a binary search that stays
// inside colptr[0 .. V] whatever it holds.
__global__ __launch_bounds__(256) void k_sp_check(int V, int N, int64_t nnz,
                                                  const int64_t *__restrict__ colptr,
                                                  const int *__restrict__ rowidx,
                                                  int *__restrict__ ecol,
                                                  unsigned *__restrict__ word) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned bad = 0;
    if (t <= V) {
        const int64_t c = colptr[t];
        if (c < 0 || c > nnz) bad |= SP_BAD_COLPTR;
        if (t == 0 && c != 0) bad |= SP_BAD_COLPTR;
        if (t == V && c != nnz) bad |= SP_BAD_COLPTR;
        if (t < V && colptr[t + 1] < c) bad |= SP_BAD_COLPTR;
    }
    if (t < nnz) {
        int lo = 0, hi = V;  // the largest v in [0, V) with colptr[v] <= t
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (colptr[mid] <= t) lo = mid; else hi = mid;
        }
        ecol[t] = lo;
        const int r = rowidx[t];
        if (r < 0 || r >= N) bad |= SP_BAD_ROW;
        if (t > 0 && t > colptr[lo] && rowidx[t - 1] >= r) bad |= SP_BAD_ORDER;
    }
    if (bad) atomicOr(word, bad);
}

// a column of squared norm 0: the reference divides by it (ref :96, :133)
template <typename real>
__global__ void k_sp_norm_check(int V, const real *__restrict__ diag,
                                unsigned *__restrict__ word) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V && diag[v] == real(0)) atomicOr(word, (unsigned)SP_BAD_NORM);
}

__global__ void k_sp_keys(int64_t nnz, const int *__restrict__ rowidx,
                          unsigned *__restrict__ keys, unsigned *__restrict__ vals) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    keys[e] = (unsigned)rowidx[e];
    vals[e] = (unsigned)e;
}

// the CSR arrays from the entries sorted by row (rows[p] = the row of sorted
// position p, perm[p] = its entry): the sort is stable and the entries were
// enumerated in column order, so every row's columns ascend.  rowptr[q] = the
// first position of a row >= q, written by the position that opens it.
template <typename real>
__global__ __launch_bounds__(256) void k_sp_csr_fill(int64_t nnz, int N,
                                                     const unsigned *__restrict__ rows,
                                                     const unsigned *__restrict__ perm,
                                                     const int *__restrict__ ecol,
                                                     const real *__restrict__ val,
                                                     int64_t *__restrict__ rowptr,
                                                     int *__restrict__ colidx,
                                                     real *__restrict__ rval) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const unsigned e = perm[p];
    colidx[p] = ecol[e];
    rval[p] = val[e];
    const long r = (long)rows[p];
    const long prev = p ? (long)rows[p - 1] : -1L;
    for (long q = prev + 1; q <= r; q++) rowptr[q] = p;
    if (p == nnz - 1)
        for (long q = r + 1; q <= N; q++) rowptr[q] = nnz;
}

// the longest segment of an offset array
__global__ void k_sp_maxlen(int n, const int64_t *__restrict__ ptr, int *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    atomicMax(out, (int)(ptr[i + 1] - ptr[i]));
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

// the first offence of a check word, by name
inline void sp_throw(unsigned w) {
    if (w & SP_BAD_COLPTR)
        throw std::runtime_error("sparse A: colptr must be non-decreasing with colptr[0] = 0 "
                                 "and colptr[V] = nnz");
    if (w & SP_BAD_ROW) throw std::runtime_error("sparse A: row index outside [0, N)");
    if (w & SP_BAD_ORDER)
        throw std::runtime_error("sparse A: row indices must be strictly ascending inside "
                                 "each column");
    if (w & SP_BAD_NORM)
        throw std::runtime_error("sparse A: a column has squared norm 0 (the reference "
                                 "divides by it)");
}

template <typename real>
struct SparseOp {
    int V = 0, N = 0;
    int64_t nnz = 0;
    DevBuf<int64_t> colptr, rowptr;
    DevBuf<int> rowidx, colidx;
    DevBuf<real> val, rval;
    DevBuf<unsigned> word;  // the checks' flags
    bool exact = false;     // sequential-order kernels
    int gc = 4, gr = 4;     // lanes per column / row of the parallel kernels
    int maxcol = 0, maxrow = 0;
    double csr_ms = 0.0;    // wall time of the CSR build (sort included)

    size_t bytes() const {
        return (colptr.n + rowptr.n) * 8 + (rowidx.n + colidx.n) * 4 +
               (val.n + rval.n) * sizeof(real);
    }

    unsigned verdict(hipStream_t s) {
        unsigned w = 0;
        PFDR_HIP(hipMemcpyAsync(&w, word.p, sizeof w, hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
        return w;
    }

    // copy the CSC in, check it, build the CSR view, choose the kernels
    void setup(int V_, int N_, const pfdr_csc *A, int mem, long exact_chain, hipStream_t s,
               HostPins &pins) {
        V = V_; N = N_; nnz = A->nnz;
        auto in = [&](void *dst, const void *src, size_t b) {
            if (mem == PFDR_MEM_DEVICE)
                PFDR_HIP(hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToDevice, s));
            else
                pins.copy(dst, src, b, hipMemcpyHostToDevice);
        };
        colptr.alloc((size_t)V + 1);
        rowidx.alloc(nnz);
        val.alloc(nnz);
        in(colptr.p, A->colptr, ((size_t)V + 1) * 8);
        in(rowidx.p, A->rowidx, (size_t)nnz * 4);
        in(val.p, A->val, (size_t)nnz * sizeof(real));
        word.alloc(1);
        PFDR_HIP(hipMemsetAsync(word.p, 0, sizeof(unsigned), s));
        DevBuf<int> ecol(nnz);
        k_sp_check<<<grid_for(std::max<long>((long)V + 1, (long)nnz)), kBlock, 0, s>>>(
            V, N, nnz, colptr.p, rowidx.p, ecol.p, word.p);
        PFDR_HIP(hipGetLastError());
        sp_throw(verdict(s));

        const auto t0 = std::chrono::steady_clock::now();
        rowptr.alloc((size_t)N + 1);
        colidx.alloc(nnz);
        rval.alloc(nnz);
        {
            DevBuf<unsigned> ki(nnz), ko(nnz), vi(nnz), vo(nnz);
            k_sp_keys<<<grid_for(nnz), kBlock, 0, s>>>(nnz, rowidx.p, ki.p, vi.p);
            PFDR_HIP(hipGetLastError());
            int bits = 1;
            while (bits < 32 && (1L << bits) < (long)N) bits++;
            radix_sort_pairs_stable<unsigned>(ki.p, ko.p, vi.p, vo.p, (long)nnz, bits, s);
            k_sp_csr_fill<real><<<grid_for(nnz), kBlock, 0, s>>>(nnz, N, ko.p, vo.p, ecol.p, val.p,
                                                                rowptr.p, colidx.p, rval.p);
            PFDR_HIP(hipGetLastError());
            DevBuf<int> mx(2);
            PFDR_HIP(hipMemsetAsync(mx.p, 0, 2 * sizeof(int), s));
            k_sp_maxlen<<<grid_for(V), kBlock, 0, s>>>(V, colptr.p, mx.p);
            k_sp_maxlen<<<grid_for(N), kBlock, 0, s>>>(N, rowptr.p, mx.p + 1);
            PFDR_HIP(hipGetLastError());
            int h[2] = {0, 0};
            PFDR_HIP(hipMemcpyAsync(h, mx.p, sizeof h, hipMemcpyDeviceToHost, s));
            PFDR_HIP(hipStreamSynchronize(s));
            maxcol = h[0];
            maxrow = h[1];
        }
        csr_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                     .count();
        const int forced = sp_exact_env();
        exact = forced < 0 ? (maxcol <= exact_chain && maxrow <= exact_chain) : forced == 1;
        gc = sp_segment((double)nnz / V);
        gr = sp_segment((double)nnz / N);
    }

    template <int EPI, int G>
    void cols_g(const SpArgs<real> &a, hipStream_t s) {
        k_spc_dot<real, EPI, G><<<grid_for((long)V * G), kBlock, 0, s>>>(a);
    }

    // column dots with epilogue EPI (ca.ncols = V; ca.A and ca.len unused)
    template <int EPI>
    void cols(const ColArgs<real> &ca, hipStream_t s) {
        SpArgs<real> a{colptr.p, rowidx.p, val.p, ca};
        a.c.A = nullptr;
        a.c.ncols = V;
        if (exact) {
            k_spc_seq<real, EPI><<<grid_for(V), kBlock, 0, s>>>(a);
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
        k_spr_rows<real, G><<<grid_for((long)N * G), kBlock, 0, s>>>(N, rowptr.p, colidx.p, rval.p,
                                                                    xp, Y, R, c, gate);
    }

    // R = Y - A X
    void rows(const R2<real> *xp, const real *Y, real *R, const Ctrl<real> *c, int gate,
              hipStream_t s) {
        if (exact) {
            k_spr_seq<real><<<grid_for(N), kBlock, 0, s>>>(N, rowptr.p, colidx.p, rval.p, xp, Y, R,
                                                          c, gate);
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
        if (rp) PFDR_HIP(hipMemcpyAsync(rp, rowptr.p, ((size_t)N + 1) * 8, hipMemcpyDeviceToHost, s));
        if (ci) PFDR_HIP(hipMemcpyAsync(ci, colidx.p, (size_t)nnz * 4, hipMemcpyDeviceToHost, s));
        if (rv) PFDR_HIP(hipMemcpyAsync(rv, rval.p, (size_t)nnz * sizeof(real),
                                        hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
    }
};

}  // namespace pfdr
