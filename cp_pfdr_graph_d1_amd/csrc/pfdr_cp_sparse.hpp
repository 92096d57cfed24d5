// Sparse observation operator of the cut-pursuit drivers: A (N-by-V) in CSC,
// resident on the device, with the three places where cut pursuit touches
// the full-size A (pfdr_cp_sparse.hip owns the kernels):
//   colsum    the component column sums rA (N-by-rV, dense) of pfdr_cp_reduce
//             and of the drivers' initialize() (one component, Vc = identity)
//   reduced   the same sums kept sparse: rA as a CSC with its CSR view
//             (CpReduced), for the direct branch of pfdr_cp_reduce and, with
//             rAA = rA^t rA and rY = rA^t Y over its entries (gram, dot), for
//             the premultiplied one
//   gradient  DfS = -A^t R, the base of pfdr_cpgraph_gradient for N > 0
//   take      the copy and the structural checks of a caller's pfdr_csc
//             (DevCsc, pfdr_spmat.hpp)
// Every sum adds the stored entries only, from +0, in the order the dense
// loops add the whole column or row -- the argument of pfdr_sparse.hpp: the
// skipped terms are +-0 -- so they give the dense kernels' bytes on the
// densified matrix.  Downstream of a dense rA and of DfS runs the dense code;
// downstream of a CpReduced run its own column norms, scaling and residual,
// which skip +-0 terms in the same way.
#pragma once
#include "pfdr_spmat.hpp"

namespace pfdr {

// The reduced operator rA (N-by-rV) on the device: a CSC (columns =
// components, rows strictly ascending inside a column) and its CSR view (the
// columns of a row ascending), both filled by CpCsc::reduced; ecol is kept.
// A pair (n, rv) is stored iff A stores some entry A[n, v] with v in
// component rv, whatever the sum comes to.
template <typename real>
struct CpReduced {
    DevCsc<real> m;  // V = rV, nnz = rnnz

    // l[rv] = sqrt of the squares of column rv's values added in ascending row
    // order from +0 (k_cp_colnorm's order).  Returns the first rv whose l is 0
    // or not finite, or -1.
    long colnorm(real *l, hipStream_t s) const;
    // every value /= (mul: *=) l[its column], in both views
    void scale(const real *l, int mul, hipStream_t s);
    // R[n] = Y[n] - (sum of rval * rX[colidx] over row n's entries, rv
    // ascending, from +0): k_cpq_residual's bytes on the densified rA
    void residual(const real *rX, const real *Y, real *R, hipStream_t s) const;
    // Upper triangle rAA[rv + rV ru], rv <= ru (device, rV^2; the rest is left
    // alone): the products over the rows stored in both columns, rows
    // ascending, each formed and then added from +0; +0 where there is none.
    // k_cp_gram_seq's bytes on the densified rA, at every size (the dense
    // entry goes to the matrix cores above 2^34 products and agrees with this
    // one to that Gram's tolerance only there: this is the one in the
    // reference's order).  No atomics; no scratch beyond a window of LDS,
    // whose rows PFDR_CP_GRAM_WINDOW overrides (read at every call).
    void gram(real *rAA, hipStream_t s) const;
    // rY[rv] = the sum of val * Y[row] over column rv's entries, rows
    // ascending, from +0: k_cp_rY_dot's bytes
    void dot(const real *Y, real *rY, hipStream_t s) const;
    pfdr_csc csc() const { return pfdr_csc{m.nnz, m.colptr.p, m.rowidx.p, m.val.p}; }
};

template <typename real>
struct CpCsc {
    DevCsc<real> m;  // the checked copy and its ecol; no CSR view of A is built

    // Copies A in (host or device per mem) and checks it on the device: throws
    // std::runtime_error naming the offence.
    void take(int N, int V, const pfdr_csc *A, int mem, hipStream_t s) {
        HostPins pins(s);
        m.take(N, V, A, mem, s, pins);
        pins.release();
        m.word.release();  // (a session's later check keeps it; nothing here reads it again)
    }
    // rA[n + N rv] = the stored entries A[n, Vc[i]], i = rVc[rv] ... rVc[rv + 1] - 1
    // ascending, added from +0; 0 where there is none.  Device arrays; rVc =
    // nullptr: one component, Vc = nullptr: the identity.  The scratch (a sort
    // of nnz pairs) is allocated by the first call and kept.
    void colsum(int rV, const int *rVc, const int *Vc, real *rA, hipStream_t s);
    // The same sums as a CpReduced: the heads of the (row, component) runs, in
    // the sorted order, are its CSR; a stable sort of them by component gives
    // its CSC.  Every value is its run's sequential sum, the byte pattern of
    // colsum's element.  Synchronises once (rnnz comes back); scratch as colsum.
    void reduced(int rV, const int *rVc, const int *Vc, CpReduced<real> &out, hipStream_t s);
    // DfS[v] = -(sum of val[e] R[rowidx[e]] over column v's entries in stored order)
    void gradient(const real *R, real *DfS, hipStream_t s) const;

  private:
    // entries sorted by row, stably, from the Vc-order numbering: ko = rows,
    // sc = components, sv = values
    void sort_entries(int rV, const int *rVc, const int *Vc, hipStream_t s);
    DevBuf<int64_t> off, sums;  // the entries before position i of Vc
    DevBuf<int> cv, sc;         // component of a vertex / of a sorted entry
    DevBuf<real> sv;            // value of a sorted entry
    DevBuf<unsigned> ki, ko, vi, vo;
    DevBuf<int64_t> pos, psums;  // reduced(): the run heads before sorted entry p
    DevBuf<unsigned> hrow;       // reduced(): the row of head h
};

// pfdr_cp_reduce_* (pfdr_cp.hip) with the column sums taken from A; every
// other array on the device.
template <typename real>
int cp_reduce_sparse(CpCsc<real> &A, const real *Y, int rV, const int *rVc, const int *Vc,
                     int preAt, real *rA, real *rAA, real *rY, real *L);

// The direct branch (preAt = 0) of pfdr_cp_reduce_* on the stored entries
// (pfdr_cp.hip): rA as a CpReduced, l = its column norms (device, rV), and
// L = l (l c) (device, rV) with c the squared norm of rA with every column
// divided by its l, by the CSC power method of pfdr_operator_norm_csc_*; the
// values go through the reference's divide-then-multiply round trip.  Returns
// -1, or the first column whose l is 0 or not finite: rA is then as summed
// and L is not written (a sparse session refuses such a column).
template <typename real>
long cp_reduce_sparse_direct(CpCsc<real> &A, int rV, const int *rVc, const int *Vc, real normTol,
                             int normItMax, int normNbInit, CpReduced<real> &rA, real *l, real *L,
                             hipStream_t s);

// The premultiplied branch (preAt = 1, N > 0) of pfdr_cp_reduce_* on the stored
// entries (pfdr_cp.hip): rA as a CpReduced (not scaled, as the dense branch
// leaves its rA), rAA = rA^t rA (device, rV^2, mirrored) and rY = rA^t Y by
// CpReduced::gram and ::dot, then the dense branch's own launches on rAA: l =
// the roots of its diagonal (device, rV), the equilibration round trip around
// operator_norm_device, and L = l (l c) (device, rV, or nullptr).  Every output
// has the dense branch's bytes while its Gram is the sequential one (see
// CpReduced::gram).  Synchronises.
template <typename real>
void cp_reduce_sparse_normal(CpCsc<real> &A, const real *Y, int rV, const int *rVc, const int *Vc,
                             real normTol, int normItMax, int normNbInit, CpReduced<real> &rA,
                             real *rAA, real *rY, real *l, real *L, hipStream_t s);

// pfdr_cpgraph_gradient (pfdr_cpgraph.hip) for N > 0 with the base taken from
// A, a CpCsc of the graph's real type; R on the device, DfS stays there.
int cpgraph_gradient_sparse(pfdr_cpgraph *g, const void *A, const void *R);

}  // namespace pfdr
