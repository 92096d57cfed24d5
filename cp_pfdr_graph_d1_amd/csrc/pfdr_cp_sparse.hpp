// Sparse observation operator of the cut-pursuit drivers: A (N-by-V) in CSC,
// resident on the device, with the three places where cut pursuit touches
// the full-size A (pfdr_cp_sparse.hip owns the kernels):
//   colsum    the component column sums rA (N-by-rV, dense) of pfdr_cp_reduce
//             and of the drivers' initialize() (one component, Vc = identity)
//   gradient  DfS = -A^t R, the base of pfdr_cpgraph_gradient for N > 0
//   take      the copy and the structural checks of a caller's pfdr_csc
// Both sums add the stored entries only, from +0, in the order the dense
// loops add the whole column or row -- the argument of pfdr_sparse.hpp: the
// skipped terms are +-0 -- so they give the dense kernels' bytes on the
// densified matrix, and everything downstream of rA and DfS is the dense code.
#pragma once
#include "pfdr_dev.hpp"

namespace pfdr {

// The checks of a pfdr_csc that need no device (NULL arrays, nnz): the
// offence, or nullptr.
const char *cp_csc_args(const pfdr_csc *A);

template <typename real>
struct CpCsc {
    int N = 0, V = 0;
    int64_t nnz = 0;
    DevBuf<int64_t> colptr;
    DevBuf<int> rowidx, ecol;  // ecol[e]: the column of entry e
    DevBuf<real> val;

    // Copies A in (host or device per mem) and checks it on the device: throws
    // std::runtime_error naming the offence.
    void take(int N_, int V_, const pfdr_csc *A, int mem, hipStream_t s);
    // rA[n + N rv] = the stored entries A[n, Vc[i]], i = rVc[rv] ... rVc[rv + 1] - 1
    // ascending, added from +0; 0 where there is none.  Device arrays; rVc =
    // nullptr: one component, Vc = nullptr: the identity.  The scratch (a sort
    // of nnz pairs) is allocated by the first call and kept.
    void colsum(int rV, const int *rVc, const int *Vc, real *rA, hipStream_t s);
    // DfS[v] = -(sum of val[e] R[rowidx[e]] over column v's entries in stored order)
    void gradient(const real *R, real *DfS, hipStream_t s) const;

  private:
    DevBuf<int64_t> off, sums;  // the entries before position i of Vc
    DevBuf<int> cv, sc;         // component of a vertex / of a sorted entry
    DevBuf<real> sv;            // value of a sorted entry
    DevBuf<unsigned> ki, ko, vi, vo;
};

// pfdr_cp_reduce_* (pfdr_cp.hip) with the column sums taken from A; every
// other array on the device.
template <typename real>
int cp_reduce_sparse(CpCsc<real> &A, const real *Y, int rV, const int *rVc, const int *Vc,
                     int preAt, real *rA, real *rAA, real *rY, real *L);

// pfdr_cpgraph_gradient (pfdr_cpgraph.hip) for N > 0 with the base taken from
// A, a CpCsc of the graph's real type; R on the device, DfS stays there.
int cpgraph_gradient_sparse(pfdr_cpgraph *g, const void *A, const void *R);

}  // namespace pfdr
