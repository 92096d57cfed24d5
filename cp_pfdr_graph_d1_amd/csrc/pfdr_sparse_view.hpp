// The checked device copy of a caller's CSC with its CSR view, for
// translation units other than pfdr_quadratic.hip.  SparseOp::setup
// (pfdr_sparse.hpp) owns the copy, the one-pass content check (k_sp_check)
// and the CSR build (stable radix sort by row); its non-template kernels can
// be compiled into one translation unit only, so the others reach it through
// sparse_view, instantiated in pfdr_quadratic.hip for float and double.
#pragma once
#include <memory>

#include "pfdr_dev.hpp"

namespace pfdr {

// Device arrays of A (N-by-V): columns colptr / rowidx / val as the caller
// stored them, rows rowptr / colidx / rval with every row's columns ascending.
template <typename real>
struct SparseView {
    int N = 0, V = 0;
    int64_t nnz = 0;
    const int64_t *colptr = nullptr, *rowptr = nullptr;
    const int *rowidx = nullptr, *colidx = nullptr;
    const real *val = nullptr, *rval = nullptr;
    int maxcol = 0, maxrow = 0;  // the longest column / row
    double csr_ms = 0.0;         // wall time of the CSR build (sort included)
};

// Copies A in (host or device arrays per mem), checks it and builds the CSR
// view on stream s; throws std::runtime_error naming the offence of a
// malformed colptr or rowidx (sp_throw's words).  The arrays of `out` live as
// long as the returned owner.  A's pointers and nnz are the caller's to have
// checked (cp_csc_args).
template <typename real>
std::shared_ptr<void> sparse_view(int N, int V, const pfdr_csc *A, int mem, hipStream_t s,
                                  SparseView<real> &out);

// ||A||^2 by the power method of pfdr_operator_norm_csc_* (pfdr_sparse_norm.hip)
// on a view whose arrays are already on the device; it reads N, V and the six
// arrays only.  nbInit starts, the best one returned.
template <typename real>
real operator_norm_sparse(const SparseView<real> &A, real nTol, int itMax, int nbInit, int verbose,
                          hipStream_t s);

}  // namespace pfdr
