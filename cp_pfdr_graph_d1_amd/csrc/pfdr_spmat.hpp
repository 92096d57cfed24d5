// A sparse matrix A (N-by-V) on the device: the CSC a caller hands in as a
// pfdr_csc, copied and checked, and the CSR view of it.  One type for the
// three holders of such a matrix -- a sparse session (SparseOp,
// pfdr_sparse.hpp), the standalone norm entries (pfdr_sparse_norm.hip) and
// cut pursuit (CpCsc, CpReduced, pfdr_cp_sparse.hpp); pfdr_spmat.hip owns the
// kernels.
#pragma once
#include "pfdr_dev.hpp"

namespace pfdr {

// The checks of a pfdr_csc that need no device (NULL arrays, nnz): the
// offence, or nullptr.
const char *cp_csc_args(const pfdr_csc *A);

// ptr[q] = the first of the n ascending ids that is >= q, q = 0 .. m (n >= 1):
// the offsets of a CSR from its sorted rows, of a CSC from its sorted columns
// (build_csr writes its own with the same code inside its fill pass)
void sorted_offsets(int64_t n, long m, const unsigned *id, int64_t *ptr, hipStream_t s);

template <typename real>
struct DevCsc {
    int N = 0, V = 0;
    int64_t nnz = 0;
    DevBuf<int64_t> colptr;  // V + 1
    DevBuf<int> rowidx;      // rows strictly ascending inside a column
    DevBuf<real> val;
    DevBuf<int> ecol;        // the column of entry e (take; build_csr consumes it)
    DevBuf<int64_t> rowptr;  // N + 1: the CSR view, every row's columns ascending
    DevBuf<int> colidx;
    DevBuf<real> rval;
    int maxcol = 0, maxrow = 0;  // the longest column / row (build_csr)
    double csr_ms = 0.0;         // wall time of build_csr (sort included)
    DevBuf<unsigned> word;       // the content check's flags: 0 once take has returned

    // Copies A in (host arrays through pins, which the caller releases, or
    // device arrays, per mem), checks colptr and rowidx in one pass that also
    // fills ecol, and throws std::runtime_error naming the first offence.  A's
    // pointers and nnz are the caller's to have checked (cp_csc_args).  One
    // host synchronisation.
    void take(int N_, int V_, const pfdr_csc *A, int mem, hipStream_t s, HostPins &pins);
    // rowptr / colidx / rval by a stable radix sort of the entries by row,
    // maxcol, maxrow and csr_ms; ecol is freed.  One host synchronisation.
    void build_csr(hipStream_t s);
    // the flag word, read back (synchronises)
    unsigned verdict(hipStream_t s) const;
};

// ||A||^2 by the power method of pfdr_operator_norm_csc_* (pfdr_sparse_norm.hip)
// on a matrix with its CSR view in place; it reads N, V and the six arrays
// only.  nbInit starts, the best one returned.
template <typename real>
real operator_norm_sparse(const DevCsc<real> &A, real nTol, int itMax, int nbInit, int verbose,
                          hipStream_t s);

}  // namespace pfdr
