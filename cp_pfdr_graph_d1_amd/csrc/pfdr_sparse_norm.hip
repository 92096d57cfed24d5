// Lipschitz information of a sparse observation operator A (N-by-V, CSC):
//   pfdr_operator_norm_csc_*   ||A||^2 by the reference's power method on
//       A^tA (src/operator_norm_matrix.cpp:170-206), never densified and
//       never symmetrised;
//   pfdr_lipschitz_diag_csc_*  the diagonal majorant L[v] = sum_i |A_iv| r_i,
//       r_i = sum_j |A_ij| (A^tA <= diag(L) by Cauchy-Schwarz), and the scalar
//       bound ||A||_1 ||A||_inf.
// The checked copy of the CSC and its CSR view are a DevCsc
// (pfdr_spmat.hpp); the stopping rule and the starting values are the
// dense entry's (pfdr_power.hpp).
//
// Power method: all starts of a batch of B = 16, 32 or 64 iterate at once, as
// operator_norm_device does in its direct branch, but the iterated blocks are
// row-major, X[r][c] = coordinate r of start c: a gathered row or column index
// then fetches B contiguous reals (64 bytes at B = 16 in f32) where the dense
// code's column-major block would touch B separate lines.  One iteration is
//   X /= b                                   k_spn_scale
//   T = A X    over the CSR view (N x B)     k_spn_apply
//   Y = A^t T  over the CSC      (V x B)     k_spn_apply
//   a = column norms of Y                    k_spn_colsum, twice
//   the stopping rule on (a, b)              power_step
// k_spn_apply gives a group of B lanes to a row (or column): the group reads
// B entries of the value and index streams at once, coalesced, hands them
// round by shuffles, and lane c adds val * in[idx][c] for start c -- every
// (row, start) sum in ascending stored order in the real type, so a start's
// trajectory depends neither on B nor on the starts that share its batch.
// The norms add fixed row sets in a fixed order (below) for the same reason.
// No floating-point atomics anywhere: two calls give the same bytes.
//
// A row or column of any length is one group's sequential loop (8 gathers in
// flight): a single row of 20,000 entries costs about a millisecond per
// iteration, which is the price of the fixed order; there is no split path.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <stdexcept>
#include <vector>

#include "pfdr_power.hpp"
#include "pfdr_spmat.hpp"

namespace pfdr {

namespace {

constexpr int kNormLanes = 16;    // row lanes of a norm block
constexpr long kNormRows = 1024;  // rows of a first-stage norm block

// X[r][cl] = the dense entry's starting value r + c V of start c = c0 + cl
template <typename real>
__global__ __launch_bounds__(256) void k_spn_init(long V, int B, int c0, real *__restrict__ X) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V * B) return;
    const unsigned long long r = (unsigned long long)(i / B), c = (unsigned long long)(c0 + i % B);
    X[i] = (real)power_start_value(r + c * (unsigned long long)V);
}

// X[r][c] /= b[c] (the reference's normalisation, a division)
template <typename real>
__global__ __launch_bounds__(256) void k_spn_scale(long n, int B, real *__restrict__ X,
                                                   const real *__restrict__ b) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * B) return;
    X[i] /= b[i & (B - 1)];
}

// out[r][c] = sum of val[e] * in[idx[e]][c] over e = ptr[r] .. ptr[r + 1] - 1,
// ascending, each product formed and then added (-ffp-contract=off).  Lanes
// r B .. r B + B - 1 serve segment r (B divides the wave, so the lanes of a
// group leave, loop and shuffle together); U gathers in flight ahead of the adds.
template <typename real, int B>
__global__ __launch_bounds__(256) void k_spn_apply(long nout, const int64_t *__restrict__ ptr,
                                                   const int *__restrict__ idx,
                                                   const real *__restrict__ val,
                                                   const real *__restrict__ in,
                                                   real *__restrict__ out) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long r = t / B;
    const int c = (int)(t & (B - 1));
    if (r >= nout) return;
    constexpr int U = 8;
    const int64_t e1 = ptr[r + 1];
    real acc = real(0);
    for (int64_t e = ptr[r]; e < e1; e += B) {
        const int m = (int)std::min<int64_t>(B, e1 - e);
        real v = real(0);
        int j = 0;
        if (c < m) {
            v = val[e + c];
            j = idx[e + c];
        }
        for (int q0 = 0; q0 < m; q0 += U) {
            real vv[U], x[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                vv[u] = __shfl(v, q0 + u, B);
                const int jj = __shfl(j, q0 + u, B);
                x[u] = q0 + u < m ? in[(long)jj * B + c] : real(0);
            }
#pragma unroll
            for (int u = 0; u < U; u++)
                if (q0 + u < m) acc += vv[u] * x[u];
        }
    }
    out[r * B + c] = acc;
}

// One stage of the column sums of X (n x B, row-major), blockDim = (B,
// kNormLanes): block k takes the rows k per .. k per + per - 1; thread (c, j)
// adds the squares (SQ) or the values of column c over the block's rows j, j +
// 16, ... ascending; thread (c, 0) adds the 16 partial sums j = 0 .. 15 in
// order and writes out[k][c] (its square root with ROOT).  Which rows meet in
// which partial sum depends on n alone, not on B.
template <typename real, bool SQ, bool ROOT>
__global__ __launch_bounds__(1024) void k_spn_colsum(long n, long per, int B,
                                                     const real *__restrict__ X,
                                                     real *__restrict__ out) {
    __shared__ real part[kNormLanes][64];
    const int c = threadIdx.x, j = threadIdx.y;
    const long r0 = (long)blockIdx.x * per, r1 = std::min(n, r0 + per);
    real s = real(0);
    for (long r = r0 + j; r < r1; r += kNormLanes) {
        const real x = X[r * B + c];
        s += SQ ? x * x : x;
    }
    part[j][c] = s;
    __syncthreads();
    if (j == 0) {
        real t = part[0][c];
        for (int q = 1; q < kNormLanes; q++) t += part[q][c];
        out[(long)blockIdx.x * B + c] = ROOT ? std::sqrt(t) : t;
    }
}

// max over the wave of a non-negative double, then one integer atomic max on
// its bit pattern (monotone for non-negative values)
__device__ __forceinline__ void wave_max_to(double v, unsigned long long *out) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, (unsigned long long)__double_as_longlong(v));
}

// r[i] = sum_j |A_ij| over row i's stored entries, columns ascending, in
// double; mx[1] = max_i r[i]
template <typename real>
__global__ __launch_bounds__(256) void k_spn_rowabs(int N, const int64_t *__restrict__ rowptr,
                                                    const real *__restrict__ rval,
                                                    double *__restrict__ r,
                                                    unsigned long long *__restrict__ mx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double s = 0.0;
    if (i < N) {
        const int64_t e1 = rowptr[i + 1];
        for (int64_t e = rowptr[i]; e < e1; e++) s += std::fabs((double)rval[e]);
        r[i] = s;
    }
    wave_max_to(s, mx + 1);
}

// L[v] = sum_i |A_iv| r_i over column v's stored entries, rows ascending, in
// double and rounded once; mx[0] = max_v sum_i |A_iv|
template <typename real>
__global__ __launch_bounds__(256) void k_spn_coldiag(int V, const int64_t *__restrict__ colptr,
                                                     const int *__restrict__ rowidx,
                                                     const real *__restrict__ val,
                                                     const double *__restrict__ r,
                                                     real *__restrict__ L,
                                                     unsigned long long *__restrict__ mx) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    double s = 0.0, l = 0.0;
    if (v < V) {
        const int64_t e1 = colptr[v + 1];
        for (int64_t e = colptr[v]; e < e1; e++) {
            const double a = std::fabs((double)val[e]);
            s += a;
            l += a * r[rowidx[e]];
        }
        L[v] = (real)l;
    }
    wave_max_to(s, mx);
}

template <typename real>
void apply(int B, long nout, const int64_t *ptr, const int *idx, const real *val, const real *in,
           real *out, hipStream_t s) {
    const int g = grid_for(nout * B);
    if (B == 16) k_spn_apply<real, 16><<<g, kBlock, 0, s>>>(nout, ptr, idx, val, in, out);
    else if (B == 32) k_spn_apply<real, 32><<<g, kBlock, 0, s>>>(nout, ptr, idx, val, in, out);
    else k_spn_apply<real, 64><<<g, kBlock, 0, s>>>(nout, ptr, idx, val, in, out);
    PFDR_HIP(hipGetLastError());
}

// nrm[c] = the norm of column c of X (n x B): the fixed two-stage tree
template <typename real>
void col_norms(long n, int B, const real *X, real *part, real *nrm, hipStream_t s) {
    const long nb = (n + kNormRows - 1) / kNormRows;
    const dim3 blk(B, kNormLanes);
    k_spn_colsum<real, true, false><<<(int)nb, blk, 0, s>>>(n, kNormRows, B, X, part);
    k_spn_colsum<real, false, true><<<1, blk, 0, s>>>(nb, nb, B, part, nrm);
    PFDR_HIP(hipGetLastError());
}

// the offence of the scalar arguments shared by both entries, or nullptr
const char *csc_entry_args(int N, int V, const pfdr_csc *A, int mem) {
    if (N <= 0) return "a sparse A needs N > 0";
    if (V <= 0) return "a sparse A needs V > 0";
    if (mem != PFDR_MEM_HOST && mem != PFDR_MEM_DEVICE)
        return "mem must be PFDR_MEM_HOST or PFDR_MEM_DEVICE";
    return cp_csc_args(A);
}

// the checked copy of a caller's CSC with its CSR view
template <typename real>
void intake(DevCsc<real> &m, int N, int V, const pfdr_csc *A, int mem, hipStream_t s) {
    HostPins pins(s);
    m.take(N, V, A, mem, s, pins);
    m.build_csr(s);
    pins.release();
}

}  // namespace

// pfdr_spmat.hpp: the entries' power method, also cut pursuit's on its
// sparse reduced operator
template <typename real>
real operator_norm_sparse(const DevCsc<real> &A, real nTol, int itMax, int nbInit, int verbose,
                          hipStream_t s) {
    const long V = A.V, N = A.N;
    const int starts = std::max(nbInit, 1);
    const int B = starts <= 16 ? 16 : starts <= 32 ? 32 : 64;
    if (verbose) {
        printf("compute sparse operator norm on %d initializations... ", starts);
        fflush(stdout);
    }
    real best = real(0);
    for (int done = 0; done < starts; done += B) {
        DevBuf<real> X((size_t)V * B), Y((size_t)V * B), T((size_t)N * B), a(B), b(B);
        DevBuf<real> part((size_t)((V + kNormRows - 1) / kNormRows) * B);
        DevBuf<int> state(B), running(1);
        PFDR_HIP(hipMemsetAsync(state.p, 0, B * sizeof(int), s));
        k_spn_init<real><<<grid_for(V * B), kBlock, 0, s>>>(V, B, done, X.p);
        auto scale = [&]() {
            k_spn_scale<real><<<grid_for(V * B), kBlock, 0, s>>>(V, B, X.p, b.p);
        };
        auto step = [&]() {  // Y = A^t (A X)
            apply<real>(B, N, A.rowptr.p, A.colidx.p, A.rval.p, X.p, T.p, s);
            apply<real>(B, V, A.colptr.p, A.rowidx.p, A.val.p, T.p, Y.p, s);
        };
        // b = ||X||; X /= b; X = A^tA X; b = ||X|| (ref :193-196)
        col_norms<real>(V, B, X.p, part.p, b.p, s);
        scale();
        step();
        col_norms<real>(V, B, Y.p, part.p, b.p, s);
        std::swap(X.p, Y.p);
        PinnedSmall pin(s);  // returned on every exit path
        int *hrun = static_cast<int *>(pin.p);
        for (int it = 0; it < itMax; it++) {
            scale();
            step();
            col_norms<real>(V, B, Y.p, part.p, a.p, s);
            PFDR_HIP(hipMemsetAsync(running.p, 0, sizeof(int), s));
            power_step<real>(B, a.p, b.p, state.p, nTol, running.p, s);
            std::swap(X.p, Y.p);
            PFDR_HIP(hipMemcpyAsync(hrun, running.p, sizeof(int), hipMemcpyDeviceToHost, s));
            PFDR_HIP(hipStreamSynchronize(s));
            if (*hrun == 0) break;
        }
        std::vector<real> hb(B);
        PFDR_HIP(hipMemcpyAsync(hb.data(), b.p, B * sizeof(real), hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
        const int use = std::min(B, starts - done);
        for (int c = 0; c < use; c++)
            if (hb[c] > best) best = hb[c];  // NaN never wins (ref :208)
    }
    if (verbose) { printf("done.\n"); fflush(stdout); }
    return best;
}
template float operator_norm_sparse<float>(const DevCsc<float> &, float, int, int, int,
                                           hipStream_t);
template double operator_norm_sparse<double>(const DevCsc<double> &, double, int, int, int,
                                             hipStream_t);

namespace {

template <typename real>
int opnorm_csc_host(const char *fn, int N, int V, const pfdr_csc *A, int mem, real nTol, int itMax,
                    int nbInit, int verbose, real *norm2, double *ms) {
    if (const char *bad = csc_entry_args(N, V, A, mem)) return report_error(fn, bad);
    if (!norm2) return report_error(fn, "norm2 is NULL");
    // (a negative itMax runs no iteration after the first product, as in the
    // dense entry)
    try {
        hipStream_t s = lib_stream();
        DevCsc<real> m;
        intake(m, N, V, A, mem, s);
        const auto t0 = std::chrono::steady_clock::now();
        *norm2 = operator_norm_sparse<real>(m, nTol, itMax, nbInit, verbose, s);
        if (ms) {
            ms[0] = m.csr_ms;
            ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                        .count();
        }
    } catch (const HipError &h) {
        return report_error(fn, h);
    } catch (const std::exception &ex) {
        return report_error(fn, ex.what());
    }
    return PFDR_OK;
}

template <typename real>
int lipschitz_csc_host(const char *fn, int N, int V, const pfdr_csc *A, int mem, real *L,
                       real *bound) {
    if (const char *bad = csc_entry_args(N, V, A, mem)) return report_error(fn, bad);
    if (!L) return report_error(fn, "L is NULL");
    try {
        hipStream_t s = lib_stream();
        DevCsc<real> m;
        intake(m, N, V, A, mem, s);
        DevBuf<double> r(N);
        DevBuf<real> buf;
        DevBuf<unsigned long long> mx(2);
        real *dL = L;
        if (mem != PFDR_MEM_DEVICE) {
            buf.alloc(V);
            dL = buf.p;
        }
        PFDR_HIP(hipMemsetAsync(mx.p, 0, 2 * sizeof(unsigned long long), s));
        k_spn_rowabs<real><<<grid_for(N), kBlock, 0, s>>>(N, m.rowptr.p, m.rval.p, r.p, mx.p);
        k_spn_coldiag<real><<<grid_for(V), kBlock, 0, s>>>(V, m.colptr.p, m.rowidx.p, m.val.p,
                                                          r.p, dL, mx.p);
        PFDR_HIP(hipGetLastError());
        double h[2] = {0.0, 0.0};  // bit patterns of non-negative doubles
        PFDR_HIP(hipMemcpyAsync(h, mx.p, sizeof h, hipMemcpyDeviceToHost, s));
        if (mem != PFDR_MEM_DEVICE)
            PFDR_HIP(hipMemcpyAsync(L, dL, (size_t)V * sizeof(real), hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
        if (bound) *bound = (real)(h[0] * h[1]);
    } catch (const HipError &h) {
        return report_error(fn, h);
    } catch (const std::exception &ex) {
        return report_error(fn, ex.what());
    }
    return PFDR_OK;
}

}  // namespace

}  // namespace pfdr

extern "C" int pfdr_operator_norm_csc_f32(int N, int V, const pfdr_csc *A, int mem, float nTol,
                                          int itMax, int nbInit, int verbose, float *norm2,
                                          double *ms) {
    return pfdr::opnorm_csc_host<float>("pfdr_operator_norm_csc_f32", N, V, A, mem, nTol, itMax,
                                        nbInit, verbose, norm2, ms);
}
extern "C" int pfdr_operator_norm_csc_f64(int N, int V, const pfdr_csc *A, int mem, double nTol,
                                          int itMax, int nbInit, int verbose, double *norm2,
                                          double *ms) {
    return pfdr::opnorm_csc_host<double>("pfdr_operator_norm_csc_f64", N, V, A, mem, nTol, itMax,
                                         nbInit, verbose, norm2, ms);
}
extern "C" int pfdr_lipschitz_diag_csc_f32(int N, int V, const pfdr_csc *A, int mem, float *L,
                                           float *bound) {
    return pfdr::lipschitz_csc_host<float>("pfdr_lipschitz_diag_csc_f32", N, V, A, mem, L, bound);
}
extern "C" int pfdr_lipschitz_diag_csc_f64(int N, int V, const pfdr_csc *A, int mem, double *L,
                                           double *bound) {
    return pfdr::lipschitz_csc_host<double>("pfdr_lipschitz_diag_csc_f64", N, V, A, mem, L, bound);
}
