// Cut-pursuit reduced-problem builder: from the
// CP's connected components (rVc offsets into the vertex list Vc, ref
// src/CP_PFDR_graph_quadratic_d1_l1.cpp:571-597) build what CP hands to PFDR
// on every iteration (:663-841):
//   N > 0: rA = component column sums of A; preAt: rAA = rA^t rA, rY = rA^t Y
//   N < 0: rY = component sums of A^tY, rAA = double component sums of A^tA
//   N = 0: rY as above, rAA = component sums of the diagonal (or sizes)
//   L: Jacobi equilibration, squared operator norm of the equilibrated
//      matrix (pfdr_gram.hip's power method), L = l^2 c (:772-839).
// Every sum runs sequentially in the reference's order (one lane per output
// entry, products rounded before the add as with -ffp-contract=off), so rA,
// rAA and rY are bit-identical to the restatement (oracle/cp_reduce_body.h);
// the equilibrate-then-revert round trip is reproduced as the reference
// does it (its revert does not restore every bit).  Only the operator norm
// differs: the reference's starts are time-seeded (:182), ours are fixed.
// Large reduced problems (rV^2 N > 2^34 multiply-adds) compute rAA on the
// matrix cores instead (pfdr_gram.hip; tolerance, not bit-exact).
// A sparse A (N > 0, pfdr_cp_reduce_csc_*) changes the column-sum step only:
// rA comes from the stored entries (pfdr_cp_sparse.hip) with the bytes of
// k_cp_colsum on the densified matrix, and the rest runs on it as it is.
// pfdr_cp_reduce_csc_sparse_* (cp_reduce_sparse_direct) keeps rA sparse
// through the direct branch: column norms, the equilibration round trip, the
// CSC power method and L on the stored entries, the dense steps' bytes but
// for c, which comes from another power method.
// pfdr_cp_reduce_csc_sparse_preAt_* (cp_reduce_sparse_normal) keeps rA sparse
// through the premultiplied branch: rAA and rY over the stored entries
// (CpReduced::gram, ::dot) in the sequential Gram's order, at every size, and
// the rest as above on rAA, so every byte is the dense branch's up to the 2^34
// multiply-adds where that one leaves the reference's order.
#include <cmath>
#include <stdexcept>
#include <string>

#include "pfdr_cp_sparse.hpp"
#include "pfdr_graph.hpp"
#include "pfdr_session.hpp"

namespace pfdr {

template <typename real>
real operator_norm_device(int M, int N, const real *A, real nTol, int itMax, int nbInit,
                          int verbose, hipStream_t s, double *gram_ms);
template <typename real>
void gram(int which, int P, long K, const real *A, long ld, real *G, hipStream_t s);

// rA[n + N rv] = sum over the component's vertices, in list order (:676-687)
template <typename real>
__global__ void k_cp_colsum(int N, int rV, const real *__restrict__ A, const int *__restrict__ rVc,
                            const int *__restrict__ Vc, real *__restrict__ rA) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    for (int rv = blockIdx.y; rv < rV; rv += gridDim.y) {
        real a = real(0);
        int s = rVc[rv];
        const int t = rVc[rv + 1];
        for (; s + 8 <= t; s += 8) {  // 8 column loads in flight, adds in order
            real x[8];
#pragma unroll
            for (int u = 0; u < 8; u++) x[u] = A[(size_t)N * Vc[s + u] + n];
#pragma unroll
            for (int u = 0; u < 8; u++) a += x[u];
        }
        for (; s < t; s++) a += A[(size_t)N * Vc[s] + n];
        rA[(size_t)N * rv + n] = a;
    }
}

// upper triangle rAA[rv + rV ru] (rv <= ru) = sum_n rA[n, rv] rA[n, ru] (:689-702)
template <typename real>
__global__ void k_cp_gram_seq(int N, int rV, const real *__restrict__ rA, real *__restrict__ rAA) {
    const int rv = blockIdx.x * blockDim.x + threadIdx.x;
    if (rv >= rV) return;
    for (int ru = blockIdx.y; ru < rV; ru += gridDim.y) {
        if (rv > ru) continue;
        // the reference's loop: a += rA[i++] * Av[n], i running down column rv
        const real *a = rA + (size_t)N * rv, *b = rA + (size_t)N * ru;
        real s = real(0);
        for (int n = 0; n < N; n++) s += a[n] * b[n];
        rAA[rv + (size_t)rV * ru] = s;
    }
}

// rY[rv] = sum_n rA[n, rv] Y[n] (:704-711)
template <typename real>
__global__ void k_cp_rY_dot(int N, int rV, const real *__restrict__ rA, const real *__restrict__ Y,
                            real *__restrict__ rY) {
    const int rv = blockIdx.x * blockDim.x + threadIdx.x;
    if (rv >= rV) return;
    const real *a = rA + (size_t)N * rv;
    real s = real(0);
    for (int n = 0; n < N; n++) s += a[n] * Y[n];
    rY[rv] = s;
}

// identity (:756-758): rAA[rv] = component size
template <typename real>
__global__ void k_cp_sizes(int rV, const int *__restrict__ rVc, real *__restrict__ rAA) {
    const int rv = blockIdx.x * blockDim.x + threadIdx.x;
    if (rv < rV) rAA[rv] = (real)(rVc[rv + 1] - rVc[rv]);
}

// upper triangle of the double component sums of A^tA (:724-741)
template <typename real>
__global__ void k_cp_ata(int V, int rV, const real *__restrict__ A, const int *__restrict__ rVc,
                         const int *__restrict__ Vc, real *__restrict__ rAA) {
    const int rv = blockIdx.x * blockDim.x + threadIdx.x;
    if (rv >= rV) return;
    for (int ru = blockIdx.y; ru < rV; ru += gridDim.y) {
        if (rv > ru) continue;
        real a = real(0);
        for (int s = rVc[ru], t = rVc[ru + 1]; s < t; s++) {
            const real *Av = A + (size_t)V * Vc[s];
            for (int q = rVc[rv], r = rVc[rv + 1]; q < r; q++) a += Av[Vc[q]];
        }
        rAA[rv + (size_t)rV * ru] = a;
    }
}

// lower triangle from the upper (:761-770)
template <typename real>
__global__ void k_cp_mirror(int rV, real *rAA) {
    const int rv = blockIdx.x * blockDim.x + threadIdx.x;
    if (rv >= rV) return;
    for (int ru = blockIdx.y; ru < rV; ru += gridDim.y)
        if (rv > ru) rAA[rv + (size_t)rV * ru] = rAA[ru + (size_t)rV * rv];
}

// l[rv] = sqrt(rAA[rv, rv]) (:778)
template <typename real>
__global__ void k_cp_diag_sqrt(int rV, const real *__restrict__ rAA, real *__restrict__ l) {
    const int rv = blockIdx.x * blockDim.x + threadIdx.x;
    if (rv < rV) l[rv] = std::sqrt(rAA[(size_t)rv * (rV + 1)]);
}

// l[rv] = ||rA[:, rv]|| summed sequentially (:803-812)
template <typename real>
__global__ void k_cp_colnorm(int N, int rV, const real *__restrict__ rA, real *__restrict__ l) {
    const int rv = blockIdx.x * blockDim.x + threadIdx.x;
    if (rv >= rV) return;
    const real *a = rA + (size_t)N * rv;
    real s = real(0);
    for (int n = 0; n < N; n++) {
        const real b = a[n];
        s += b * b;
    }
    l[rv] = std::sqrt(s);
}

// symmetric: M[rv + rV ru] /= (or *=) l[ru] l[rv] (:779-800)
template <typename real>
__global__ void k_cp_scale_sym(int rV, real *M, const real *__restrict__ l, int mul) {
    const int rv = blockIdx.x * blockDim.x + threadIdx.x;
    if (rv >= rV) return;
    for (int ru = blockIdx.y; ru < rV; ru += gridDim.y) {
        const real a = l[ru];
        real &m = M[rv + (size_t)rV * ru];
        if (mul) m *= (a * l[rv]);
        else m /= (a * l[rv]);
    }
}

// columns: M[n + N rv] /= (or *=) l[rv] (:813-825)
template <typename real>
__global__ void k_cp_scale_cols(int N, int rV, real *M, const real *__restrict__ l, int mul) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    for (int rv = blockIdx.y; rv < rV; rv += gridDim.y) {
        real &m = M[n + (size_t)N * rv];
        if (mul) m *= l[rv];
        else m /= l[rv];
    }
}

// L[rv] = l[rv] (l[rv] c) (:827-839)
template <typename real>
__global__ void k_cp_lipschitz(int rV, const real *__restrict__ l, real c, real *__restrict__ L) {
    const int rv = blockIdx.x * blockDim.x + threadIdx.x;
    if (rv >= rV) return;
    real x = l[rv];
    x *= l[rv] * c;
    L[rv] = x;
}

// the components on the device: the caller's rVc (rV + 1) and Vc (V), or
// copies of its host arrays
struct CpPartition {
    const int *rVc, *Vc;
    DevBuf<int> bptr, bVc;
    CpPartition(int rV, const int *rVc_, int V, const int *Vc_, bool dev, hipStream_t s)
        : rVc(rVc_), Vc(Vc_) {
        if (dev) return;
        upload(bptr, rVc_, (size_t)rV + 1, s);
        upload(bVc, Vc_, (size_t)V, s);
        rVc = bptr.p;
        Vc = bVc.p;
    }
};

// sp: the sparse A of N > 0 (A is then unused), already on the device
template <typename real>
static int cp_reduce_host(const char *fn, int N, int V, const real *A, const real *Y, int rV,
                          const int *rVc, const int *Vc, int preAt, int mem, real normTol,
                          int normItMax, int normNbInit, real *rA, real *rAA, real *rY, real *L,
                          real *Leq, CpCsc<real> *sp = nullptr) {
    if (V <= 0 || rV <= 0 || rV > V || !Y || !rVc || !Vc)
        return report_error(fn, "invalid arguments");
    if (N > 0 && ((!A && !sp) || !rA)) return report_error(fn, "N > 0 needs A and rA");
    if (N < 0 && (!A || -N != V)) return report_error(fn, "N < 0 needs A = A^tA and N = -V");
    if (N <= 0) preAt = 1;  // ref :671
    if (preAt && (!rAA || !rY)) return report_error(fn, "rAA and rY are required for this case");
    // N > 0 without preAt: CP hands PFDR the whole Y and rA (ref :847-859), no rY
    try {
        hipStream_t s = lib_stream();
        const bool dev = mem == PFDR_MEM_DEVICE;
        const auto kin = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        auto in = [&](DevBuf<real> &b, const real *h, size_t n) -> const real * {
            if (dev || !h) return h;
            b.alloc(n);
            PFDR_HIP(hipMemcpyAsync(b.p, h, n * sizeof(real), kin, s));
            return b.p;
        };
        DevBuf<real> bA, bY, brA, brAA, brY, bL, bl;
        const size_t asz = N > 0 ? (size_t)N * V : N < 0 ? (size_t)V * V : (size_t)V;
        const real *dA = in(bA, A, asz);
        const real *dY = in(bY, Y, N > 0 ? (size_t)N : (size_t)V);
        CpPartition part(rV, rVc, V, Vc, dev, s);
        const int *dptr = part.rVc, *dVc = part.Vc;
        auto out = [&](DevBuf<real> &b, real *h, size_t n) -> real * {
            if (dev && h) return h;
            b.alloc(n ? n : 1);
            return b.p;
        };
        const size_t rAAn = N == 0 ? (size_t)rV : (size_t)rV * rV;
        real *drA = N > 0 ? out(brA, rA, (size_t)N * rV) : nullptr;
        real *drAA = preAt ? out(brAA, rAA, rAAn) : nullptr;
        real *drY = preAt ? out(brY, rY, rV) : nullptr;
        bl.alloc(rV);
        real *dl = bl.p;
        const int gy = rV < 65535 ? rV : 65535;  // rows per launch; kernels loop over the rest
        const dim3 b1(kBlock), gV(grid_for(rV));
        const dim3 gVV(grid_for(rV), gy);
        if (N > 0) {
            if (sp) sp->colsum(rV, dptr, dVc, drA, s);
            else k_cp_colsum<real><<<dim3(grid_for(N), gy), b1, 0, s>>>(N, rV, dA, dptr, dVc, drA);
            if (preAt) {
                const double work = (double)rV * rV * N / 2;
                if (work <= 17179869184.0) {
                    k_cp_gram_seq<real><<<gVV, b1, 0, s>>>(N, rV, drA, drAA);
                    k_cp_mirror<real><<<gVV, b1, 0, s>>>(rV, drAA);
                } else {
                    gram<real>(0, rV, N, drA, N, drAA, s);  // matrix cores, mirrored
                }
                k_cp_rY_dot<real><<<gV, b1, 0, s>>>(N, rV, drA, dY, drY);
            }
        } else {
            // rY = component sums of Y (:715-723); N = 0: rAA = component sums
            // of the diagonal (:744-755) or the sizes (:756-758) — each sum in
            // Vc order, giant components by one LDS-staged workgroup
            ordered_segment_sums<real>(rV, dptr, dVc, dY, drY, s);
            if (N == 0 && dA) ordered_segment_sums<real>(rV, dptr, dVc, dA, drAA, s);
            else if (N == 0) k_cp_sizes<real><<<gV, b1, 0, s>>>(rV, dptr, drAA);
            if (N < 0) {
                k_cp_ata<real><<<gVV, b1, 0, s>>>(V, rV, dA, dptr, dVc, drAA);
                k_cp_mirror<real><<<gVV, b1, 0, s>>>(rV, drAA);
            }
        }
        PFDR_HIP(hipGetLastError());
        if (N != 0) {
            real c;
            if (preAt) {  // equilibrate rAA, norm, revert (:776-800)
                k_cp_diag_sqrt<real><<<gV, b1, 0, s>>>(rV, drAA, dl);
                k_cp_scale_sym<real><<<gVV, b1, 0, s>>>(rV, drAA, dl, 0);
                c = operator_norm_device<real>(0, rV, drAA, normTol, normItMax, normNbInit, 0, s,
                                               nullptr);
                k_cp_scale_sym<real><<<gVV, b1, 0, s>>>(rV, drAA, dl, 1);
            } else {  // equilibrate rA (:801-825)
                k_cp_colnorm<real><<<gV, b1, 0, s>>>(N, rV, drA, dl);
                k_cp_scale_cols<real><<<dim3(grid_for(N), gy), b1, 0, s>>>(N, rV, drA, dl, 0);
                c = operator_norm_device<real>(N, rV, drA, normTol, normItMax, normNbInit, 0, s,
                                               nullptr);
                k_cp_scale_cols<real><<<dim3(grid_for(N), gy), b1, 0, s>>>(N, rV, drA, dl, 1);
            }
            if (L) {
                real *dL = out(bL, L, rV);
                k_cp_lipschitz<real><<<gV, b1, 0, s>>>(rV, dl, c, dL);
                if (!dev) PFDR_HIP(hipMemcpyAsync(L, dL, rV * sizeof(real), hipMemcpyDeviceToHost, s));
            }
            if (Leq) PFDR_HIP(hipMemcpyAsync(Leq, dl, rV * sizeof(real),
                                             dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        } else if (L) {
            PFDR_HIP(hipMemcpyAsync(L, drAA, rV * sizeof(real),
                                    dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        }
        PFDR_HIP(hipGetLastError());
        if (!dev) {
            if (drA) PFDR_HIP(hipMemcpyAsync(rA, drA, (size_t)N * rV * sizeof(real), hipMemcpyDeviceToHost, s));
            if (drAA) PFDR_HIP(hipMemcpyAsync(rAA, drAA, rAAn * sizeof(real), hipMemcpyDeviceToHost, s));
            if (drY) PFDR_HIP(hipMemcpyAsync(rY, drY, rV * sizeof(real), hipMemcpyDeviceToHost, s));
        }
        PFDR_HIP(hipStreamSynchronize(s));
    } catch (const HipError &h) {
        return report_error(fn, h);
    } catch (const std::exception &ex) {
        return report_error(fn, ex.what());
    }
    return PFDR_OK;
}

template <typename real>
int cp_reduce_sparse(CpCsc<real> &A, const real *Y, int rV, const int *rVc, const int *Vc,
                     int preAt, real *rA, real *rAA, real *rY, real *L) {
    return cp_reduce_host<real>("pfdr_cp_reduce_csc", A.m.N, A.m.V, nullptr, Y, rV, rVc, Vc, preAt,
                                PFDR_MEM_DEVICE, real(1e-3), 100, 10, rA, rAA, rY, L, nullptr,
                                &A);
}
template int cp_reduce_sparse<float>(CpCsc<float> &, const float *, int, const int *, const int *,
                                     int, float *, float *, float *, float *);
template int cp_reduce_sparse<double>(CpCsc<double> &, const double *, int, const int *,
                                      const int *, int, double *, double *, double *, double *);

// the public entry: the caller's CSC is copied in and checked first
template <typename real>
static int cp_reduce_csc(const char *fn, int N, int V, const pfdr_csc *A, const real *Y, int rV,
                         const int *rVc, const int *Vc, int preAt, int mem, real normTol,
                         int normItMax, int normNbInit, real *rA, real *rAA, real *rY, real *L,
                         real *Leq) {
    if (N <= 0) return report_error(fn, "a sparse A needs N > 0");
    if (V <= 0 || (mem != PFDR_MEM_HOST && mem != PFDR_MEM_DEVICE))
        return report_error(fn, "invalid arguments");
    if (const char *bad = cp_csc_args(A)) return report_error(fn, bad);
    CpCsc<real> sp;
    try {
        sp.take(N, V, A, mem, lib_stream());
    } catch (const HipError &h) {
        return report_error(fn, h);
    } catch (const std::exception &ex) {
        return report_error(fn, ex.what());
    }
    return cp_reduce_host<real>(fn, N, V, nullptr, Y, rV, rVc, Vc, preAt, mem, normTol, normItMax,
                                normNbInit, rA, rAA, rY, L, Leq, &sp);
}

// The direct branch above (:801-839) on the stored entries of a sparse rA:
// every step skips the +-0 terms of the dense one and so gives its bytes.
template <typename real>
long cp_reduce_sparse_direct(CpCsc<real> &A, int rV, const int *rVc, const int *Vc, real normTol,
                             int normItMax, int normNbInit, CpReduced<real> &rA, real *l, real *L,
                             hipStream_t s) {
    A.reduced(rV, rVc, Vc, rA, s);
    const long bad = rA.colnorm(l, s);
    if (bad >= 0) return bad;
    rA.scale(l, 0, s);
    const real c = operator_norm_sparse<real>(rA.m, normTol, normItMax, normNbInit, 0, s);
    rA.scale(l, 1, s);
    k_cp_lipschitz<real><<<grid_for(rV), kBlock, 0, s>>>(rV, l, c, L);
    PFDR_HIP(hipGetLastError());
    PFDR_HIP(hipStreamSynchronize(s));  // as cp_reduce_host: a session need not run on s
    return -1;
}
template long cp_reduce_sparse_direct<float>(CpCsc<float> &, int, const int *, const int *, float,
                                             int, int, CpReduced<float> &, float *, float *,
                                             hipStream_t);
template long cp_reduce_sparse_direct<double>(CpCsc<double> &, int, const int *, const int *,
                                              double, int, int, CpReduced<double> &, double *,
                                              double *, hipStream_t);

// The premultiplied branch above (:689-711, :776-800) with rAA and rY summed
// over the stored entries of a sparse rA; from the mirror on, cp_reduce_host's
// own launches.
template <typename real>
void cp_reduce_sparse_normal(CpCsc<real> &A, const real *Y, int rV, const int *rVc, const int *Vc,
                             real normTol, int normItMax, int normNbInit, CpReduced<real> &rA,
                             real *rAA, real *rY, real *l, real *L, hipStream_t s) {
    A.reduced(rV, rVc, Vc, rA, s);
    const int gy = rV < 65535 ? rV : 65535;
    const dim3 b1(kBlock), gV(grid_for(rV)), gVV(grid_for(rV), gy);
    rA.gram(rAA, s);
    k_cp_mirror<real><<<gVV, b1, 0, s>>>(rV, rAA);
    rA.dot(Y, rY, s);
    k_cp_diag_sqrt<real><<<gV, b1, 0, s>>>(rV, rAA, l);
    k_cp_scale_sym<real><<<gVV, b1, 0, s>>>(rV, rAA, l, 0);
    PFDR_HIP(hipGetLastError());
    const real c = operator_norm_device<real>(0, rV, rAA, normTol, normItMax, normNbInit, 0, s,
                                              nullptr);
    k_cp_scale_sym<real><<<gVV, b1, 0, s>>>(rV, rAA, l, 1);
    if (L) k_cp_lipschitz<real><<<gV, b1, 0, s>>>(rV, l, c, L);
    PFDR_HIP(hipGetLastError());
    PFDR_HIP(hipStreamSynchronize(s));  // as cp_reduce_host: a session need not run on s
}
template void cp_reduce_sparse_normal<float>(CpCsc<float> &, const float *, int, const int *,
                                             const int *, float, int, int, CpReduced<float> &,
                                             float *, float *, float *, float *, hipStream_t);
template void cp_reduce_sparse_normal<double>(CpCsc<double> &, const double *, int, const int *,
                                              const int *, double, int, int, CpReduced<double> &,
                                              double *, double *, double *, double *, hipStream_t);

// the public entry of the premultiplied branch, rA returned as a CSC where asked for
template <typename real>
static int cp_reduce_csc_sparse_preAt(const char *fn, int N, int V, const pfdr_csc *A,
                                      const real *Y, int rV, const int *rVc, const int *Vc,
                                      int mem, real normTol, int normItMax, int normNbInit,
                                      real *rAA, real *rY, real *L, real *Leq, int64_t *rnnz,
                                      int64_t *rcolptr, int32_t *rrowidx, real *rval) {
    if (N <= 0) return report_error(fn, "a sparse A needs N > 0");
    if (V <= 0 || (mem != PFDR_MEM_HOST && mem != PFDR_MEM_DEVICE))
        return report_error(fn, "invalid arguments");
    if (const char *bad = cp_csc_args(A)) return report_error(fn, bad);
    if (rV <= 0 || rV > V || !Y || !rVc || !Vc) return report_error(fn, "invalid arguments");
    if (!rAA || !rY) return report_error(fn, "rAA and rY are required");
    const int outs = (rnnz != nullptr) + (rcolptr != nullptr) + (rrowidx != nullptr) +
                     (rval != nullptr);
    if (outs != 0 && outs != 4)
        return report_error(fn, "rnnz, rcolptr, rrowidx and rval must be all set or all NULL");
    try {
        hipStream_t s = lib_stream();
        const bool dev = mem == PFDR_MEM_DEVICE;
        CpCsc<real> sp;
        sp.take(N, V, A, mem, s);
        CpPartition part(rV, rVc, V, Vc, dev, s);
        DevBuf<real> bY, brAA, brY, l(rV), dL(rV);
        const real *dY = Y;
        real *drAA = rAA, *drY = rY;
        if (!dev) {
            upload(bY, Y, (size_t)N, s);
            brAA.alloc((size_t)rV * rV);
            brY.alloc(rV);
            dY = bY.p, drAA = brAA.p, drY = brY.p;
        }
        CpReduced<real> r;
        cp_reduce_sparse_normal<real>(sp, dY, rV, part.rVc, part.Vc, normTol, normItMax,
                                      normNbInit, r, drAA, drY, l.p, dL.p, s);
        const auto k = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (!dev) {
            PFDR_HIP(hipMemcpyAsync(rAA, drAA, (size_t)rV * rV * sizeof(real), k, s));
            PFDR_HIP(hipMemcpyAsync(rY, drY, rV * sizeof(real), k, s));
        }
        if (rnnz) {
            *rnnz = r.m.nnz;
            PFDR_HIP(hipMemcpyAsync(rcolptr, r.m.colptr.p, ((size_t)rV + 1) * 8, k, s));
            PFDR_HIP(hipMemcpyAsync(rrowidx, r.m.rowidx.p, (size_t)r.m.nnz * 4, k, s));
            PFDR_HIP(hipMemcpyAsync(rval, r.m.val.p, (size_t)r.m.nnz * sizeof(real), k, s));
        }
        if (L) PFDR_HIP(hipMemcpyAsync(L, dL.p, rV * sizeof(real), k, s));
        if (Leq) PFDR_HIP(hipMemcpyAsync(Leq, l.p, rV * sizeof(real), k, s));
        PFDR_HIP(hipStreamSynchronize(s));
    } catch (const HipError &h) {
        return report_error(fn, h);
    } catch (const std::exception &ex) {
        return report_error(fn, ex.what());
    }
    return PFDR_OK;
}

// the public entry of the direct branch with rA returned as a CSC
template <typename real>
static int cp_reduce_csc_sparse(const char *fn, int N, int V, const pfdr_csc *A, const real *Y,
                                int rV, const int *rVc, const int *Vc, int mem, real normTol,
                                int normItMax, int normNbInit, int64_t *rnnz, int64_t *rcolptr,
                                int32_t *rrowidx, real *rval, real *L, real *Leq) {
    if (N <= 0) return report_error(fn, "a sparse A needs N > 0");
    if (V <= 0 || (mem != PFDR_MEM_HOST && mem != PFDR_MEM_DEVICE))
        return report_error(fn, "invalid arguments");
    if (const char *bad = cp_csc_args(A)) return report_error(fn, bad);
    if (rV <= 0 || rV > V || !Y || !rVc || !Vc) return report_error(fn, "invalid arguments");
    if (!rnnz || !rcolptr || !rrowidx || !rval)
        return report_error(fn, "rnnz, rcolptr, rrowidx and rval are required");
    try {
        hipStream_t s = lib_stream();
        const bool dev = mem == PFDR_MEM_DEVICE;
        CpCsc<real> sp;
        sp.take(N, V, A, mem, s);
        CpPartition part(rV, rVc, V, Vc, dev, s);
        const int *dptr = part.rVc, *dVc = part.Vc;
        CpReduced<real> r;
        DevBuf<real> l(rV), dL(rV);
        const long bad = cp_reduce_sparse_direct<real>(sp, rV, dptr, dVc, normTol, normItMax,
                                                       normNbInit, r, l.p, dL.p, s);
        if (bad >= 0) {
            const std::string msg = "reduced column " + std::to_string(bad) +
                                    " has norm 0 (or not finite): a sparse reduced operator "
                                    "needs every column's norm positive";
            return report_error(fn, msg.c_str());
        }
        const auto k = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        *rnnz = r.m.nnz;
        PFDR_HIP(hipMemcpyAsync(rcolptr, r.m.colptr.p, ((size_t)rV + 1) * 8, k, s));
        PFDR_HIP(hipMemcpyAsync(rrowidx, r.m.rowidx.p, (size_t)r.m.nnz * 4, k, s));
        PFDR_HIP(hipMemcpyAsync(rval, r.m.val.p, (size_t)r.m.nnz * sizeof(real), k, s));
        if (L) PFDR_HIP(hipMemcpyAsync(L, dL.p, rV * sizeof(real), k, s));
        if (Leq) PFDR_HIP(hipMemcpyAsync(Leq, l.p, rV * sizeof(real), k, s));
        PFDR_HIP(hipStreamSynchronize(s));
    } catch (const HipError &h) {
        return report_error(fn, h);
    } catch (const std::exception &ex) {
        return report_error(fn, ex.what());
    }
    return PFDR_OK;
}

}  // namespace pfdr

extern "C" int pfdr_cp_reduce_csc_sparse_f32(int N, int V, const pfdr_csc *A, const float *Y,
                                             int rV, const int *rVc, const int *Vc, int mem,
                                             float normTol, int normItMax, int normNbInit,
                                             int64_t *rnnz, int64_t *rcolptr, int32_t *rrowidx,
                                             float *rval, float *L, float *Leq) {
    return pfdr::cp_reduce_csc_sparse<float>("pfdr_cp_reduce_csc_sparse_f32", N, V, A, Y, rV, rVc,
                                             Vc, mem, normTol, normItMax, normNbInit, rnnz,
                                             rcolptr, rrowidx, rval, L, Leq);
}
extern "C" int pfdr_cp_reduce_csc_sparse_f64(int N, int V, const pfdr_csc *A, const double *Y,
                                             int rV, const int *rVc, const int *Vc, int mem,
                                             double normTol, int normItMax, int normNbInit,
                                             int64_t *rnnz, int64_t *rcolptr, int32_t *rrowidx,
                                             double *rval, double *L, double *Leq) {
    return pfdr::cp_reduce_csc_sparse<double>("pfdr_cp_reduce_csc_sparse_f64", N, V, A, Y, rV,
                                              rVc, Vc, mem, normTol, normItMax, normNbInit, rnnz,
                                              rcolptr, rrowidx, rval, L, Leq);
}

extern "C" int pfdr_cp_reduce_csc_sparse_preAt_f32(
    int N, int V, const pfdr_csc *A, const float *Y, int rV, const int *rVc, const int *Vc, int mem,
    float normTol, int normItMax, int normNbInit, float *rAA, float *rY, float *L, float *Leq,
    int64_t *rnnz, int64_t *rcolptr, int32_t *rrowidx, float *rval) {
    return pfdr::cp_reduce_csc_sparse_preAt<float>(
        "pfdr_cp_reduce_csc_sparse_preAt_f32", N, V, A, Y, rV, rVc, Vc, mem, normTol, normItMax,
        normNbInit, rAA, rY, L, Leq, rnnz, rcolptr, rrowidx, rval);
}
extern "C" int pfdr_cp_reduce_csc_sparse_preAt_f64(
    int N, int V, const pfdr_csc *A, const double *Y, int rV, const int *rVc, const int *Vc,
    int mem, double normTol, int normItMax, int normNbInit, double *rAA, double *rY, double *L,
    double *Leq, int64_t *rnnz, int64_t *rcolptr, int32_t *rrowidx, double *rval) {
    return pfdr::cp_reduce_csc_sparse_preAt<double>(
        "pfdr_cp_reduce_csc_sparse_preAt_f64", N, V, A, Y, rV, rVc, Vc, mem, normTol, normItMax,
        normNbInit, rAA, rY, L, Leq, rnnz, rcolptr, rrowidx, rval);
}

extern "C" int pfdr_cp_reduce_csc_f32(int N, int V, const pfdr_csc *A, const float *Y, int rV,
                                      const int *rVc, const int *Vc, int preAt, int mem,
                                      float normTol, int normItMax, int normNbInit, float *rA,
                                      float *rAA, float *rY, float *L, float *Leq) {
    return pfdr::cp_reduce_csc<float>("pfdr_cp_reduce_csc_f32", N, V, A, Y, rV, rVc, Vc, preAt,
                                      mem, normTol, normItMax, normNbInit, rA, rAA, rY, L, Leq);
}
extern "C" int pfdr_cp_reduce_csc_f64(int N, int V, const pfdr_csc *A, const double *Y, int rV,
                                      const int *rVc, const int *Vc, int preAt, int mem,
                                      double normTol, int normItMax, int normNbInit, double *rA,
                                      double *rAA, double *rY, double *L, double *Leq) {
    return pfdr::cp_reduce_csc<double>("pfdr_cp_reduce_csc_f64", N, V, A, Y, rV, rVc, Vc, preAt,
                                       mem, normTol, normItMax, normNbInit, rA, rAA, rY, L, Leq);
}

extern "C" int pfdr_cp_reduce_f32(int N, int V, const float *A, const float *Y, int rV,
                                  const int *rVc, const int *Vc, int preAt, int mem,
                                  float normTol, int normItMax, int normNbInit, float *rA,
                                  float *rAA, float *rY, float *L, float *Leq) {
    return pfdr::cp_reduce_host<float>("pfdr_cp_reduce_f32", N, V, A, Y, rV, rVc, Vc, preAt, mem,
                                       normTol, normItMax, normNbInit, rA, rAA, rY, L, Leq);
}
extern "C" int pfdr_cp_reduce_f64(int N, int V, const double *A, const double *Y, int rV,
                                  const int *rVc, const int *Vc, int preAt, int mem,
                                  double normTol, int normItMax, int normNbInit, double *rA,
                                  double *rAA, double *rY, double *L, double *Leq) {
    return pfdr::cp_reduce_host<double>("pfdr_cp_reduce_f64", N, V, A, Y, rV, rVc, Vc, preAt,
                                        mem, normTol, normItMax, normNbInit, rA, rAA, rY, L, Leq);
}
