// Kernels of the cut-pursuit drivers' sparse operator (pfdr_cp_sparse.hpp).
//
// Component column sums.  The dense kernel (k_cp_colsum, pfdr_cp.hip) walks
// the positions i of a component's range of Vc and adds A[n, Vc[i]].  Here:
//   1. off[i] = the stored entries of the columns Vc[0 .. i - 1] (a scan of the
//      column lengths in Vc order), so the entries are numbered in Vc order;
//   2. one lane per entry in that numbering writes (row, entry) and the pairs
//      are sorted by row (radix_sort_pairs_stable).  The sort is stable: inside
//      a row the entries stay in Vc-position order, and those of one component,
//      whose positions are one range of Vc, are consecutive;
//   3. the lane of the first entry of a (row, component) run adds the run in
//      order from +0 and stores one element of the zeroed rA.
// Integer work and one writer per element: the same bytes on every run.  A
// run of any length is walked by its one lane.
//
// The reduced operator kept sparse (CpCsc::reduced -> CpReduced).  Steps 1
// and 2 as above; then
//   3'. a scan of the run-head flags numbers the runs h = 0 .. rnnz - 1 in the
//       sorted order (rows ascending, and inside a row the components
//       ascending, since a component's positions are one range of Vc); the
//       head's lane adds its run as in 3 and stores (component, sum) at h:
//       the CSR view, its row offsets from the heads' rows (sorted_offsets);
//   4'. the pairs (component, h) are sorted by component, stably, so a
//       column's rows ascend strictly: the CSC.
// A run is stored whatever its sum (a cancellation is a stored zero), so the
// structure depends on A's structure and the partition only.  The column
// norms, the scaling and the residual on a CpReduced walk stored entries in
// the dense kernels' order (k_cp_colnorm, k_cp_scale_cols, k_cpq_residual).
//
// Gradient: one lane per column, products formed, then added in stored order.
//
// The reduced normal equations of a premultiplied iteration (CpReduced::gram,
// ::dot): rAA = rA^t rA and rY = rA^t Y over the stored entries, in the order
// of k_cp_gram_seq and k_cp_rY_dot (pfdr_cp.hip) and so with their bytes; the
// Gram kernel densifies one column at a time in a window of LDS and is
// described at k_cpsp_gram.
#include <cstdlib>

#include "pfdr_cp_sparse.hpp"
#include "pfdr_sort.hpp"

namespace pfdr {

namespace {

// ---- an exclusive scan of len(0), len(1), ... over the positions 0 .. n
// (len = 0 from n on), 16 per lane, a chunk of 4096 per workgroup.  Two
// lengths: the columns in Vc order, and the run heads of the sorted entries.
constexpr int kPer = 16, kChunk = kBlock * kPer;

// stored entries of the column at position i (none at i = V, or for a vertex outside [0, V))
struct CpspColLen {
    int V;
    const int64_t *colptr;
    const int *Vc;
    __device__ __forceinline__ int64_t operator()(long i) const {
        if (i >= V) return 0;
        const int v = Vc ? Vc[i] : (int)i;
        if ((unsigned)v >= (unsigned)V) return 0;
        return colptr[v + 1] - colptr[v];
    }
};

// 1 where sorted entry p opens a (row, component) run
struct CpspRunHead {
    int64_t nnz;
    const unsigned *rows;
    const int *sc;
    __device__ __forceinline__ int64_t operator()(long p) const {
        if (p >= nnz) return 0;
        return p == 0 || rows[p - 1] != rows[p] || sc[p - 1] != sc[p];
    }
};

template <typename Len>
__global__ __launch_bounds__(256) void k_cpsp_chunk_sums(Len len, int64_t *__restrict__ sums) {
    __shared__ int64_t part[kBlock];
    const long i0 = (long)blockIdx.x * kChunk + (long)threadIdx.x * kPer;
    int64_t a = 0;
    for (int k = 0; k < kPer; k++) a += len(i0 + k);
    part[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t t = 0;
        for (int k = 0; k < kBlock; k++) t += part[k];
        sums[blockIdx.x] = t;
    }
}

// exclusive scan of the chunk sums, in place (one lane: V / 4096 terms)
__global__ void k_cpsp_scan_sums(int nc, int64_t *__restrict__ sums) {
    if (blockIdx.x || threadIdx.x) return;
    int64_t t = 0;
    for (int c = 0; c < nc; c++) {
        const int64_t a = sums[c];
        sums[c] = t;
        t += a;
    }
}

// off[i] = len(0) + ... + len(i - 1), i = 0 .. n
template <typename Len>
__global__ __launch_bounds__(256) void k_cpsp_chunk_scan(long n, Len lenf,
                                                         const int64_t *__restrict__ sums,
                                                         int64_t *__restrict__ off) {
    __shared__ int64_t part[kBlock];
    const long i0 = (long)blockIdx.x * kChunk + (long)threadIdx.x * kPer;
    int64_t len[kPer], a = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        len[k] = lenf(i0 + k);
        a += len[k];
    }
    part[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t t = 0;
        for (int k = 0; k < kBlock; k++) {
            const int64_t b = part[k];
            part[k] = t;
            t += b;
        }
    }
    __syncthreads();
    int64_t run = sums[blockIdx.x] + part[threadIdx.x];
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        if (i0 + k <= n) off[i0 + k] = run;
        run += len[k];
    }
}

// off[0 .. n] on stream s; sums: (n + kChunk) / kChunk words of scratch
template <typename Len>
void cpsp_scan(long n, Len len, int64_t *sums, int64_t *off, hipStream_t s) {
    const int nc = (int)((n + kChunk) / kChunk);  // chunks of the positions 0 .. n
    k_cpsp_chunk_sums<Len><<<nc, kBlock, 0, s>>>(len, sums);
    k_cpsp_scan_sums<<<1, kWave, 0, s>>>(nc, sums);
    k_cpsp_chunk_scan<Len><<<nc, kBlock, 0, s>>>(n, len, sums, off);
}

// cv[Vc[i]] = the component whose range of Vc holds position i (rVc = nullptr: 0)
__global__ void k_cpsp_comp(int V, int rV, const int *__restrict__ rVc,
                            const int *__restrict__ Vc, int *__restrict__ cv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    int lo = 0;
    if (rVc) {
        int hi = rV;  // rVc[lo] <= i < rVc[hi]; any rVc content stays in [0, rV)
        while (hi - lo > 1) {
            const int m = lo + (hi - lo) / 2;
            if (rVc[m] <= i) lo = m;
            else hi = m;
        }
    }
    const int v = Vc ? Vc[i] : i;
    if ((unsigned)v < (unsigned)V) cv[v] = lo;
}

// entry t of the Vc-order numbering: its row as the key, its CSC index as the value
__global__ __launch_bounds__(256) void k_cpsp_keys(int V, int64_t nnz,
                                                   const int64_t *__restrict__ off,
                                                   const int64_t *__restrict__ colptr,
                                                   const int *__restrict__ Vc,
                                                   const int *__restrict__ rowidx,
                                                   unsigned *__restrict__ keys,
                                                   unsigned *__restrict__ vals) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nnz) return;
    int lo = 0, hi = V;  // the largest i in [0, V) with off[i] <= t: off[i + 1] > t
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (off[mid] <= t) lo = mid;
        else hi = mid;
    }
    const int v = Vc ? Vc[lo] : lo;
    int64_t e = 0;  // off[V] < nnz (Vc no permutation): any entry, the sums are then void
    if ((unsigned)v < (unsigned)V) {
        e = colptr[v] + (t - off[lo]);
        if (e >= colptr[v + 1]) e = 0;
    }
    keys[t] = (unsigned)rowidx[e];
    vals[t] = (unsigned)e;
}

// value and component of every sorted entry
template <typename real>
__global__ __launch_bounds__(256) void k_cpsp_gather(int64_t nnz, const unsigned *__restrict__ ent,
                                                     const int *__restrict__ ecol,
                                                     const int *__restrict__ cv,
                                                     const real *__restrict__ val,
                                                     real *__restrict__ sv, int *__restrict__ sc) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const unsigned e = ent[p];
    sv[p] = val[e];
    sc[p] = cv[ecol[e]];
}

// The sequential sum of the (row, component) run that sorted entry p opens:
// a += sv[q], q ascending from p, from +0.  False where p opens no run.
template <typename real>
__device__ __forceinline__ bool cpsp_run(int64_t p, int64_t nnz, const unsigned *__restrict__ rows,
                                         const int *__restrict__ sc, const real *__restrict__ sv,
                                         unsigned &r, int &c, real &a) {
    if (p >= nnz) return false;
    r = rows[p];
    c = sc[p];
    if (p > 0 && rows[p - 1] == r && sc[p - 1] == c) return false;
    a = real(0);
    int64_t q = p;
    do {
        a += sv[q];
        q++;
    } while (q < nnz && rows[q] == r && sc[q] == c);
    return true;
}

// every run's sum into its element of the zeroed dense rA
template <typename real>
__global__ __launch_bounds__(256) void k_cpsp_runs(int64_t nnz, int N,
                                                   const unsigned *__restrict__ rows,
                                                   const int *__restrict__ sc,
                                                   const real *__restrict__ sv,
                                                   real *__restrict__ rA) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned r;
    int c;
    real a;
    if (cpsp_run<real>(p, nnz, rows, sc, sv, r, c, a)) rA[(size_t)N * c + r] = a;
}

// ---- the reduced operator kept sparse (CpReduced)
// every run's sum at the run's number h = pos[p]: CSR column and value of
// entry h, its row, and the (component, h) pair that the sort by component
// takes
template <typename real>
__global__ __launch_bounds__(256) void k_cpsp_runs_csr(int64_t nnz,
                                                       const unsigned *__restrict__ rows,
                                                       const int *__restrict__ sc,
                                                       const real *__restrict__ sv,
                                                       const int64_t *__restrict__ pos,
                                                       int *__restrict__ colidx,
                                                       real *__restrict__ rval,
                                                       unsigned *__restrict__ hrow,
                                                       unsigned *__restrict__ keys,
                                                       unsigned *__restrict__ vals) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned r;
    int c;
    real a;
    if (!cpsp_run<real>(p, nnz, rows, sc, sv, r, c, a)) return;
    const int64_t h = pos[p];
    colidx[h] = c;
    rval[h] = a;
    hrow[h] = r;
    keys[h] = (unsigned)c;
    vals[h] = (unsigned)h;
}

// the CSC from the heads sorted by component (comp[j], head[j])
template <typename real>
__global__ __launch_bounds__(256) void k_cpsp_csc_fill(int64_t n, const unsigned *__restrict__ comp,
                                                       const unsigned *__restrict__ head,
                                                       const unsigned *__restrict__ hrow,
                                                       const real *__restrict__ rval,
                                                       int *__restrict__ rowidx,
                                                       int *__restrict__ ecol,
                                                       real *__restrict__ val) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned h = head[j];
    rowidx[j] = (int)hrow[h];
    ecol[j] = (int)comp[j];
    val[j] = rval[h];
}

// l[rv] = ||rA[:, rv]||, the stored squares added in ascending row order
// (k_cp_colnorm without its +0 terms); *bad = the first rv with l 0 or not finite
template <typename real>
__global__ __launch_bounds__(256) void k_cpsp_colnorm(int rV, const int64_t *__restrict__ colptr,
                                                      const real *__restrict__ val,
                                                      real *__restrict__ l, int *__restrict__ bad) {
    const int rv = blockIdx.x * blockDim.x + threadIdx.x;
    if (rv >= rV) return;
    real s = real(0);
    for (int64_t e = colptr[rv], e1 = colptr[rv + 1]; e < e1; e++) {
        const real b = val[e];
        s += b * b;
    }
    const real x = std::sqrt(s);
    l[rv] = x;
    if (!(x > real(0)) || x - x != real(0)) atomicMin(bad, rv);
}

// val[e] /= (mul: *=) l[col[e]] (k_cp_scale_cols, element by element)
template <typename real>
__global__ __launch_bounds__(256) void k_cpsp_scale(int64_t n, const int *__restrict__ col,
                                                    const real *__restrict__ l,
                                                    real *__restrict__ val, int mul) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    if (mul) val[e] *= l[col[e]];
    else val[e] /= l[col[e]];
}

// R[n] = Y[n] - sum of rval[e] rX[colidx[e]] over row n's entries, rv
// ascending, each product formed and then added from +0 (k_cpq_residual
// without its +-0 terms); one lane per row, 4 entries' loads in flight
template <typename real>
__global__ __launch_bounds__(256) void k_cpsp_residual(int N, const int64_t *__restrict__ rowptr,
                                                       const int *__restrict__ colidx,
                                                       const real *__restrict__ rval,
                                                       const real *__restrict__ rX,
                                                       const real *__restrict__ Y,
                                                       real *__restrict__ R) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int64_t e = rowptr[n];
    const int64_t e1 = rowptr[n + 1];
    constexpr int U = 4;
    real a = real(0);
    for (; e + U <= e1; e += U) {
        real x[U], y[U];
#pragma unroll
        for (int q = 0; q < U; q++) {
            x[q] = rval[e + q];
            y[q] = rX[colidx[e + q]];
        }
#pragma unroll
        for (int q = 0; q < U; q++) {
            const real b = x[q] * y[q];
            a += b;
        }
    }
    for (; e < e1; e++) {
        const real b = rval[e] * rX[colidx[e]];
        a += b;
    }
    R[n] = Y[n] - a;
}

// ---- rAA = rA^t rA over the stored entries (CpReduced::gram)
// The window of rows that one workgroup holds densified in LDS: 32 KiB, so
// that five workgroups fit a CU's 160 KiB.
constexpr int kGramLdsBytes = 32 * 1024;

// the first e in [lo, hi) with rowidx[e] >= row (hi where there is none)
__device__ __forceinline__ int64_t cpsp_lower(const int *__restrict__ rowidx, int64_t lo,
                                              int64_t hi, long row) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (rowidx[mid] < row) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Upper triangle rAA[rv + rV ru], rv <= ru: the products of the rows stored in
// both columns, rows ascending, each product formed and then added from +0
// (k_cp_gram_seq without its +-0 terms).  One workgroup per column ru, the
// longest triangle columns first.  It walks ru's row range in windows of W
// rows: the window is zeroed in LDS and ru's entries in it are scattered in;
// then lane t takes rv = t, t + 256, ... <= ru and adds val * win[row - base]
// over column rv's entries in the window, found by binary search, 4 entries'
// loads ahead of the adds.  Where ru stores nothing the factor is the window's
// +0, the dense loop's own term.  A pair's sum is carried from window to
// window in rAA itself, written and read back by the same lane; a window in
// which ru stores nothing is skipped, and so is a column rv that stores
// nothing in a later window.  No atomics.
template <typename real>
__global__ __launch_bounds__(256) void k_cpsp_gram(int rV, int W,
                                                   const int64_t *__restrict__ colptr,
                                                   const int *__restrict__ rowidx,
                                                   const real *__restrict__ val,
                                                   real *__restrict__ rAA) {
    __shared__ real win[kGramLdsBytes / sizeof(real)];
    const int ru = rV - 1 - (int)blockIdx.x;
    const int64_t u0 = colptr[ru], u1 = colptr[ru + 1];
    real *out = rAA + (size_t)rV * ru;
    if (u0 == u1) {  // an empty column: no common row with any
        for (long rv = threadIdx.x; rv <= ru; rv += kBlock) out[rv] = real(0);
        return;
    }
    const long first = rowidx[u0], last = rowidx[u1 - 1];
    bool fresh = true;  // no window has written the sums yet
    int64_t ua = u0;    // ru's first entry at or after the window
    for (long base = first; base <= last; base += W) {
        const long lim = base + W;
        const int64_t ub = cpsp_lower(rowidx, ua, u1, lim);
        if (ub == ua) continue;  // (never the first window: it holds row `first`)
        for (int i = threadIdx.x; i < W; i += kBlock) win[i] = real(0);
        __syncthreads();
        for (int64_t e = ua + threadIdx.x; e < ub; e += kBlock) win[rowidx[e] - base] = val[e];
        __syncthreads();
        for (long rv = threadIdx.x; rv <= ru; rv += kBlock) {
            const int64_t e1 = colptr[rv + 1];
            int64_t e = cpsp_lower(rowidx, colptr[rv], e1, base);
            if (!fresh && (e == e1 || rowidx[e] >= lim)) continue;
            real s = fresh ? real(0) : out[rv];
            constexpr int U = 4;
            for (; e + U <= e1; e += U) {
                int r[U];
                real x[U], y[U];
#pragma unroll
                for (int q = 0; q < U; q++) {
                    r[q] = rowidx[e + q];
                    x[q] = val[e + q];
                }
                if (r[U - 1] >= lim) break;  // the window ends inside these: one by one below
#pragma unroll
                for (int q = 0; q < U; q++) y[q] = win[r[q] - base];
#pragma unroll
                for (int q = 0; q < U; q++) {
                    const real b = x[q] * y[q];
                    s += b;
                }
            }
            for (; e < e1; e++) {
                const long r = rowidx[e];
                if (r >= lim) break;
                const real b = val[e] * win[r - base];
                s += b;
            }
            out[rv] = s;
        }
        fresh = false;
        ua = ub;
        __syncthreads();  // the window is zeroed again
    }
}

// out[v] = the sum of val[e] w[rowidx[e]] over column v's entries in stored
// order, each product formed and then added from +0 (NEG: its negative); 4
// entries' loads in flight ahead of the adds.  The gradient DfS = -A^t R and
// rY = rA^t Y (k_cp_rY_dot without its +-0 terms).
template <typename real, bool NEG>
__global__ __launch_bounds__(256) void k_cpsp_coldot(int V, const int64_t *__restrict__ colptr,
                                                     const int *__restrict__ rowidx,
                                                     const real *__restrict__ val,
                                                     const real *__restrict__ R,
                                                     real *__restrict__ DfS) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    int64_t e = colptr[v];
    const int64_t e1 = colptr[v + 1];
    constexpr int U = 4;
    real s = real(0);
    for (; e + U <= e1; e += U) {
        real x[U], y[U];
#pragma unroll
        for (int q = 0; q < U; q++) {
            x[q] = val[e + q];
            y[q] = R[rowidx[e + q]];
        }
#pragma unroll
        for (int q = 0; q < U; q++) {
            const real b = x[q] * y[q];
            s += b;
        }
    }
    for (; e < e1; e++) {
        const real b = val[e] * R[rowidx[e]];
        s += b;
    }
    DfS[v] = NEG ? -s : s;
}

}  // namespace

template <typename real>
void CpCsc<real>::sort_entries(int rV, const int *rVc, const int *Vc, hipStream_t s) {
    const int N = m.N, V = m.V;
    const int64_t nnz = m.nnz;
    if (!ki.p) {
        off.alloc((size_t)V + 1);
        sums.alloc(((size_t)V + kChunk) / kChunk);
        cv.alloc(V);
        sc.alloc(nnz);
        sv.alloc(nnz);
        ki.alloc(nnz), ko.alloc(nnz), vi.alloc(nnz), vo.alloc(nnz);
    }
    PFDR_HIP(hipMemsetAsync(cv.p, 0, sizeof(int) * (size_t)V, s));
    cpsp_scan(V, CpspColLen{V, m.colptr.p, Vc}, sums.p, off.p, s);
    k_cpsp_comp<<<grid_for(V), kBlock, 0, s>>>(V, rV, rVc, Vc, cv.p);
    k_cpsp_keys<<<grid_for(nnz), kBlock, 0, s>>>(V, nnz, off.p, m.colptr.p, Vc, m.rowidx.p, ki.p,
                                                 vi.p);
    PFDR_HIP(hipGetLastError());
    radix_sort_pairs_stable<unsigned>(ki.p, ko.p, vi.p, vo.p, (long)nnz, radix_key_bits(N), s);
    k_cpsp_gather<real><<<grid_for(nnz), kBlock, 0, s>>>(nnz, vo.p, m.ecol.p, cv.p, m.val.p, sv.p,
                                                         sc.p);
    PFDR_HIP(hipGetLastError());
}

template <typename real>
void CpCsc<real>::colsum(int rV, const int *rVc, const int *Vc, real *rA, hipStream_t s) {
    PFDR_HIP(hipMemsetAsync(rA, 0, sizeof(real) * (size_t)m.N * rV, s));
    sort_entries(rV, rVc, Vc, s);
    k_cpsp_runs<real><<<grid_for(m.nnz), kBlock, 0, s>>>(m.nnz, m.N, ko.p, sc.p, sv.p, rA);
    PFDR_HIP(hipGetLastError());
}

template <typename real>
void CpCsc<real>::reduced(int rV, const int *rVc, const int *Vc, CpReduced<real> &out,
                          hipStream_t s) {
    sort_entries(rV, rVc, Vc, s);
    const int N = m.N;
    const int64_t nnz = m.nnz;
    if (!pos.p) {
        pos.alloc((size_t)nnz + 1);
        psums.alloc(((size_t)nnz + kChunk) / kChunk);
        hrow.alloc(nnz);
    }
    // the run heads before every sorted entry; their count comes back
    cpsp_scan((long)nnz, CpspRunHead{nnz, ko.p, sc.p}, psums.p, pos.p, s);
    PFDR_HIP(hipGetLastError());
    int64_t rnnz = 0;
    PFDR_HIP(hipMemcpyAsync(&rnnz, pos.p + nnz, sizeof rnnz, hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
    DevCsc<real> &o = out.m;
    o.N = N, o.V = rV, o.nnz = rnnz;
    o.rowptr.alloc((size_t)N + 1);
    o.colptr.alloc((size_t)rV + 1);
    o.colidx.alloc(rnnz), o.rval.alloc(rnnz);
    o.rowidx.alloc(rnnz), o.ecol.alloc(rnnz), o.val.alloc(rnnz);
    // CSR: the heads in sorted order (rows ascending, components ascending inside a row)
    k_cpsp_runs_csr<real><<<grid_for(nnz), kBlock, 0, s>>>(nnz, ko.p, sc.p, sv.p, pos.p,
                                                           o.colidx.p, o.rval.p, hrow.p, ki.p,
                                                           vi.p);
    PFDR_HIP(hipGetLastError());
    sorted_offsets(rnnz, N, hrow.p, o.rowptr.p, s);
    // CSC: the heads sorted by component, stably, so that a column's rows ascend
    radix_sort_pairs_stable<unsigned>(ki.p, ko.p, vi.p, vo.p, (long)rnnz, radix_key_bits(rV), s);
    k_cpsp_csc_fill<real><<<grid_for(rnnz), kBlock, 0, s>>>(rnnz, ko.p, vo.p, hrow.p, o.rval.p,
                                                            o.rowidx.p, o.ecol.p, o.val.p);
    PFDR_HIP(hipGetLastError());
    sorted_offsets(rnnz, rV, ko.p, o.colptr.p, s);
}

template <typename real>
long CpReduced<real>::colnorm(real *l, hipStream_t s) const {
    DevBuf<int> bad(1);
    const int none = 0x7fffffff;
    int first = none;
    PFDR_HIP(hipMemcpyAsync(bad.p, &none, sizeof none, hipMemcpyHostToDevice, s));
    k_cpsp_colnorm<real><<<grid_for(m.V), kBlock, 0, s>>>(m.V, m.colptr.p, m.val.p, l, bad.p);
    PFDR_HIP(hipGetLastError());
    PFDR_HIP(hipMemcpyAsync(&first, bad.p, sizeof first, hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
    return first == none ? -1L : (long)first;
}

template <typename real>
void CpReduced<real>::scale(const real *l, int mul, hipStream_t s) {
    k_cpsp_scale<real><<<grid_for(m.nnz), kBlock, 0, s>>>(m.nnz, m.ecol.p, l, m.val.p, mul);
    k_cpsp_scale<real><<<grid_for(m.nnz), kBlock, 0, s>>>(m.nnz, m.colidx.p, l, m.rval.p, mul);
    PFDR_HIP(hipGetLastError());
}

template <typename real>
void CpReduced<real>::residual(const real *rX, const real *Y, real *R, hipStream_t s) const {
    k_cpsp_residual<real><<<grid_for(m.N), kBlock, 0, s>>>(m.N, m.rowptr.p, m.colidx.p, m.rval.p,
                                                           rX, Y, R);
    PFDR_HIP(hipGetLastError());
}

template <typename real>
void CpCsc<real>::gradient(const real *R, real *DfS, hipStream_t s) const {
    k_cpsp_coldot<real, true><<<grid_for(m.V), kBlock, 0, s>>>(m.V, m.colptr.p, m.rowidx.p,
                                                               m.val.p, R, DfS);
    PFDR_HIP(hipGetLastError());
}

// The rows of k_cpsp_gram's window: as many as its LDS holds (cap), or
// PFDR_CP_GRAM_WINDOW where that is a whole number in [1, cap); read at every
// call, so a test may change it between two calls of one process.
static int cp_gram_window(int cap) {
    if (const char *e = std::getenv("PFDR_CP_GRAM_WINDOW")) {
        char *end = nullptr;
        const long w = std::strtol(e, &end, 10);
        if (end != e && *end == 0 && w >= 1 && w < cap) return (int)w;
    }
    return cap;
}

template <typename real>
void CpReduced<real>::gram(real *rAA, hipStream_t s) const {
    const int W = cp_gram_window(kGramLdsBytes / (int)sizeof(real));
    k_cpsp_gram<real><<<m.V, kBlock, 0, s>>>(m.V, W, m.colptr.p, m.rowidx.p, m.val.p, rAA);
    PFDR_HIP(hipGetLastError());
}

template <typename real>
void CpReduced<real>::dot(const real *Y, real *rY, hipStream_t s) const {
    k_cpsp_coldot<real, false><<<grid_for(m.V), kBlock, 0, s>>>(m.V, m.colptr.p, m.rowidx.p,
                                                                m.val.p, Y, rY);
    PFDR_HIP(hipGetLastError());
}

template struct CpCsc<float>;
template struct CpCsc<double>;
template struct CpReduced<float>;
template struct CpReduced<double>;

}  // namespace pfdr
