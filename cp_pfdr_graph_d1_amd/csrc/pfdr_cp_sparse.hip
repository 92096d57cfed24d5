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
// Gradient: one lane per column, products formed, then added in stored order.
#include <algorithm>
#include <stdexcept>

#include "pfdr_cp_sparse.hpp"
#include "pfdr_sort.hpp"

namespace pfdr {

namespace {

enum : unsigned { kBadColptr = 1u, kBadRow = 2u, kBadOrder = 4u };

// colptr[0] = 0, colptr[V] = nnz, non-decreasing (threads 0 .. V); every row
// index in [0, N) and above its predecessor in the same column (threads
// 0 .. nnz - 1).  ecol[e] by a binary search that stays inside colptr[0 .. V)
// whatever it holds.
__global__ __launch_bounds__(256) void k_cpsp_check(int V, int N, int64_t nnz,
                                                    const int64_t *__restrict__ colptr,
                                                    const int *__restrict__ rowidx,
                                                    int *__restrict__ ecol,
                                                    unsigned *__restrict__ word) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned bad = 0;
    if (t <= V) {
        const int64_t c = colptr[t];
        if (c < 0 || c > nnz) bad |= kBadColptr;
        if (t == 0 && c != 0) bad |= kBadColptr;
        if (t == V && c != nnz) bad |= kBadColptr;
        if (t < V && colptr[t + 1] < c) bad |= kBadColptr;
    }
    if (t < nnz) {
        int lo = 0, hi = V;  // the largest v in [0, V) with colptr[v] <= t
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (colptr[mid] <= t) lo = mid;
            else hi = mid;
        }
        ecol[t] = lo;
        const int r = rowidx[t];
        if (r < 0 || r >= N) bad |= kBadRow;
        if (t > 0 && t > colptr[lo] && rowidx[t - 1] >= r) bad |= kBadOrder;
    }
    if (bad) atomicOr(word, bad);
}

// ---- the scan of the column lengths in Vc order: positions 0 .. V, 16 per
// lane, a chunk of 4096 per workgroup
constexpr int kPer = 16, kChunk = kBlock * kPer;

// stored entries of the column at position i (none at i = V, or for a vertex outside [0, V))
__device__ __forceinline__ int64_t cpsp_len(int V, const int64_t *__restrict__ colptr,
                                            const int *__restrict__ Vc, long i) {
    if (i >= V) return 0;
    const int v = Vc ? Vc[i] : (int)i;
    if ((unsigned)v >= (unsigned)V) return 0;
    return colptr[v + 1] - colptr[v];
}

__global__ __launch_bounds__(256) void k_cpsp_chunk_sums(int V, const int64_t *__restrict__ colptr,
                                                         const int *__restrict__ Vc,
                                                         int64_t *__restrict__ sums) {
    __shared__ int64_t part[kBlock];
    const long i0 = (long)blockIdx.x * kChunk + (long)threadIdx.x * kPer;
    int64_t a = 0;
    for (int k = 0; k < kPer; k++) a += cpsp_len(V, colptr, Vc, i0 + k);
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

__global__ __launch_bounds__(256) void k_cpsp_chunk_scan(int V, const int64_t *__restrict__ colptr,
                                                         const int *__restrict__ Vc,
                                                         const int64_t *__restrict__ sums,
                                                         int64_t *__restrict__ off) {
    __shared__ int64_t part[kBlock];
    const long i0 = (long)blockIdx.x * kChunk + (long)threadIdx.x * kPer;
    int64_t len[kPer], a = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        len[k] = cpsp_len(V, colptr, Vc, i0 + k);
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
        if (i0 + k <= V) off[i0 + k] = run;
        run += len[k];
    }
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

// the first entry of a (row, component) run adds the run in order
template <typename real>
__global__ __launch_bounds__(256) void k_cpsp_runs(int64_t nnz, int N,
                                                   const unsigned *__restrict__ rows,
                                                   const int *__restrict__ sc,
                                                   const real *__restrict__ sv,
                                                   real *__restrict__ rA) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const unsigned r = rows[p];
    const int c = sc[p];
    if (p > 0 && rows[p - 1] == r && sc[p - 1] == c) return;
    real a = real(0);
    int64_t q = p;
    do {
        a += sv[q];
        q++;
    } while (q < nnz && rows[q] == r && sc[q] == c);
    rA[(size_t)N * c + r] = a;
}

// DfS[v] = -(sum of val[e] R[rowidx[e]]), column v's entries in stored order;
// 4 entries' loads in flight ahead of the adds
template <typename real>
__global__ __launch_bounds__(256) void k_cpsp_grad(int V, const int64_t *__restrict__ colptr,
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
    DfS[v] = -s;
}

}  // namespace

const char *cp_csc_args(const pfdr_csc *A) {
    if (!A) return "sparse A: the pfdr_csc is NULL";
    if (!A->colptr || !A->rowidx || !A->val) return "sparse A: a NULL array";
    if (A->nnz < 1 || A->nnz >= 2147483648LL - 256)
        return "sparse A: nnz must lie in [1, 2^31 - 256)";
    return nullptr;
}

template <typename real>
void CpCsc<real>::take(int N_, int V_, const pfdr_csc *A, int mem, hipStream_t s) {
    N = N_, V = V_, nnz = A->nnz;
    colptr.alloc((size_t)V + 1);
    rowidx.alloc(nnz);
    val.alloc(nnz);
    ecol.alloc(nnz);
    DevBuf<unsigned> word(1);
    HostPins pins(s);
    auto in = [&](void *dst, const void *src, size_t b) {
        if (mem == PFDR_MEM_DEVICE)
            PFDR_HIP(hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToDevice, s));
        else
            pins.copy(dst, src, b, hipMemcpyHostToDevice);
    };
    in(colptr.p, A->colptr, ((size_t)V + 1) * 8);
    in(rowidx.p, A->rowidx, (size_t)nnz * 4);
    in(val.p, A->val, (size_t)nnz * sizeof(real));
    PFDR_HIP(hipMemsetAsync(word.p, 0, sizeof(unsigned), s));
    k_cpsp_check<<<grid_for(std::max<long>((long)V + 1, (long)nnz)), kBlock, 0, s>>>(
        V, N, nnz, colptr.p, rowidx.p, ecol.p, word.p);
    PFDR_HIP(hipGetLastError());
    unsigned w = 0;
    PFDR_HIP(hipMemcpyAsync(&w, word.p, sizeof w, hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
    pins.release();
    if (w & kBadColptr)
        throw std::runtime_error("sparse A: colptr must be non-decreasing with colptr[0] = 0 "
                                 "and colptr[V] = nnz");
    if (w & kBadRow) throw std::runtime_error("sparse A: row index outside [0, N)");
    if (w & kBadOrder)
        throw std::runtime_error("sparse A: row indices must be strictly ascending inside "
                                 "each column");
}

template <typename real>
void CpCsc<real>::colsum(int rV, const int *rVc, const int *Vc, real *rA, hipStream_t s) {
    if (!ki.p) {
        off.alloc((size_t)V + 1);
        sums.alloc(((size_t)V + kChunk) / kChunk);
        cv.alloc(V);
        sc.alloc(nnz);
        sv.alloc(nnz);
        ki.alloc(nnz), ko.alloc(nnz), vi.alloc(nnz), vo.alloc(nnz);
    }
    const int nc = (int)sums.n;  // chunks of the positions 0 .. V
    PFDR_HIP(hipMemsetAsync(rA, 0, sizeof(real) * (size_t)N * rV, s));
    PFDR_HIP(hipMemsetAsync(cv.p, 0, sizeof(int) * (size_t)V, s));
    k_cpsp_chunk_sums<<<nc, kBlock, 0, s>>>(V, colptr.p, Vc, sums.p);
    k_cpsp_scan_sums<<<1, kWave, 0, s>>>(nc, sums.p);
    k_cpsp_chunk_scan<<<nc, kBlock, 0, s>>>(V, colptr.p, Vc, sums.p, off.p);
    k_cpsp_comp<<<grid_for(V), kBlock, 0, s>>>(V, rV, rVc, Vc, cv.p);
    k_cpsp_keys<<<grid_for(nnz), kBlock, 0, s>>>(V, nnz, off.p, colptr.p, Vc, rowidx.p, ki.p,
                                                 vi.p);
    PFDR_HIP(hipGetLastError());
    int bits = 1;
    while (bits < 32 && (1L << bits) < (long)N) bits++;
    radix_sort_pairs_stable<unsigned>(ki.p, ko.p, vi.p, vo.p, (long)nnz, bits, s);
    k_cpsp_gather<real><<<grid_for(nnz), kBlock, 0, s>>>(nnz, vo.p, ecol.p, cv.p, val.p, sv.p,
                                                         sc.p);
    k_cpsp_runs<real><<<grid_for(nnz), kBlock, 0, s>>>(nnz, N, ko.p, sc.p, sv.p, rA);
    PFDR_HIP(hipGetLastError());
}

template <typename real>
void CpCsc<real>::gradient(const real *R, real *DfS, hipStream_t s) const {
    k_cpsp_grad<real><<<grid_for(V), kBlock, 0, s>>>(V, colptr.p, rowidx.p, val.p, R, DfS);
    PFDR_HIP(hipGetLastError());
}

template struct CpCsc<float>;
template struct CpCsc<double>;

}  // namespace pfdr
