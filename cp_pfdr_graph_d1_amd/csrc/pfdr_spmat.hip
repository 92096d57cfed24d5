// DevCsc (pfdr_spmat.hpp): the intake of a caller's CSC and its CSR view.
#include <algorithm>
#include <chrono>
#include <stdexcept>

#include "pfdr_sort.hpp"
#include "pfdr_spmat.hpp"

namespace pfdr {

namespace {

// content checks of a CSC, folded into one word
enum : unsigned { kBadColptr = 1u, kBadRow = 2u, kBadOrder = 4u };

// One pass over colptr (threads 0 .. V) and rowidx (threads 0 .. nnz - 1):
// colptr[0] = 0, colptr[V] = nnz, non-decreasing; every row index in [0, N)
// and above its predecessor in the same column.  ecol[e] = the column of
// entry e, by a binary search that stays inside colptr[0 .. V) whatever it
// holds.
__global__ __launch_bounds__(256) void k_csc_check(int V, int N, int64_t nnz,
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
            if (colptr[mid] <= t) lo = mid; else hi = mid;
        }
        ecol[t] = lo;
        const int r = rowidx[t];
        if (r < 0 || r >= N) bad |= kBadRow;
        if (t > 0 && t > colptr[lo] && rowidx[t - 1] >= r) bad |= kBadOrder;
    }
    if (bad) atomicOr(word, bad);
}

__global__ void k_csr_keys(int64_t nnz, const int *__restrict__ rowidx,
                           unsigned *__restrict__ keys, unsigned *__restrict__ vals) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    keys[e] = (unsigned)rowidx[e];
    vals[e] = (unsigned)e;
}

// Position h < n of sorted_offsets: it writes the offsets of the ids it opens,
// and the last position the tail.
__device__ __forceinline__ void offsets_at(int64_t h, int64_t n, long m,
                                           const unsigned *__restrict__ id,
                                           int64_t *__restrict__ ptr) {
    const long r = (long)id[h];
    const long prev = h ? (long)id[h - 1] : -1L;
    for (long q = prev + 1; q <= r && q <= m; q++) ptr[q] = h;
    if (h == n - 1)
        for (long q = r + 1; q <= m; q++) ptr[q] = n;
}

__global__ __launch_bounds__(256) void k_sorted_offsets(int64_t n, long m,
                                                        const unsigned *__restrict__ id,
                                                        int64_t *__restrict__ ptr) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h < n) offsets_at(h, n, m, id, ptr);
}

// the CSR arrays from the entries sorted by row (rows[p] = the row of sorted
// position p, perm[p] = its entry): the sort is stable and the entries were
// enumerated in column order, so every row's columns ascend.  The row offsets
// in the same pass (a launch of their own: +1.2 % on the build, measured).
template <typename real>
__global__ __launch_bounds__(256) void k_csr_fill(int64_t nnz, int N,
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
    offsets_at(p, nnz, N, rows, rowptr);
}

// the longest segment of an offset array
__global__ void k_maxlen(int n, const int64_t *__restrict__ ptr, int *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    atomicMax(out, (int)(ptr[i + 1] - ptr[i]));
}

}  // namespace

const char *cp_csc_args(const pfdr_csc *A) {
    if (!A) return "sparse A: the pfdr_csc is NULL";
    if (!A->colptr || !A->rowidx || !A->val) return "sparse A: a NULL array";
    if (A->nnz < 1 || A->nnz >= 2147483648LL - 256)
        return "sparse A: nnz must lie in [1, 2^31 - 256)";
    return nullptr;
}

void sorted_offsets(int64_t n, long m, const unsigned *id, int64_t *ptr, hipStream_t s) {
    k_sorted_offsets<<<grid_for(n), kBlock, 0, s>>>(n, m, id, ptr);
    PFDR_HIP(hipGetLastError());
}

template <typename real>
unsigned DevCsc<real>::verdict(hipStream_t s) const {
    unsigned w = 0;
    PFDR_HIP(hipMemcpyAsync(&w, word.p, sizeof w, hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
    return w;
}

template <typename real>
void DevCsc<real>::take(int N_, int V_, const pfdr_csc *A, int mem, hipStream_t s,
                        HostPins &pins) {
    N = N_, V = V_, nnz = A->nnz;
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
    ecol.alloc(nnz);
    k_csc_check<<<grid_for(std::max<long>((long)V + 1, (long)nnz)), kBlock, 0, s>>>(
        V, N, nnz, colptr.p, rowidx.p, ecol.p, word.p);
    PFDR_HIP(hipGetLastError());
    const unsigned w = verdict(s);
    if (w & kBadColptr)
        throw std::runtime_error("sparse A: colptr must be non-decreasing with colptr[0] = 0 "
                                 "and colptr[V] = nnz");
    if (w & kBadRow) throw std::runtime_error("sparse A: row index outside [0, N)");
    if (w & kBadOrder)
        throw std::runtime_error("sparse A: row indices must be strictly ascending inside "
                                 "each column");
}

template <typename real>
void DevCsc<real>::build_csr(hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    rowptr.alloc((size_t)N + 1);
    colidx.alloc(nnz);
    rval.alloc(nnz);
    {
        DevBuf<unsigned> ki(nnz), ko(nnz), vi(nnz), vo(nnz);
        k_csr_keys<<<grid_for(nnz), kBlock, 0, s>>>(nnz, rowidx.p, ki.p, vi.p);
        PFDR_HIP(hipGetLastError());
        radix_sort_pairs_stable<unsigned>(ki.p, ko.p, vi.p, vo.p, (long)nnz, radix_key_bits(N), s);
        k_csr_fill<real><<<grid_for(nnz), kBlock, 0, s>>>(nnz, N, ko.p, vo.p, ecol.p, val.p,
                                                         rowptr.p, colidx.p, rval.p);
        PFDR_HIP(hipGetLastError());
        DevBuf<int> mx(2);
        PFDR_HIP(hipMemsetAsync(mx.p, 0, 2 * sizeof(int), s));
        k_maxlen<<<grid_for(V), kBlock, 0, s>>>(V, colptr.p, mx.p);
        k_maxlen<<<grid_for(N), kBlock, 0, s>>>(N, rowptr.p, mx.p + 1);
        PFDR_HIP(hipGetLastError());
        int h[2] = {0, 0};
        PFDR_HIP(hipMemcpyAsync(h, mx.p, sizeof h, hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
        maxcol = h[0];
        maxrow = h[1];
    }
    csr_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                 .count();
    ecol.release();
}

template struct DevCsc<float>;
template struct DevCsc<double>;

}  // namespace pfdr
