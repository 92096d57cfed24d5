// Build of the tile and split layouts (formats: pfdr_layout.hpp): setup
// kernels, their host orchestration, and the debug hooks of the edge-block
// records.  Nothing here runs per iteration.
#include <algorithm>
#include <unordered_map>
#include <vector>

#include "pfdr_halo.hpp"
#include "pfdr_layout.hpp"
#include "pfdr_sort.hpp"

namespace pfdr {

// tile-order keys: (u block, v block) in the high bits, edge position the
// value; a partitioned rank (split) puts the edges with a ghost end after
// all the others (bit 2 vbits)
static __global__ void k_tile_keys(long E, const int *__restrict__ Eu, const int *__restrict__ Ev,
                                   int vbits, unsigned long long *__restrict__ keys,
                                   unsigned *__restrict__ vals, int V = 0, bool split = false) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int u = Eu[e], v = Ev[e];
    const unsigned long long g = split && (u >= V || v >= V) ? 1ull << (2 * vbits) : 0ull;
    keys[e] = g | ((unsigned long long)(u / kBlock) << vbits) | (unsigned)(v / kBlock);
    vals[e] = (unsigned)e;
}

// *out = the number of sorted keys below `bound` (one lane, binary search)
static __global__ void k_count_below(long n, const unsigned long long *__restrict__ keys,
                                     unsigned long long bound, unsigned long long *out) {
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (keys[mid] < bound) lo = mid + 1;
        else hi = mid;
    }
    *out = (unsigned long long)lo;
}

// tile order: position p takes the edge now at perm[p].  eo = its id for the
// incidence keys: ids[perm[p]], or e_offset + perm[p].  One GPU (inv null):
// emap = that id too (the weights' permutation); a partitioned rank: emap =
// the rank-local position perm[p], and inv its inverse
static __global__ void k_edge_tile_order(
    long E, const unsigned *__restrict__ perm, const unsigned *__restrict__ ids, long e_offset,
    const int *__restrict__ Eu, const int *__restrict__ Ev, int *__restrict__ nEu,
    int *__restrict__ nEv, unsigned *__restrict__ eo, int *__restrict__ emap,
    unsigned *__restrict__ inv) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    const unsigned q = perm[p];
    nEu[p] = Eu[q];
    nEv[p] = Ev[q];
    const unsigned e = ids ? ids[q] : (unsigned)(e_offset + q);
    eo[p] = e;
    emap[p] = inv ? (int)q : (int)e;
    if (inv) inv[q] = (unsigned)p;
}

// the halo's push addresses (side E + e) into the tile order
static __global__ void k_remap_push(long n, long E, const unsigned *__restrict__ inv,
                                    unsigned *__restrict__ addr) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned a = addr[i];
    const unsigned side = a >= (unsigned)E ? 1u : 0u;
    addr[i] = side * (unsigned)E + inv[a - side * (unsigned)E];
}

// d2[address] = CSR slot of the (edge, side) at that address, relative to the
// first slot of its vertex block; one lane per vertex
static __global__ void k_tile_slots(int V, const int *__restrict__ ptr,
                                    const unsigned *__restrict__ idx,
                                    unsigned short *__restrict__ d2) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int base = ptr[v - v % kBlock];
    for (int j = ptr[v]; j < ptr[v + 1]; j++) d2[idx[j]] = (unsigned short)(j - base);
}

// the slots of addresses [8 g, 8 g + 8) below n packed into group g (a tiled
// block's slots are < kTileCap)
static __global__ void k_pack_slots(long ngroups, long n, const unsigned short *__restrict__ d2,
                                    Slots12 *__restrict__ out) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < ngroups) out[g] = pack_slots12(d2 + g * kSlotGroup, n - g * kSlotGroup);
}

// ustart[b] = first position whose u end is in block >= b (tile order sorts by
// u block), ustart[nb] = E
static __global__ void k_tile_ustart(long E, int nb, const int *__restrict__ Eu,
                                     int *__restrict__ ustart) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > E) return;
    const int lo = p == 0 ? 0 : Eu[p - 1] / kBlock + 1;
    const int hi = p == E ? nb : Eu[p] / kBlock;
    for (int b = lo; b <= hi; b++) ustart[b] = (int)p;
}

// Runs of a vertex block's contributions outside its u run, each a maximal
// stretch of entries i of one source whose vertex lies in that block:
//   v ends (a = Ev over [0, E), rs = 0): wz[E + i];
//   u ends of a partitioned rank's boundary edges (a = Eu + Eint, rs = Eint - E):
//     wz[Eint + i];
//   received contributions (keys = the halo's recv_keys, rs = E): wz[2E + i];
// vertices >= V (ghosts) belong to no block.  A run is stored as its start
// relative to E (tstart = rs + i: the vertex sweep reads wz[E + tstart + k])
// and its length.
__device__ __forceinline__ int run_block(long i, const int *__restrict__ a,
                                         const unsigned long long *__restrict__ keys, int V) {
    const int x = keys ? (int)(keys[i] >> 32) : a[i];
    return x < V ? x / kBlock : -1;
}
static __global__ void k_tile_runs_count(long n, const int *__restrict__ a,
                                         const unsigned long long *__restrict__ keys, int V,
                                         int *__restrict__ cnt) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = run_block(i, a, keys, V);
    if (b >= 0 && (i == 0 || run_block(i - 1, a, keys, V) != b)) atomicAdd(cnt + b, 1);
}

// each run at its block's next slot (the order of a block's runs does not
// matter: every entry carries its slot), with its length
static __global__ void k_tile_runs_fill(long n, const int *__restrict__ a,
                                        const unsigned long long *__restrict__ keys, int V,
                                        long rs, const int *__restrict__ tptr,
                                        int *__restrict__ fill, int *__restrict__ tstart,
                                        int *__restrict__ tlen) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = run_block(i, a, keys, V);
    if (b < 0 || (i != 0 && run_block(i - 1, a, keys, V) == b)) return;
    long q = i + 1;
    while (q < n && run_block(q, a, keys, V) == b) q++;
    const int j = tptr[b] + atomicAdd(fill + b, 1);
    tstart[j] = (int)(rs + i);
    tlen[j] = (int)(q - i);
}

// tok[b] = 1: block b's list fits the LDS (cap entries), its runs the run
// table, and every degree a byte (deg8, tile_sum)
static __global__ void k_tile_ok(int V, int nb, const int *__restrict__ ptr,
                                 const int *__restrict__ tptr, int cap, int *__restrict__ tok) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const int v0 = b * kBlock, v1 = min(v0 + kBlock, V);
    bool ok = ptr[v1] - ptr[v0] <= cap && tptr[b + 1] - tptr[b] <= kTileRuns;
    for (int v = v0; ok && v < v1; v++) ok = ptr[v + 1] - ptr[v] < 256;
    tok[b] = ok ? 1 : 0;
}

// the per-block records of tile_sum_rec for tiled blocks with at most
// kRecRuns v-end runs (tok 1 -> 2)
static __global__ void k_tile_rec(int nb, const int *__restrict__ ustart,
                                  const int *__restrict__ tptr, const int *__restrict__ tstart,
                                  const int *__restrict__ tlen, int *__restrict__ tok,
                                  int *__restrict__ rec) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const int t0 = tptr[b], nt = tptr[b + 1] - t0;
    int *r = rec + (long)b * kTileRec;
    for (int q = 0; q < kTileRec; q++) r[q] = 0;
    if (!tok[b] || nt > kRecRuns) return;
    r[0] = ustart[b];
    r[1] = ustart[b + 1] - ustart[b];
    r[2] = nt;
    for (int q = 0; q < nt; q++) {
        r[3 + 2 * q] = tstart[t0 + q];
        r[4 + 2 * q] = tlen[t0 + q];
    }
    tok[b] = 2;
}

// hash of run q of record block b (~0: no run / not a record block)
static __global__ void k_run_hash(int nb, long E, const int *__restrict__ tok,
                                  const int *__restrict__ trec, const unsigned short *__restrict__ d2,
                                  unsigned long long *__restrict__ h) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)nb * kPrec) return;
    const int b = (int)(id / kPrec), q = (int)(id - (long)b * kPrec);
    unsigned long long x = ~0ull;
    long A;
    int len;
    if (tok[b] == 2 && rec_run(trec + (long)b * kTileRec, E, q, A, len)) {
        x = 0x9e3779b97f4a7c15ull * (unsigned long long)((A & 7) + 1) ^ (unsigned long long)len << 20;
        for (int i = 0; i < len; i++) {
            x ^= d2[A + i] + 0x9e3779b97f4a7c15ull + (x << 6) + (x >> 2);
            x *= 0xbf58476d1ce4e5b9ull;
        }
        if (x == ~0ull) x = 0;
    }
    h[id] = x;
}

// every run's slots equal those of its pattern's representative, a run of
// the same length (the host's check) at repA (else *bad)
static __global__ void k_run_verify(int nb, long E, const int *__restrict__ tok,
                                    const int *__restrict__ trec,
                                    const unsigned short *__restrict__ d2,
                                    const long long *__restrict__ repA, int *__restrict__ bad) {
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)nb * kPrec) return;
    const int b = (int)(id / kPrec), q = (int)(id - (long)b * kPrec);
    long A;
    int len;
    if (tok[b] != 2 || !rec_run(trec + (long)b * kTileRec, E, q, A, len)) return;
    const long R = repA[id];
    bool ok = R >= 0 && (R & 7) == (A & 7);
    for (int i = 0; ok && i < len; i++) ok = d2[A + i] == d2[R + i];
    if (!ok) atomicAdd(bad, 1);
}

// deg8[v] = the vertex's CSR entries (clamped; blocks with a larger one are
// not tiled)
static __global__ void k_tile_deg(int V, const int *__restrict__ ptr,
                                  unsigned char *__restrict__ deg8) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V) deg8[v] = (unsigned char)min(ptr[v + 1] - ptr[v], 255);
}

// luv[p] = (Eu[p] mod 256) | (Ev[p] mod 256) << 8: both ends within their blocks
static __global__ void k_tile_luv(long E, const int *__restrict__ Eu, const int *__restrict__ Ev,
                                  unsigned short *__restrict__ luv) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < E) luv[p] = (unsigned short)((Eu[p] % kBlock) | ((Ev[p] % kBlock) << 8));
}

// the records of edge blocks [b0, nblk) of EB edges, one wave per block;
// only the block's own record is written
static __global__ void k_tile_erec(long E, int EB, int b0, int nblk, const int *__restrict__ Eu,
                                   const int *__restrict__ Ev, int *__restrict__ erec) {
    const int blk = b0 + blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    if (blk >= nblk) return;  // whole wave
    const long eb = (long)blk * EB, ee = min(eb + EB, E);
    int *r = erec + (long)blk * kErec;
    const int ub0 = Eu[eb] / kBlock;
    bool drop = false;
    for (long p = eb + 1 + lane; p < ee; p += kWave) drop |= Eu[p] / kBlock < Eu[p - 1] / kBlock;
    drop = __ballot(drop) != 0;  // wave-uniform
    int count = 0, umin = 0x7fffffff, umax = -1;
    for (long c = eb; c < ee; c += kWave) {
        const long p = c + lane;
        bool st = false;
        int vb = 0;
        if (p < ee) {
            vb = Ev[p] / kBlock;
            st = p == eb || Ev[p - 1] / kBlock != vb;
            const int u = Eu[p];
            umin = min(umin, u);
            umax = max(umax, u);
            // u blocks ub0 + q starting here (edges sorted by u block: q1 >= q0 >= 0)
            const int q1 = u / kBlock - ub0;
            const int q0 = p == eb ? q1 : Eu[p - 1] / kBlock - ub0;
            if (!drop)
                for (int q = q0 + 1; q <= q1 && q < kErecS - kErecU; q++)
                    r[kErecU + q] = (int)(p - eb);
        }
        const unsigned long long m = __ballot(st);
        const int k = count + __popcll(m & ((1ull << lane) - 1));
        if (st && k < kEbRuns) {
            r[kErecS + 2 * k] = (int)(p - eb);
            r[kErecS + 2 * k + 1] = vb * kBlock;
        }
        count += __popcll(m);
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        umin = min(umin, __shfl_xor(umin, o, kWave));
        umax = max(umax, __shfl_xor(umax, o, kWave));
    }
    const int nub = drop ? kErecNoStage : Eu[ee - 1] / kBlock - ub0 + 1;
    for (int k = count + lane; k < kEbRuns; k += kWave) {  // padding: never reached
        r[kErecS + 2 * k] = 0x7fffffff;
        r[kErecS + 2 * k + 1] = 0;
    }
    if (lane == 0) {
        r[0] = ub0;
        r[1] = nub;
        r[2] = count <= kEbRuns ? count : 0;
        r[3] = umin - ub0 * kBlock;
        r[kErecU] = umax - umin + 1;
        for (int q = drop ? 1 : max(nub, 1); q < kErecS - kErecU; q++) r[kErecU + q] = 0x7fffffff;
    }
}

// entries of each record block's list (0 for the others): the pair sweep's
// LDS list per block is the largest
static __global__ void k_rec_entries(int V, int nb, const int *__restrict__ ptr,
                                     const int *__restrict__ tok, int *__restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    out[b] = tok[b] == 2 ? ptr[min((b + 1) * kBlock, V)] - ptr[b * kBlock] : 0;
}

// ------------------------------------------------ split incidence setup --
// counts edges out of u order or with a u end outside [0, V)
static __global__ void k_u_order_check(long E, int V, const int *__restrict__ Eu,
                                       unsigned long long *__restrict__ bad) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int u = Eu[e];
    if (u < 0 || u >= V || (e + 1 < E && u > Eu[e + 1])) atomicAdd(bad, 1ull);
}

// uptr[v] = first edge whose u end is >= v, v in [0, V] (Eu sorted)
static __global__ void k_uptr(long E, int V, const int *__restrict__ Eu, int *__restrict__ uptr) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > E) return;
    const int lo = e == 0 ? 0 : Eu[e - 1] + 1;
    const int hi = e == E ? V : Eu[e];
    for (int v = lo; v <= hi; v++) uptr[v] = (int)e;
}

// One lane per vertex: code (bit i: the i-th CSR entry is the vertex's next
// own u-run contribution; terminator bit at the degree) and the other
// entries' addresses in CSR order.  blkok[b] = 1 when every vertex of block
// b has <= 31 entries with its u-run in edge order, and the block's runs
// fit the LDS halves (cap).
static __global__ __launch_bounds__(256) void k_split_build(
    int V, long E, const int *__restrict__ ptr, const unsigned *__restrict__ idx,
    const int *__restrict__ uptr, long ototal, unsigned *__restrict__ mask,
    unsigned *__restrict__ oidx, int *__restrict__ blkok, int cap) {
    const int v0 = blockIdx.x * kBlock;
    const int v = v0 + threadIdx.x;
    int ok = 1;
    if (v < V) {
        const int p0 = ptr[v], p1 = ptr[v + 1], u0 = uptr[v], u1 = uptr[v + 1];
        const long o0 = (long)p0 - u0;
        unsigned m = 0u;
        int cu = 0, co = 0;
        if (p1 - p0 > 31) ok = 0;
        for (int j = p0; j < p1; j++) {
            const unsigned id = idx[j];
            if ((long)id < E) {
                if ((long)id != (long)u0 + cu) ok = 0;
                if (j - p0 < 32) m |= 1u << (j - p0);
                cu++;
            } else {
                if (o0 + co >= 0 && o0 + co < ototal) oidx[o0 + co] = id;
                co++;
            }
        }
        if (cu != u1 - u0) ok = 0;
        mask[v] = (p1 - p0 <= 31) ? (m | (1u << (p1 - p0))) : 0u;
    }
    const int all = __syncthreads_and(ok);
    if (threadIdx.x == 0) {
        const int vend = min(v0 + kBlock, V);
        const int nu = uptr[vend] - uptr[v0];
        const int no = (ptr[vend] - uptr[vend]) - (ptr[v0] - uptr[v0]);
        blkok[blockIdx.x] = (all && nu <= cap && no >= 0 && no <= cap) ? 1 : 0;
    }
}

// ------------------------------------------------------------ host build --
void TileLayout::order(long E, int V, int Vg, DevBuf<int> &Eu, DevBuf<int> &Ev,
                       const unsigned *ids, long e_offset, DevBuf<unsigned> &eo, DevBuf<int> &emap,
                       Halo *halo, hipStream_t s) {
    const int nb = grid_for(Vg);
    int vbits = 1;
    while (vbits < 31 && (1L << vbits) < (long)nb) vbits++;
    DevBuf<unsigned long long> k(E), ks(E), nint(1);
    DevBuf<unsigned> v(E), perm(E);
    k_tile_keys<<<grid_for(E), kBlock, 0, s>>>(E, Eu.p, Ev.p, vbits, k.p, v.p, V, halo != nullptr);
    PFDR_HIP(hipGetLastError());
    radix_sort_pairs_stable<unsigned long long>(k.p, ks.p, v.p, perm.p, E,
                                                2 * vbits + (halo ? 1 : 0), s);
    if (halo) k_count_below<<<1, 1, 0, s>>>(E, ks.p, 1ull << (2 * vbits), nint.p);
    DevBuf<int> nu(E), nv(E);
    DevBuf<unsigned> neo(E), inv(halo ? E : 0);
    emap.alloc(E);
    k_edge_tile_order<<<grid_for(E), kBlock, 0, s>>>(E, perm.p, ids, e_offset, Eu.p, Ev.p, nu.p,
                                                     nv.p, neo.p, emap.p, inv.p);
    const long np = halo ? halo->push_send_off.back() : 0;
    if (np) k_remap_push<<<grid_for(np), kBlock, 0, s>>>(np, E, inv.p, halo->push_addr.p);
    PFDR_HIP(hipGetLastError());
    unsigned long long ni = E;
    if (halo) PFDR_HIP(hipMemcpyAsync(&ni, nint.p, sizeof(ni), hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
    Eint = (long)ni;
    std::swap(Eu.p, nu.p);
    std::swap(Ev.p, nv.p);
    std::swap(eo.p, neo.p);  // (ids may be eo's old block: freed on return)
    std::swap(eo.n, neo.n);
}

void TileLayout::build(long E, int V, const int *Eu, const int *Ev, const Incidence &inc,
                       const Halo *halo, size_t elem, hipStream_t s) {
    const long R = halo ? halo->R : 0, n = 2 * E + R, ng = n / kSlotGroup + 1;  // (+1: whole groups)
    DevBuf<unsigned short> d2(n);
    k_tile_slots<<<grid_for(V), kBlock, 0, s>>>(V, inc.ptr.p, inc.idx.p, d2.p);
    slots.alloc(ng);
    k_pack_slots<<<grid_for(ng), kBlock, 0, s>>>(ng, n, d2.p, slots.p);
    PFDR_HIP(hipGetLastError());
    // the record and run tables of the tiled blocks
    const int nb = grid_for(V);
    luv.alloc((size_t)E);
    k_tile_luv<<<grid_for(E), kBlock, 0, s>>>(E, Eu, Ev, luv.p);
    const int EB = kBlock * (int)(16 / elem);  // edges per k_edge_sweep_tl block
    const int neb = (int)((E + EB - 1) / EB);
    erec.alloc((size_t)neb * kErec);
    k_tile_erec<<<(neb + kBlock / kWave - 1) / (kBlock / kWave), kBlock, 0, s>>>(E, EB, 0, neb, Eu,
                                                                                 Ev, erec.p);
    PFDR_HIP(hipGetLastError());
    ustart.alloc((size_t)nb + 1);
    // u runs: the interior edges (sorted by u block); a partitioned rank's
    // boundary edges [Eint, E) add their owned u ends as runs, its received
    // contributions theirs (k_tile_runs_count)
    k_tile_ustart<<<grid_for(Eint + 1), kBlock, 0, s>>>(Eint, nb, Eu, ustart.p);
    DevBuf<int> cnt(nb), fill(nb);
    PFDR_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int) * nb, s));
    PFDR_HIP(hipMemsetAsync(fill.p, 0, sizeof(int) * nb, s));
    struct Src { long n; const int *a; const unsigned long long *keys; long rs; };
    const Src src[3] = {{E, Ev, nullptr, 0},
                        {E - Eint, Eu + Eint, nullptr, Eint - E},
                        {R, nullptr, halo ? halo->recv_keys.p : nullptr, E}};
    for (const Src &q : src)
        if (q.n > 0) k_tile_runs_count<<<grid_for(q.n), kBlock, 0, s>>>(q.n, q.a, q.keys, V, cnt.p);
    PFDR_HIP(hipGetLastError());
    std::vector<int> h(nb), tp((size_t)nb + 1, 0);
    PFDR_HIP(hipMemcpyAsync(h.data(), cnt.p, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
    for (int b = 0; b < nb; b++) tp[b + 1] = tp[b] + h[b];
    const int nruns = tp[nb];
    tptr.alloc((size_t)nb + 1);
    PFDR_HIP(hipMemcpyAsync(tptr.p, tp.data(), sizeof(int) * (nb + 1), hipMemcpyHostToDevice, s));
    tstart.alloc(nruns ? nruns : 1);
    tlen.alloc(nruns ? nruns : 1);
    for (const Src &q : src)
        if (q.n > 0)
            k_tile_runs_fill<<<grid_for(q.n), kBlock, 0, s>>>(q.n, q.a, q.keys, V, q.rs, tptr.p,
                                                              fill.p, tstart.p, tlen.p);
    tok.alloc(nb);
    k_tile_ok<<<grid_for(nb), kBlock, 0, s>>>(V, nb, inc.ptr.p, tptr.p, kTileCap, tok.p);
    trec.alloc((size_t)nb * kTileRec);
    k_tile_rec<<<grid_for(nb), kBlock, 0, s>>>(nb, ustart.p, tptr.p, tstart.p, tlen.p, tok.p,
                                               trec.p);
    deg8.alloc(V);
    k_tile_deg<<<grid_for(V), kBlock, 0, s>>>(V, inc.ptr.p, deg8.p);
    PFDR_HIP(hipGetLastError());
    PFDR_HIP(hipMemcpyAsync(h.data(), tok.p, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
    for (int x : h) {
        tiled_blocks += x != 0;
        record_blocks += x == 2;
    }
    // the pair vertex sweep (k_vertex_sweep_pair): f32 sessions whose every
    // block is a record block, when two blocks' lists still leave LDS for
    // seven workgroups per CU (the kernel's seven waves per SIMD): C5 (6
    // entries per vertex) vertex sweep 3.15-3.22 -> 2.83-2.85 ms, C2 -2 %;
    // the headline's 12 per vertex would halve the resident workgroups
    // (0.174 -> 0.226 ms, f6j), so it keeps the one-block sweep.
    // PFDR_VPAIR=0: the one-block sweep throughout
    const char *e = getenv("PFDR_VPAIR");
    if (elem == 4 && record_blocks == nb && !(e && e[0] == '0')) {
        DevBuf<int> ent(nb);
        k_rec_entries<<<grid_for(nb), kBlock, 0, s>>>(V, nb, inc.ptr.p, tok.p, ent.p);
        PFDR_HIP(hipGetLastError());
        PFDR_HIP(hipMemcpyAsync(h.data(), ent.p, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
        const int cap = std::max(1, *std::max_element(h.begin(), h.end()));
        const size_t per_wg = 2 * (size_t)cap * elem + 2048;  // (+ the static arrays)
        if (per_wg * 7 <= 160 * 1024) vpair_cap = cap;
    }
    build_patterns(E, V, d2.p, n, s);
}  // (d2's block is reused only once the stream is idle, dev_free)

// the pattern table of the record blocks' runs, when they repeat
void TileLayout::build_patterns(long E, int V, const unsigned short *d2, long n, hipStream_t s) {
    const char *e = getenv("PFDR_TILE_PATTERNS");
    if ((e && e[0] == '0') || !record_blocks) return;
    const int nb = grid_for(V);
    const long nr = (long)nb * kPrec;
    std::vector<unsigned long long> hh(nr);
    std::vector<int> rec((size_t)nb * kTileRec);
    {
        DevBuf<unsigned long long> h(nr);
        k_run_hash<<<grid_for(nr), kBlock, 0, s>>>(nb, E, tok.p, trec.p, d2, h.p);
        PFDR_HIP(hipGetLastError());
        PFDR_HIP(hipMemcpyAsync(hh.data(), h.p, sizeof(unsigned long long) * nr,
                                hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipMemcpyAsync(rec.data(), trec.p, sizeof(int) * rec.size(),
                                hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
    }
    constexpr size_t kMaxPatterns = 65536;
    std::unordered_map<unsigned long long, int> pat;
    std::vector<long> pA;
    std::vector<int> pLen, pOff, prc(nr, 0);
    std::vector<long long> repA(nr, -1);
    long groups = 0;
    for (long id = 0; id < nr; id++) {
        if (hh[id] == ~0ull) continue;
        long A;
        int len;
        rec_run(&rec[(size_t)(id / kPrec) * kTileRec], E, (int)(id % kPrec), A, len);
        auto it = pat.find(hh[id]);
        int pi;
        if (it == pat.end()) {
            pi = (int)pA.size();
            pat.emplace(hh[id], pi);
            pA.push_back(A);
            pLen.push_back(len);
            pOff.push_back((int)groups);
            groups += ((A & 7) + len + 7) / 8;
            if (pat.size() > kMaxPatterns || groups * kSlotGroup > n / 4) return;  // no repeats
        } else {
            pi = it->second;
            // (a collision of unlike runs: k_run_verify would read past the shorter)
            if (len != pLen[pi] || ((A ^ pA[pi]) & 7)) return;
        }
        prc[id] = pOff[pi];
        repA[id] = pA[pi];
    }
    if (!groups) return;
    {   // same hash, same slots: checked entry by entry on the device
        DevBuf<long long> dr(nr);
        DevBuf<int> bad(1);
        PFDR_HIP(hipMemcpyAsync(dr.p, repA.data(), sizeof(long long) * nr, hipMemcpyHostToDevice, s));
        PFDR_HIP(hipMemsetAsync(bad.p, 0, sizeof(int), s));
        k_run_verify<<<grid_for(nr), kBlock, 0, s>>>(nb, E, tok.p, trec.p, d2, dr.p, bad.p);
        PFDR_HIP(hipGetLastError());
        int hb = 1;
        PFDR_HIP(hipMemcpyAsync(&hb, bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
        if (hb) return;
    }
    // the table: each pattern's groups packed from its representative's
    // slots (entries outside the run are 0)
    std::vector<Slots12> tab((size_t)groups);
    std::vector<unsigned short> sl;
    for (size_t pi = 0; pi < pA.size(); pi++) {
        const long A = pA[pi], g0 = A / kSlotGroup;
        const int len = pLen[pi];
        const long gn = ((A & 7) + len + 7) / 8;
        if (!gn) continue;
        sl.assign((size_t)gn * kSlotGroup, 0);
        PFDR_HIP(hipMemcpy(sl.data() + (A - g0 * kSlotGroup), d2 + A, sizeof(unsigned short) * len,
                           hipMemcpyDeviceToHost));
        for (long g = 0; g < gn; g++)
            tab[(size_t)pOff[pi] + g] = pack_slots12(&sl[(size_t)g * kSlotGroup], kSlotGroup);
    }
    ptab.alloc((size_t)groups);
    prec.alloc((size_t)nr);
    PFDR_HIP(hipMemcpyAsync(ptab.p, tab.data(), sizeof(Slots12) * groups, hipMemcpyHostToDevice, s));
    PFDR_HIP(hipMemcpyAsync(prec.p, prc.data(), sizeof(int) * nr, hipMemcpyHostToDevice, s));
    PFDR_HIP(hipStreamSynchronize(s));
    slot_patterns = (long)pA.size();
}

// when the edges are sorted by their u end (natural emission order,
// relabelled sessions), each vertex's u-end contributions are a contiguous
// run of wz and need no address
void SplitLayout::build(long E, int V, const int *Eu, const Incidence &inc, int cap,
                        hipStream_t s) {
    if (!E) return;
    DevBuf<unsigned long long> bad(1);
    PFDR_HIP(hipMemsetAsync(bad.p, 0, sizeof(unsigned long long), s));
    k_u_order_check<<<grid_for(E), kBlock, 0, s>>>(E, V, Eu, bad.p);
    PFDR_HIP(hipGetLastError());
    unsigned long long nbad = 0;
    PFDR_HIP(hipMemcpyAsync(&nbad, bad.p, sizeof(nbad), hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
    if (nbad) return;
    const int nb = grid_for(V);
    const long ototal = inc.n - E;  // every local edge's u end is an owned row
    if (ototal < 0) return;
    uptr.alloc((size_t)V + 1);
    k_uptr<<<grid_for(E + 1), kBlock, 0, s>>>(E, V, Eu, uptr.p);
    PFDR_HIP(hipGetLastError());
    mask.alloc(V);
    oidx.alloc(ototal ? ototal : 1);
    blkok.alloc(nb);
    k_split_build<<<nb, kBlock, 0, s>>>(V, E, inc.ptr.p, inc.idx.p, uptr.p, ototal, mask.p, oidx.p,
                                        blkok.p, cap);
    PFDR_HIP(hipGetLastError());
    std::vector<int> h(nb);
    PFDR_HIP(hipMemcpyAsync(h.data(), blkok.p, nb * sizeof(int), hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
    for (int x : h) split_blocks += x;
    if (!split_blocks) { mask.release(); oidx.release(); blkok.release(); }  // uptr serves the edge sweep
}

}  // namespace pfdr

// Test hook (pfdr_mi355x.h, "debug"): the edge-block records of
// k_edge_sweep_tl for host arrays; only blocks [blk_begin, blk_begin +
// blk_count) are built, every other record keeps the caller's contents.
extern "C" int pfdr_debug_tile_erec(int64_t E, int dtype, const int *Eu, const int *Ev,
                                    int blk_begin, int blk_count, int *rec, int64_t rec_ints) {
    using namespace pfdr;
    const char *fn = "pfdr_debug_tile_erec";
    try {
        if (E <= 0 || !Eu || !Ev || !rec || (dtype != PFDR_F32 && dtype != PFDR_F64))
            return report_error(fn, "invalid argument");
        const int EB = kBlock * (dtype == PFDR_F32 ? Vec<float>::kPer16B : Vec<double>::kPer16B);
        const long neb = (E + EB - 1) / EB;
        if (rec_ints != neb * kErec || blk_begin < 0 || blk_count < 0 || blk_begin + blk_count > neb)
            return report_error(fn, "record array or block range does not match E");
        hipStream_t s = lib_stream();
        DevBuf<int> dEu(E), dEv(E), dr(rec_ints);
        PFDR_HIP(hipMemcpyAsync(dEu.p, Eu, E * 4, hipMemcpyHostToDevice, s));
        PFDR_HIP(hipMemcpyAsync(dEv.p, Ev, E * 4, hipMemcpyHostToDevice, s));
        PFDR_HIP(hipMemcpyAsync(dr.p, rec, rec_ints * 4, hipMemcpyHostToDevice, s));
        if (blk_count) {
            const int wpb = kBlock / kWave;
            k_tile_erec<<<(blk_count + wpb - 1) / wpb, kBlock, 0, s>>>(
                E, EB, blk_begin, blk_begin + blk_count, dEu.p, dEv.p, dr.p);
            PFDR_HIP(hipGetLastError());
        }
        PFDR_HIP(hipMemcpyAsync(rec, dr.p, rec_ints * 4, hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
    } catch (const HipError &h) {
        return report_error(fn, h);
    } catch (const std::exception &ex) {
        return report_error(fn, ex.what());
    }
    return PFDR_OK;
}

// the record layout the hook writes: ints per record, v runs per record,
// nub of an unstaged (u-block drop) block
extern "C" int pfdr_debug_erec_layout(int *ints, int *runs, int *nostage) {
    if (ints) *ints = pfdr::kErec;
    if (runs) *runs = pfdr::kEbRuns;
    if (nostage) *nostage = pfdr::kErecNoStage;
    return PFDR_OK;
}
