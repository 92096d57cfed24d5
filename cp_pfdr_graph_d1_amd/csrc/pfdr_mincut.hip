// Minimum cut of a cut-pursuit step on the GPU: the steepest cut the
// reference takes with Boykov-Kolmogorov's sequential maxflow
// (include/graph.hpp), here by synchronous push-relabel on the
// device-resident graph.
//
// Which cut.  The reference labels a vertex SOURCE when it is in BK's source
// tree at termination and everything else SINK (what_segment's default,
// include/graph.hpp:131): the set reachable from the source in the residual
// graph, the smallest source side, the same for every maximum flow.  The
// first phase of push-relabel yields the nodes that can reach the
// preflow's SINK in the residual graph.  So the preflow runs on the reversed
// network: its source is the cut's sink, every arc is turned round, and "can
// reach the preflow's sink" reads "reachable from the cut's source".  Run
// forward, the first phase would give the largest source side instead.
// Nodes whose height reaches V keep their excess (no second phase).
//
// State, per node: a signed excess ex[v] = -tr_cap[v] at the start.  A
// negative excess is the unused capacity of the node's arc to the preflow's
// sink: such a node has height 0 and absorbs what is pushed into it; an
// infinite terminal never changes (only finite amounts are added to it).
// Per incidence slot a = 2e + side: the residual of the arc tail(a) ->
// head(a) of the reversed network; the reverse arc is slot a ^ 1.
//
// One round is two kernels and uses no atomics on reals, so every run gives
// the same bits:
//   push    every active node (ex > 0, height < V) walks its out-arcs in
//           incidence order against a snapshot of heights, residuals and its
//           own excess and stores delta[a] = min(remaining, residual) on the
//           admissible ones; each slot is written by its tail only
//   apply   every node updates its own residuals and excess from its deltas
//           and its neighbours' (out first, then in, in incidence order);
//           a node that was active and pushed nothing is relabelled from the
//           residuals AFTER this round's pushes (a push v -> u of the same
//           round opens u -> v; missing it makes the labelling invalid) and
//           the snapshot heights, into the other height buffer
// Every so many rounds, and at the start, the heights are set to the exact
// distances by a level-synchronous breadth-first search from the nodes with
// negative excess; unreached nodes get height V and drop out for good.  The
// last such search, run when no active node is left, is the answer.
//
// The duplex driver's two-layer cut (mincut_duplex) runs the same rounds over
// a CSR of 2V nodes: only the residuals' initialisation and the cut's value
// know the edge classes (layer edges with both arcs, one-way links).
#include <climits>
#include <stdexcept>

#include "pfdr_mincut.hpp"

namespace pfdr {

namespace {

constexpr int kUnset = INT_MAX;
constexpr int kCutGrid = 1024;

struct McCtl {
    int bfs_last;  // last breadth-first level that labelled a node
    int any;       // after a global relabel: an active node exists
    int act;       // last round after which an active node existed
    int bad;       // invalid capacities
};

__device__ __forceinline__ int ld_relaxed(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void k_mc_nbr(long n, const unsigned *__restrict__ idx, const int *__restrict__ Eu,
                         const int *__restrict__ Ev, int *__restrict__ nbr) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n;
         p += (long)gridDim.x * blockDim.x) {
        const unsigned a = idx[p];
        nbr[p] = (a & 1u) ? Eu[a >> 1] : Ev[a >> 1];
    }
}

// the two-layer network's edge list: e and E + e (endpoints + V) for edge e,
// 2E + v for the link (v, V + v)
__global__ void k_mc_duplex_edges(int V, long E, const int *__restrict__ Eu,
                                  const int *__restrict__ Ev, int *__restrict__ u,
                                  int *__restrict__ v) {
    const long m = max((long)V, E);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < m;
         i += (long)gridDim.x * blockDim.x) {
        if (i < E) {
            const int a = Eu[i], b = Ev[i];
            u[i] = a;
            v[i] = b;
            u[E + i] = V + a;
            v[E + i] = V + b;
        }
        if (i < V) {
            u[2 * E + i] = (int)i;
            v[2 * E + i] = V + (int)i;
        }
    }
}

// ex = -tr_cap; residuals of the reversed network: both slots r_cap[e], or
// (forward arcs Eu -> Ev only) slot 2e + 1 alone.  n nodes, E edges with a
// capacity.  Two layers (L > 0 link arcs, n = 2L): edge e has r_cap[e] on both
// slots of edge ids e and E + e, link v (edge id 2E + v, arc v -> L + v) has
// r_link[v] on its reversed-network slot only.
template <typename real>
__global__ void k_mc_init(int n, long E, int both, int L, const real *__restrict__ tr,
                          const real *__restrict__ rc, const real *__restrict__ link,
                          real *__restrict__ ex, real *__restrict__ res,
                          int *__restrict__ pushed, McCtl *ctl) {
    int b = 0;
    const long m = max((long)n, E);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < m;
         i += (long)gridDim.x * blockDim.x) {
        if (i < n) {
            const real t = tr[i];
            if (t != t) b = 1;
            ex[i] = -t;
            pushed[i] = 0;
        }
        if (i < E) {
            const real c = rc[i];
            if (!(c >= real(0) && c < Lim<real>::huge)) b = 1;
            Pk<real, 2> r;
            r.v[0] = both ? c : real(0);
            r.v[1] = c;
            *reinterpret_cast<Pk<real, 2> *>(res + 2 * i) = r;
            if (L > 0) *reinterpret_cast<Pk<real, 2> *>(res + 2 * (E + i)) = r;
        }
        if (i < L) {
            const real c = link[i];
            if (!(c >= real(0) && c < Lim<real>::huge)) b = 1;
            Pk<real, 2> r;
            r.v[0] = real(0);
            r.v[1] = c;
            *reinterpret_cast<Pk<real, 2> *>(res + 2 * (2 * E + i)) = r;
        }
    }
    if (__syncthreads_or(b) && threadIdx.x == 0) atomicOr(&ctl->bad, 1);
}

// ---- global relabel: heights = distances to the nodes of negative excess
template <typename real>
__global__ void k_mc_bfs_init(int V, const real *__restrict__ ex, int *__restrict__ h,
                              McCtl *ctl) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0) {
        ctl->bfs_last = -1;
        ctl->any = 0;
    }
    if (v < V) h[v] = ex[v] < real(0) ? 0 : kUnset;
}

// level l: an unlabelled node with a residual arc into a node of height l
// takes height l + 1.  A neighbour labelled by this very launch holds l + 1
// or kUnset, neither equal to l, so the result does not depend on timing.
template <typename real>
__global__ void k_mc_bfs_level(int V, int l, const int *__restrict__ ptr,
                               const unsigned *__restrict__ idx, const int *__restrict__ nbr,
                               const real *__restrict__ res, int *h, McCtl *ctl) {
    if (ld_relaxed(&ctl->bfs_last) < l - 1) return;  // the search has ended
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    int lab = 0;
    if (v < V && ld_relaxed(h + v) == kUnset) {
        const int p1 = ptr[v + 1];
        for (int p = ptr[v]; p < p1; p++) {
            if (ld_relaxed(h + nbr[p]) != l) continue;
            if (res[idx[p]] > real(0)) {
                lab = 1;
                break;
            }
        }
        if (lab) h[v] = l + 1;
    }
    if (__syncthreads_or(lab) && threadIdx.x == 0) atomicMax(&ctl->bfs_last, l);
}

template <typename real>
__global__ void k_mc_bfs_final(int V, const real *__restrict__ ex, int *__restrict__ h,
                               McCtl *ctl) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    int a = 0;
    if (v < V) {
        int hv = h[v];
        if (hv == kUnset) h[v] = hv = V;
        a = ex[v] > real(0) && hv < V;
    }
    if (__syncthreads_or(a) && threadIdx.x == 0) atomicOr(&ctl->any, 1);
}

// ---- one round
template <typename real>
__global__ void k_mc_push(int V, int R, const int *__restrict__ ptr,
                          const unsigned *__restrict__ idx, const int *__restrict__ nbr,
                          const real *__restrict__ ex, const int *__restrict__ h,
                          const real *__restrict__ res, real *__restrict__ delta,
                          int *__restrict__ pushed, const McCtl *ctl) {
    if (ld_relaxed(&ctl->act) < R - 1) return;  // no active node is left
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= V) return;
    real rem = ex[u];
    const int hu = h[u];
    if (!(rem > real(0)) || hu >= V) return;
    const int p0 = ptr[u], p1 = ptr[u + 1];
    bool any = false;
    for (int p = p0; p < p1; p++) {
        const unsigned a = idx[p];
        real d = real(0);
        if (rem > real(0) && h[nbr[p]] + 1 == hu) {
            const real r = res[a];
            if (r > real(0)) {
                d = rem < r ? rem : r;
                rem -= d;  // rem - rem = 0 exactly; an infinite excess stays infinite
                any = true;
            }
        }
        delta[a] = d;
    }
    if (any) pushed[u] = R;
}

template <typename real>
__global__ void k_mc_apply(int V, int R, const int *__restrict__ ptr,
                           const unsigned *__restrict__ idx, const int *__restrict__ nbr,
                           real *__restrict__ ex, const int *__restrict__ hA,
                           int *__restrict__ hB, real *__restrict__ res,
                           const real *__restrict__ delta, const int *__restrict__ pushed,
                           McCtl *ctl) {
    if (ld_relaxed(&ctl->act) < R - 1) return;
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    int still = 0;
    if (u < V) {
        const real e = ex[u];
        const int hu = hA[u];
        const bool was = e > real(0) && hu < V;
        const bool did = pushed[u] == R;
        const bool lift = was && !did;
        real eo = e, in = real(0);
        int hm = INT_MAX;
        bool moved = false;
        const int p1 = ptr[u + 1];
        for (int p = ptr[u]; p < p1; p++) {
            const int v = nbr[p];
            const bool vin = pushed[v] == R;
            if (!did && !vin && !lift) continue;
            const unsigned a = idx[p];
            const real o = did ? delta[a] : real(0);
            const real i = vin ? delta[a ^ 1u] : real(0);
            real r = res[a];
            // an edge carries flow one way per round (the heights differ by
            // one either way), so at most one of o, i is nonzero
            if (o > real(0)) {
                r -= o;  // o <= r: stays >= 0
                eo -= o;
                res[a] = r;
                moved = true;
            } else if (i > real(0)) {
                r += i;
                in += i;
                res[a] = r;
                moved = true;
            }
            if (lift && r > real(0)) hm = min(hm, hA[v] + 1);
        }
        int hn = hu;
        if (lift) hn = min(hm, V);
        hB[u] = hn;
        real en = e;
        if (moved) {
            en = eo + in;
            ex[u] = en;
        }
        still = en > real(0) && hn < V;
    }
    if (__syncthreads_or(still) && threadIdx.x == 0) atomicMax(&ctl->act, R);
}

// ---- the answer
__global__ void k_mc_segment(int V, const int *__restrict__ h, uint8_t *__restrict__ seg) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V) seg[v] = h[v] < V ? 0 : 1;
}

// value of the cut (SOURCE = 0 -> SINK = 1 arcs of the original network) in
// f64: per-thread sums over a fixed grid, a fixed tree per block, the block
// sums stored and added in order.  Two layers (L > 0, n = 2L): the n
// terminals, every edge once per layer, then the links.
template <typename real>
__global__ __launch_bounds__(kBlock) void k_mc_cut(int n, long E, int both, int L,
                                                  const real *__restrict__ tr,
                                                  const real *__restrict__ rc,
                                                  const real *__restrict__ link,
                                                  const int *__restrict__ Eu,
                                                  const int *__restrict__ Ev,
                                                  const uint8_t *__restrict__ seg,
                                                  double *__restrict__ part) {
    __shared__ double lds[kBlock / kWave];
    double c = 0;
    const long m = (long)n + E + L;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < m;
         i += (long)gridDim.x * blockDim.x) {
        if (i < n) {
            const real t = tr[i];
            if (seg[i]) {
                if (t > real(0)) c += (double)t;
            } else if (t < real(0)) {
                c -= (double)t;
            }
        } else if (i < n + E) {
            const long e = i - n;
            const int u = Eu[e], v = Ev[e];
            const int su = seg[u], sv = seg[v];
            if (su != sv && (both || su == 0)) c += (double)rc[e];
            if (L > 0 && seg[L + u] != seg[L + v]) c += (double)rc[e];
        } else {
            const long v = i - n - E;
            if (seg[v] == 0 && seg[L + v] != 0) c += (double)link[v];
        }
    }
    c = block_sum(c, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = c;
}

__global__ void k_mc_cut_sum(int n, const double *__restrict__ part, double *__restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0;
        for (int i = 0; i < n; i++) s += part[i];
        *out = s;
    }
}

}  // namespace

// The rounds over a CSR of n nodes and Et edges (2 Et slots).  One layer
// (L = 0): n = V, Et = E.  Two layers: n = 2L, Et = 2E + L.
template <typename real>
static void run_cut(int n, long E, int L, const Incidence &inc, const int *nbr, const int *Eu,
                    const int *Ev, int both, const real *tr, const real *rc, const real *link,
                    uint8_t *seg, MincutStats &st, hipStream_t s) {
    const int V = n;  // the nodes of the network
    const long Et = L > 0 ? 2 * E + L : E;
    const long n2 = 2 * Et;
    const int gv = grid_for(V);
    DevBuf<real> ex(V), res(n2 > 0 ? n2 : 2), delta(n2 > 0 ? n2 : 2);
    DevBuf<int> hA(V), hB(V), pushed(V);
    DevBuf<McCtl> ctl(1);
    DevBuf<double> part(kCutGrid + 1);
    PinnedSmall pin(s);
    McCtl *hc = static_cast<McCtl *>(pin.p);
    auto poll = [&]() {
        PFDR_HIP(hipMemcpyAsync(hc, ctl.p, sizeof(McCtl), hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
    };

    PFDR_HIP(hipMemsetAsync(ctl.p, 0, sizeof(McCtl), s));
    k_mc_init<real><<<std::min(grid_for(std::max((long)V, E)), 8192), kBlock, 0, s>>>(
        V, E, both, L, tr, rc, link, ex.p, res.p, pushed.p, ctl.p);
    PFDR_HIP(hipGetLastError());
    poll();
    if (hc->bad)
        throw std::invalid_argument(
            L > 0 ? "mincut_duplex: tr_cap must not be NaN, r_cap and r_link must be finite "
                    "and >= 0"
                  : "mincut: tr_cap must not be NaN, r_cap must be finite and >= 0");

    // exact heights into hA; returns the number of levels that labelled
    auto relabel = [&]() {
        k_mc_bfs_init<real><<<gv, kBlock, 0, s>>>(V, ex.p, hA.p, ctl.p);
        int depth = 0;
        if (Et > 0) {
            int l = 0;
            for (int batch = 16;; batch = 64) {
                for (int i = 0; i < batch; i++, l++)
                    k_mc_bfs_level<real><<<gv, kBlock, 0, s>>>(V, l, inc.ptr.p, inc.idx.p, nbr,
                                                               res.p, hA.p, ctl.p);
                PFDR_HIP(hipGetLastError());
                poll();
                if (hc->bfs_last < l - 1) break;
                if (l > V) throw std::runtime_error("mincut: breadth-first search did not end");
            }
            depth = hc->bfs_last + 1;
        }
        k_mc_bfs_final<real><<<gv, kBlock, 0, s>>>(V, ex.p, hA.p, ctl.p);
        PFDR_HIP(hipGetLastError());
        poll();
        st.relabels++;
        return depth;
    };

    st = MincutStats();
    int R = 0;  // rounds enqueued
    int depth = relabel();
    // heights rise monotonically and are bounded by V: the rounds end; the
    // limit only guards the loop
    const long limit = std::max(1L << 22, 64L * V);
    while (hc->any) {
        // period of the global relabel: the depth of the last one, within
        // [kMinPeriod, kMaxPeriod], even (the heights end in hA)
        constexpr int kMinPeriod = 16, kMaxPeriod = 512;
        const int P = std::min(kMaxPeriod, std::max(kMinPeriod, depth + (depth & 1)));
        const int R0 = R;
        // act = R0: round R0 + 1 runs
        PFDR_HIP(hipMemcpyAsync(&ctl.p->act, &R0, sizeof(int), hipMemcpyHostToDevice, s));
        for (int i = 0; i < P; i += 2) {
            k_mc_push<real><<<gv, kBlock, 0, s>>>(V, R + 1, inc.ptr.p, inc.idx.p, nbr, ex.p,
                                                  hA.p, res.p, delta.p, pushed.p, ctl.p);
            k_mc_apply<real><<<gv, kBlock, 0, s>>>(V, R + 1, inc.ptr.p, inc.idx.p, nbr, ex.p,
                                                   hA.p, hB.p, res.p, delta.p, pushed.p, ctl.p);
            k_mc_push<real><<<gv, kBlock, 0, s>>>(V, R + 2, inc.ptr.p, inc.idx.p, nbr, ex.p,
                                                  hB.p, res.p, delta.p, pushed.p, ctl.p);
            k_mc_apply<real><<<gv, kBlock, 0, s>>>(V, R + 2, inc.ptr.p, inc.idx.p, nbr, ex.p,
                                                   hB.p, hA.p, res.p, delta.p, pushed.p, ctl.p);
            R += 2;
        }
        PFDR_HIP(hipGetLastError());
        depth = relabel();  // polls: hc->act is the batch's
        st.rounds += std::min(hc->act + 1, R) - R0;
        if (R > limit) throw std::runtime_error("mincut: push-relabel did not end");
    }

    k_mc_segment<<<gv, kBlock, 0, s>>>(V, hA.p, seg);
    k_mc_cut<real><<<kCutGrid, kBlock, 0, s>>>(V, E, both, L, tr, rc, link, Eu, Ev, seg, part.p);
    k_mc_cut_sum<<<1, kWave, 0, s>>>(kCutGrid, part.p, part.p + kCutGrid);
    PFDR_HIP(hipGetLastError());
    double *hf = reinterpret_cast<double *>(hc);
    PFDR_HIP(hipMemcpyAsync(hf, part.p + kCutGrid, sizeof(double), hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
    st.flow = *hf;
}

template <typename real>
void mincut(int V, long E, const Incidence &inc, const int *Eu, const int *Ev, DevBuf<int> &nbr,
            int arcs, const real *tr, const real *rc, uint8_t *seg, MincutStats &st,
            hipStream_t s) {
    const long n2 = 2 * E;
    if (E > 0 && nbr.n != (size_t)n2) {
        nbr.alloc(n2);
        k_mc_nbr<<<std::min(grid_for(n2), 8192), kBlock, 0, s>>>(n2, inc.idx.p, Eu, Ev, nbr.p);
        PFDR_HIP(hipGetLastError());
    }
    run_cut<real>(V, E, 0, inc, nbr.p, Eu, Ev, arcs == PFDR_ARCS_BOTH, tr, rc, nullptr, seg, st,
                  s);
}

void DuplexNet::build(int V, long E, const int *Eu, const int *Ev, hipStream_t s) {
    const long Et = 2 * E + V;
    if (2 * Et > (long)INT_MAX)
        throw std::invalid_argument(
            "mincut_duplex: 2 (2E + V) incidence slots do not fit the CSR's int offsets");
    DevBuf<int> u(Et), v(Et);
    k_mc_duplex_edges<<<std::min(grid_for(std::max((long)V, E)), 8192), kBlock, 0, s>>>(
        V, E, Eu, Ev, u.p, v.p);
    PFDR_HIP(hipGetLastError());
    build_incidence(u.p, v.p, 2 * V, Et, inc, s);
    nbr.alloc(2 * Et);
    k_mc_nbr<<<std::min(grid_for(2 * Et), 8192), kBlock, 0, s>>>(2 * Et, inc.idx.p, u.p, v.p,
                                                                 nbr.p);
    PFDR_HIP(hipGetLastError());
    PFDR_HIP(hipStreamSynchronize(s));  // u, v leave scope
    built = true;
}

template <typename real>
void mincut_duplex(int V, long E, DuplexNet &net, const int *Eu, const int *Ev, const real *tr,
                   const real *link, const real *rc, uint8_t *seg, MincutStats &st,
                   hipStream_t s) {
    if (!net.built) net.build(V, E, Eu, Ev, s);
    run_cut<real>(2 * V, E, V, net.inc, net.nbr.p, Eu, Ev, 1, tr, rc, link, seg, st, s);
}

template void mincut<float>(int, long, const Incidence &, const int *, const int *,
                            DevBuf<int> &, int, const float *, const float *, uint8_t *,
                            MincutStats &, hipStream_t);
template void mincut<double>(int, long, const Incidence &, const int *, const int *,
                             DevBuf<int> &, int, const double *, const double *, uint8_t *,
                             MincutStats &, hipStream_t);
template void mincut_duplex<float>(int, long, DuplexNet &, const int *, const int *,
                                   const float *, const float *, const float *, uint8_t *,
                                   MincutStats &, hipStream_t);
template void mincut_duplex<double>(int, long, DuplexNet &, const int *, const int *,
                                    const double *, const double *, const double *, uint8_t *,
                                    MincutStats &, hipStream_t);

}  // namespace pfdr
