// Minimum cut on the device-resident cut-pursuit graph (see pfdr_mincut.hip).
#pragma once
#include "pfdr_graph.hpp"

namespace pfdr {

struct MincutStats {
    double flow = 0;    // value of the returned cut, summed in f64
    long rounds = 0;    // push / relabel rounds run
    long relabels = 0;  // global relabels (breadth-first labellings), the final one included
};

// segment[v] = 0 (SOURCE) when v is reachable from the source in the residual
// graph of a maximum flow, else 1 (SINK).  All pointers are device memory;
// nbr[2E] caches the head of every incidence position (filled when empty).
// Throws std::invalid_argument on a NaN terminal or a negative / non-finite
// edge capacity.
template <typename real>
void mincut(int V, long E, const Incidence &inc, const int *Eu, const int *Ev, DevBuf<int> &nbr,
            int arcs, const real *tr_cap, const real *r_cap, uint8_t *segment, MincutStats &st,
            hipStream_t s);

// The duplex driver's two-layer network as a CSR over 2V nodes (node v and
// node V + v per vertex): edge ids e (layer 1), E + e (layer 2, endpoints + V)
// and 2E + v (the link v -> V + v), slot = 2 edge + side.  Built on the first
// two-layer cut of a graph and kept with it.
struct DuplexNet {
    Incidence inc;
    DevBuf<int> nbr;
    bool built = false;
    // Throws std::invalid_argument when 2 (2E + V) slots do not fit an int.
    void build(int V, long E, const int *Eu, const int *Ev, hipStream_t s);
};

// The two-layer cut: tr_cap[2V], r_link[V] (arc v -> V + v only), r_cap[E]
// (both arcs of edge e in both layers); segment[2V] as above.  The rounds are
// mincut's, over the 2V-node CSR.  Throws std::invalid_argument on a NaN
// terminal or a negative / non-finite r_cap or r_link.
template <typename real>
void mincut_duplex(int V, long E, DuplexNet &net, const int *Eu, const int *Ev,
                   const real *tr_cap, const real *r_link, const real *r_cap, uint8_t *segment,
                   MincutStats &st, hipStream_t s);

}  // namespace pfdr
