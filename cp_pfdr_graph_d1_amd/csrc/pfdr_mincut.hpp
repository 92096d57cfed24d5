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

}  // namespace pfdr
