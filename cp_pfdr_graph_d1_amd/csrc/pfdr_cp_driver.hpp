// What the one-call cut-pursuit entries and the resumable solver
// (pfdr_cp_solver.hip) share: a driver owns the resident problem, its
// pfdr_cpgraph and the cut-pursuit state between three phases --
//   setup()    upload or adopt the problem, create the graph, the reference's
//              initialize(): the one-component state, its objective, R (N > 0)
//   loop()     the reference's cut-pursuit loop from the state the driver holds
//   download() Cv and the component values to the host
// An entry is setup + loop + download on a driver of its own; the solver keeps
// the driver and calls loop() again, possibly after adopt() of another state.
// A loop that does not start from the fresh state is the reference's warm
// restart (src/CP_PFDR_graph_quadratic_d1_l1.cpp:293-319): iteration 0,
// dif = max(CP_difTol^2, 1), PFDR_it = PFDR_itMax, the state as its own
// previous iterate -- the values the fresh start has too.
#pragma once

#include <chrono>
#include <cstdint>

#include "pfdr_graph.hpp"

namespace pfdr {

struct CpAbiFail {  // a library call failed: its message is already recorded
    int status;
};
#define CP_ABI(call)                                      \
    do {                                                  \
        const int st_ = (call);                           \
        if (st_ != PFDR_OK) throw ::pfdr::CpAbiFail{st_}; \
    } while (0)

struct CpDriverBase {
    using clock = std::chrono::steady_clock;
    virtual ~CpDriverBase() {
        if (g) pfdr_cpgraph_destroy(g);
    }
    hipStream_t s = lib_stream();
    pfdr_cpgraph *g = nullptr;
    int V = 0, E = 0, N = 0, K = 0;
    int rV = 1;
    bool has_l1 = false;

    // p.mem = PFDR_MEM_DEVICE: the arrays are device memory, copied except A,
    // which is borrowed.  want_obj: evaluate the functional at the initial state.
    virtual void setup(const pfdr_cp_problem &p, bool want_obj) = 0;
    // Time counts from t0.  Obj[0]: the functional at the state the loop starts
    // from, as far as the driver knows it (else NaN).
    virtual void loop(clock::time_point t0, const pfdr_cp_params &q, int *CP_it, double *Time,
                      void *Obj, void *Dif) = 0;
    virtual void download(int *rV_out, int *Cv, void *rX) = 0;
    // The graph's activity and components were replaced: take rV components
    // with the device values rX (rV, simplex rV K) and residual R (N > 0;
    // nullptr: recomputed by the loop's own kernels).
    virtual void adopt(int rV_new, const void *rX, const void *R) = 0;
    virtual const void *values() const = 0;    // device, rV (simplex rV K)
    virtual const void *residual() const = 0;  // device, N > 0 only
    virtual void forget_objective() = 0;
    // seconds[6], counts[4] of the last loop, pfdr_cp_quadratic_d1_bounds_stats' layout
    virtual void stats(double *seconds, int64_t *counts) const = 0;
};

CpDriverBase *cp_make_l1_driver(int dtype, bool duplex);
CpDriverBase *cp_make_bounds_driver(int dtype);
CpDriverBase *cp_make_simplex_driver(int dtype);

// d = h (host) or a device-to-device copy, n elements (at least one allocated)
template <typename T>
void cp_take(DevBuf<T> &d, const T *src, size_t n, int mem, HostPins &hp, hipStream_t s) {
    d.alloc(n ? n : 1);
    if (!n) return;
    if (mem == PFDR_MEM_DEVICE)
        PFDR_HIP(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyDeviceToDevice, s));
    else
        hp.copy(d.p, src, n * sizeof(T), hipMemcpyHostToDevice);
}

}  // namespace pfdr
