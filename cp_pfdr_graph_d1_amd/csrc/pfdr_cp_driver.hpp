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
//
// Also here, once for the quadratic driver (pfdr_cutpursuit.hip) and the
// simplex driver (pfdr_cutpursuit_simplex.hip): the phase record and its C
// layout, the ordered sum, one PFDR solve of a reduced problem, the download
// and the frame of a one-call entry.
#pragma once

#include <chrono>
#include <cstdint>
#include <exception>
#include <stdexcept>

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

// What a run spent where: the host clock around synchronous steps, the cuts
// (simplex: expansions), their push/relabel rounds and global relabels, the
// PFDR iterations over all reduced problems.
struct CpStats {
    double gradient = 0, cuts = 0, graph = 0, pfdr = 0, sums = 0, total = 0;
    int64_t ncuts = 0, rounds = 0, relabels = 0, pfdr_it = 0;
};

// seconds[6], counts[4] in pfdr_cp_quadratic_d1_bounds_stats' layout (either may be null)
inline void cp_write_stats(const CpStats &st, double *seconds, int64_t *counts) {
    if (seconds) {
        const double v[6] = {st.gradient, st.cuts, st.graph, st.pfdr, st.sums, st.total};
        for (int i = 0; i < 6; i++) seconds[i] = v[i];
    }
    if (counts) {
        counts[0] = st.ncuts;
        counts[1] = st.rounds;
        counts[2] = st.relabels;
        counts[3] = st.pfdr_it;
    }
}

struct CpDriverBase {
    using clock = std::chrono::steady_clock;
    static double since(clock::time_point t) {
        return std::chrono::duration<double>(clock::now() - t).count();
    }
    virtual ~CpDriverBase() {
        if (g) pfdr_cpgraph_destroy(g);
    }
    hipStream_t s = lib_stream();
    pfdr_cpgraph *g = nullptr;
    int V = 0, E = 0, N = 0, K = 0;
    int rV = 1;
    bool has_l1 = false;
    double setup_sums = 0;  // seconds of setup()'s sums; loop() leaves it alone
    // Set before setup() by pfdr_cp_solver_create_sparse (quadratic drivers,
    // N > 0, p.A null): the observation operator in CSC, arrays per p.mem;
    // setup() copies it, and nothing reads the pointer afterwards.
    const pfdr_csc *sparse = nullptr;
    // pfdr_cp_solver_set_reduced: how a quadratic driver that holds a sparse A
    // keeps the reduced operator of a direct iteration (PFDR_REDUCED_*), and
    // what the last loop did: iterations solved on a sparse rA, direct
    // iterations solved on a dense one, the most entries a sparse rA stored.
    int reduced = PFDR_REDUCED_DENSE;
    int64_t sparse_its = 0, dense_direct_its = 0, max_rnnz = 0;
    // The same of the premultiplied iterations (N > 0), which only
    // PFDR_REDUCED_SPARSE_ALL solves from stored entries
    // (pfdr_cp_solver_premultiplied_stats).
    int64_t pre_sparse_its = 0, pre_dense_its = 0, pre_max_rnnz = 0;
    virtual bool holds_sparse_A() const { return false; }

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

// d = src (host) or a device-to-device copy, n elements (at least one allocated)
template <typename T>
void cp_take(DevBuf<T> &d, const T *src, size_t n, int mem, HostPins &hp, hipStream_t s) {
    d.alloc(n ? n : 1);
    if (!n) return;
    if (mem == PFDR_MEM_DEVICE)
        PFDR_HIP(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyDeviceToDevice, s));
    else
        hp.copy(d.p, src, n * sizeof(T), hipMemcpyHostToDevice);
}

// The drivers' common pieces, local to each driver file (the library exports none).
namespace {

// ((0 + x[0]) + x[1]) + ... in real, on the driver's stream
template <typename real>
struct CpSeqSum {
    hipStream_t s;
    DevBuf<int> off{2};
    DevBuf<real> one{1};
    explicit CpSeqSum(hipStream_t st) : s(st) {}
    real operator()(const real *x, long n) {
        if (n <= 0) return real(0);
        if (n >= (1L << 31)) throw std::runtime_error("sum of 2^31 or more terms");
        const int h[2] = {0, (int)n};
        PFDR_HIP(hipMemcpyAsync(off.p, h, sizeof h, hipMemcpyHostToDevice, s));
        ordered_segment_sums<real>(1, off.p, nullptr, x, one.p, s);
        real r;
        PFDR_HIP(hipMemcpyAsync(&r, one.p, sizeof(real), hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
        return r;
    }
};

// One reduced problem: a PFDR session on p (A: a sparse session on this
// matrix, p.A null), run to its end; its iterate (bytes of it) replaces p.X.
// Returns PFDR_it.
inline int cp_pfdr_solve(const pfdr_problem &p, size_t bytes, hipStream_t s,
                         const pfdr_csc *A = nullptr) {
    pfdr_session *ses = nullptr;
    if (A) CP_ABI(pfdr_session_create_sparse(&ses, &p, A));
    else CP_ABI(pfdr_session_create(&ses, &p));
    struct Hold {
        pfdr_session *q;
        ~Hold() { pfdr_session_destroy(q); }
    } hold{ses};
    int pit = 0;
    CP_ABI(pfdr_session_run(ses, p.itMax, &pit));
    CP_ABI(pfdr_session_sync(ses));
    const void *x = pfdr_session_device_x(ses);
    if (!x) throw CpAbiFail{PFDR_ERR_STATE};
    PFDR_HIP(hipMemcpyAsync(p.X, x, bytes, hipMemcpyDeviceToDevice, s));
    PFDR_HIP(hipStreamSynchronize(s));
    return pit;
}

// The same for a reduced operator kept sparse: p.A is null and A (device
// arrays) takes its place.
inline int cp_pfdr_solve_sparse(const pfdr_problem &p, const pfdr_csc &A, size_t bytes,
                                hipStream_t s) {
    return cp_pfdr_solve(p, bytes, s, &A);
}

// Cv and n component values to the host
template <typename real>
void cp_download(hipStream_t s, int V, const int *dCv, int *Cv, const real *dx, size_t n,
                 void *x) {
    HostPins hp(s);
    hp.copy(Cv, dCv, sizeof(int) * V, hipMemcpyDeviceToHost);
    hp.copy(x, dx, sizeof(real) * n, hipMemcpyDeviceToHost);
    hp.release();
}

// A one-call entry: setup + loop + download on a driver D(a...) of its own.
// *record (nullptr: none) becomes what the call spent, also when it fails half
// way; setup's sums count among the call's.
template <typename D, typename S, typename... A>
int cp_run_entry(const char *fn, S *record, const pfdr_cp_problem &p, const pfdr_cp_params &q,
                 int *rV, int *Cv, void *rX, int *CP_it, double *Time, void *Obj, void *Dif,
                 A... a) {
    try {
        const auto t0 = CpDriverBase::clock::now();
        if (record) *record = S{};
        D d(a...);
        struct Keep {
            D &d;
            S *record;
            ~Keep() {
                if (record) *record = d.st;
            }
        } keep{d, record};
        d.setup(p, Obj != nullptr);
        d.loop(t0, q, CP_it, Time, Obj, Dif);
        d.download(rV, Cv, rX);
        d.st.sums += d.setup_sums;
        d.st.total = CpDriverBase::since(t0);
    } catch (const CpAbiFail &f) {
        return f.status;
    } catch (const HipError &h) {
        return report_error(fn, h);
    } catch (const std::exception &ex) {
        return report_error(fn, ex.what());
    }
    return PFDR_OK;
}

}  // namespace

}  // namespace pfdr
