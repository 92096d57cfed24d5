// The whole cut pursuit of the bounds driver,
// CP_PFDR_graph_quadratic_d1_bounds<real> of the reference
// (src/CP_PFDR_graph_quadratic_d1_bounds.cpp:206-973), on one GPU: the loop of
// INTEGRATION.md §7 over the library's own steps -- the graph steps of
// pfdr_cpgraph.hip (capacities_bounds), the cut of pfdr_mincut.hip
// (PFDR_ARCS_BOTH), the reduced problem of pfdr_cp.hip and the bounds PFDR
// session -- with PFDR_MEM_DEVICE throughout.  Host arrays come in once and
// Cv / rX go out once; in between only scalars cross PCIe (counts, rV, rE, the
// sums of initialize(), of the iterate evolution and of the objective).
//
// The scalar sums (initialize :94-135, :157-166, the iterate evolution
// :883-901 and the objective :906-942) are added one by one in `real` in the
// reference's order (ordered_segment_sums), like the reference built without
// OpenMP.  Their terms -- every a*b the reference then adds -- are formed by
// the kernels of this file, so that no product meets its sum in one
// instruction.
//
// One departure from the reference: min > max or a NaN bound is an
// argument error (the reference clamps to min and hands PFDR an empty box).
//
// The driver runs in three phases (pfdr_cp_driver.hpp): setup (upload, graph,
// the reference's initialize()), the loop from the state the driver holds, and
// the download.  An entry is the three in a row; the resumable solver
// (pfdr_cp_solver.hip) keeps the driver and runs the same loop again.
#include <algorithm>
#include <chrono>
#include <limits>
#include <stdexcept>

#include "pfdr_cp_driver.hpp"

namespace pfdr {

namespace {

#define CPB_ABI(call) CP_ABI(call)

// What the last call on this thread spent where (pfdr_cp_quadratic_d1_bounds_stats).
struct Stats {
    double gradient = 0, cuts = 0, graph = 0, pfdr = 0, sums = 0, total = 0;
    int64_t ncuts = 0, rounds = 0, relabels = 0, pfdr_it = 0;
};
thread_local Stats g_stats;

// rA[n] = sum over the columns of A (N-by-V, column major), v ascending (:101-109)
template <typename real>
__global__ void k_cpb_colsum(int N, int V, const real *__restrict__ A, real *__restrict__ rA) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    real a = real(0);
    for (long v = 0; v < V; v++) a += A[n + (long)N * v];
    rA[n] = a;
}

// terms of <A1|Y> and ||A1||^2 (:112-116)
template <typename real>
__global__ void k_cpb_init_products(int N, const real *__restrict__ rA,
                                    const real *__restrict__ Y, real *__restrict__ tY,
                                    real *__restrict__ tAA) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const real a = rA[n];
    tY[n] = a * Y[n];
    tAA[n] = a * a;
}

// R = Y - rA x0 at the one-component value (:153)
template <typename real>
__global__ void k_cpb_init_residual(int N, const real *__restrict__ rA,
                                    const real *__restrict__ Y, real x0, real *__restrict__ R) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const real b = rA[n] * x0;
    R[n] = Y[n] - b;
}

// terms of ||R||^2 (:162, :911)
template <typename real>
__global__ void k_cpb_square(int N, const real *__restrict__ R, real *__restrict__ t) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const real r = R[n];
    t[n] = r * r;
}

// R = Y - rA rX, rv ascending (:866-878)
template <typename real>
__global__ void k_cpb_residual(int N, int rV, const real *__restrict__ rA,
                               const real *__restrict__ rX, const real *__restrict__ Y,
                               real *__restrict__ R) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    real a = real(0);
    for (long rv = 0; rv < rV; rv++) {
        const real b = rA[n + (long)N * rv] * rX[rv];
        a += b;
    }
    R[n] = Y[n] - a;
}

// terms of the iterate evolution (:888-895); the last partition becomes this one
template <typename real>
__global__ void k_cpb_evolution(int V, const int *__restrict__ Cv, const real *__restrict__ rX,
                                int *__restrict__ Cv_, const real *__restrict__ rX_,
                                real *__restrict__ td, real *__restrict__ tc) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int rv = Cv[v];
    const real a = rX[rv];
    const real b = rX_[Cv_[v]] - a;
    td[v] = b * b;
    tc[v] = a * a;
    Cv_[v] = rv;
}

// terms of 1/2 <X, AtA X> - <X, AtY> (:914-929): rows of a full rAA, or its diagonal
template <typename real>
__global__ void k_cpb_obj_quad(int rV, int full, const real *__restrict__ rAA,
                               const real *__restrict__ rY, const real *__restrict__ rX,
                               real *__restrict__ t) {
    const int ru = blockIdx.x * blockDim.x + threadIdx.x;
    if (ru >= rV) return;
    const real x = rX[ru];
    if (full) {
        const real *row = rAA + (long)rV * ru;
        real b = real(0);
        for (int rv = 0; rv < rV; rv++) {
            const real c = row[rv] * rX[rv];
            b += c;
        }
        t[ru] = x * (real(0.5) * b - rY[ru]);
    } else {
        t[ru] = x * (real(0.5) * rAA[ru] * x - rY[ru]);
    }
}

// terms of ||x||_{d1, La_d1} over the reduced edges (:936-940)
template <typename real>
__global__ void k_cpb_obj_d1(int rE, const int *__restrict__ rEu, const int *__restrict__ rEv,
                             const real *__restrict__ rLa, const real *__restrict__ rX,
                             real *__restrict__ t) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rE) return;
    real b = rX[rEu[e]] - rX[rEv[e]];
    if (b < real(0)) b = -b;
    t[e] = rLa[e] * b;
}

template <typename real>
struct BdDriver : CpDriverBase {
    Stats st;  // of the last run
    DevBuf<int> off{2};
    DevBuf<real> one{1};
    // the resident problem
    DevBuf<real> dY, dA;
    const real *pA = nullptr;  // dA, or the caller's device A
    real min = real(0), max = real(0);
    // the state besides the graph's: values, Cv, residual (N > 0)
    DevBuf<real> drX, dR, dtN;  // dtN: the terms of the residual's sums
    DevBuf<int> dCv, dVc, drVc;
    real obj = real(0);  // the functional at the state, when known
    bool obj_known = false;

    // ((0 + x[0]) + x[1]) + ... in real
    real seq_sum(const real *x, long n) {
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

    template <typename T>
    void up(DevBuf<T> &d, const T *h, size_t n, HostPins &hp) {
        d.alloc(n ? n : 1);
        if (n) hp.copy(d.p, h, n * sizeof(T), hipMemcpyHostToDevice);
    }

    static double since(clock::time_point t) {
        return std::chrono::duration<double>(clock::now() - t).count();
    }

    // 1/2 ||R||^2 (:159-163, :908-912)
    real half_norm2(int N, const real *R, real *t) {
        k_cpb_square<real><<<grid_for(N), kBlock, 0, s>>>(N, R, t);
        PFDR_HIP(hipGetLastError());
        real a = seq_sum(t, N);
        a *= real(0.5);
        return a;
    }

    void setup(const pfdr_cp_problem &p, bool want_obj) override {
        V = p.V, E = p.E, N = p.N;
        min = (real)p.min, max = (real)p.max;
        const real *Y = (const real *)p.Y, *A = (const real *)p.A;
        const int dt = sizeof(real) == 4 ? PFDR_F32 : PFDR_F64;
        const bool dev = p.mem == PFDR_MEM_DEVICE;
        // ---- the problem, once, into HBM
        DevBuf<real> dLa;
        DevBuf<int> dEu, dEv;
        {
            HostPins hp(s);
            const size_t asz = N > 0 ? (size_t)N * V : N < 0 ? (size_t)V * V : A ? (size_t)V : 0;
            cp_take(dY, Y, N > 0 ? (size_t)N : (size_t)V, p.mem, hp, s);
            if (!dev) up(dA, A, asz, hp);
            cp_take(dEu, p.Eu, (size_t)E, p.mem, hp, s);
            cp_take(dEv, p.Ev, (size_t)E, p.mem, hp, s);
            cp_take(dLa, (const real *)p.La_d1, (size_t)E, p.mem, hp, s);
            hp.release();
        }
        pA = !A ? nullptr : dev ? A : dA.p;
        CPB_ABI(pfdr_cpgraph_create(&g, dt, V, E, dEu.p, dEv.p, dLa.p, nullptr, PFDR_MEM_DEVICE));

        // ---- initialize (:66-170): the one-component solution, projected on the box
        auto t = clock::now();
        real rY = real(0), rAA = real(0);
        DevBuf<real> drA0;
        if (N > 0) {
            drA0.alloc(N);
            dtN.alloc(N);
            dR.alloc(N);
            k_cpb_colsum<real><<<grid_for(N), kBlock, 0, s>>>(N, V, pA, drA0.p);
            k_cpb_init_products<real><<<grid_for(N), kBlock, 0, s>>>(N, drA0.p, dY.p, dtN.p,
                                                                    dR.p);
            PFDR_HIP(hipGetLastError());
            rY = seq_sum(dtN.p, N);
            rAA = seq_sum(dR.p, N);
        } else {
            rY = seq_sum(dY.p, V);
            if (N < 0) rAA = seq_sum(pA, (long)V * V);
            else if (A) rAA = seq_sum(pA, V);
            else rAA = (real)V;
        }
        real x0 = rY / rAA;
        if (x0 < min) x0 = min;  // :138-139
        else if (x0 > max) x0 = max;
        rV = 1;
        drX.alloc(1);
        PFDR_HIP(hipMemcpyAsync(drX.p, &x0, sizeof(real), hipMemcpyHostToDevice, s));
        PFDR_HIP(hipStreamSynchronize(s));
        CPB_ABI(pfdr_cpgraph_set_values(g, drX.p, PFDR_MEM_DEVICE));
        if (N > 0) {
            k_cpb_init_residual<real><<<grid_for(N), kBlock, 0, s>>>(N, drA0.p, dY.p, x0, dR.p);
            PFDR_HIP(hipGetLastError());
        }
        obj_known = false;
        if (want_obj) {
            if (N > 0) obj = half_norm2(N, dR.p, dtN.p);
            else obj = x0 * (real(0.5) * rAA * x0 - rY);
            obj_known = true;
        }
        PFDR_HIP(hipStreamSynchronize(s));
        st.sums += since(t);
        dCv.alloc(V);
        dVc.alloc(V);
        drVc.alloc((size_t)V + 1);
        CPB_ABI(pfdr_cpgraph_get_components(g, nullptr, dCv.p, nullptr, nullptr, PFDR_MEM_DEVICE));
    }

    // R = Y - A X at the graph's components and drX (:866-878): the component
    // column sums of pfdr_cp_reduce, then k_cpb_residual, as the loop does
    void residual_from_state() {
        CPB_ABI(pfdr_cpgraph_get_components(g, nullptr, nullptr, dVc.p, drVc.p, PFDR_MEM_DEVICE));
        DevBuf<real> rA((size_t)N * rV), L(rV);
        if (sizeof(real) == 4)
            CPB_ABI(pfdr_cp_reduce_f32(N, V, (const float *)pA, (const float *)dY.p, rV, drVc.p,
                                       dVc.p, 0, PFDR_MEM_DEVICE, 1e-3f, 100, 10, (float *)rA.p,
                                       nullptr, nullptr, (float *)L.p, nullptr));
        else
            CPB_ABI(pfdr_cp_reduce_f64(N, V, (const double *)pA, (const double *)dY.p, rV, drVc.p,
                                       dVc.p, 0, PFDR_MEM_DEVICE, 1e-3, 100, 10, (double *)rA.p,
                                       nullptr, nullptr, (double *)L.p, nullptr));
        k_cpb_residual<real><<<grid_for(N), kBlock, 0, s>>>(N, rV, rA.p, drX.p, dY.p, dR.p);
        PFDR_HIP(hipGetLastError());
        PFDR_HIP(hipStreamSynchronize(s));
    }

    void adopt(int rV_new, const void *x, const void *R) override {
        rV = rV_new;
        drX.alloc(rV);
        PFDR_HIP(hipMemcpyAsync(drX.p, x, sizeof(real) * rV, hipMemcpyDeviceToDevice, s));
        PFDR_HIP(hipStreamSynchronize(s));
        CPB_ABI(pfdr_cpgraph_set_values(g, drX.p, PFDR_MEM_DEVICE));
        CPB_ABI(pfdr_cpgraph_get_components(g, nullptr, dCv.p, nullptr, nullptr, PFDR_MEM_DEVICE));
        if (N > 0) {
            if (R) {
                PFDR_HIP(hipMemcpyAsync(dR.p, R, sizeof(real) * N, hipMemcpyDeviceToDevice, s));
                PFDR_HIP(hipStreamSynchronize(s));
            } else {
                residual_from_state();
            }
        }
        obj_known = false;
    }
    const void *values() const override { return drX.p; }
    const void *residual() const override { return N > 0 ? dR.p : nullptr; }
    void forget_objective() override { obj_known = false; }
    void stats(double *seconds, int64_t *counts) const override {
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

    void loop(clock::time_point t0, const pfdr_cp_params &q, int *CP_it_out, double *Time,
              void *Obj_, void *Dif_) override {
        const real CP_difTol = (real)q.CP_difTol, rho = (real)q.rho, condMin = (real)q.condMin,
                   difRcd = (real)q.difRcd, difTol = (real)q.difTol;
        const int CP_itMax = q.CP_itMax, itMax = q.itMax, verbose = q.verbose;
        real *Obj = (real *)Obj_, *Dif = (real *)Dif_;
        const int dt = sizeof(real) == 4 ? PFDR_F32 : PFDR_F64;
        const real eps = (real(0) < CP_difTol && CP_difTol < Lim<real>::eps) ? CP_difTol
                                                                            : Lim<real>::eps;
        const real inf = Lim<real>::huge;
        const int gV = grid_for(V);
        auto t = t0;
        st = Stats{};
        int rE = 0;  // a restart reports no reduced edge before its first iteration
        if (Obj) Obj[0] = obj_known ? obj : std::numeric_limits<real>::quiet_NaN();

        // ---- cut pursuit
        DevBuf<int> dCv_;
        DevBuf<real> drX_, dtr(V), drc(E > 0 ? E : 1), t1, t2;
        DevBuf<uint8_t> dseg(V);
        const bool track = CP_difTol > real(0) || Dif;
        if (track) {
            drX_.alloc(rV);
            dCv_.alloc(V);
            t1.alloc(V);
            t2.alloc(V);
            PFDR_HIP(hipMemcpyAsync(drX_.p, drX.p, sizeof(real) * rV, hipMemcpyDeviceToDevice, s));
            PFDR_HIP(hipMemcpyAsync(dCv_.p, dCv.p, sizeof(int) * V, hipMemcpyDeviceToDevice, s));
            PFDR_HIP(hipStreamSynchronize(s));
        }
        const real difTol2 = CP_difTol * CP_difTol;
        real dif = difTol2 > real(1) ? difTol2 : real(1);
        int it = 0, pit = itMax;
        auto cut = [&]() {
            int64_t rounds = 0, relabels = 0;
            CPB_ABI(pfdr_cpgraph_mincut(g, PFDR_ARCS_BOTH, dtr.p, drc.p, PFDR_MEM_DEVICE, dseg.p,
                                        nullptr, &rounds));
            CPB_ABI(pfdr_cpgraph_mincut_relabels(g, &relabels));
            st.ncuts++;
            st.rounds += rounds;
            st.relabels += relabels;
        };
        for (;;) {
            if (Time) Time[it] = since(t0);
            if (verbose) {
                printf("\n\tCut pursuit iteration %d (max. %d)\n", it, CP_itMax);
                if (difTol2 > real(0)) printf("\trelative iterate evolution %g (tol. %g)\n",
                                              (double)dif, (double)difTol2);
                printf("\t%d connected component(s), %d reduced edge(s)\n", rV, rE);
                fflush(stdout);
            }
            if (it == CP_itMax || dif < difTol2) break;
            // steepest cuts (:331-529)
            t = clock::now();
            CPB_ABI(pfdr_cpgraph_gradient(g, N, pA, dY.p, N > 0 ? dR.p : nullptr, PFDR_MEM_DEVICE,
                                          nullptr));
            st.gradient += since(t);
            t = clock::now();
            int w = 0, n = 0;
            if (-inf == min && max == inf) {  // :392
                CPB_ABI(pfdr_cpgraph_capacities_bounds(g, 0, (double)min, (double)max, dtr.p,
                                                       drc.p, PFDR_MEM_DEVICE));
                cut();
                CPB_ABI(pfdr_cpgraph_activate(g, dseg.p, PFDR_MEM_DEVICE, &w));
            } else {
                CPB_ABI(pfdr_cpgraph_capacities_bounds(g, 1, (double)min, (double)max, dtr.p,
                                                       drc.p, PFDR_MEM_DEVICE));
                cut();
                // the second cut's capacities, from the activity before the first's activations
                CPB_ABI(pfdr_cpgraph_capacities_bounds(g, 2, (double)min, (double)max, dtr.p,
                                                       drc.p, PFDR_MEM_DEVICE));
                CPB_ABI(pfdr_cpgraph_activate(g, dseg.p, PFDR_MEM_DEVICE, &w));
                cut();
                CPB_ABI(pfdr_cpgraph_activate(g, dseg.p, PFDR_MEM_DEVICE, &n));
                w += n;
            }
            st.cuts += since(t);
            if (w == 0) {  // :535-542
                if (track) {
                    dif = real(0);
                    if (Dif) Dif[it] = dif;
                }
                it++;
                if (Obj) Obj[it] = Obj[it - 1];
                continue;
            }
            // reduced graph and problem (:547-813)
            t = clock::now();
            CPB_ABI(pfdr_cpgraph_components(g, &rV));
            CPB_ABI(pfdr_cpgraph_reduced_graph(g, (double)eps, &rE));
            CPB_ABI(pfdr_cpgraph_get_components(g, nullptr, dCv.p, dVc.p, drVc.p, PFDR_MEM_DEVICE));
            DevBuf<int> rEu(rE > 0 ? rE : 1), rEv(rE > 0 ? rE : 1);
            DevBuf<real> rLa(rE > 0 ? rE : 1);
            CPB_ABI(pfdr_cpgraph_get_reduced(g, rEu.p, rEv.p, rLa.p, nullptr, PFDR_MEM_DEVICE));
            const int preAt = N <= 0 || rV < (2L * N * pit) / ((long)N + pit);  // :648
            DevBuf<real> rA, rAAd, rYd, L(rV);
            if (N > 0) rA.alloc((size_t)N * rV);
            if (preAt) {
                rYd.alloc(rV);
                rAAd.alloc(N == 0 ? (size_t)rV : (size_t)rV * rV);
            }
            if (sizeof(real) == 4)
                CPB_ABI(pfdr_cp_reduce_f32(N, V, (const float *)pA, (const float *)dY.p, rV, drVc.p,
                                          dVc.p, preAt, PFDR_MEM_DEVICE, 1e-3f, 100, 10,
                                          (float *)rA.p, (float *)rAAd.p, (float *)rYd.p,
                                          (float *)L.p, nullptr));
            else
                CPB_ABI(pfdr_cp_reduce_f64(N, V, (const double *)pA, (const double *)dY.p, rV,
                                          drVc.p, dVc.p, preAt, PFDR_MEM_DEVICE, 1e-3, 100, 10,
                                          (double *)rA.p, (double *)rAAd.p, (double *)rYd.p,
                                          (double *)L.p, nullptr));
            st.graph += since(t);
            // PFDR from zero (:824-836)
            t = clock::now();
            drX.alloc(rV);
            PFDR_HIP(hipMemsetAsync(drX.p, 0, sizeof(real) * rV, s));
            PFDR_HIP(hipStreamSynchronize(s));
            {
                pfdr_problem p{};
                p.kind = PFDR_KIND_BOUNDS;
                p.dtype = dt;
                p.mem = PFDR_MEM_DEVICE;
                p.V = rV;
                p.E = rE;
                p.N = preAt ? (N == 0 ? 0 : -rV) : N;
                p.X = drX.p;
                p.Y = preAt ? rYd.p : dY.p;
                p.A = preAt ? rAAd.p : rA.p;
                p.Eu = rEu.p;
                p.Ev = rEv.p;
                p.La_d1 = rLa.p;
                p.min = (double)min;
                p.max = (double)max;
                p.Ltype = PFDR_LIPSCHITZ_DIAG;
                p.L = L.p;
                p.rho = rho;
                p.condMin = condMin;
                p.difRcd = difRcd;
                p.difTol = difTol;
                p.itMax = itMax;
                p.verbose = verbose;
                pfdr_session *ses = nullptr;
                CPB_ABI(pfdr_session_create(&ses, &p));
                struct SHold {
                    pfdr_session *q;
                    ~SHold() { pfdr_session_destroy(q); }
                } sh{ses};
                CPB_ABI(pfdr_session_run(ses, itMax, &pit));
                CPB_ABI(pfdr_session_sync(ses));
                st.pfdr_it += pit;
                const void *x = pfdr_session_device_x(ses);
                if (!x) throw CpAbiFail{PFDR_ERR_STATE};
                PFDR_HIP(hipMemcpyAsync(drX.p, x, sizeof(real) * rV, hipMemcpyDeviceToDevice, s));
                PFDR_HIP(hipStreamSynchronize(s));
            }
            st.pfdr += since(t);
            t = clock::now();
            CPB_ABI(pfdr_cpgraph_set_values(g, drX.p, PFDR_MEM_DEVICE));
            CPB_ABI(pfdr_cpgraph_merge(g, (double)eps, (double)CP_difTol, &n));
            st.graph += since(t);
            // progress (:865-901)
            t = clock::now();
            if (N > 0) {
                k_cpb_residual<real><<<grid_for(N), kBlock, 0, s>>>(N, rV, rA.p, drX.p, dY.p, dR.p);
                PFDR_HIP(hipGetLastError());
            }
            if (track) {
                k_cpb_evolution<real><<<gV, kBlock, 0, s>>>(V, dCv.p, drX.p, dCv_.p, drX_.p, t1.p,
                                                           t2.p);
                PFDR_HIP(hipGetLastError());
                dif = seq_sum(t1.p, V);
                const real c = seq_sum(t2.p, V);
                dif = c > eps ? dif / c : dif / eps;
                drX_.alloc(rV);
                PFDR_HIP(hipMemcpyAsync(drX_.p, drX.p, sizeof(real) * rV, hipMemcpyDeviceToDevice,
                                        s));
                PFDR_HIP(hipStreamSynchronize(s));
                if (Dif) Dif[it] = dif;
            }
            it++;
            if (Obj) {  // :906-942
                real a;
                DevBuf<real> tt((size_t)std::max(rV, std::max(rE, 1)));
                if (N > 0) {
                    a = half_norm2(N, dR.p, dtN.p);
                } else {
                    k_cpb_obj_quad<real><<<grid_for(rV), kBlock, 0, s>>>(rV, N < 0, rAAd.p, rYd.p,
                                                                        drX.p, tt.p);
                    PFDR_HIP(hipGetLastError());
                    a = seq_sum(tt.p, rV);
                }
                Obj[it] = a;
                a = real(0);
                if (rE > 0) {
                    k_cpb_obj_d1<real><<<grid_for(rE), kBlock, 0, s>>>(rE, rEu.p, rEv.p, rLa.p,
                                                                      drX.p, tt.p);
                    PFDR_HIP(hipGetLastError());
                    a = seq_sum(tt.p, rE);
                }
                Obj[it] += a;
                obj = Obj[it];
            }
            obj_known = Obj != nullptr;
            PFDR_HIP(hipStreamSynchronize(s));  // the iteration's buffers leave scope
            st.sums += since(t);
        }
        if (CP_it_out) *CP_it_out = it;
        st.total = since(t0);
    }

    void download(int *rV_out, int *Cv, void *rX_out) override {
        *rV_out = rV;
        HostPins hp(s);
        hp.copy(Cv, dCv.p, sizeof(int) * V, hipMemcpyDeviceToHost);
        hp.copy(rX_out, drX.p, sizeof(real) * rV, hipMemcpyDeviceToHost);
        hp.release();
    }
};

template <typename real>
int cpb_entry(const char *fn, int V, int E, int N, int *rV, int *Cv, real *rX, const real *Y,
              const real *A, const int *Eu, const int *Ev, const real *La_d1, real min, real max,
              real CP_difTol, int CP_itMax, int *CP_it, real rho, real condMin, real difRcd,
              real difTol, int itMax, double *Time, real *Obj, real *Dif, int verbose) {
    if (V <= 0 || E < 0 || !rV || !Cv || !rX || !Y || CP_itMax < 0 ||
        (E > 0 && (!Eu || !Ev || !La_d1)))
        return report_error(fn, "invalid arguments");
    if (N != 0 && !A) return report_error(fn, "N != 0 needs A");
    if (N < 0 && -N != V) return report_error(fn, "N < 0 needs A = A^tA and N = -V");
    if (!(min <= max)) return report_error(fn, "the bounds need min <= max");
    try {
        const auto t0 = std::chrono::steady_clock::now();
        g_stats = Stats{};
        BdDriver<real> d;
        struct Keep {  // what the call spent, also when it fails half way
            BdDriver<real> &d;
            ~Keep() { g_stats = d.st; }
        } keep{d};
        pfdr_cp_problem p{};
        p.kind = PFDR_KIND_BOUNDS;
        p.mem = PFDR_MEM_HOST;
        p.V = V, p.E = E, p.N = N;
        p.Y = Y, p.A = A, p.Eu = Eu, p.Ev = Ev, p.La_d1 = La_d1;
        p.min = min, p.max = max;
        const pfdr_cp_params q{CP_difTol, CP_itMax, rho, condMin, difRcd, difTol, itMax, verbose};
        d.setup(p, Obj != nullptr);
        const double init_sums = d.st.sums;
        d.loop(t0, q, CP_it, Time, Obj, Dif);
        d.download(rV, Cv, rX);
        d.st.sums += init_sums;
        d.st.total = BdDriver<real>::since(t0);
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

CpDriverBase *cp_make_bounds_driver(int dtype) {
    if (dtype == PFDR_F32) return new BdDriver<float>();
    return new BdDriver<double>();
}

}  // namespace pfdr

extern "C" int pfdr_cp_quadratic_d1_bounds_f32(int V, int E, int N, int *rV, int *Cv, float *rX,
    const float *Y, const float *A, const int *Eu, const int *Ev, const float *La_d1, float min,
    float max, float CP_difTol, int CP_itMax, int *CP_it, float rho, float condMin, float difRcd,
    float difTol, int itMax, double *Time, float *Obj, float *Dif, int verbose) {
    return pfdr::cpb_entry<float>("pfdr_cp_quadratic_d1_bounds_f32", V, E, N, rV, Cv, rX, Y, A, Eu,
                                  Ev, La_d1, min, max, CP_difTol, CP_itMax, CP_it, rho, condMin,
                                  difRcd, difTol, itMax, Time, Obj, Dif, verbose);
}

extern "C" int pfdr_cp_quadratic_d1_bounds_f64(int V, int E, int N, int *rV, int *Cv, double *rX,
    const double *Y, const double *A, const int *Eu, const int *Ev, const double *La_d1,
    double min, double max, double CP_difTol, int CP_itMax, int *CP_it, double rho,
    double condMin, double difRcd, double difTol, int itMax, double *Time, double *Obj,
    double *Dif, int verbose) {
    return pfdr::cpb_entry<double>("pfdr_cp_quadratic_d1_bounds_f64", V, E, N, rV, Cv, rX, Y, A,
                                   Eu, Ev, La_d1, min, max, CP_difTol, CP_itMax, CP_it, rho,
                                   condMin, difRcd, difTol, itMax, Time, Obj, Dif, verbose);
}

extern "C" int pfdr_cp_quadratic_d1_bounds_stats(double *seconds, int64_t *counts) {
    const pfdr::Stats &st = pfdr::g_stats;
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
    return PFDR_OK;
}
