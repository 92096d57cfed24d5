// The whole cut pursuit of the three quadratic drivers of the reference, on one
// GPU, as one driver with a flavour:
//   l1      CP_PFDR_graph_quadratic_d1_l1<real>
//           (src/CP_PFDR_graph_quadratic_d1_l1.cpp, cited as l1 :NNN)
//   duplex  CP_PFDR_graph_quadratic_d1_l1_duplex<real>
//           (src/CP_PFDR_graph_quadratic_d1_l1_duplex.cpp), whose source differs
//           from the l1 driver's in the graph and the cut only: one two-layer
//           cut per iteration when there is an l1 term or positivity
//   bounds  CP_PFDR_graph_quadratic_d1_bounds<real>
//           (src/CP_PFDR_graph_quadratic_d1_bounds.cpp, cited as bounds :NNN)
// It is the loop of INTEGRATION.md §7 over the library's own steps -- the graph
// steps of pfdr_cpgraph.hip, the cut of pfdr_mincut.hip (PFDR_ARCS_BOTH), the
// reduced problem of pfdr_cp.hip and the PFDR session -- with PFDR_MEM_DEVICE
// throughout.  Host arrays come in once and Cv / rX go out once; in between
// only scalars cross PCIe (counts, rV, rE, the sums of initialize(), of the
// iterate evolution and of the objective), for a dense A (N > 0) too.
//
// The flavours differ in five places, each marked `flavour:` below: what is
// uploaded, the one-component value of initialize(), the cuts, the kind of the
// PFDR problem, and the l1 term of the objective.
//
// The scalar sums (initialize l1 :94-136, :157-174 / bounds :94-135, :157-166;
// the iterate evolution l1 :905-923 / bounds :883-901; the objective
// l1 :927-975 / bounds :906-942) are added one by one in `real` in the
// reference's order (ordered_segment_sums), like the reference built without
// OpenMP.  Their terms -- every a*b the reference then adds -- are formed by
// the kernels of this file, so that no product meets its sum in one
// instruction.
//
// One departure from the reference: for the bounds flavour min > max
// or a NaN bound is an argument error (the reference clamps to min and hands
// PFDR an empty box).
//
// The driver runs in three phases (pfdr_cp_driver.hpp): setup (upload, graph,
// the reference's initialize()), the loop from the state the driver holds, and
// the download.  An entry is the three in a row; the resumable solver
// (pfdr_cp_solver.hip) keeps the driver and runs the same loop again.
#include <algorithm>
#include <limits>

#include "pfdr_cp_driver.hpp"
#include "pfdr_cp_sparse.hpp"

namespace pfdr {

namespace {

enum class Flavour { L1, Duplex, Bounds };

// What the calling thread's last duplex / bounds call spent where
// (pfdr_cp_quadratic_d1_l1_duplex_stats, pfdr_cp_quadratic_d1_bounds_stats).
thread_local CpStats g_duplex_stats, g_bounds_stats;

// rA[n] = sum over the columns of A (N-by-V, column major), v ascending
// (l1 :99-109 / bounds :101-109)
template <typename real>
__global__ void k_cpq_colsum(int N, int V, const real *__restrict__ A, real *__restrict__ rA) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    real a = real(0);
    for (long v = 0; v < V; v++) a += A[n + (long)N * v];
    rA[n] = a;
}

// terms of <A1|Y> and ||A1||^2 (l1 :111-115 / bounds :112-116)
template <typename real>
__global__ void k_cpq_init_products(int N, const real *__restrict__ rA,
                                    const real *__restrict__ Y, real *__restrict__ tY,
                                    real *__restrict__ tAA) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const real a = rA[n];
    tY[n] = a * Y[n];
    tAA[n] = a * a;
}

// R = Y - rA x0 at the one-component value (l1 :154 / bounds :153)
template <typename real>
__global__ void k_cpq_init_residual(int N, const real *__restrict__ rA,
                                    const real *__restrict__ Y, real x0, real *__restrict__ R) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const real b = rA[n] * x0;
    R[n] = Y[n] - b;
}

// terms of ||R||^2 (l1 :162, :933 / bounds :162, :911)
template <typename real>
__global__ void k_cpq_square(int N, const real *__restrict__ R, real *__restrict__ t) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const real r = R[n];
    t[n] = r * r;
}

// R = Y - rA rX, rv ascending (l1 :889-901 / bounds :866-878)
template <typename real>
__global__ void k_cpq_residual(int N, int rV, const real *__restrict__ rA,
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

// terms of the iterate evolution (l1 :911-918 / bounds :888-895); the last
// partition becomes this one
template <typename real>
__global__ void k_cpq_evolution(int V, const int *__restrict__ Cv, const real *__restrict__ rX,
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

// terms of 1/2 <X, AtA X> - <X, AtY> (l1 :936-951 / bounds :914-929): rows of a
// full rAA, or its diagonal
template <typename real>
__global__ void k_cpq_obj_quad(int rV, int full, const real *__restrict__ rAA,
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

// terms of ||x||_{d1, La_d1} over the reduced edges (l1 :958-962 / bounds :936-940)
template <typename real>
__global__ void k_cpq_obj_d1(int rE, const int *__restrict__ rEu, const int *__restrict__ rEv,
                             const real *__restrict__ rLa, const real *__restrict__ rX,
                             real *__restrict__ t) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rE) return;
    real b = rX[rEu[e]] - rX[rEv[e]];
    if (b < real(0)) b = -b;
    t[e] = rLa[e] * b;
}

// terms of ||x||_{l1, La_l1} over the components (l1 :968-972)
template <typename real>
__global__ void k_cpq_obj_l1(int rV, const real *__restrict__ rL1, const real *__restrict__ rX,
                             real *__restrict__ t) {
    const int rv = blockIdx.x * blockDim.x + threadIdx.x;
    if (rv >= rV) return;
    real b = rX[rv];
    if (b < real(0)) b = -b;
    t[rv] = rL1[rv] * b;
}

template <typename real>
struct QuadDriver : CpDriverBase {
    const Flavour flavour;
    CpStats st;  // of the last run
    CpSeqSum<real> seq_sum{s};
    // the resident problem
    DevBuf<real> dY, dA;
    const real *pA = nullptr;  // dA, or the caller's device A
    CpCsc<real> sp;            // the copy of a sparse A (N > 0), when the problem came with one
    int positivity = 0;                // l1, duplex
    real min = real(0), max = real(0);  // bounds
    // the state besides the graph's: values, Cv, residual (N > 0)
    DevBuf<real> drX, dR, dtN;  // dtN: the terms of the residual's sums
    DevBuf<int> dCv, dVc, drVc;
    real obj = real(0);  // the functional at the state, when known
    bool obj_known = false;

    explicit QuadDriver(Flavour f) : flavour(f) {}

    // 1/2 ||R||^2 (l1 :159-163, :930-934 / bounds :159-163, :908-912)
    real half_norm2(const real *R) {
        k_cpq_square<real><<<grid_for(N), kBlock, 0, s>>>(N, R, dtN.p);
        PFDR_HIP(hipGetLastError());
        real a = seq_sum(dtN.p, N);
        a *= real(0.5);
        return a;
    }

    void setup(const pfdr_cp_problem &p, bool want_obj) override {
        V = p.V, E = p.E, N = p.N;
        const bool bounds = flavour == Flavour::Bounds;
        // flavour: the l1 weights and positivity, or the box
        has_l1 = !bounds && p.La_l1 != nullptr;
        if (bounds) min = (real)p.min, max = (real)p.max;
        else positivity = p.positivity;
        const real *Y = (const real *)p.Y, *A = (const real *)p.A;
        const int dt = sizeof(real) == 4 ? PFDR_F32 : PFDR_F64;
        const bool dev = p.mem == PFDR_MEM_DEVICE;
        // ---- the problem, once, into HBM
        DevBuf<real> dLa, dL1;
        DevBuf<int> dEu, dEv;
        {
            HostPins hp(s);
            const size_t asz = N > 0 ? (size_t)N * V : N < 0 ? (size_t)V * V : A ? (size_t)V : 0;
            cp_take(dY, Y, N > 0 ? (size_t)N : (size_t)V, p.mem, hp, s);
            if (!dev && !sparse) cp_take(dA, A, asz, p.mem, hp, s);
            cp_take(dEu, p.Eu, (size_t)E, p.mem, hp, s);
            cp_take(dEv, p.Ev, (size_t)E, p.mem, hp, s);
            cp_take(dLa, (const real *)p.La_d1, (size_t)E, p.mem, hp, s);
            if (has_l1) cp_take(dL1, (const real *)p.La_l1, (size_t)V, p.mem, hp, s);
            hp.release();
        }
        pA = !A ? nullptr : dev ? A : dA.p;
        if (sparse) sp.take(N, V, sparse, p.mem, s);
        CP_ABI(pfdr_cpgraph_create(&g, dt, V, E, dEu.p, dEv.p, dLa.p, has_l1 ? dL1.p : nullptr,
                                   PFDR_MEM_DEVICE));

        // ---- initialize (l1 :94-175 / bounds :66-170): the one-component solution
        const auto t = clock::now();
        real rY = real(0), rAA = real(0), rL1s = real(0);
        DevBuf<real> drA0;
        if (N > 0) {
            drA0.alloc(N);
            dtN.alloc(N);
            dR.alloc(N);
            if (sparse) sp.colsum(1, nullptr, nullptr, drA0.p, s);
            else k_cpq_colsum<real><<<grid_for(N), kBlock, 0, s>>>(N, V, pA, drA0.p);
            k_cpq_init_products<real><<<grid_for(N), kBlock, 0, s>>>(N, drA0.p, dY.p, dtN.p,
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
        if (has_l1) rL1s = seq_sum(dL1.p, V);
        // flavour: the least-square value under the prox of l1 + positivity
        // (l1 :138-140), or projected on the box (bounds :138-139)
        real x0 = real(0);
        if (bounds) {
            x0 = rY / rAA;
            if (x0 < min) x0 = min;
            else if (x0 > max) x0 = max;
        } else if (rY > rL1s) {
            x0 = (rY - rL1s) / rAA;
        } else if (!positivity && rY < -rL1s) {
            x0 = (rY + rL1s) / rAA;
        }
        rV = 1;
        drX.alloc(1);
        PFDR_HIP(hipMemcpyAsync(drX.p, &x0, sizeof(real), hipMemcpyHostToDevice, s));
        PFDR_HIP(hipStreamSynchronize(s));
        CP_ABI(pfdr_cpgraph_set_values(g, drX.p, PFDR_MEM_DEVICE));
        if (N > 0) {
            k_cpq_init_residual<real><<<grid_for(N), kBlock, 0, s>>>(N, drA0.p, dY.p, x0, dR.p);
            PFDR_HIP(hipGetLastError());
        }
        obj_known = false;
        if (want_obj) {
            if (N > 0) obj = half_norm2(dR.p);
            else obj = x0 * (real(0.5) * rAA * x0 - rY);
            if (has_l1) obj += rL1s * (x0 < real(0) ? -x0 : x0);
            obj_known = true;
        }
        PFDR_HIP(hipStreamSynchronize(s));
        setup_sums = since(t);
        dCv.alloc(V);
        dVc.alloc(V);
        drVc.alloc((size_t)V + 1);
        CP_ABI(pfdr_cpgraph_get_components(g, nullptr, dCv.p, nullptr, nullptr, PFDR_MEM_DEVICE));
    }

    // component column sums (and, preAt, the reduced normal equations) of pfdr_cp_reduce
    void reduce(int preAt, real *rA, real *rAA, real *rY, real *L) {
        if (sp.m.nnz)
            CP_ABI(cp_reduce_sparse<real>(sp, dY.p, rV, drVc.p, dVc.p, preAt, rA, rAA, rY, L));
        else if (sizeof(real) == 4)
            CP_ABI(pfdr_cp_reduce_f32(N, V, (const float *)pA, (const float *)dY.p, rV, drVc.p,
                                      dVc.p, preAt, PFDR_MEM_DEVICE, 1e-3f, 100, 10, (float *)rA,
                                      (float *)rAA, (float *)rY, (float *)L, nullptr));
        else
            CP_ABI(pfdr_cp_reduce_f64(N, V, (const double *)pA, (const double *)dY.p, rV, drVc.p,
                                      dVc.p, preAt, PFDR_MEM_DEVICE, 1e-3, 100, 10, (double *)rA,
                                      (double *)rAA, (double *)rY, (double *)L, nullptr));
    }

    // R = Y - A X at the graph's components and drX (l1 :889-901 / bounds
    // :866-878): the component column sums of pfdr_cp_reduce, then
    // k_cpq_residual, as the loop does
    void residual_from_state() {
        CP_ABI(pfdr_cpgraph_get_components(g, nullptr, nullptr, dVc.p, drVc.p, PFDR_MEM_DEVICE));
        DevBuf<real> L(rV);
        if (reduced != PFDR_REDUCED_DENSE) {
            // the same sums over the stored entries, through the equilibration's
            // divide and multiply (no norm: R does not read L); a column of
            // norm 0 takes the dense branch, as in the loop
            CpReduced<real> rs;
            sp.reduced(rV, drVc.p, dVc.p, rs, s);
            if (rs.colnorm(L.p, s) < 0) {
                rs.scale(L.p, 0, s);
                rs.scale(L.p, 1, s);
                rs.residual(drX.p, dY.p, dR.p, s);
                PFDR_HIP(hipStreamSynchronize(s));
                return;
            }
        }
        DevBuf<real> rA((size_t)N * rV);
        reduce(0, rA.p, nullptr, nullptr, L.p);
        k_cpq_residual<real><<<grid_for(N), kBlock, 0, s>>>(N, rV, rA.p, drX.p, dY.p, dR.p);
        PFDR_HIP(hipGetLastError());
        PFDR_HIP(hipStreamSynchronize(s));
    }

    void adopt(int rV_new, const void *x, const void *R) override {
        rV = rV_new;
        drX.alloc(rV);
        PFDR_HIP(hipMemcpyAsync(drX.p, x, sizeof(real) * rV, hipMemcpyDeviceToDevice, s));
        PFDR_HIP(hipStreamSynchronize(s));
        CP_ABI(pfdr_cpgraph_set_values(g, drX.p, PFDR_MEM_DEVICE));
        CP_ABI(pfdr_cpgraph_get_components(g, nullptr, dCv.p, nullptr, nullptr, PFDR_MEM_DEVICE));
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
    bool holds_sparse_A() const override { return sp.m.nnz > 0; }
    const void *values() const override { return drX.p; }
    const void *residual() const override { return N > 0 ? dR.p : nullptr; }
    void forget_objective() override { obj_known = false; }
    void stats(double *seconds, int64_t *counts) const override {
        cp_write_stats(st, seconds, counts);
    }

    void loop(clock::time_point t0, const pfdr_cp_params &q, int *CP_it_out, double *Time,
              void *Obj_, void *Dif_) override {
        const real CP_difTol = (real)q.CP_difTol;
        const int CP_itMax = q.CP_itMax, verbose = q.verbose;
        real *Obj = (real *)Obj_, *Dif = (real *)Dif_;
        auto t = t0;
        st = CpStats{};
        sparse_its = dense_direct_its = max_rnnz = 0;
        pre_sparse_its = pre_dense_its = pre_max_rnnz = 0;
        const bool bounds = flavour == Flavour::Bounds;
        // flavour: the two-layer cut (duplex :469-545); else one cut when nothing
        // but the d1 term bends the functional (bounds :392), or two
        const bool two = flavour == Flavour::Duplex && (has_l1 || positivity);
        const bool one = bounds ? -Lim<real>::huge == min && max == Lim<real>::huge
                                : !has_l1 && !positivity;
        const real eps = (real(0) < CP_difTol && CP_difTol < Lim<real>::eps) ? CP_difTol
                                                                            : Lim<real>::eps;
        int rE = 0;  // a restart reports no reduced edge before its first iteration
        if (Obj) Obj[0] = obj_known ? obj : std::numeric_limits<real>::quiet_NaN();

        // ---- cut pursuit
        DevBuf<int> dCv_;
        const size_t nodes = two ? 2 * (size_t)V : (size_t)V;  // of the cut's network
        DevBuf<real> drX_, dtr(nodes), drc(E > 0 ? E : 1), dlink, t1, t2;
        DevBuf<uint8_t> dseg(nodes);
        if (two) dlink.alloc(V);
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
        int it = 0, pit = q.itMax;
        auto capacities = [&](int which) {
            if (bounds)
                CP_ABI(pfdr_cpgraph_capacities_bounds(g, which, (double)min, (double)max, dtr.p,
                                                      drc.p, PFDR_MEM_DEVICE));
            else
                CP_ABI(pfdr_cpgraph_capacities(g, which, positivity, dtr.p, drc.p,
                                               PFDR_MEM_DEVICE));
        };
        auto cut = [&]() {
            int64_t rounds = 0, relabels = 0;
            if (two)
                CP_ABI(pfdr_cpgraph_mincut_duplex(g, dtr.p, dlink.p, drc.p, PFDR_MEM_DEVICE,
                                                  dseg.p, nullptr, &rounds));
            else
                CP_ABI(pfdr_cpgraph_mincut(g, PFDR_ARCS_BOTH, dtr.p, drc.p, PFDR_MEM_DEVICE,
                                           dseg.p, nullptr, &rounds));
            CP_ABI(pfdr_cpgraph_mincut_relabels(g, &relabels));
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
            // steepest cuts (l1 :337-556 / bounds :331-529)
            t = clock::now();
            if (sp.m.nnz)
                CP_ABI(cpgraph_gradient_sparse(g, &sp, dR.p));
            else
                CP_ABI(pfdr_cpgraph_gradient(g, N, pA, dY.p, N > 0 ? dR.p : nullptr,
                                             PFDR_MEM_DEVICE, nullptr));
            st.gradient += since(t);
            t = clock::now();
            int w = 0, n = 0;
            if (two) {
                CP_ABI(pfdr_cpgraph_capacities_duplex(g, positivity, dtr.p, dlink.p, drc.p,
                                                      PFDR_MEM_DEVICE));
                cut();
                CP_ABI(pfdr_cpgraph_activate_duplex(g, dseg.p, PFDR_MEM_DEVICE, &w));
            } else if (one) {
                capacities(0);
                cut();
                CP_ABI(pfdr_cpgraph_activate(g, dseg.p, PFDR_MEM_DEVICE, &w));
            } else {
                capacities(1);
                cut();
                // the second cut's capacities, from the activity before the first's activations
                capacities(2);
                CP_ABI(pfdr_cpgraph_activate(g, dseg.p, PFDR_MEM_DEVICE, &w));
                cut();
                CP_ABI(pfdr_cpgraph_activate(g, dseg.p, PFDR_MEM_DEVICE, &n));
                w += n;
            }
            st.cuts += since(t);
            if (w == 0) {  // l1 :556-563 / bounds :535-542
                if (track) {
                    dif = real(0);
                    if (Dif) Dif[it] = dif;
                }
                it++;
                if (Obj) Obj[it] = Obj[it - 1];
                continue;
            }
            // reduced graph and problem (l1 :568-841 / bounds :547-813)
            t = clock::now();
            CP_ABI(pfdr_cpgraph_components(g, &rV));
            CP_ABI(pfdr_cpgraph_reduced_graph(g, (double)eps, &rE));
            CP_ABI(pfdr_cpgraph_get_components(g, nullptr, dCv.p, dVc.p, drVc.p, PFDR_MEM_DEVICE));
            DevBuf<int> rEu(rE > 0 ? rE : 1), rEv(rE > 0 ? rE : 1);
            DevBuf<real> rLa(rE > 0 ? rE : 1), rL1;
            if (has_l1) rL1.alloc(rV);
            CP_ABI(pfdr_cpgraph_get_reduced(g, rEu.p, rEv.p, rLa.p, has_l1 ? rL1.p : nullptr,
                                            PFDR_MEM_DEVICE));
            // l1 :671 / bounds :648
            const int preAt = N <= 0 || rV < (2L * N * pit) / ((long)N + pit);
            DevBuf<real> rA, rAAd, rYd, L(rV);
            // a direct iteration of the sparse mode keeps rA sparse, unless a
            // reduced column has norm 0 (a sparse session refuses it): then,
            // and in every other case, the dense rA -- but for a premultiplied
            // iteration (N > 0) of PFDR_REDUCED_SPARSE_ALL, which keeps rA
            // sparse too and sums rAA and rY over its entries
            CpReduced<real> rs;
            bool sparse_rA = false;
            if (!preAt && reduced != PFDR_REDUCED_DENSE) {
                DevBuf<real> l(rV);
                sparse_rA = cp_reduce_sparse_direct<real>(sp, rV, drVc.p, dVc.p, real(1e-3), 100,
                                                          10, rs, l.p, L.p, s) < 0;
            } else if (preAt && N > 0 && reduced == PFDR_REDUCED_SPARSE_ALL) {
                DevBuf<real> l(rV);
                rYd.alloc(rV);
                rAAd.alloc((size_t)rV * rV);
                cp_reduce_sparse_normal<real>(sp, dY.p, rV, drVc.p, dVc.p, real(1e-3), 100, 10, rs,
                                              rAAd.p, rYd.p, l.p, L.p, s);
                sparse_rA = true;
            }
            if (!sparse_rA) {
                if (N > 0) rA.alloc((size_t)N * rV);
                if (preAt) {
                    rYd.alloc(rV);
                    rAAd.alloc(N == 0 ? (size_t)rV : (size_t)rV * rV);
                }
                reduce(preAt, rA.p, rAAd.p, rYd.p, L.p);
            }
            if (preAt && N > 0) {
                if (sparse_rA) {
                    pre_sparse_its++;
                    if (rs.m.nnz > pre_max_rnnz) pre_max_rnnz = rs.m.nnz;
                } else {
                    pre_dense_its++;
                }
            } else if (sparse_rA) {
                sparse_its++;
                if (rs.m.nnz > max_rnnz) max_rnnz = rs.m.nnz;
            } else if (!preAt) {
                dense_direct_its++;
            }
            st.graph += since(t);
            // PFDR from zero (l1 :843-859 / bounds :824-836)
            t = clock::now();
            drX.alloc(rV);
            PFDR_HIP(hipMemsetAsync(drX.p, 0, sizeof(real) * rV, s));
            PFDR_HIP(hipStreamSynchronize(s));
            {
                pfdr_problem p{};
                p.kind = bounds ? PFDR_KIND_BOUNDS : PFDR_KIND_L1;  // flavour
                p.dtype = sizeof(real) == 4 ? PFDR_F32 : PFDR_F64;
                p.mem = PFDR_MEM_DEVICE;
                p.V = rV;
                p.E = rE;
                p.N = preAt ? (N == 0 ? 0 : -rV) : N;
                p.X = drX.p;
                p.Y = preAt ? rYd.p : dY.p;
                p.A = preAt ? rAAd.p : sparse_rA ? nullptr : rA.p;
                p.Eu = rEu.p;
                p.Ev = rEv.p;
                p.La_d1 = rLa.p;
                p.La_l1 = has_l1 ? rL1.p : nullptr;  // these four: null / zero
                p.positivity = positivity;           // where the flavour has none
                p.min = (double)min;
                p.max = (double)max;
                p.Ltype = PFDR_LIPSCHITZ_DIAG;
                p.L = L.p;
                p.rho = (real)q.rho;
                p.condMin = (real)q.condMin;
                p.difRcd = (real)q.difRcd;
                p.difTol = (real)q.difTol;
                p.itMax = q.itMax;
                p.verbose = verbose;
                if (sparse_rA && !preAt)
                    pit = cp_pfdr_solve_sparse(p, rs.csc(), sizeof(real) * rV, s);
                else
                    pit = cp_pfdr_solve(p, sizeof(real) * rV, s);
            }
            st.pfdr += since(t);
            st.pfdr_it += pit;
            t = clock::now();
            CP_ABI(pfdr_cpgraph_set_values(g, drX.p, PFDR_MEM_DEVICE));
            CP_ABI(pfdr_cpgraph_merge(g, (double)eps, (double)CP_difTol, &n));
            st.graph += since(t);
            // progress (l1 :888-923 / bounds :865-901)
            t = clock::now();
            if (sparse_rA) {
                rs.residual(drX.p, dY.p, dR.p, s);
            } else if (N > 0) {
                k_cpq_residual<real><<<grid_for(N), kBlock, 0, s>>>(N, rV, rA.p, drX.p, dY.p, dR.p);
                PFDR_HIP(hipGetLastError());
            }
            if (track) {
                k_cpq_evolution<real><<<grid_for(V), kBlock, 0, s>>>(V, dCv.p, drX.p, dCv_.p,
                                                                    drX_.p, t1.p, t2.p);
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
            if (Obj) {  // l1 :927-975 / bounds :906-942
                DevBuf<real> tt((size_t)std::max(rV, std::max(rE, 1)));
                if (N > 0) {
                    Obj[it] = half_norm2(dR.p);
                } else {
                    k_cpq_obj_quad<real><<<grid_for(rV), kBlock, 0, s>>>(rV, N < 0, rAAd.p, rYd.p,
                                                                        drX.p, tt.p);
                    PFDR_HIP(hipGetLastError());
                    Obj[it] = seq_sum(tt.p, rV);
                }
                if (rE > 0) {
                    k_cpq_obj_d1<real><<<grid_for(rE), kBlock, 0, s>>>(rE, rEu.p, rEv.p, rLa.p,
                                                                      drX.p, tt.p);
                    PFDR_HIP(hipGetLastError());
                    Obj[it] += seq_sum(tt.p, rE);
                }
                if (has_l1) {  // flavour: the l1 term
                    k_cpq_obj_l1<real><<<grid_for(rV), kBlock, 0, s>>>(rV, rL1.p, drX.p, tt.p);
                    PFDR_HIP(hipGetLastError());
                    Obj[it] += seq_sum(tt.p, rV);
                }
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
        cp_download<real>(s, V, dCv.p, Cv, drX.p, (size_t)rV, rX_out);
    }
};

// The entries' common part; min, max: bounds only, La_l1, positivity: l1 and duplex only.
template <typename real>
int cp_entry(const char *fn, Flavour f, int V, int E, int N, int *rV, int *Cv, real *rX,
             const real *Y, const real *A, const int *Eu, const int *Ev, const real *La_d1,
             const real *La_l1, int positivity, real min, real max, real CP_difTol, int CP_itMax,
             int *CP_it, real rho, real condMin, real difRcd, real difTol, int itMax,
             double *Time, real *Obj, real *Dif, int verbose) {
    if (V <= 0 || E < 0 || !rV || !Cv || !rX || !Y || CP_itMax < 0 ||
        (E > 0 && (!Eu || !Ev || !La_d1)))
        return report_error(fn, "invalid arguments");
    if (N != 0 && !A) return report_error(fn, "N != 0 needs A");
    if (N < 0 && -N != V) return report_error(fn, "N < 0 needs A = A^tA and N = -V");
    if (f == Flavour::Bounds && !(min <= max))
        return report_error(fn, "the bounds need min <= max");
    pfdr_cp_problem p{};
    p.kind = f == Flavour::Bounds ? PFDR_KIND_BOUNDS : PFDR_KIND_L1;
    p.duplex = f == Flavour::Duplex;
    p.mem = PFDR_MEM_HOST;
    p.V = V, p.E = E, p.N = N;
    p.Y = Y, p.A = A, p.Eu = Eu, p.Ev = Ev, p.La_d1 = La_d1, p.La_l1 = La_l1;
    p.positivity = positivity;
    p.min = min, p.max = max;
    const pfdr_cp_params q{CP_difTol, CP_itMax, rho, condMin, difRcd, difTol, itMax, verbose};
    CpStats *record = f == Flavour::Duplex   ? &g_duplex_stats
                      : f == Flavour::Bounds ? &g_bounds_stats
                                             : nullptr;
    return cp_run_entry<QuadDriver<real>>(fn, record, p, q, rV, Cv, rX, CP_it, Time, Obj, Dif, f);
}

CpDriverBase *make_driver(int dtype, Flavour f) {
    if (dtype == PFDR_F32) return new QuadDriver<float>(f);
    return new QuadDriver<double>(f);
}

}  // namespace

CpDriverBase *cp_make_l1_driver(int dtype, bool duplex) {
    return make_driver(dtype, duplex ? Flavour::Duplex : Flavour::L1);
}

CpDriverBase *cp_make_bounds_driver(int dtype) { return make_driver(dtype, Flavour::Bounds); }

}  // namespace pfdr

extern "C" int pfdr_cp_quadratic_d1_l1_f32(int V, int E, int N, int *rV, int *Cv, float *rX,
    const float *Y, const float *A, const int *Eu, const int *Ev, const float *La_d1,
    const float *La_l1, int positivity, float CP_difTol, int CP_itMax, int *CP_it, float rho,
    float condMin, float difRcd, float difTol, int itMax, double *Time, float *Obj, float *Dif,
    int verbose) {
    return pfdr::cp_entry<float>("pfdr_cp_quadratic_d1_l1_f32", pfdr::Flavour::L1, V, E, N, rV,
                                 Cv, rX, Y, A, Eu, Ev, La_d1, La_l1, positivity, 0, 0, CP_difTol,
                                 CP_itMax, CP_it, rho, condMin, difRcd, difTol, itMax, Time, Obj,
                                 Dif, verbose);
}

extern "C" int pfdr_cp_quadratic_d1_l1_f64(int V, int E, int N, int *rV, int *Cv, double *rX,
    const double *Y, const double *A, const int *Eu, const int *Ev, const double *La_d1,
    const double *La_l1, int positivity, double CP_difTol, int CP_itMax, int *CP_it, double rho,
    double condMin, double difRcd, double difTol, int itMax, double *Time, double *Obj,
    double *Dif, int verbose) {
    return pfdr::cp_entry<double>("pfdr_cp_quadratic_d1_l1_f64", pfdr::Flavour::L1, V, E, N, rV,
                                  Cv, rX, Y, A, Eu, Ev, La_d1, La_l1, positivity, 0, 0,
                                  CP_difTol, CP_itMax, CP_it, rho, condMin, difRcd, difTol, itMax,
                                  Time, Obj, Dif, verbose);
}

extern "C" int pfdr_cp_quadratic_d1_l1_duplex_f32(int V, int E, int N, int *rV, int *Cv,
    float *rX, const float *Y, const float *A, const int *Eu, const int *Ev, const float *La_d1,
    const float *La_l1, int positivity, float CP_difTol, int CP_itMax, int *CP_it, float rho,
    float condMin, float difRcd, float difTol, int itMax, double *Time, float *Obj, float *Dif,
    int verbose) {
    return pfdr::cp_entry<float>("pfdr_cp_quadratic_d1_l1_duplex_f32", pfdr::Flavour::Duplex, V,
                                 E, N, rV, Cv, rX, Y, A, Eu, Ev, La_d1, La_l1, positivity, 0, 0,
                                 CP_difTol, CP_itMax, CP_it, rho, condMin, difRcd, difTol, itMax,
                                 Time, Obj, Dif, verbose);
}

extern "C" int pfdr_cp_quadratic_d1_l1_duplex_f64(int V, int E, int N, int *rV, int *Cv,
    double *rX, const double *Y, const double *A, const int *Eu, const int *Ev,
    const double *La_d1, const double *La_l1, int positivity, double CP_difTol, int CP_itMax,
    int *CP_it, double rho, double condMin, double difRcd, double difTol, int itMax,
    double *Time, double *Obj, double *Dif, int verbose) {
    return pfdr::cp_entry<double>("pfdr_cp_quadratic_d1_l1_duplex_f64", pfdr::Flavour::Duplex, V,
                                  E, N, rV, Cv, rX, Y, A, Eu, Ev, La_d1, La_l1, positivity, 0, 0,
                                  CP_difTol, CP_itMax, CP_it, rho, condMin, difRcd, difTol, itMax,
                                  Time, Obj, Dif, verbose);
}

extern "C" int pfdr_cp_quadratic_d1_l1_duplex_stats(double *seconds, int64_t *counts) {
    pfdr::cp_write_stats(pfdr::g_duplex_stats, seconds, counts);
    return PFDR_OK;
}

extern "C" int pfdr_cp_quadratic_d1_bounds_f32(int V, int E, int N, int *rV, int *Cv, float *rX,
    const float *Y, const float *A, const int *Eu, const int *Ev, const float *La_d1, float min,
    float max, float CP_difTol, int CP_itMax, int *CP_it, float rho, float condMin, float difRcd,
    float difTol, int itMax, double *Time, float *Obj, float *Dif, int verbose) {
    return pfdr::cp_entry<float>("pfdr_cp_quadratic_d1_bounds_f32", pfdr::Flavour::Bounds, V, E,
                                 N, rV, Cv, rX, Y, A, Eu, Ev, La_d1, nullptr, 0, min, max,
                                 CP_difTol, CP_itMax, CP_it, rho, condMin, difRcd, difTol, itMax,
                                 Time, Obj, Dif, verbose);
}

extern "C" int pfdr_cp_quadratic_d1_bounds_f64(int V, int E, int N, int *rV, int *Cv, double *rX,
    const double *Y, const double *A, const int *Eu, const int *Ev, const double *La_d1,
    double min, double max, double CP_difTol, int CP_itMax, int *CP_it, double rho,
    double condMin, double difRcd, double difTol, int itMax, double *Time, double *Obj,
    double *Dif, int verbose) {
    return pfdr::cp_entry<double>("pfdr_cp_quadratic_d1_bounds_f64", pfdr::Flavour::Bounds, V, E,
                                  N, rV, Cv, rX, Y, A, Eu, Ev, La_d1, nullptr, 0, min, max,
                                  CP_difTol, CP_itMax, CP_it, rho, condMin, difRcd, difTol, itMax,
                                  Time, Obj, Dif, verbose);
}

extern "C" int pfdr_cp_quadratic_d1_bounds_stats(double *seconds, int64_t *counts) {
    pfdr::cp_write_stats(pfdr::g_bounds_stats, seconds, counts);
    return PFDR_OK;
}
