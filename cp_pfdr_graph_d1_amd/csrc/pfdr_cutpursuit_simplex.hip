// The whole cut pursuit of the simplex driver, CP_PFDR_graph_loss_d1_simplex<real>
// of the reference (src/CP_PFDR_graph_loss_d1_simplex.cpp), on one GPU: the
// loop of INTEGRATION.md §7 over the library's own steps -- the simplex graph
// steps of pfdr_cpgraph.hip, the cut of pfdr_mincut.hip (PFDR_ARCS_FORWARD) and
// the simplex PFDR session -- with PFDR_MEM_DEVICE throughout.  Host arrays
// come in once and Cv / rP go out once; in between only scalars cross PCIe
// (counts, rV, rE, the evolution and objective sums).
//
// The scalar sums (the iterate evolution :808-866 and the objective :870-917)
// are added one by one in `real` in the reference's order
// (ordered_segment_sums), like the reference built without OpenMP.
//
// Two departures from the reference, both in DESIGN §8: Obj[0] is the
// functional at the one-component solution (the reference's initialize()
// :119-146 does not evaluate it for al != 0), and al outside [0, 1] is an
// argument error (the reference's KL branch then reads constants it never set).
//
// The driver runs in three phases (pfdr_cp_driver.hpp): setup (upload, graph,
// the reference's initialize()), the loop from the state the driver holds, and
// the download.  An entry is the three in a row; the resumable solver
// (pfdr_cp_solver.hip) keeps the driver and runs the same loop again.
#include <algorithm>
#include <cmath>
#include <limits>

#include "pfdr_cp_driver.hpp"

namespace pfdr {

namespace {

// What the last call on this thread spent where (pfdr_cp_loss_d1_simplex_stats).
constexpr int kStatExp = 64;  // expansions whose rounds / relabels are kept one by one
struct Stats : CpStats {  // ncuts: the expansions
    int64_t exp_rounds[kStatExp] = {}, exp_relabels[kStatExp] = {};
};
thread_local Stats g_stats;

// terms |rP[Cv[v]] - rP_[Cv_[v]]| of the iterate evolution, (v, k) order (:848-860)
template <typename real>
__global__ void k_cps_evolution(long n, int K, const int *__restrict__ Cv,
                                const real *__restrict__ rP, const int *__restrict__ Cv_,
                                const real *__restrict__ rP_, real *__restrict__ t) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long v = i / K;
    const int k = (int)(i - v * K);
    real d = rP[(long)Cv[v] * K + k] - rP_[(long)Cv_[v] * K + k];
    if (d < real(0)) d = -d;
    t[i] = d;
}

// first largest label of every component (:289-298, :815-820)
template <typename real>
__global__ void k_cps_labels(int rV, int K, const real *__restrict__ rP, int *__restrict__ lab) {
    const int rv = blockIdx.x * blockDim.x + threadIdx.x;
    if (rv >= rV) return;
    const real *p = rP + (long)rv * K;
    real a = p[0];
    int i = 0;
    for (int k = 1; k < K; k++)
        if (p[k] > a) {
            a = p[k];
            i = k;
        }
    lab[rv] = i;
}

// 1 for every vertex whose component's label changed (:823-826)
template <typename real>
__global__ void k_cps_label_evolution(int V, const int *__restrict__ Cv,
                                      const int *__restrict__ lab, const int *__restrict__ Cv_,
                                      const int *__restrict__ lab_, real *__restrict__ t) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    t[v] = lab[Cv[v]] != lab_[Cv_[v]] ? real(1) : real(0);
}

// linear loss: -rP[i] rQ[i] over rV K (:875)
template <typename real>
__global__ void k_cps_obj_linear(long n, const real *__restrict__ rP,
                                 const real *__restrict__ rQ, real *__restrict__ t) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    t[i] = -(rP[i] * rQ[i]);
}

// quadratic loss: (rP[Cv[v]] - Q[v])^2 over (v, k) (:879-886)
template <typename real>
__global__ void k_cps_obj_quadratic(long n, int K, const int *__restrict__ Cv,
                                    const real *__restrict__ rP, const real *__restrict__ Q,
                                    real *__restrict__ t) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long v = i / K;
    const int k = (int)(i - v * K);
    const real c = rP[(long)Cv[v] * K + k] - Q[i];
    t[i] = c * c;
}

// smoothed Kullback-Leibler: c log(c / (al/K + (1 - al) p)), c = al/K + (1 - al) q (:891-898)
template <typename real>
__global__ void k_cps_obj_kl(long n, int K, real alK, real al1, const int *__restrict__ Cv,
                             const real *__restrict__ rP, const real *__restrict__ Q,
                             real *__restrict__ t) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long v = i / K;
    const int k = (int)(i - v * K);
    const real c = alK + al1 * Q[i];
    const real p = alK + al1 * rP[(long)Cv[v] * K + k];
    t[i] = c * log(c / p);
}

// rLa_d1[re] sum_k |rP_u[k] - rP_v[k]|, k in order (:905-915)
template <typename real>
__global__ void k_cps_obj_d1(int rE, int K, const int *__restrict__ rEu,
                             const int *__restrict__ rEv, const real *__restrict__ rLa,
                             const real *__restrict__ rP, real *__restrict__ t) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rE) return;
    const real *pu = rP + (long)rEu[e] * K, *pv = rP + (long)rEv[e] * K;
    real b = real(0);
    for (int k = 0; k < K; k++) {
        real c = pu[k] - pv[k];
        if (c < real(0)) c = -c;
        b += c;
    }
    t[e] = rLa[e] * b;
}

// out[i] = log(x[i]) as k_cps_obj_kl computes it (pfdr_debug_device_log)
template <typename real>
__global__ void k_cps_log(long n, const real *__restrict__ x, real *__restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = log(x[i]);
}

template <typename real>
void debug_log(long n, const real *x, real *out) {
    hipStream_t s = lib_stream();
    DevBuf<real> dx((size_t)n), dy((size_t)n);
    PFDR_HIP(hipMemcpyAsync(dx.p, x, sizeof(real) * n, hipMemcpyHostToDevice, s));
    k_cps_log<real><<<grid_for(n), kBlock, 0, s>>>(n, dx.p, dy.p);
    PFDR_HIP(hipGetLastError());
    PFDR_HIP(hipMemcpyAsync(out, dy.p, sizeof(real) * n, hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
}

template <typename real>
struct SxDriver : CpDriverBase {
    Stats st;  // of the last run
    CpSeqSum<real> seq_sum{s};
    // the resident problem
    DevBuf<real> dQ;
    real al = real(0);
    // the state besides the graph's: label vectors, reduced observations, Cv
    DevBuf<real> drP, drQ;
    DevBuf<int> dCv;
    real obj = real(0);  // the functional at the state, when known
    bool obj_known = false;

    // the functional at (Cv, rP) with the reduced graph given (:870-917)
    real objective(int K, int V, real al, int rV, int rE, const int *Cv, const real *rP,
                   const real *rQ, const real *Q, const int *rEu, const int *rEv,
                   const real *rLa) {
        const long VK = (long)V * K, rVK = (long)rV * K;
        if (VK >= (1L << 31)) throw std::runtime_error("sum of 2^31 or more terms");
        DevBuf<real> t((size_t)std::max(al == real(0) ? rVK : VK, (long)std::max(rE, 1)));
        real a;
        if (al == real(0)) {
            k_cps_obj_linear<real><<<grid_for(rVK), kBlock, 0, s>>>(rVK, rP, rQ, t.p);
            PFDR_HIP(hipGetLastError());
            a = seq_sum(t.p, rVK);
        } else if (al == real(1)) {
            k_cps_obj_quadratic<real><<<grid_for(VK), kBlock, 0, s>>>(VK, K, Cv, rP, Q, t.p);
            PFDR_HIP(hipGetLastError());
            a = seq_sum(t.p, VK);
            a *= real(0.5);
        } else {
            const real alK = al / (real)K, al1 = real(1) - al;
            k_cps_obj_kl<real><<<grid_for(VK), kBlock, 0, s>>>(VK, K, alK, al1, Cv, rP, Q, t.p);
            PFDR_HIP(hipGetLastError());
            a = seq_sum(t.p, VK);
        }
        real b = real(0);
        if (rE > 0) {
            k_cps_obj_d1<real><<<grid_for(rE), kBlock, 0, s>>>(rE, K, rEu, rEv, rLa, rP, t.p);
            PFDR_HIP(hipGetLastError());
            b = seq_sum(t.p, rE);
        }
        return a + b;
    }

    void setup(const pfdr_cp_problem &p, bool want_obj) override {
        V = p.V, E = p.E, K = p.K;
        al = (real)p.al;
        const int dt = sizeof(real) == 4 ? PFDR_F32 : PFDR_F64;
        const long VK = (long)V * K;
        // ---- the problem, once, into HBM
        DevBuf<real> dLa;
        DevBuf<int> dEu, dEv;
        {
            HostPins hp(s);
            cp_take(dQ, (const real *)p.Y, (size_t)VK, p.mem, hp, s);
            cp_take(dEu, p.Eu, (size_t)E, p.mem, hp, s);
            cp_take(dEv, p.Ev, (size_t)E, p.mem, hp, s);
            cp_take(dLa, (const real *)p.La_d1, (size_t)E, p.mem, hp, s);
            hp.release();
        }
        CP_ABI(pfdr_cpgraph_create(&g, dt, V, E, dEu.p, dEv.p, dLa.p, nullptr, PFDR_MEM_DEVICE));
        CP_ABI(pfdr_cpgraph_simplex_setup(g, K, (double)al, dQ.p, PFDR_MEM_DEVICE));

        // ---- initialize (:96-116): one component, its rP from the observations
        rV = 1;
        drP.alloc((size_t)K);
        drQ.alloc((size_t)K);
        CP_ABI(pfdr_cpgraph_simplex_observations(g, drP.p, drQ.p, nullptr, PFDR_MEM_DEVICE));
        dCv.alloc(V);
        CP_ABI(pfdr_cpgraph_get_components(g, nullptr, dCv.p, nullptr, nullptr, PFDR_MEM_DEVICE));
        // the functional itself, as every later Obj[k] with rV = 1
        obj_known = false;
        if (want_obj) {
            const auto t = clock::now();
            obj = objective(K, V, al, 1, 0, dCv.p, drP.p, drQ.p, dQ.p, nullptr, nullptr, nullptr);
            obj_known = true;
            setup_sums = since(t);
        }
    }

    void adopt(int rV_new, const void *x, const void *) override {
        rV = rV_new;
        drP.alloc((size_t)rV * K);
        PFDR_HIP(hipMemcpyAsync(drP.p, x, sizeof(real) * rV * K, hipMemcpyDeviceToDevice, s));
        PFDR_HIP(hipStreamSynchronize(s));
        CP_ABI(pfdr_cpgraph_simplex_set_values(g, drP.p, PFDR_MEM_DEVICE));
        CP_ABI(pfdr_cpgraph_get_components(g, nullptr, dCv.p, nullptr, nullptr, PFDR_MEM_DEVICE));
        obj_known = false;
    }
    const void *values() const override { return drP.p; }
    const void *residual() const override { return nullptr; }
    void forget_objective() override { obj_known = false; }
    void stats(double *seconds, int64_t *counts) const override {
        cp_write_stats(st, seconds, counts);
    }

    void loop(clock::time_point t0, const pfdr_cp_params &q, int *CP_it_out, double *Time,
              void *Obj_, void *Dif_) override {
        const real CP_difTol = (real)q.CP_difTol, rho = (real)q.rho, condMin = (real)q.condMin,
                   difRcd = (real)q.difRcd, difTol = (real)q.difTol;
        const int CP_itMax = q.CP_itMax, itMax = q.itMax, verbose = q.verbose;
        real *Obj = (real *)Obj_, *Dif = (real *)Dif_;
        st = Stats{};
        const int dt = sizeof(real) == 4 ? PFDR_F32 : PFDR_F64;
        // :214-231 as compiled: (ZERO < c < a) is ((0 < c) < a), 1 < a never holds
        real eps;
        {
            const real a = Lim<real>::eps;
            const real b = CP_difTol >= real(1) ? CP_difTol / (real)V : CP_difTol;
            real c = difTol >= real(1) ? difTol / (real)V : difTol;
            c = b < c ? b : c;
            eps = ((real)(real(0) < c) < a) ? c : a;
        }
        const long VK = (long)V * K;
        int rE = 0;  // a restart reports no reduced edge before its first iteration
        if (Obj) Obj[0] = obj_known ? obj : std::numeric_limits<real>::quiet_NaN();
        DevBuf<int> dCv_, dlab, dlab_;
        DevBuf<real> drP_, drLaf(1), dtr(V), drc(E > 0 ? E : 1), tt;
        DevBuf<uint8_t> dseg(V);
        // ---- tracking (:282-306)
        const bool track = CP_difTol > real(0) || Dif;
        const bool labels = CP_difTol >= real(1);
        if (track) {
            if (labels) {
                dlab.alloc(rV);
                dlab_.alloc(rV);
                k_cps_labels<real><<<grid_for(rV), kBlock, 0, s>>>(rV, K, drP.p, dlab_.p);
                PFDR_HIP(hipGetLastError());
                tt.alloc(V);
            } else {
                if (VK >= (1L << 31)) throw std::runtime_error("sum of 2^31 or more terms");
                drP_.alloc((size_t)rV * K);
                PFDR_HIP(hipMemcpyAsync(drP_.p, drP.p, sizeof(real) * rV * K,
                                        hipMemcpyDeviceToDevice, s));
                tt.alloc((size_t)VK);
            }
            dCv_.alloc(V);
            PFDR_HIP(hipMemcpyAsync(dCv_.p, dCv.p, sizeof(int) * V, hipMemcpyDeviceToDevice, s));
            PFDR_HIP(hipStreamSynchronize(s));
        }
        real dif = CP_difTol > real(1) ? CP_difTol : real(1);
        int it = 0;
        DevBuf<int> rEu, rEv;
        DevBuf<real> rLa;
        for (;;) {
            if (Time) Time[it] = since(t0);
            if (verbose) {
                printf("\n\tCut pursuit iteration %d (max. %d)\n", it, CP_itMax);
                if (CP_difTol >= real(1))
                    printf("\tlabel evolution %d (tol. %d)\n", (int)dif, (int)CP_difTol);
                else if (CP_difTol > real(0))
                    printf("\titerate evolution %g (tol. %g)\n", (double)dif, (double)CP_difTol);
                printf("\t%d connected component(s), %d reduced edge(s)\n", rV, rE);
                fflush(stdout);
            }
            if (it == CP_itMax || dif < CP_difTol) break;
            // steepest cuts (:327-618)
            auto t = clock::now();
            CP_ABI(pfdr_cpgraph_simplex_gradient(g, (double)eps, nullptr, nullptr,
                                                 PFDR_MEM_DEVICE));
            st.gradient += since(t);
            t = clock::now();
            for (int n = 1; n < K; n++) {
                int64_t rounds = 0, relabels = 0;
                CP_ABI(pfdr_cpgraph_simplex_capacities(g, n, dtr.p, drc.p, PFDR_MEM_DEVICE));
                CP_ABI(pfdr_cpgraph_mincut(g, PFDR_ARCS_FORWARD, dtr.p, drc.p, PFDR_MEM_DEVICE,
                                           dseg.p, nullptr, &rounds));
                CP_ABI(pfdr_cpgraph_mincut_relabels(g, &relabels));
                CP_ABI(pfdr_cpgraph_simplex_expand(g, n, dseg.p, PFDR_MEM_DEVICE));
                if (st.ncuts < kStatExp) {
                    st.exp_rounds[st.ncuts] = rounds;
                    st.exp_relabels[st.ncuts] = relabels;
                }
                st.ncuts++;
                st.rounds += rounds;
                st.relabels += relabels;
            }
            st.cuts += since(t);
            t = clock::now();
            int w = 0, n = 0;
            CP_ABI(pfdr_cpgraph_simplex_activate(g, &w));
            if (verbose) printf("\t%d new activated edge(s).\n", w);
            if (w == 0) {  // :631-639
                st.graph += since(t);
                if (track) {
                    dif = real(0);
                    if (Dif) Dif[it] = dif;
                }
                it++;
                if (Obj) Obj[it] = Obj[it - 1];
                continue;
            }
            // reduced graph and observations (:643-766)
            CP_ABI(pfdr_cpgraph_components(g, &rV));
            CP_ABI(pfdr_cpgraph_reduced_graph(g, (double)eps, &rE));
            CP_ABI(pfdr_cpgraph_get_components(g, nullptr, dCv.p, nullptr, nullptr,
                                               PFDR_MEM_DEVICE));
            rEu.alloc(rE > 0 ? rE : 1);
            rEv.alloc(rE > 0 ? rE : 1);
            rLa.alloc(rE > 0 ? rE : 1);
            CP_ABI(pfdr_cpgraph_get_reduced(g, rEu.p, rEv.p, rLa.p, nullptr, PFDR_MEM_DEVICE));
            const size_t rVK = (size_t)rV * K;
            drP.alloc(rVK);
            drQ.alloc(rVK);
            drLaf.alloc(rV);
            CP_ABI(pfdr_cpgraph_simplex_observations(g, drP.p, drQ.p,
                                                     al > real(0) ? drLaf.p : nullptr,
                                                     PFDR_MEM_DEVICE));
            st.graph += since(t);
            // PFDR from the components' own optima (:778-780)
            t = clock::now();
            {
                pfdr_problem p{};
                p.kind = PFDR_KIND_SIMPLEX;
                p.dtype = dt;
                p.mem = PFDR_MEM_DEVICE;
                p.V = rV;
                p.E = rE;
                p.K = K;
                p.al = al;
                p.X = drP.p;
                p.Y = drQ.p;
                p.Eu = rEu.p;
                p.Ev = rEv.p;
                p.La_d1 = rLa.p;
                p.La_l1 = al > real(0) ? drLaf.p : nullptr;
                p.rho = rho;
                p.condMin = condMin;
                p.difRcd = difRcd;
                p.difTol = difTol;
                p.itMax = itMax;
                p.verbose = verbose;
                st.pfdr_it += cp_pfdr_solve(p, sizeof(real) * rVK, s);
            }
            st.pfdr += since(t);
            t = clock::now();
            CP_ABI(pfdr_cpgraph_simplex_set_values(g, drP.p, PFDR_MEM_DEVICE));
            CP_ABI(pfdr_cpgraph_simplex_merge(g, (double)eps, &n));
            if (verbose) printf("\t%d deactivated edge(s).\n", n);
            st.graph += since(t);
            // iterate evolution (:808-866); the last partition then becomes this one,
            // in a pass of its own: every lane of a vertex reads Cv_[v]
            t = clock::now();
            if (track) {
                if (labels) {
                    dlab.alloc(rV);
                    k_cps_labels<real><<<grid_for(rV), kBlock, 0, s>>>(rV, K, drP.p, dlab.p);
                    k_cps_label_evolution<real><<<grid_for(V), kBlock, 0, s>>>(
                        V, dCv.p, dlab.p, dCv_.p, dlab_.p, tt.p);
                    PFDR_HIP(hipGetLastError());
                    dif = seq_sum(tt.p, V);
                    std::swap(dlab.p, dlab_.p);
                    std::swap(dlab.n, dlab_.n);
                } else {
                    k_cps_evolution<real><<<grid_for(VK), kBlock, 0, s>>>(VK, K, dCv.p, drP.p,
                                                                         dCv_.p, drP_.p, tt.p);
                    PFDR_HIP(hipGetLastError());
                    dif = seq_sum(tt.p, VK);
                    dif /= (real)V;
                    drP_.alloc(rVK);
                    PFDR_HIP(hipMemcpyAsync(drP_.p, drP.p, sizeof(real) * rVK,
                                            hipMemcpyDeviceToDevice, s));
                }
                PFDR_HIP(hipMemcpyAsync(dCv_.p, dCv.p, sizeof(int) * V, hipMemcpyDeviceToDevice,
                                        s));
                PFDR_HIP(hipStreamSynchronize(s));
                if (Dif) Dif[it] = dif;
            }
            it++;
            if (Obj)  // :870-917
                obj = Obj[it] = objective(K, V, al, rV, rE, dCv.p, drP.p, drQ.p, dQ.p, rEu.p,
                                          rEv.p, rLa.p);
            obj_known = Obj != nullptr;
            PFDR_HIP(hipStreamSynchronize(s));
            st.sums += since(t);
        }
        if (CP_it_out) *CP_it_out = it;
        st.total = since(t0);
    }

    void download(int *rV_out, int *Cv, void *rP_out) override {
        *rV_out = rV;
        cp_download<real>(s, V, dCv.p, Cv, drP.p, (size_t)rV * K, rP_out);
    }
};

template <typename real>
int cps_entry(const char *fn, int K, int V, int E, real al, int *rV, int *Cv, real *rP,
              const real *Q, const int *Eu, const int *Ev, const real *La_d1, real CP_difTol,
              int CP_itMax, int *CP_it, real rho, real condMin, real difRcd, real difTol,
              int itMax, double *Time, real *Obj, real *Dif, int verbose) {
    if (K < 2 || V <= 0 || E < 0 || !rV || !Cv || !rP || !Q || CP_itMax < 0 ||
        (E > 0 && (!Eu || !Ev || !La_d1)))
        return report_error(fn, "invalid arguments");
    if (!(al >= real(0) && al <= real(1))) return report_error(fn, "al must lie in [0, 1]");
    pfdr_cp_problem p{};
    p.kind = PFDR_KIND_SIMPLEX;
    p.mem = PFDR_MEM_HOST;
    p.V = V, p.E = E, p.K = K;
    p.Y = Q, p.Eu = Eu, p.Ev = Ev, p.La_d1 = La_d1;
    p.al = al;
    const pfdr_cp_params q{CP_difTol, CP_itMax, rho, condMin, difRcd, difTol, itMax, verbose};
    return cp_run_entry<SxDriver<real>>(fn, &g_stats, p, q, rV, Cv, rP, CP_it, Time, Obj, Dif);
}

}  // namespace

CpDriverBase *cp_make_simplex_driver(int dtype) {
    if (dtype == PFDR_F32) return new SxDriver<float>();
    return new SxDriver<double>();
}

}  // namespace pfdr

extern "C" int pfdr_cp_loss_d1_simplex_f32(int K, int V, int E, float al, int *rV, int *Cv,
    float *rP, const float *Q, const int *Eu, const int *Ev, const float *La_d1, float CP_difTol,
    int CP_itMax, int *CP_it, float rho, float condMin, float difRcd, float difTol, int itMax,
    double *Time, float *Obj, float *Dif, int verbose) {
    return pfdr::cps_entry<float>("pfdr_cp_loss_d1_simplex_f32", K, V, E, al, rV, Cv, rP, Q, Eu,
                                  Ev, La_d1, CP_difTol, CP_itMax, CP_it, rho, condMin, difRcd,
                                  difTol, itMax, Time, Obj, Dif, verbose);
}

extern "C" int pfdr_cp_loss_d1_simplex_f64(int K, int V, int E, double al, int *rV, int *Cv,
    double *rP, const double *Q, const int *Eu, const int *Ev, const double *La_d1,
    double CP_difTol, int CP_itMax, int *CP_it, double rho, double condMin, double difRcd,
    double difTol, int itMax, double *Time, double *Obj, double *Dif, int verbose) {
    return pfdr::cps_entry<double>("pfdr_cp_loss_d1_simplex_f64", K, V, E, al, rV, Cv, rP, Q, Eu,
                                   Ev, La_d1, CP_difTol, CP_itMax, CP_it, rho, condMin, difRcd,
                                   difTol, itMax, Time, Obj, Dif, verbose);
}

extern "C" int pfdr_debug_device_log(int dtype, int64_t n, const void *x, void *out) {
    const char *fn = "pfdr_debug_device_log";
    if (n < 0 || (n > 0 && (!x || !out)) || (dtype != PFDR_F32 && dtype != PFDR_F64))
        return pfdr::report_error(fn, "invalid arguments");
    if (n == 0) return PFDR_OK;
    try {
        if (dtype == PFDR_F32) pfdr::debug_log<float>((long)n, (const float *)x, (float *)out);
        else pfdr::debug_log<double>((long)n, (const double *)x, (double *)out);
    } catch (const pfdr::HipError &h) {
        return pfdr::report_error(fn, h);
    } catch (const std::exception &ex) {
        return pfdr::report_error(fn, ex.what());
    }
    return PFDR_OK;
}

extern "C" int pfdr_cp_loss_d1_simplex_stats(double *seconds, int64_t *counts,
                                             int64_t *exp_rounds, int64_t *exp_relabels,
                                             int n_exp) {
    const pfdr::Stats &st = pfdr::g_stats;
    pfdr::cp_write_stats(st, seconds, counts);
    const int64_t kept = st.ncuts < pfdr::kStatExp ? st.ncuts : pfdr::kStatExp;
    for (int i = 0; i < n_exp; i++) {
        if (exp_rounds) exp_rounds[i] = i < kept ? st.exp_rounds[i] : -1;
        if (exp_relabels) exp_relabels[i] = i < kept ? st.exp_relabels[i] : -1;
    }
    return PFDR_OK;
}
