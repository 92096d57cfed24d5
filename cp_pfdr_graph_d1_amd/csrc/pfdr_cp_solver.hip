// The resumable cut-pursuit solver (pfdr_cp_solver_*): the reference drivers'
// restart record (CP_restart) as a handle.  The handle owns one driver
// (pfdr_cp_driver.hpp) -- the resident problem, its pfdr_cpgraph and the state
// -- and calls the driver's loop again and again; the one-call entries run the
// same setup and the same loop once.  This file adds what moves a state in and
// out: the checks of an imported state (on the device, one flag word back),
// the partition import and the change of penalties.
//
// The check kernels are streaming, one element (or one 16-byte packet) per
// lane; they use integer atomics only and report through plain stores of 1
// into a flag array, which one last kernel packs into a word.
#include <chrono>
#include <cstdint>
#include <memory>
#include <stdexcept>

#include "pfdr_cp_driver.hpp"
#include "pfdr_cp_sparse.hpp"

namespace pfdr {

namespace {

// one flag per check, in the order the checks are named
enum {
    kChkRvcEnds = 0,   // rVc[0] = 0 and rVc[rV] = V
    kChkRvcOrder,      // rVc strictly increasing
    kChkVcRange,       // Vc[i] in [0, V)
    kChkVcOnce,        // every vertex once in Vc
    kChkCv,            // Cv[Vc[i]] = the component whose range holds i
    kChkActive,        // active[e] in {0, 1}
    kChkValuesNaN,     // no NaN in rX
    kChkResidualNaN,   // no NaN in R
    kChkBox,           // bounds: min <= rX <= max
    kChkLabel,         // label[v] in [0, nlabels)
    kChkWeight,        // weights >= 0, not NaN
    kChkCount
};
const char *const kChkName[kChkCount] = {
    "rVc must start at 0 and end at V",
    "rVc must be strictly increasing",
    "Vc holds a vertex outside [0, V)",
    "Vc is not a permutation of the vertices (a vertex is repeated)",
    "Cv disagrees with Vc and rVc",
    "active must be 0 or 1",
    "NaN in rX",
    "NaN in R",
    "rX outside [min, max]",
    "label outside [0, nlabels)",
    "weights must be nonnegative and not NaN",
};

__global__ void k_cps_rvc(int rV, int V, const int *__restrict__ rVc, int *__restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > rV) return;
    const int a = rVc[i];
    if ((i == 0 && a != 0) || (i == rV && a != V)) flag[kChkRvcEnds] = 1;
    if (i < rV && !(a < rVc[i + 1])) flag[kChkRvcOrder] = 1;
}

// seen[v] += 1 for every position holding v
__global__ void k_cps_vc_count(int V, const int *__restrict__ Vc, int *__restrict__ seen,
                               int *__restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    const int v = Vc[i];
    if (v < 0 || v >= V) {
        flag[kChkVcRange] = 1;
        return;
    }
    atomicAdd(seen + v, 1);
}

__global__ void k_cps_vc_once(int V, const int *__restrict__ seen, int *__restrict__ flag) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    if (seen[v] != 1) flag[kChkVcOnce] = 1;
}

// position i -> the last rv with rVc[rv] <= i (any rVc content stays in bounds)
__global__ void k_cps_cv(int V, int rV, const int *__restrict__ Cv, const int *__restrict__ Vc,
                         const int *__restrict__ rVc, int *__restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    int lo = 0, hi = rV;  // rVc[lo] <= i < rVc[hi] when rVc is valid
    while (hi - lo > 1) {
        const int m = lo + (hi - lo) / 2;
        if (rVc[m] <= i) lo = m;
        else hi = m;
    }
    const int v = Vc[i];
    if (v < 0 || v >= V) return;  // kChkVcRange
    if (Cv[v] != lo) flag[kChkCv] = 1;
}

// bytes above 1, sixteen per lane where the array is 16-byte aligned
__global__ void k_cps_active16(long n16, const uint4 *__restrict__ a, int *__restrict__ flag) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n16) return;
    const uint4 w = a[i];
    if ((w.x | w.y | w.z | w.w) & 0xfefefefeu) flag[kChkActive] = 1;
}
__global__ void k_cps_active1(long n, const uint8_t *__restrict__ a, int *__restrict__ flag) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (a[i] > 1) flag[kChkActive] = 1;
}

// mode 0: NaN; 1: outside [lo, hi] (NaN included); 2: negative or NaN
template <typename real>
__device__ __forceinline__ bool cps_bad(real x, int mode, real lo, real hi) {
    if (mode == 0) return x != x;
    if (mode == 1) return !(lo <= x && x <= hi);
    return !(x >= real(0));
}
template <typename real>
__global__ void k_cps_reals16(long np, const Pk<real, Vec<real>::kPer16B> *__restrict__ x,
                              int mode, real lo, real hi, int which, int *__restrict__ flag) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    const Pk<real, Vec<real>::kPer16B> p = x[i];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < Vec<real>::kPer16B; k++) bad |= cps_bad<real>(p.v[k], mode, lo, hi);
    if (bad) flag[which] = 1;
}
template <typename real>
__global__ void k_cps_reals1(long n, const real *__restrict__ x, int mode, real lo, real hi,
                             int which, int *__restrict__ flag) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (cps_bad<real>(x[i], mode, lo, hi)) flag[which] = 1;
}

__global__ void k_cps_labels(int V, int nlabels, const int *__restrict__ label,
                             int *__restrict__ flag) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int l = label[v];
    if (l < 0 || l >= nlabels) flag[kChkLabel] = 1;
}

// every component takes the value of the label of the first vertex of its range
template <typename real>
__global__ void k_cps_gather(long n, int K, const int *__restrict__ Vc,
                             const int *__restrict__ rVc, const int *__restrict__ label,
                             const real *__restrict__ values, real *__restrict__ rX) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long rv = i / K;
    const int k = (int)(i - rv * K);
    rX[i] = values[(long)label[Vc[rVc[rv]]] * K + k];
}

__global__ void k_cps_pack(const int *__restrict__ flag, unsigned *__restrict__ word) {
    if (blockIdx.x || threadIdx.x) return;
    unsigned w = 0;
    for (int i = 0; i < kChkCount; i++)
        if (flag[i]) w |= 1u << i;
    *word = w;
}

struct CheckFail {
    int which;
};

struct Checks {
    hipStream_t s;
    DevBuf<int> flag{kChkCount + 1};
    explicit Checks(hipStream_t st) : s(st) {
        PFDR_HIP(hipMemsetAsync(flag.p, 0, sizeof(int) * (kChkCount + 1), s));
    }
    void active(long E, const uint8_t *a) {
        if (E <= 0) return;
        if (((uintptr_t)a & 15) == 0) {
            const long n16 = E / 16;
            if (n16)
                k_cps_active16<<<grid_for(n16), kBlock, 0, s>>>(n16, (const uint4 *)a, flag.p);
            if (E - n16 * 16)
                k_cps_active1<<<1, kBlock, 0, s>>>(E - n16 * 16, a + n16 * 16, flag.p);
        } else {
            k_cps_active1<<<grid_for(E), kBlock, 0, s>>>(E, a, flag.p);
        }
        PFDR_HIP(hipGetLastError());
    }
    template <typename real>
    void reals(long n, const real *x, int mode, real lo, real hi, int which) {
        if (n <= 0) return;
        constexpr int W = Vec<real>::kPer16B;
        if (((uintptr_t)x & 15) == 0) {
            const long np = n / W;
            if (np)
                k_cps_reals16<real><<<grid_for(np), kBlock, 0, s>>>(
                    np, (const Pk<real, W> *)x, mode, lo, hi, which, flag.p);
            if (n - np * W)
                k_cps_reals1<real><<<1, kBlock, 0, s>>>(n - np * W, x + np * W, mode, lo, hi,
                                                        which, flag.p);
        } else {
            k_cps_reals1<real><<<grid_for(n), kBlock, 0, s>>>(n, x, mode, lo, hi, which, flag.p);
        }
        PFDR_HIP(hipGetLastError());
    }
    // the one word that comes back: throws the first failed check
    void verdict() {
        unsigned *word = reinterpret_cast<unsigned *>(flag.p + kChkCount);
        k_cps_pack<<<1, kWave, 0, s>>>(flag.p, word);
        PFDR_HIP(hipGetLastError());
        unsigned w = 0;
        PFDR_HIP(hipMemcpyAsync(&w, word, sizeof w, hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < kChkCount; i++)
            if (w & (1u << i)) throw CheckFail{i};
    }
};

// the caller's array on the device: itself, or an upload
template <typename T>
struct OnDevice {
    DevBuf<T> buf;
    const T *p = nullptr;
    OnDevice(const T *src, size_t n, int mem, hipStream_t s) {
        if (!src) return;
        if (mem == PFDR_MEM_DEVICE) {
            p = src;
            return;
        }
        buf.alloc(n ? n : 1);
        if (n) PFDR_HIP(hipMemcpyAsync(buf.p, src, n * sizeof(T), hipMemcpyHostToDevice, s));
        p = buf.p;
    }
};

}  // namespace

}  // namespace pfdr

struct pfdr_cp_solver {
    std::unique_ptr<pfdr::CpDriverBase> d;
    int kind = 0, dtype = 0, V = 0, E = 0, N = 0, K = 1;
    double min = 0, max = 0;
    hipStream_t s = nullptr;
    int dev = 0;
    double setup_seconds = 0;
};

using pfdr::report_error;

#define CPS_TRY(fn, body)                                   \
    try {                                                   \
        pfdr::StreamScope sc_(h->s, h->dev);                \
        body;                                               \
    } catch (const pfdr::CheckFail &c) {                    \
        return report_error(fn, pfdr::kChkName[c.which]);   \
    } catch (const pfdr::CpAbiFail &f) {                    \
        return f.status;                                    \
    } catch (const pfdr::HipError &e) {                     \
        return report_error(fn, e);                         \
    } catch (const std::exception &ex) {                    \
        return report_error(fn, ex.what());                 \
    }                                                       \
    return PFDR_OK;

// csc: the sparse A of pfdr_cp_solver_create_sparse, whose own checks are done
static int cps_create(const char *fn, pfdr_cp_solver **out, const pfdr_cp_problem *p,
                      const pfdr_csc *csc) {
    if ((p->dtype != PFDR_F32 && p->dtype != PFDR_F64) ||
        (p->mem != PFDR_MEM_HOST && p->mem != PFDR_MEM_DEVICE) ||
        (p->kind != PFDR_KIND_L1 && p->kind != PFDR_KIND_BOUNDS && p->kind != PFDR_KIND_SIMPLEX))
        return report_error(fn, "invalid arguments");
    if (p->V <= 0 || p->E < 0 || !p->Y || (p->E > 0 && (!p->Eu || !p->Ev || !p->La_d1)))
        return report_error(fn, "invalid arguments");
    if (p->kind == PFDR_KIND_SIMPLEX) {
        if (p->K < 2 || p->N != 0 || p->A || p->La_l1 || p->duplex)
            return report_error(fn, "invalid arguments");
        if (!(p->al >= 0.0 && p->al <= 1.0)) return report_error(fn, "al must lie in [0, 1]");
    } else {
        if (p->N != 0 && !p->A && !csc) return report_error(fn, "N != 0 needs A");
        if (p->N < 0 && -p->N != p->V)
            return report_error(fn, "N < 0 needs A = A^tA and N = -V");
        if (p->kind == PFDR_KIND_BOUNDS) {
            if (p->La_l1 || p->duplex || p->positivity)
                return report_error(fn, "invalid arguments");
            if (!(p->min <= p->max)) return report_error(fn, "the bounds need min <= max");
        }
    }
    try {
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_ptr<pfdr_cp_solver> h(new pfdr_cp_solver());
        h->kind = p->kind, h->dtype = p->dtype, h->V = p->V, h->E = p->E;
        h->N = p->kind == PFDR_KIND_SIMPLEX ? 0 : p->N;
        h->K = p->kind == PFDR_KIND_SIMPLEX ? p->K : 1;
        h->min = p->min, h->max = p->max;
        h->s = pfdr::lib_stream();
        PFDR_HIP(hipGetDevice(&h->dev));
        h->d.reset(p->kind == PFDR_KIND_L1       ? pfdr::cp_make_l1_driver(p->dtype, p->duplex != 0)
                   : p->kind == PFDR_KIND_BOUNDS ? pfdr::cp_make_bounds_driver(p->dtype)
                                                 : pfdr::cp_make_simplex_driver(p->dtype));
        h->d->sparse = csc;
        h->d->setup(*p, true);
        h->d->sparse = nullptr;
        h->setup_seconds =
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        *out = h.release();
    } catch (const pfdr::CpAbiFail &f) {
        return f.status;
    } catch (const pfdr::HipError &e) {
        return report_error(fn, e);
    } catch (const std::exception &ex) {
        return report_error(fn, ex.what());
    }
    return PFDR_OK;
}

extern "C" int pfdr_cp_solver_create(pfdr_cp_solver **out, const pfdr_cp_problem *p) {
    const char *fn = "pfdr_cp_solver_create";
    if (!out || !p) return report_error(fn, "invalid arguments");
    *out = nullptr;
    return cps_create(fn, out, p, nullptr);
}

extern "C" int pfdr_cp_solver_create_sparse(pfdr_cp_solver **out, const pfdr_cp_problem *p,
                                            const pfdr_csc *A) {
    const char *fn = "pfdr_cp_solver_create_sparse";
    if (!out || !p) return report_error(fn, "invalid arguments");
    *out = nullptr;
    if (p->kind == PFDR_KIND_SIMPLEX)
        return report_error(fn, "a sparse A: the simplex kind has no A");
    if (p->N <= 0) return report_error(fn, "a sparse A needs N > 0");
    if (p->A) return report_error(fn, "a sparse A and p->A are both set");
    if (const char *bad = pfdr::cp_csc_args(A)) return report_error(fn, bad);
    return cps_create(fn, out, p, A);
}

extern "C" void pfdr_cp_solver_destroy(pfdr_cp_solver *h) {
    if (!h) return;
    try {
        pfdr::StreamScope sc(h->s, h->dev);
        (void)hipStreamSynchronize(h->s);
        h->d.reset();
    } catch (...) {
    }
    delete h;
}

extern "C" int pfdr_cp_solver_run(pfdr_cp_solver *h, const pfdr_cp_params *q, int *CP_it,
                                  double *Time, void *Obj, void *Dif) {
    const char *fn = "pfdr_cp_solver_run";
    if (!h || !q || q->CP_itMax < 0) return report_error(fn, "invalid arguments");
    CPS_TRY(fn, h->d->loop(std::chrono::steady_clock::now(), *q, CP_it, Time, Obj, Dif))
}

extern "C" int pfdr_cp_solver_get_state(pfdr_cp_solver *h, int *rV, int *Cv, int *Vc, int *rVc,
                                        uint8_t *active, void *rX, void *R, int mem) {
    const char *fn = "pfdr_cp_solver_get_state";
    if (!h || (mem != PFDR_MEM_HOST && mem != PFDR_MEM_DEVICE))
        return report_error(fn, "invalid arguments");
    if (R && h->N <= 0) return report_error(fn, "R exists only for N > 0");
    CPS_TRY(fn, {
        auto *d = h->d.get();
        CP_ABI(pfdr_cpgraph_get_components(d->g, rV, Cv, Vc, rVc, mem));
        if (active) CP_ABI(pfdr_cpgraph_get_active(d->g, active, mem));
        const size_t sz = h->dtype == PFDR_F32 ? 4 : 8;
        const auto k = mem == PFDR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (rX) PFDR_HIP(hipMemcpyAsync(rX, d->values(), sz * d->rV * h->K, k, h->s));
        if (R) PFDR_HIP(hipMemcpyAsync(R, d->residual(), sz * h->N, k, h->s));
        PFDR_HIP(hipStreamSynchronize(h->s));
    })
}

namespace pfdr {
namespace {

template <typename real>
void solver_set_state(pfdr_cp_solver *h, int rV, const int *Cv, const int *Vc, const int *rVc,
                      const uint8_t *active, const void *rX, const void *R, int mem) {
    hipStream_t s = h->s;
    const int V = h->V;
    const long nX = (long)rV * h->K;
    OnDevice<int> dCv(Cv, V, mem, s), dVc(Vc, V, mem, s), drVc(rVc, (size_t)rV + 1, mem, s);
    OnDevice<uint8_t> dAct(active, h->E, mem, s);
    OnDevice<real> dX((const real *)rX, nX, mem, s), dR((const real *)R, h->N, mem, s);
    Checks c(s);
    DevBuf<int> seen(V);
    PFDR_HIP(hipMemsetAsync(seen.p, 0, sizeof(int) * V, s));
    k_cps_rvc<<<grid_for(rV + 1), kBlock, 0, s>>>(rV, V, drVc.p, c.flag.p);
    k_cps_vc_count<<<grid_for(V), kBlock, 0, s>>>(V, dVc.p, seen.p, c.flag.p);
    k_cps_vc_once<<<grid_for(V), kBlock, 0, s>>>(V, seen.p, c.flag.p);
    k_cps_cv<<<grid_for(V), kBlock, 0, s>>>(V, rV, dCv.p, dVc.p, drVc.p, c.flag.p);
    PFDR_HIP(hipGetLastError());
    c.active(h->E, dAct.p);
    c.reals<real>(nX, dX.p, 0, real(0), real(0), kChkValuesNaN);
    if (dR.p) c.reals<real>(h->N, dR.p, 0, real(0), real(0), kChkResidualNaN);
    if (h->kind == PFDR_KIND_BOUNDS)
        c.reals<real>(nX, dX.p, 1, (real)h->min, (real)h->max, kChkBox);
    c.verdict();
    // accepted: the graph's activity and components, then the driver's part
    auto *d = h->d.get();
    if (h->E > 0) CP_ABI(pfdr_cpgraph_set_active(d->g, dAct.p, PFDR_MEM_DEVICE));
    CP_ABI(pfdr_cpgraph_set_components(d->g, rV, dCv.p, dVc.p, drVc.p, PFDR_MEM_DEVICE));
    d->adopt(rV, dX.p, dR.p);
}

template <typename real>
void solver_set_partition(pfdr_cp_solver *h, int nlabels, const int *label, const void *values,
                          int mem) {
    hipStream_t s = h->s;
    const int V = h->V, K = h->K;
    OnDevice<int> dl(label, V, mem, s);
    OnDevice<real> dv((const real *)values, (size_t)nlabels * K, mem, s);
    Checks c(s);
    k_cps_labels<<<grid_for(V), kBlock, 0, s>>>(V, nlabels, dl.p, c.flag.p);
    PFDR_HIP(hipGetLastError());
    c.reals<real>((long)nlabels * K, dv.p, 0, real(0), real(0), kChkValuesNaN);
    if (h->kind == PFDR_KIND_BOUNDS)
        c.reals<real>((long)nlabels * K, dv.p, 1, (real)h->min, (real)h->max, kChkBox);
    c.verdict();
    auto *d = h->d.get();
    int rV = 0;
    CP_ABI(pfdr_cpgraph_set_active_by_labels(d->g, dl.p, PFDR_MEM_DEVICE));
    CP_ABI(pfdr_cpgraph_components(d->g, &rV));
    DevBuf<int> Vc(V), rVc((size_t)V + 1);
    CP_ABI(pfdr_cpgraph_get_components(d->g, nullptr, nullptr, Vc.p, rVc.p, PFDR_MEM_DEVICE));
    const long n = (long)rV * K;
    DevBuf<real> x((size_t)n);
    k_cps_gather<real><<<grid_for(n), kBlock, 0, s>>>(n, K, Vc.p, rVc.p, dl.p, dv.p, x.p);
    PFDR_HIP(hipGetLastError());
    PFDR_HIP(hipStreamSynchronize(s));
    d->adopt(rV, x.p, nullptr);
}

template <typename real>
void solver_set_penalties(pfdr_cp_solver *h, const void *La_d1, const void *La_l1, int mem) {
    hipStream_t s = h->s;
    OnDevice<real> da((const real *)La_d1, h->E, mem, s), dl((const real *)La_l1, h->V, mem, s);
    Checks c(s);
    if (da.p) c.reals<real>(h->E, da.p, 2, real(0), real(0), kChkWeight);
    if (dl.p) c.reals<real>(h->V, dl.p, 2, real(0), real(0), kChkWeight);
    c.verdict();
    CP_ABI(pfdr_cpgraph_set_weights(h->d->g, da.p, dl.p, PFDR_MEM_DEVICE));
    h->d->forget_objective();
}

}  // namespace
}  // namespace pfdr

extern "C" int pfdr_cp_solver_set_state(pfdr_cp_solver *h, int rV, const int *Cv, const int *Vc,
                                        const int *rVc, const uint8_t *active, const void *rX,
                                        const void *R, int mem) {
    const char *fn = "pfdr_cp_solver_set_state";
    if (!h || !Cv || !Vc || !rVc || !rX || (h->E > 0 && !active) ||
        (mem != PFDR_MEM_HOST && mem != PFDR_MEM_DEVICE))
        return report_error(fn, "invalid arguments");
    if (rV < 1 || rV > h->V) return report_error(fn, "rV must lie in [1, V]");
    if (R && h->N <= 0) return report_error(fn, "R exists only for N > 0");
    CPS_TRY(fn, {
        if (h->dtype == PFDR_F32)
            pfdr::solver_set_state<float>(h, rV, Cv, Vc, rVc, active, rX, R, mem);
        else
            pfdr::solver_set_state<double>(h, rV, Cv, Vc, rVc, active, rX, R, mem);
    })
}

extern "C" int pfdr_cp_solver_set_partition(pfdr_cp_solver *h, int nlabels, const int *label,
                                            const void *values, int mem) {
    const char *fn = "pfdr_cp_solver_set_partition";
    if (!h || nlabels < 1 || !label || !values ||
        (mem != PFDR_MEM_HOST && mem != PFDR_MEM_DEVICE))
        return report_error(fn, "invalid arguments");
    CPS_TRY(fn, {
        if (h->dtype == PFDR_F32) pfdr::solver_set_partition<float>(h, nlabels, label, values, mem);
        else pfdr::solver_set_partition<double>(h, nlabels, label, values, mem);
    })
}

extern "C" int pfdr_cp_solver_set_penalties(pfdr_cp_solver *h, const void *La_d1,
                                            const void *La_l1, int mem) {
    const char *fn = "pfdr_cp_solver_set_penalties";
    if (!h || (mem != PFDR_MEM_HOST && mem != PFDR_MEM_DEVICE))
        return report_error(fn, "invalid arguments");
    if (La_l1 && !h->d->has_l1)
        return report_error(fn, "La_l1 can only replace the one the solver was created with");
    CPS_TRY(fn, {
        if (h->dtype == PFDR_F32) pfdr::solver_set_penalties<float>(h, La_d1, La_l1, mem);
        else pfdr::solver_set_penalties<double>(h, La_d1, La_l1, mem);
    })
}

extern "C" int pfdr_cp_solver_set_reduced(pfdr_cp_solver *h, int mode) {
    const char *fn = "pfdr_cp_solver_set_reduced";
    if (!h) return report_error(fn, "invalid arguments");
    if (h->kind == PFDR_KIND_SIMPLEX)
        return report_error(fn, "the simplex kind has no reduced operator");
    if (!h->d->holds_sparse_A())
        return report_error(fn, "the solver was not created by pfdr_cp_solver_create_sparse");
    if (mode != PFDR_REDUCED_DENSE && mode != PFDR_REDUCED_SPARSE &&
        mode != PFDR_REDUCED_SPARSE_ALL)
        return report_error(fn, "mode must be PFDR_REDUCED_DENSE, PFDR_REDUCED_SPARSE or "
                                "PFDR_REDUCED_SPARSE_ALL");
    h->d->reduced = mode;
    return PFDR_OK;
}

extern "C" int pfdr_cp_solver_premultiplied_stats(pfdr_cp_solver *h, int64_t *sparse_iterations,
                                                  int64_t *dense_iterations, int64_t *max_rnnz) {
    if (!h) return report_error("pfdr_cp_solver_premultiplied_stats", "invalid arguments");
    if (sparse_iterations) *sparse_iterations = h->d->pre_sparse_its;
    if (dense_iterations) *dense_iterations = h->d->pre_dense_its;
    if (max_rnnz) *max_rnnz = h->d->pre_max_rnnz;
    return PFDR_OK;
}

extern "C" int pfdr_cp_solver_reduced_stats(pfdr_cp_solver *h, int64_t *sparse_iterations,
                                            int64_t *dense_direct_iterations,
                                            int64_t *max_rnnz) {
    if (!h) return report_error("pfdr_cp_solver_reduced_stats", "invalid arguments");
    if (sparse_iterations) *sparse_iterations = h->d->sparse_its;
    if (dense_direct_iterations) *dense_direct_iterations = h->d->dense_direct_its;
    if (max_rnnz) *max_rnnz = h->d->max_rnnz;
    return PFDR_OK;
}

extern "C" int pfdr_cp_solver_stats(pfdr_cp_solver *h, double *seconds, int64_t *counts,
                                    double *setup_seconds) {
    if (!h) return report_error("pfdr_cp_solver_stats", "invalid arguments");
    h->d->stats(seconds, counts);
    if (setup_seconds) *setup_seconds = h->setup_seconds;
    return PFDR_OK;
}
