// Batched dense-A PFDR sessions: the batch, its lock-step loop and the
// batched product kernels (pfdr_batch.hpp; include/pfdr_mi355x.h, "batched
// dense sessions").
//
// The forward step of the dense modes is the stream of A (HBM bound at one
// right-hand side, pfdr_quadratic_kernels.hpp).  With several observation
// vectors in flight one pass over A serves a group of up to kBatchG channels:
//   direct (N > 0)   k_rows_partial_b, k_rows_finish_b : R_g = Y_g - A X_g
//                    k_col_dot_b<EPI_FWD_DIRECT>       : P_g = 2 X_g + Ga_g A^t R_g
//   A^tA (N = -V)    k_x_extract_b, then k_symv_tiles_b + k_symv_finish_b
//                    (exactly symmetric matrix) or k_col_dot_b<EPI_FWD_ATA>
// Each (row or column, channel) sum is added in the order and precision of
// the scalar kernel of pfdr_quadratic_kernels.hpp that it replaces (the order
// is restated at each kernel), so a channel's bytes are those of a scalar
// session on that channel.  A channel's stores are gated by its own control
// block: a halted channel is read but never written.
//
// The small problems on the sequential-order path (dense_exact) keep the
// scalar kernels, one launch per channel: their products are a few
// microseconds and their order is one lane's chain.
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "pfdr_quadratic_kernels.hpp"
#include "pfdr_batch.hpp"

namespace pfdr {

// Channels served by one pass over A.  8: the column dots then hold 4 columns
// x 8 channels = 32 double accumulators per lane (64 VGPRs) beside 4 + 8
// 16-byte vectors in flight, the row partials 8 x 4 doubles; 16 would halve
// the waves per SIMD that keep the HBM loads in flight.
constexpr int kBatchG = 8;
constexpr int kBatchCols = 4;  // columns per wave of k_col_dot_b
constexpr int kBatchMax = 64;  // channels per batch
constexpr int kBatchChunk = 32;  // iterations between two reads of the control blocks

// one group of up to G channels: the lanes' buffers (LaneView).  Slots past
// nch repeat channel 0 (read, never written).
template <typename real, int G>
struct ChanArgs {
    int nch;
    R2<real> *xp[G];
    real *R[G];
    const real *Y[G];
    const real *Ga[G];
    const Ctrl<real> *ctrl[G];
    double *rpart[G];
    real *w[G];
    real *spart[G];
};

// live[g]: channel g of the group takes this launch's stores; false: none does
template <typename real, int G>
__device__ __forceinline__ bool chan_live(const ChanArgs<real, G> &a, int gate, bool (&live)[G]) {
    bool any = false;
#pragma unroll
    for (int g = 0; g < G; g++) {
        live[g] = g < a.nch && !gated(a.ctrl[g], gate);
        any |= live[g];
    }
    return any;
}

// p[ch] of a kernel-argument array (uniform ch), without indexing it dynamically
template <typename T, int G>
__device__ __forceinline__ T chan_pick(T const (&p)[G], int ch) {
    T r = p[0];
#pragma unroll
    for (int g = 1; g < G; g++)
        if (ch == g) r = p[g];
    return r;
}

// xfull_g[v] = xp_g[v].x (k_x_extract), channel blockIdx.y
template <typename real, int G>
__global__ void k_x_extract_b(int V, ChanArgs<real, G> a) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = blockIdx.y;
    if (v >= V || ch >= a.nch) return;
    const R2<real> *xp = chan_pick(a.xp, ch);
    real *w = chan_pick(a.w, ch);
    w[v] = xp[v].x;
}

// k_rows_partial for a group: part_g[b][n] = sum_{v in block b} A[n + N v] X_g[v].
// Order kept per (n, g): v ascending over [v0, v1) in double through dacc
// (the four columns in flight are added in their order), the scalar
// session's rows_nb_ / rows_cpb_ split.
template <typename real, int G>
__global__ __launch_bounds__(256) void k_rows_partial_b(int N, int V, const real *__restrict__ A,
                                                        int cpb, int gate, ChanArgs<real, G> a) {
    bool live[G];
    if (!chan_live(a, gate, live)) return;
    const int b = blockIdx.x;
    const int v0 = b * cpb, v1 = min(v0 + cpb, V);
    constexpr int VW = Vec<real>::kPer16B;
    if ((N % VW) == 0) {
        for (int n0 = threadIdx.x * VW; n0 < N; n0 += kBlock * VW) {
            double acc[G][VW];
#pragma unroll
            for (int g = 0; g < G; g++)
#pragma unroll
                for (int j = 0; j < VW; j++) acc[g][j] = 0.0;
            int v = v0;
            for (; v + 4 <= v1; v += 4) {
                Pk<real, VW> c[4];
#pragma unroll
                for (int q = 0; q < 4; q++) c[q] = ldv<real, VW>(A + (size_t)N * (v + q) + n0);
#pragma unroll
                for (int g = 0; g < G; g++) {
                    double x[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) x[q] = (double)a.xp[g][v + q].x;
#pragma unroll
                    for (int q = 0; q < 4; q++)
#pragma unroll
                        for (int j = 0; j < VW; j++)
                            acc[g][j] = dacc<real>(acc[g][j], c[q].v[j], x[q]);
                }
            }
            for (; v < v1; v++) {
                const Pk<real, VW> c = ldv<real, VW>(A + (size_t)N * v + n0);
#pragma unroll
                for (int g = 0; g < G; g++) {
                    const double x = (double)a.xp[g][v].x;
#pragma unroll
                    for (int j = 0; j < VW; j++) acc[g][j] = dacc<real>(acc[g][j], c.v[j], x);
                }
            }
#pragma unroll
            for (int g = 0; g < G; g++)
                if (live[g]) {
#pragma unroll
                    for (int j = 0; j < VW; j++) a.rpart[g][(size_t)b * N + n0 + j] = acc[g][j];
                }
        }
    } else {
        for (int n = threadIdx.x; n < N; n += kBlock) {
            double acc[G];
#pragma unroll
            for (int g = 0; g < G; g++) acc[g] = 0.0;
            for (int v = v0; v < v1; v++) {
                const real c = A[(size_t)N * v + n];
#pragma unroll
                for (int g = 0; g < G; g++) acc[g] = dacc<real>(acc[g], c, a.xp[g][v].x);
            }
#pragma unroll
            for (int g = 0; g < G; g++)
                if (live[g]) a.rpart[g][(size_t)b * N + n] = acc[g];
        }
    }
}

// k_rows_finish, channel blockIdx.y: R_g[n] = (real)((double)Y_g[n] - sum_b
// part_g[b][n]), the blocks added in ascending order in double
template <typename real, int G>
__global__ void k_rows_finish_b(int N, int nb, int gate, ChanArgs<real, G> a) {
    const int ch = blockIdx.y;
    if (ch >= a.nch || gated(chan_pick(a.ctrl, ch), gate)) return;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const double *part = chan_pick(a.rpart, ch);
    const real *Y = chan_pick(a.Y, ch);
    real *R = chan_pick(a.R, ch);
    double s = 0.0;
    int b = 0;
    for (; b + 8 <= nb; b += 8) {
        double t[8];
#pragma unroll
        for (int q = 0; q < 8; q++) t[q] = part[(size_t)(b + q) * N + n];
#pragma unroll
        for (int q = 0; q < 8; q++) s += t[q];
    }
    for (; b < nb; b++) s += part[(size_t)b * N + n];
    R[n] = (real)((double)Y[n] - s);
}

// wave_sum of NA accumulators at once.  Lane L of wave_sum ends with the
// butterfly's value ((v[L] + v[L^32]) + ...) for offsets 32, 16, ..., 1.  Here
// the lanes split the accumulators while they add: at offset o the lanes
// with bit o clear keep the even accumulator of each pair and the others the
// odd one, each adding its own value and its partner's -- the same two
// operands the butterfly adds in that lane -- so every total is the
// butterfly's, bit for bit, for NA + log2(64 / NA) shuffles, not 6 NA.
// Returns the lane's accumulator index; its total is in acc[0].
template <int NA>
__device__ __forceinline__ int wave_sum_many(double (&acc)[NA], int lane) {
    static_assert(NA >= 1 && NA <= 64 && (NA & (NA - 1)) == 0, "a power of two of accumulators");
    int idx = 0, t = 0, n = NA;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1, t++) {
        if (n > 1) {
            const bool odd = (lane & o) != 0;
#pragma unroll
            for (int i = 0; i < NA / 2; i++) {
                if (i < n / 2) {
                    const double keep = odd ? acc[2 * i + 1] : acc[2 * i];
                    const double send = odd ? acc[2 * i] : acc[2 * i + 1];
                    acc[i] = keep + __shfl_xor(send, o, 64);
                }
            }
            idx |= (odd ? 1 : 0) << t;
            n >>= 1;
        } else {
            acc[0] += __shfl_xor(acc[0], o, 64);
        }
    }
    return idx;
}

// k_col_dot for a group: one wave per kBatchCols columns, so that each w_g
// vector (L2) meets four columns of A (HBM) in registers.  Order kept per
// (column, g): lane l adds the 16-byte vectors i = l, l + 64, ..., elements
// ascending inside a vector (the scalar loop i = l, l + 64, ... when len %
// VW != 0), in double through dacc; the wave's butterfly sum (wave_sum_many);
// one rounding to real; col_epilogue.
template <typename real, int EPI, int G>
__global__ __launch_bounds__(256) void k_col_dot_b(const real *__restrict__ A, int ncols, int len,
                                                   int gate, ChanArgs<real, G> a) {
    static_assert(EPI == EPI_FWD_DIRECT || EPI == EPI_FWD_ATA, "forward steps only");
    constexpr int C = kBatchCols, VW = Vec<real>::kPer16B;
    bool live[G];
    if (!chan_live(a, gate, live)) return;
    const int lane = threadIdx.x & 63;
    const long col0 = ((((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6)) * C;
    if (col0 >= ncols) return;
    const real *c[C];
#pragma unroll
    for (int k = 0; k < C; k++)  // (past the last column: the last again, not stored)
        c[k] = A + (size_t)len * min(col0 + k, (long)ncols - 1);
    const real *w[G];
#pragma unroll
    for (int g = 0; g < G; g++) w[g] = EPI == EPI_FWD_DIRECT ? a.R[g] : a.w[g];
    double acc[C * G];
#pragma unroll
    for (int i = 0; i < C * G; i++) acc[i] = 0.0;
    if ((len % VW) == 0) {
        const int nv = len / VW;
        for (int i = lane; i < nv; i += 64) {
            Pk<real, VW> x[C], y[G];
#pragma unroll
            for (int k = 0; k < C; k++) x[k] = ldv<real, VW>(c[k] + (size_t)i * VW);
#pragma unroll
            for (int g = 0; g < G; g++) y[g] = ldv<real, VW>(w[g] + (size_t)i * VW);
#pragma unroll
            for (int k = 0; k < C; k++)
#pragma unroll
                for (int g = 0; g < G; g++)
#pragma unroll
                    for (int j = 0; j < VW; j++)
                        acc[k * G + g] = dacc<real>(acc[k * G + g], x[k].v[j], y[g].v[j]);
        }
    } else {
        for (int i = lane; i < len; i += 64) {
            real x[C], y[G];
#pragma unroll
            for (int k = 0; k < C; k++) x[k] = c[k][i];
#pragma unroll
            for (int g = 0; g < G; g++) y[g] = w[g][i];
#pragma unroll
            for (int k = 0; k < C; k++)
#pragma unroll
                for (int g = 0; g < G; g++) acc[k * G + g] = dacc<real>(acc[k * G + g], x[k], y[g]);
        }
    }
    const int mine = wave_sum_many<C * G>(acc, lane);
    // the first lane of each run of lanes that hold the same total stores it
    constexpr int kRun = 64 / (C * G);
    if (lane % kRun) return;
    const real s = (real)acc[0];
#pragma unroll
    for (int k = 0; k < C; k++)
#pragma unroll
        for (int g = 0; g < G; g++)
            if (mine == k * G + g && col0 + k < ncols && live[g]) {
                ColArgs<real> ca{};
                ca.xp = a.xp[g];
                ca.Ga = a.Ga[g];
                ca.Y = a.Y[g];
                col_epilogue<real, EPI>(ca, col0 + k, s);
            }
}

// k_symv_tiles for a group: the tile of A is loaded once into registers and
// meets the channels one after the other through the same LDS arrays.  Order
// kept per channel: row part, the lane's CPT columns ascending in real, then
// the eight column groups g = 0 ... 7; column part, the VW products from 0,
// then the xor butterfly 16 ... 1 inside the half-wave.
template <typename real, int G>
__global__ __launch_bounds__(256) void k_symv_tiles_b(int V, const real *__restrict__ A, int gate,
                                                      ChanArgs<real, G> a) {
    bool live[G];
    if (!chan_live(a, gate, live)) return;
    using S = SymT<real>;
    constexpr int VW = S::VW, T = S::T, CPT = S::CPT;
    __shared__ real wI[T], wJ[T], csum[T];
    __shared__ real rsum[8][T];
    int bi, bj;
    tri_index(blockIdx.x, bi, bj);
    const int I0 = bi * T, J0 = bj * T;
    const int tid = threadIdx.x;
    const int rg = tid & 31, cg = tid >> 5;
    const int r0 = I0 + rg * VW;
    const bool rok = r0 < V;
    Pk<real, VW> t[CPT];
#pragma unroll
    for (int k = 0; k < CPT; k++) {
        const int c = J0 + cg * CPT + k;
        if (rok && c < V) {
            t[k] = ldv<real, VW>(A + (size_t)V * c + r0);
        } else {
#pragma unroll
            for (int j = 0; j < VW; j++) t[k].v[j] = real(0);
        }
    }
    const bool offdiag = bi != bj;
#pragma unroll
    for (int g = 0; g < G; g++) {
        if (g >= a.nch) break;  // (uniform: the barriers below are the block's)
        const real *w = a.w[g];
        if (tid < T) {
            wI[tid] = (I0 + tid < V) ? w[I0 + tid] : real(0);
            wJ[tid] = (J0 + tid < V) ? w[J0 + tid] : real(0);
        }
        __syncthreads();  // (also: every lane has read the last channel's sums)
        real racc[VW];
#pragma unroll
        for (int j = 0; j < VW; j++) racc[j] = real(0);
#pragma unroll
        for (int k = 0; k < CPT; k++) {
            const real wc = wJ[cg * CPT + k];
#pragma unroll
            for (int j = 0; j < VW; j++) racc[j] += t[k].v[j] * wc;
        }
#pragma unroll
        for (int j = 0; j < VW; j++) rsum[cg][rg * VW + j] = racc[j];
        if (offdiag) {
            real wr[VW];
#pragma unroll
            for (int j = 0; j < VW; j++) wr[j] = wI[rg * VW + j];
#pragma unroll
            for (int k = 0; k < CPT; k++) {
                real s = real(0);
#pragma unroll
                for (int j = 0; j < VW; j++) s += t[k].v[j] * wr[j];
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 32);
                if (rg == k) csum[cg * CPT + k] = s;
            }
        }
        __syncthreads();
        if (tid < T && live[g]) {
            real *part = a.spart[g];
            const int r = I0 + tid;
            if (r < V) {
                real s = rsum[0][tid];
#pragma unroll
                for (int q = 1; q < 8; q++) s += rsum[q][tid];
                part[(size_t)bj * V + r] = s;
            }
            const int c = J0 + tid;
            if (offdiag && c < V) part[(size_t)bi * V + c] = csum[tid];
        }
    }
}

// k_symv_finish, channel blockIdx.y: the four quarter sums ((q0 + q1) + q2) +
// q3, each over its ascending slice of the nb partials
template <typename real, int EPI, int G>
__global__ __launch_bounds__(256) void k_symv_finish_b(int nb, int ncols, int gate,
                                                       ChanArgs<real, G> a) {
    const int ch = blockIdx.y;
    if (ch >= a.nch || gated(chan_pick(a.ctrl, ch), gate)) return;
    __shared__ real q4[4][64];
    const real *part = chan_pick(a.spart, ch);
    const int rl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int r = blockIdx.x * 64 + rl;
    const int per = (nb + 3) / 4, b0 = g * per, b1 = min(nb, b0 + per);
    real acc = real(0);
    if (r < ncols) {
#pragma unroll 8
        for (int b = b0; b < b1; b++) acc += part[(size_t)b * ncols + r];
    }
    q4[g][rl] = acc;
    __syncthreads();
    if (g == 0 && r < ncols) {
        ColArgs<real> ca{};
        ca.xp = chan_pick(a.xp, ch);
        ca.Ga = chan_pick(a.Ga, ch);
        ca.Y = chan_pick(a.Y, ch);
        col_epilogue<real, EPI>(ca, r, ((q4[0][rl] + q4[1][rl]) + q4[2][rl]) + q4[3][rl]);
    }
}

// ------------------------------------------------------------- the batch --
class BatchBase {
  public:
    virtual ~BatchBase() = default;
    virtual void run(int iters, int *it) = 0;
    virtual void result(void *X, int *it, void *Obj, void *Dif) = 0;
    virtual void reload(const pfdr_reload *r) = 0;
    virtual bool query(const char *what, int64_t *value) = 0;
    hipStream_t stream = nullptr;
    int device = 0;
};

template <typename real>
class QuadBatch final : public BatchBase {
  public:
    QuadBatch(const pfdr_problem *p, int B);
    ~QuadBatch() override {
        (void)hipStreamSynchronize(stream);
        while (!lanes_.empty()) lanes_.pop_back();  // (the first lane's diagonal goes last)
    }
    void run(int iters, int *it) override;
    void result(void *X, int *it, void *Obj, void *Dif) override;
    void reload(const pfdr_reload *r) override;
    bool query(const char *what, int64_t *value) override;

  private:
    int B_, V_, len_, itMax0_;
    LaneFacts f_{};
    DevBuf<real> A_;  // the one copy of the matrix
    std::vector<std::unique_ptr<DenseLane<real>>> lanes_;
    int64_t shared_products_ = 0;
    void forward(const std::vector<int> &cur);
    template <int G> void forward_group(const int *ch, int m);
    static const char *at(const void *base, size_t elems) {
        return base ? static_cast<const char *>(base) + elems * sizeof(real) : nullptr;
    }
};

template <typename real>
QuadBatch<real>::QuadBatch(const pfdr_problem *p, int B) : B_(B), V_(p->V), itMax0_(p->itMax) {
    PFDR_HIP(hipGetDevice(&device));
    stream = lib_stream();
    len_ = p->N > 0 ? p->N : p->V;
    {
        HostPins pins(stream);
        const size_t asz = p->N > 0 ? (size_t)p->N * V_ : (size_t)V_ * V_;
        copy_in(A_, p->A, asz, p->mem, stream, pins);
        pins.release();
    }
    for (int b = 0; b < B_; b++) {
        pfdr_problem lp = *p;
        lp.X = const_cast<char *>(at(p->X, (size_t)b * V_));
        lp.Y = at(p->Y, (size_t)b * len_);
        lp.A = A_.p;
        LaneShare<real> sh;
        sh.A = A_.p;
        if (b) {
            sh.diag = lanes_[0]->diag();
            sh.symv = f_.symv ? 1 : 0;
        }
        lanes_.emplace_back(create_quadratic_lane<real>(&lp, sh));
        if (!b) f_ = lanes_[0]->facts();
    }
}

// one group of m <= G channels through the batched products
template <typename real>
template <int G>
void QuadBatch<real>::forward_group(const int *ch, int m) {
    hipStream_t s = stream;
    ChanArgs<real, G> a{};
    a.nch = m;
    for (int g = 0; g < G; g++) {
        const LaneView<real> v = lanes_[ch[g < m ? g : 0]]->view();
        a.xp[g] = v.xp; a.R[g] = v.R; a.Y[g] = v.Y; a.Ga[g] = v.Ga; a.ctrl[g] = v.ctrl;
        a.rpart[g] = v.rpart; a.w[g] = v.xfull; a.spart[g] = v.spart;
    }
    const int gate = f_.gated ? GATE_ACTIVE : GATE_NONE;
    const int ncw = (V_ + kBatchCols - 1) / kBatchCols;  // waves of the column dots
    if (f_.direct) {
        // (the residual is also what the objective needs)
        const int rgate = !f_.gated ? GATE_NONE : f_.rec_obj ? GATE_ACTIVE_OR_OBJ : GATE_ACTIVE;
        k_rows_partial_b<real, G><<<f_.rows_nb, kBlock, 0, s>>>(f_.N, V_, A_.p, f_.rows_cpb, rgate,
                                                               a);
        k_rows_finish_b<real, G><<<dim3(grid_for(f_.N), m), kBlock, 0, s>>>(f_.N, f_.rows_nb, rgate,
                                                                           a);
        k_col_dot_b<real, EPI_FWD_DIRECT, G><<<grid_for((long)ncw * 64), kBlock, 0, s>>>(
            A_.p, V_, f_.N, gate, a);
        shared_products_ += 2;
    } else {
        k_x_extract_b<real, G><<<dim3(grid_for(V_), m), kBlock, 0, s>>>(V_, a);
        if (f_.symv) {
            const long nt = (long)f_.snb * (f_.snb + 1) / 2;
            k_symv_tiles_b<real, G><<<nt, kBlock, 0, s>>>(V_, A_.p, gate, a);
            k_symv_finish_b<real, EPI_FWD_ATA, G><<<dim3((V_ + 63) / 64, m), kBlock, 0, s>>>(
                f_.snb, V_, gate, a);
        } else {
            k_col_dot_b<real, EPI_FWD_ATA, G><<<grid_for((long)ncw * 64), kBlock, 0, s>>>(
                A_.p, V_, V_, gate, a);
        }
        shared_products_ += 1;
    }
    PFDR_HIP(hipGetLastError());
}

// the forward step of the lanes `cur`: groups of kBatchG channels, each one
// pass over A; a group of one channel is that lane's own scalar step
template <typename real>
void QuadBatch<real>::forward(const std::vector<int> &cur) {
    if (f_.exact) {
        for (int b : cur) lanes_[b]->lane_forward();
        return;
    }
    for (size_t i = 0; i < cur.size(); i += kBatchG) {
        const int m = (int)std::min<size_t>(kBatchG, cur.size() - i);
        const int *ch = cur.data() + i;
        if (m == 1) lanes_[ch[0]]->lane_forward();
        else if (m == 2) forward_group<2>(ch, m);
        else if (m <= 4) forward_group<4>(ch, m);
        else forward_group<kBatchG>(ch, m);
    }
}

// IterLoop::run for B lanes in lock step: chunks of at most kBatchChunk
// bodies, the control blocks read and settled between them.  A lane that
// decided to stop or to recondition inside a chunk runs the rest of it
// halted, as a pipelined session's extra chunk does.
template <typename real>
void QuadBatch<real>::run(int iters, int *it) {
    std::vector<int> target(B_), nb(B_, 0), act, cur;
    for (int b = 0; b < B_; b++)
        target[b] = (int)std::min<long>((long)lanes_[b]->lane_it() + std::max(iters, 0),
                                        (long)lanes_[b]->lane_itmax());
    for (;;) {
        act.clear();
        int nmax = 0;
        for (int b = 0; b < B_; b++) {
            DenseLane<real> &l = *lanes_[b];
            if (l.lane_stopped() || l.lane_it() >= target[b]) continue;
            nb[b] = std::min(target[b] - l.lane_it(), kBatchChunk);
            nmax = std::max(nmax, nb[b]);
            act.push_back(b);
        }
        if (act.empty()) break;
        for (int b : act) lanes_[b]->lane_chunk_begin();
        for (int i = 0; i < nmax; i++) {
            cur.clear();
            for (int b : act)
                if (i < nb[b]) cur.push_back(b);
            for (int b : cur) lanes_[b]->lane_head();
            forward(cur);
            if (f_.rec_obj)
                for (int b : cur) lanes_[b]->lane_objective();
        }
        if (f_.gated) {
            for (int b : act) lanes_[b]->lane_snapshot();
            PFDR_HIP(hipStreamSynchronize(stream));
        }
        for (int b : act) lanes_[b]->lane_settle(nb[b]);
    }
    PFDR_HIP(hipStreamSynchronize(stream));
    for (int b = 0; b < B_; b++) {
        SessionBase &sb = lanes_[b]->base();
        if (sb.prof.on) sb.prof.resolve();
        if (it) it[b] = lanes_[b]->lane_it();
    }
}

template <typename real>
void QuadBatch<real>::result(void *X, int *it, void *Obj, void *Dif) {
    for (int b = 0; b < B_; b++)
        lanes_[b]->base().result(const_cast<char *>(at(X, (size_t)b * V_)), it ? it + b : nullptr,
                                 const_cast<char *>(at(Obj, (size_t)b * ((size_t)itMax0_ + 1))),
                                 const_cast<char *>(at(Dif, (size_t)b * (size_t)itMax0_)));
}

// every lane's own reload: the checks are the session's and read only what
// the lanes share, so the first lane refuses before any lane has changed
template <typename real>
void QuadBatch<real>::reload(const pfdr_reload *r) {
    for (int b = 0; b < B_; b++) {
        pfdr_reload lr = *r;
        lr.X = at(r->X, (size_t)b * V_);
        lr.Y = at(r->Y, (size_t)b * len_);
        lanes_[b]->base().reload(&lr);
    }
}

template <typename real>
bool QuadBatch<real>::query(const char *what, int64_t *value) {
    if (!strcmp(what, "channels")) {
        *value = B_;
    } else if (!strcmp(what, "channel_group")) {
        *value = kBatchG;
    } else if (!strcmp(what, "active")) {
        int64_t n = 0;
        for (auto &l : lanes_) n += l->lane_stopped() ? 0 : 1;
        *value = n;
    } else if (!strcmp(what, "shared_products")) {
        *value = shared_products_;
    } else if (!strcmp(what, "device_bytes")) {
        int64_t n = (int64_t)(A_.n * sizeof(real));
        for (auto &l : lanes_) n += l->base().device_bytes;
        *value = n;
    } else if (!strcmp(what, "symv")) {
        *value = lanes_[0]->base().symv;
    } else if (!strcmp(what, "dense_exact")) {
        *value = lanes_[0]->base().dense_exact;
    } else {
        return false;
    }
    return true;
}

// what pfdr_batch_create refuses, read from the arguments alone (null: none)
static std::string batch_offence(const pfdr_problem *p, int B) {
    if (B < 1 || B > kBatchMax)
        return "B must be in [1, " + std::to_string(kBatchMax) + "], got " + std::to_string(B);
    if (p->kind == PFDR_KIND_SIMPLEX) return "the simplex kind has no batched sessions";
    if (p->kind != PFDR_KIND_L1 && p->kind != PFDR_KIND_BOUNDS) return "unknown problem kind";
    if (p->dtype != PFDR_F32 && p->dtype != PFDR_F64) return "dtype must be PFDR_F32 or PFDR_F64";
    if (p->mem != PFDR_MEM_HOST && p->mem != PFDR_MEM_DEVICE)
        return "mem must be PFDR_MEM_HOST or PFDR_MEM_DEVICE";
    if (p->nranks > 1 || p->comm)
        return "a batch is for one GPU (no partition, no communicator; a device group does not "
               "apply)";
    if (p->N == 0)
        return "N == 0: an identity or diagonal A has no product to share between the channels; "
               "solve them with one reusable session (pfdr_session_create_reusable, "
               "pfdr_session_reload)";
    if (!p->A) return "A is required (A == NULL): a batch shares the dense matrix's products";
    if (p->V <= 0 || p->E < 0) return "V must be > 0 and E >= 0";
    if (!p->X || !p->Y || !p->Eu || !p->Ev || !p->La_d1)
        return "X, Y, Eu, Ev and La_d1 are required";
    if (p->N < 0 && -(long)p->N != (long)p->V) return "N < 0 requires A = A^tA and N = -V";
    if (p->kind == PFDR_KIND_BOUNDS && !(p->min <= p->max)) return "bounds: min > max or NaN";
    return std::string();
}

}  // namespace pfdr

struct pfdr_batch {
    pfdr::BatchBase *impl;
};

using namespace pfdr;

#define PFDR_BATCH_GUARD(fn, body)               \
    try {                                        \
        body;                                    \
    } catch (const HipError &h) {                \
        return report_error(fn, h);              \
    } catch (const std::exception &ex) {         \
        return report_error(fn, ex.what());      \
    }

extern "C" int pfdr_batch_create(pfdr_batch **out, const pfdr_problem *p, int B) {
    const char *fn = "pfdr_batch_create";
    if (!out || !p) return report_error(fn, "null argument");
    *out = nullptr;
    const std::string bad = batch_offence(p, B);
    if (!bad.empty()) return report_error(fn, bad.c_str());
    PFDR_BATCH_GUARD(fn, {
        BatchBase *impl = p->dtype == PFDR_F32 ? static_cast<BatchBase *>(new QuadBatch<float>(p, B))
                                               : new QuadBatch<double>(p, B);
        *out = new pfdr_batch{impl};
    });
    return PFDR_OK;
}

extern "C" int pfdr_batch_run(pfdr_batch *b, int iters, int *it) {
    const char *fn = "pfdr_batch_run";
    if (!b) return report_error(fn, "null batch");
    PFDR_BATCH_GUARD(fn, {
        StreamScope sc(b->impl->stream, b->impl->device);
        b->impl->run(iters, it);
    });
    return PFDR_OK;
}

extern "C" int pfdr_batch_result(pfdr_batch *b, void *X, int *it, void *Obj, void *Dif) {
    const char *fn = "pfdr_batch_result";
    if (!b) return report_error(fn, "null batch");
    PFDR_BATCH_GUARD(fn, {
        StreamScope sc(b->impl->stream, b->impl->device);
        b->impl->result(X, it, Obj, Dif);
    });
    return PFDR_OK;
}

extern "C" int pfdr_batch_reload(pfdr_batch *b, const pfdr_reload *r) {
    const char *fn = "pfdr_batch_reload";
    if (!b) return report_error(fn, "null batch");
    if (!r) return report_error(fn, "null argument");
    PFDR_BATCH_GUARD(fn, {
        StreamScope sc(b->impl->stream, b->impl->device);
        b->impl->reload(r);
    });
    return PFDR_OK;
}

extern "C" int pfdr_batch_query(pfdr_batch *b, const char *what, int64_t *value) {
    const char *fn = "pfdr_batch_query";
    if (!b) return report_error(fn, "null batch");
    if (!what || !value) return report_error(fn, "null argument");
    if (!b->impl->query(what, value))
        return report_error(fn, (std::string("unknown key ") + what).c_str());
    return PFDR_OK;
}

extern "C" void pfdr_batch_destroy(pfdr_batch *b) {
    if (!b) return;
    try {
        StreamScope sc(b->impl->stream, b->impl->device);
        (void)hipStreamSynchronize(b->impl->stream);
        delete b->impl;
    } catch (...) {
    }
    delete b;
}
