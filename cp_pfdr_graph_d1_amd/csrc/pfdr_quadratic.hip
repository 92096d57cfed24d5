// Session (host orchestration) of the MI355X quadratic PFDR solvers
// (reference src/PFDR_graph_quadratic_d1_l1.cpp:270-553,
//  src/PFDR_graph_quadratic_d1_bounds.cpp:244-530), single GPU or one rank
// of a 1-D vertex-range partition (pfdr_halo.hpp).  Kernels: see
// pfdr_quadratic_kernels.hpp.
#include <cstring>
#include <stdexcept>

#include "pfdr_batch.hpp"
#include "pfdr_loop.hpp"
#include "pfdr_order.hpp"
#include "pfdr_quadratic_kernels.hpp"
#include "pfdr_sort.hpp"
#include "pfdr_sparse.hpp"

namespace pfdr {

// d <- d[map] (map[i] = source index of element i)
template <typename T>
static void permute(DevBuf<T> &d, const int *map, size_t n, hipStream_t s) {
    if (!d.p || !n) return;
    DevBuf<T> t(n);
    k_gather<T><<<grid_for(n), kBlock, 0, s>>>((long)n, d.p, map, t.p);
    PFDR_HIP(hipGetLastError());
    std::swap(d.p, t.p);
    std::swap(d.n, t.n);
}

// edges sorted by their new u end (stable in the edge id): eorig[p] = the
// original id of the edge now at position p; endpoints relabelled by where
__global__ void k_edge_order_keys(long E, const int *__restrict__ Eu, const int *__restrict__ where,
                                  unsigned long long *__restrict__ keys, unsigned *__restrict__ vals) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    keys[e] = ((unsigned long long)where[Eu[e]] << 32) | (unsigned)e;
    vals[e] = (unsigned)e;
}

__global__ void k_edge_relabel(long E, const unsigned *__restrict__ eorig,
                               const int *__restrict__ Eu, const int *__restrict__ Ev,
                               const int *__restrict__ where, int *__restrict__ nEu,
                               int *__restrict__ nEv, int *__restrict__ emap) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    const unsigned e = eorig[p];
    nEu[p] = where[Eu[e]];
    nEv[p] = where[Ev[e]];
    emap[p] = (int)e;
}

template <typename real>
class QuadSession final : public IterLoop<real>, public DenseLane<real> {
  public:
    // share: the session is a lane of a batch (pfdr_batch.hpp) on that
    // batch's matrix
    explicit QuadSession(const pfdr_problem *p, const pfdr_csc *csc = nullptr,
                         bool reusable = false, const LaneShare<real> *share = nullptr);
    void reload(const pfdr_reload *r) override;
    ~QuadSession() override {
        this->close();  // (the loop's streams are drained before any buffer goes)
        for (hipEvent_t e : ev_) if (e) (void)hipEventDestroy(e);
        if (comm_) (void)hipStreamDestroy(comm_);
    }
    void result(void *X_host, int *it, void *Obj_host, void *Dif_host) override;
    void *device_x() override;
    // the seams a batch drives its lanes through (DenseLane)
    SessionBase &base() override { return *this; }
    LaneFacts facts() const override {
        return LaneFacts{V_, mode_ == A_DIRECT ? N_ : V_, mode_ == A_DIRECT, exact_, symv_,
                         gated(), rec_obj_, rows_nb_, rows_cpb_, snb_};
    }
    LaneView<real> view() override {
        return LaneView<real>{xp_.p, R_.p, Y_.p, Ga_.p, gated() ? ctrl_.p : nullptr, Rpart_.p,
                              xfull_.p, spart_.p};
    }
    const real *diag() const override { return diag_.p; }
    void lane_head() override { head(); }
    void lane_forward() override { forward_dense(gated() ? GATE_ACTIVE : GATE_NONE); }
    void lane_objective() override { objective(); }
    // the chunk boundary of a lane, whose bodies the batch launches in lock
    // step with the other lanes': the control block into the mirror (the batch
    // waits once for all its lanes), then what IterLoop::run does after a
    // chunk of n bodies (its bookkeeping and settle(), restated here)
    void lane_chunk_begin() override { it0_ = it_; }
    void lane_snapshot() override {
        PFDR_HIP(hipMemcpyAsync(hctrl_, ctrl_.p, sizeof(Ctrl<real>), hipMemcpyDeviceToHost, stream));
    }
    void lane_settle(int n) override;
    int lane_it() const override { return it_; }
    int lane_itmax() const override { return itMax_; }
    bool lane_stopped() const override { return stopped_; }

  private:
    using L = IterLoop<real>;
    using L::stream, L::prof, L::device, L::device_bytes, L::interior_edges;
    using L::reordered, L::split_blocks, L::tiled_blocks, L::record_blocks, L::slot_patterns;
    using L::edge_ratio, L::vertex_pair, L::ustaged, L::symv, L::tiny, L::fused, L::padded;
    using L::seqdif, L::la_uniform, L::dense_exact, L::sparse_exact, L::sparse_nnz, L::ghosts;
    using L::sparse_seg_col, L::sparse_seg_row, L::sparse_csr_us, L::speculative;
    using L::halo_, L::evtr_, L::ctrl_, L::hctrl_, L::itMax_, L::verbose_, L::it_;
    using L::stopped_, L::chunk_, L::tiny_, L::graphs_ok_, L::capturable_, L::kSpecMax;
    using L::spec_, L::sd_, L::seqdif_, L::chain_, L::route_, L::dws_, L::red_;
    using L::push_ctrl, L::drop_graphs, L::evolution_sum;
    using L::reusable, L::staging_bytes, L::reconditionings, L::it0_, L::next_print_;
    // The values of a problem, in the caller's order (host or device per
    // mem): everything a reload may replace.  load_values() brings them into
    // the session's order and starts the solve at iteration 0 -- the
    // constructor's and pfdr_session_reload's one path; finish_values() then
    // fills what the loop variant keeps beside the iterate.
    struct Values { int mem; const void *X, *Y, *La_d1, *La_l1, *L; };
    void set_params(double rho, double condMin, double difRcd, double difTol, double mn,
                    double mx);
    void load_values(const Values &in);
    void finish_values();
    // a caller's array where the load passes read it: device arrays as they
    // are, host arrays copied into the session's own buffer (no map) or
    // staged (st)
    const real *device_source(DevBuf<real> &st, const void *src, size_t n, int mem, real *dst,
                              bool mapped);
    bool reusable_ = false;
    int itMax0_ = 0;          // the creation's itMax (the records' size)
    bool rcd_zero_ = false;   // the creation's difRcd == 0
    bool rcd0_ = false;       // and its square in `real` == 0 (speculative sessions)
    int it_prev_ = 0;         // load_values: the iteration whose buffer a null X keeps
    bool has_l1_ = false;     // created with La_l1 (l1 kind)
    bool tracked(real difRcd, real difTol) const {
        return difTol > real(0) || difRcd > real(0) || rec_dif_;
    }
    bool hasL_ = false;       // created with L
    real L0_ = real(1);       // a scalar L
    DevBuf<real> stg_e_, stg_v_[4];  // staged La_d1; Y, La_l1, L, X
    DevBuf<int> flags_;       // the load passes' verdicts (VF_*)
    int64_t rr_counted_ = 0;  // rr_'s bytes within device_bytes
    int64_t stage_bytes() const {
        size_t n = stg_e_.n;
        for (const DevBuf<real> &b : stg_v_) n += b.n;
        return (int64_t)(n * sizeof(real));
    }
    // problem
    int flavour_;  // 0 l1, 1 bounds
    int V_, Vg_, N_, mode_;
    long E_;
    real rho_, condMin_, difTol_, difRcd2_, cap_;
    int prox_, positivity_;
    real lo_, hi_;
    bool Ldiag_;
    bool rec_obj_, rec_dif_, track_;
    // XCD-aware block order (xcd_block): runs of 64 edge blocks / 16 vertex
    // blocks per XCD, so the neighbour bands a run gathers share one L2
    // (paired A/B on the headline: 0.754 -> 0.727 ms/iter; profiles/r1/r1zk)
    static constexpr int xcd_e_ = 64, xcd_v_ = 16;
    // the edge sweep stages the u ends of u-sorted edges in LDS (k_edge_sweep_us)
    // for graphs of at least 4 edges per vertex and for small (latency-bound)
    // graphs.  Measured (r2zf, paired, ms per edge sweep): headline 6 edges
    // per vertex 0.457 staged vs 0.472, shuffled headline 0.468 vs 0.500, C1
    // (130K edges) 0.008-0.010 vs 0.019; but 3 edges per vertex C2 0.450 vs
    // 0.394 and C5 6.55 vs 5.81 -- with few edges per u end the block's
    // staging barrier and search cost more than the Eu stream and the
    // (cache-served) u-end gathers they replace.
    bool us_ = true;
    DevBuf<char> mono_ws_;       // mono_sum scratch (tile summaries)
    // uniform La_d1 (k_load_edge's verdict): the iteration kernels take
    // the one value la0_ instead of streaming the array (4 B per edge)
    bool la_uniform_ = false;
    real la0_ = real(0);
    // uniform La_l1 (the headline's 0.01): the vertex sweep forms Th_l1 =
    // Ga * l1u instead of reading it (4 B per vertex)
    bool l1_uniform_ = false;
    real l1u_ = real(0);
    const real *la_it() const { return la_uniform_ ? nullptr : La_d1_.p; }
    // iterate evolution with the reference's sequential rounding
    // (PFDR_EVOLUTION_*, include/pfdr_mi355x.h): the vertex sweep stores the
    // terms (X_ - X)^2 and X^2 in the caller's vertex order, two binade-scan
    // sums (mono_sum) replace the tree of k_reduce_decide, k_decide decides
    int evo_ = PFDR_EVOLUTION_AUTO;
    long tstride_ = 0;
    DevBuf<real> terms_;
    void seq_evolution(real *terms, const real *part, hipStream_t s);
    void sweeps(const Ctrl<real> *c);  // halo pull, edge sweep, halo push, vertex sweep
    // Speculative iteration (IterLoop::spec_; here: difRcd = 0, identity /
    // diagonal A): X cycles through D buffers (iteration t reads xpb(t - 1),
    // writes xpb(t)) and the terms and their block sums through D
    DevBuf<R2<real>> xpx_[kSpecMax - 1];  // X buffers 1 .. D - 1 (0 is xp_)
    R2<real> *xpb(int t) { return spec_ && t % sd_ ? xpx_[t % sd_ - 1].p : xp_.p; }
    R2<real> *xr_ = nullptr, *xw_ = nullptr;  // the sweeps' read / write (X, P)
    void spec_sweeps(int t, int b) override;
    void spec_decide(int b, hipStream_t s) override;
    static constexpr long kSeqDifMin = 1L << 17;  // AUTO: sums of at least this many terms
    // internal relabelling (pfdr_order.hpp): order_[new] = old, where_[old] = new,
    // emap_[edge position] = original edge id (both maps: the value loads; a
    // reusable session keeps them)
    bool reordered_ = false;
    DevBuf<int> order_, where_, emap_;
    DevBuf<unsigned> eorig_;
    DevBuf<real> amp_orig_;
    // device state
    DevBuf<int> Eu_, Ev_;
    DevBuf<real> La_d1_, La_l1_, Y_, A_, L_;
    DevBuf<R2<real>> xp_;
    DevBuf<real> diag_, Ga_, invAux_, Th_l1_, absval_, grad_, pre_, xout_;
    // a lane of a batch borrows A_ and, past the first lane, diag_ (their n
    // stays 0: the owner counts them).  Declared after them, so destroyed
    // before them -- also when the constructor throws: a borrowed pointer is
    // dropped, never freed here
    struct Borrowed {
        DevBuf<real> *a = nullptr, *d = nullptr;
        ~Borrowed() {
            if (a) a->p = nullptr;
            if (d) d->p = nullptr;
        }
    } borrowed_;
    DevBuf<real> Z2_, wz_;
    // splitting weights as factors (k_d1_weights): a_e = cw_ La_d1[e] until the
    // first reconditioning, then A1_[e]; (Ga, invAux) pairs of every vertex
    DevBuf<real> A1_;
    DevBuf<R2<real>> gi_;
    DevBuf<real> rr_;  // per-vertex (cw la0 / Aux) / Ga of the ratio edge sweep (rat())
    bool rat_on_ = false;  // rr_ formed at setup (see rat())
    real cw_ = real(0);
    DevBuf<real> R_, vpart_, opart_, Obj_, Dif_, csum_;
    DevBuf<double> Rpart_;  // k_rows_partial's double partials
    DevBuf<real> Rsum_, xfull_;  // dense A on a partition: summed A X, gathered X
    // relabelled partition (pfdr_problem.vtx_label): the caller's label of
    // each owned vertex; the amplitudes are all-reduced into ampg_ at those
    // labels and summed in the caller's order on every rank
    DevBuf<int> lab_;
    DevBuf<real> ampg_;
    long v0_ = 0, Vglob_ = 0;
    DevBuf<long long> ccnt_;
    DevBuf<int> cnt_part_;
    Incidence inc_;
    HostPins pins_;  // caller arrays pinned for the setup copies
    // the contribution layouts (pfdr_layout.hpp): large single-GPU graphs and
    // partitioned ranks keep their edges in tile order (tiled_), the others
    // get the split incidence where their edges are sorted by u
    bool tiled_ = false;
    TileLayout tile_;
    SplitLayout split_;
    int nbv_, nbe_, nbn_, rows_nb_, rows_cpb_;

    void setup_graph(const pfdr_problem *p);
    void amplitude(bool init);
    void precondition(bool init);
    void gemv_rows(int gate);
    void forward_dense(int gate);
    void gradient();
    void objective();
    void head();  // the sweeps and the loop decision of one iteration (not fused)
    void body(int i, int n) override;
    void recondition() override;
    void print_progress() override;
    bool gated() const override { return track_ || rec_obj_; }
    void pull(void *base, int eb) { if (halo_) halo_->pull(base, eb, stream); }
    // halo / compute overlap (partitioned sessions): the halo exchanges run
    // on comm_ while the sweeps of interior edges [elo_, ehi_) and interior
    // vertex blocks [blo_, bhi_) (no ghost endpoint, no received
    // contribution) run on the session stream
    hipStream_t comm_ = nullptr;
    hipEvent_t ev_[4] = {};  // xp ready, pulled, boundary W*Z ready, pushed
    long elo_ = 0, ehi_ = 0;
    long zs_ = 0;    // Z layout: 0 half-edge pairs, E side-major (tiled sessions)
    // Z-direct: a tiled single-GPU session with one edge weight and no A1
    // (before any reconditioning) skips the W * Z stores of the edge sweep;
    // the vertex sweep reads Z and forms each term with its own weight
    // (a partitioned session only when every rank qualifies with the same
    // weight, zd_ranks_: the ranks then push Z, and each owner forms the
    // received terms with its own weight like the local ones)
    bool zd_ranks_ = false;
    bool zdirect() const { return tiled_ && !A1_.p && (halo_ ? zd_ranks_ : !la_it()); }
    // one edge weight and no W * Z stream (until the first reconditioning):
    // the tiled edge sweep reads the ends' formed ratios (k_ratio_vertex)
    // instead of their (Ga, invAux) pairs
    bool rat() const { return rat_on_ && zdirect() && !la_it(); }
    int blo_ = 0, bhi_ = 0;
    bool overlap_ = false;
    void plan_overlap();
    // one launch over [ebeg, eend) and, if not empty, [ebeg2, eend2)
    void edge_sweep(long ebeg, long eend, const Ctrl<real> *c, const char *name,
                    long ebeg2 = 0, long eend2 = 0, const FuseDecide<real> *fd = nullptr);
    // one launch over the blocks [bbeg, bend) and, if not empty, [bbeg2, bend2)
    void vertex_sweep(int bbeg, int bend, const Ctrl<real> *c, const char *name,
                      int bbeg2 = 0, int bend2 = 0);
    VArgs<real> vargs(int bbeg, int bend, const Ctrl<real> *c);
    // small single-GPU graphs: a chunk of iterations in one workgroup launch
    // (k_tiny_iterate; PFDR_TINY = max edges, 0 = off)
    void tiny_chunk(int n) override;
    const real *full_x();  // X of every vertex (A^tA mode), gathered over the ranks
    // A^tA mode on one GPU with an exactly symmetric matrix: products from the
    // block upper triangle (k_symv_tiles / k_symv_finish, half the bytes)
    bool symv_ = false;
    int snb_ = 0;
    // small dense problems on one GPU (CP's reduced problems): every dot
    // product in the reference's sequential order (k_col_seq, k_rows_seq),
    // bit-exact, when the longest chain (max(N, V) direct, V for A^tA) is
    // <= kExactChain
    bool exact_ = false;
    static constexpr long kExactChain = 8192;
    // small graphs (<= kFuseBlocks vertex blocks, dif tracked, one GPU):
    // the loop decision on iteration t taken inside the edge sweep of t + 1,
    // two launches per iteration instead of three (FuseDecide in
    // pfdr_quadratic_kernels.hpp); the decisions alternate between ctrl_
    // (even bodies of a chunk) and ctrl2_ (odd), the chunk's closing
    // decision lands in ctrl_.
    bool fuse_ = false;
    DevBuf<Ctrl<real>> ctrl2_;
    // fused sessions whose vertex blocks have at most kPadPer * kBlock CSR
    // entries: the edge sweep stores each contribution at its slot sl_[2e +
    // side] of its block's list in wzp_ (stride pad_nmax_), and the vertex
    // sweep (k_vertex_sweep_pad) stages its block's list with one dependent
    // round trip instead of three.
    bool pad_ = false;
    static constexpr int kPadBlocks = 512;
    int pad_nmax_ = 0;
    DevBuf<int> sl_;
    DevBuf<real> wzp_;
    // and, in f32 up to kEndsBlocks, the endpoint data as per-edge copies: (X, P)
    // and (Ga, 1/Aux) of both ends at xpe_ / gie_ [2e + side], scattered by
    // the vertex sweep through pidx_ (the end of each list entry), so the
    // edge sweep (k_edge_sweep_ends) streams everything: one dependent
    // round trip.
    bool ends_ = false;
    static constexpr int kEndsBlocks = 512;
    DevBuf<int> pidx_;
    DevBuf<R2<real>> xpe_, gie_;
    void refresh_ends();
    void plan_pad();
    PadOut<real> pad_out() const { return PadOut<real>{pad_ ? sl_.p : nullptr, wzp_.p}; }
    template <int EPI> void col_product(ColArgs<real> ca);
    // sparse A (pfdr_sparse.hpp): the session runs as a direct-mode one
    // (mode_ = A_DIRECT: Y of length N, R_, the objective's residual term, no
    // tiny or fused path) whose four products walk the CSC / CSR instead of A_
    bool sparse_ = false;
    SparseOp<real> sp_;
    // Sessions whose products run in the reference's order (exact_, or a
    // sparse A on its sequential kernels; weights >= 0) sum the recorded
    // objective in that order too (k_obj_terms, three mono_sum's; in A^tA
    // mode the data term, whose terms change sign, through k_obj_data_seq):
    // Obj is then the reference's, bit for bit, like X, it and Dif.
    // oterms_ = the terms of the N rows, E edges (caller's edge order: a
    // tiled session keeps emap_, its edge positions, for it) and V vertices,
    // each part 16-byte aligned.
    bool seqobj_ = false;
    DevBuf<real> oterms_;
    bool keep_oemap() const { return sparse_ && rec_obj_; }
    const int *oemap() const { return keep_oemap() ? emap_.p : nullptr; }
    DevBuf<char> ows_;
    long ot_e_ = 0, ot_v_ = 0;  // offsets of the edge and vertex terms
  public:
    bool sparse_csr(int64_t *rowptr, int32_t *colidx, void *rval) override {
        if (!sparse_) return false;
        sp_.read_csr(rowptr, colidx, rval, stream);
        return true;
    }
  private:
    DevBuf<real> spart_;
    void plan_symv(int known);
    template <int EPI> void ata_product(ColArgs<real> ca);
};

// ----------------------------------------------------------------- setup --
template <typename real>
QuadSession<real>::QuadSession(const pfdr_problem *p, const pfdr_csc *csc, bool reusable_session,
                               const LaneShare<real> *share) {
    if (p->V <= 0 || p->E < 0) throw std::runtime_error("V must be > 0 and E >= 0");
    if (!p->X || !p->Y || !p->Eu || !p->Ev || !p->La_d1)
        throw std::runtime_error("X, Y, Eu, Ev and La_d1 are required");
    if (reusable_session && (p->nranks > 1 || p->comm))
        throw std::runtime_error("a reusable session is for one GPU (no partition, no "
                                 "communicator)");
    reusable_ = reusable_session;
    reusable = reusable_ ? 1 : 0;
    PFDR_HIP(hipGetDevice(&device));
    stream = lib_stream();
    pins_.set_stream(stream);
    hipStream_t s = stream;
    flavour_ = (p->kind == PFDR_KIND_BOUNDS) ? 1 : 0;
    V_ = p->V;
    E_ = p->E;
    N_ = p->N;
    itMax_ = p->itMax;
    verbose_ = p->verbose;
    if (N_ > 0) mode_ = A_DIRECT;
    else if (N_ < 0) mode_ = A_ATA;
    else mode_ = p->A ? A_DIAG : A_IDENT;
    sparse_ = csc != nullptr;
    if (sparse_) {
        if (N_ <= 0) throw std::runtime_error("sparse A requires N > 0");
        if (p->A) throw std::runtime_error("sparse A given together with a dense A");
        if (p->nranks > 1 || p->comm)
            throw std::runtime_error("sparse A is for one GPU (no partition, no communicator)");
        if (!csc->colptr || !csc->rowidx || !csc->val)
            throw std::runtime_error("sparse A: colptr, rowidx and val are required");
        if (csc->nnz <= 0 || csc->nnz >= (1LL << 31) - 256)
            throw std::runtime_error("sparse A: nnz must be in [1, 2^31 - 256)");
    }
    if (mode_ == A_DIRECT && !p->A && !sparse_) throw std::runtime_error("N > 0 requires A");
    if (mode_ == A_ATA && !p->A) throw std::runtime_error("N < 0 requires A = A^tA");
    itMax0_ = itMax_;
    rec_obj_ = p->record_obj != 0;
    rec_dif_ = p->record_dif != 0;
    positivity_ = flavour_ == 0 && p->positivity != 0;
    has_l1_ = flavour_ == 0 && p->La_l1;
    set_params(p->rho, p->condMin, p->difRcd, p->difTol, p->min, p->max);
    track_ = tracked((real)p->difRcd, (real)p->difTol);
    rcd_zero_ = p->difRcd == 0.0;
    rcd0_ = difRcd2_ == real(0);
    evo_ = p->evolution;
    if (evo_ < PFDR_EVOLUTION_AUTO || evo_ > PFDR_EVOLUTION_TREE)
        throw std::runtime_error("evolution must be PFDR_EVOLUTION_AUTO, _SEQUENTIAL or _TREE");
    const bool want_seq = track_ && evo_ == PFDR_EVOLUTION_SEQUENTIAL;
    Ldiag_ = (p->Ltype == PFDR_LIPSCHITZ_DIAG) && p->L;
    hasL_ = p->L != nullptr;
    us_ = E_ >= 4L * V_ || E_ < (1L << 22);

    // small single-GPU graphs iterate in one 1024-lane workgroup
    // (k_tiny_iterate, four vertex blocks at a time): against the two-launch
    // loop (fused decision, per-block lists) on 4-NN grids, us/iteration
    // (profiles/r2/r2zv_exp_tiny.log): f32 1 block 4.4 vs 8.9, 4: 6.6 vs
    // 10.8, 8: 10.5 vs 10.8, 16: 19.3 vs 11.1; f64 4: 8.0 vs 10.0, 8: 13.5
    // vs 9.8 -- so up to 8 blocks in f32, 5 in f64, and 8192 edges.  The
    // split incidence is not built for them (one setup round trip less).
    if (!(p->nranks > 1 || p->comm) && !rec_obj_ && (mode_ == A_IDENT || mode_ == A_DIAG) &&
        E_ > 0 && !want_seq) {
        const char *t = getenv("PFDR_TINY");
        const long maxE = t ? atol(t) : 8192;
        const int maxB = t ? kTinyMaxBlocks : (sizeof(real) == 4 ? 8 : 5);
        tiny_ = E_ <= maxE && (V_ + kBlock - 1) / kBlock <= maxB;
        tiny = tiny_ ? 1 : 0;
    }
    // graph, partition plan, incidence CSR
    setup_graph(p);
    // dense A on a partition: this rank's columns (its vertices); A^tA columns
    // have the global length
    v0_ = halo_ ? (long)halo_->vtx_begin : 0;
    Vglob_ = halo_ ? (long)halo_->off.back() : V_;
    if (p->vtx_label) {
        if (!halo_) throw std::runtime_error("vtx_label is for partitioned sessions");
        caller_labels(p->vtx_label, p->mem, V_, Vglob_, lab_, *halo_->tr, s);
    }
    if (mode_ == A_ATA && -(long)N_ != Vglob_)
        throw std::runtime_error("N < 0 requires A = A^tA (columns of the owned vertices, "
                                 "length V) and N = -V (V over all ranks)");
    if ((mode_ == A_DIRECT || mode_ == A_ATA) && !halo_ && !sparse_) {
        const long chain = mode_ == A_DIRECT ? std::max<long>(N_, V_) : (long)V_;
        exact_ = chain <= kExactChain;
        dense_exact = exact_ ? 1 : 0;
    }
    const int mem = p->mem;
    const size_t V = V_, E = E_, Vg = Vg_;
    // the matrix and what depends on it alone: kept by a reload
    const size_t asz = sparse_ ? 0 : mode_ == A_DIRECT ? (size_t)N_ * V
                     : mode_ == A_ATA ? (size_t)Vglob_ * V : mode_ == A_DIAG ? V : 0;
    if (share) {  // (a lane: the batch holds and counts the matrix)
        A_.p = const_cast<real *>(share->A);
        borrowed_.a = &A_;
    }
    else copy_in(A_, p->A, asz, mem, s, pins_);
    if (sparse_) {  // checked copy of the CSC, CSR view, kernel family
        sp_.setup(V_, N_, csc, mem, kExactChain, s, pins_);
        sparse_exact = sp_.exact ? 1 : 0;
        sparse_nnz = sp_.m.nnz;
        sparse_seg_col = sp_.gc;
        sparse_seg_row = sp_.gr;
        sparse_csr_us = (int64_t)(sp_.m.csr_ms * 1e3);
    }
    if (reordered_) {  // into the internal labels (identity / diagonal A only)
        permute(A_, order_.p, V, s);
        amp_orig_.alloc(V);
    }
    // the session's copies of the values (load_values fills them), the
    // iterate's (X, P) pairs, owned then ghost vertices
    if (E) La_d1_.alloc(E);
    if (has_l1_) La_l1_.alloc(V);
    Y_.alloc(mode_ == A_DIRECT ? (size_t)N_ : V);
    if (Ldiag_) L_.alloc(V);
    xp_.alloc(Vg + 2);  // (+2: the tiled edge sweep stages vertex pairs, k_edge_sweep_tl)
    PFDR_HIP(hipMemsetAsync(xp_.p, 0, (Vg + 2) * sizeof(R2<real>), s));
    flags_.alloc(4);
    // edge state and per-vertex metric
    const size_t En = E ? E : 1;
    // (tiled partitioned ranks: Z's received tail after the 2E local entries,
    // for the Z-direct iteration)
    // (+kSlotGroup: the tiled vertex sweep reads whole groups of a run's tail, tile_sum)
    Z2_.alloc(2 * En + (halo_ ? (size_t)halo_->R : 0) + kSlotGroup);
    gi_.alloc(Vg + 2);
    PFDR_HIP(hipMemsetAsync(gi_.p, 0, (Vg + 2) * sizeof(R2<real>), s));
    if (share && share->diag) {
        diag_.p = const_cast<real *>(share->diag);
        borrowed_.d = &diag_;
    } else {
        diag_.alloc(V);
    }
    Ga_.alloc(Vg); invAux_.alloc(Vg); absval_.alloc(V);
    if (flavour_ == 0 && p->La_l1) Th_l1_.alloc(V);
    nbv_ = grid_for(V);
    nbe_ = grid_for(E);
    nbn_ = mode_ == A_DIRECT ? grid_for(N_) : 0;
    cnt_part_.alloc(nbv_);
    vpart_.alloc(2 * (size_t)nbv_);
    red_.alloc(4);
    csum_.alloc(1);
    ccnt_.alloc(1);
    if (rec_obj_) {
        opart_.alloc(2 * (size_t)nbv_ + nbe_ + nbn_ + 1);
        Obj_.alloc((size_t)itMax_ + 1);
    }
    if (rec_dif_) Dif_.alloc(itMax_ > 0 ? itMax_ : 1);
    if (mode_ == A_DIRECT) {
        R_.alloc(N_);
        pre_.alloc(V);
        rows_nb_ = std::max(1, std::min(512, (V_ + 63) / 64));
        rows_cpb_ = (V_ + rows_nb_ - 1) / rows_nb_;
        rows_nb_ = (V_ + rows_cpb_ - 1) / rows_cpb_;
        if (!sparse_) Rpart_.alloc((size_t)rows_nb_ * N_);
    }
    if (mode_ == A_ATA) {
        pre_.alloc(V); xout_.alloc(V); xfull_.alloc(Vglob_);
        plan_symv(share ? share->symv : -1);
    }
    if (mode_ == A_DIRECT && halo_) Rsum_.alloc(N_);

    this->alloc_ctrl();

    // diagonal of A^t A
    if (borrowed_.d) {
        // (a lane: the first lane's)
    } else if (mode_ == A_DIRECT) {
        ColArgs<real> ca{};
        ca.A = A_.p; ca.ncols = V_; ca.len = N_; ca.out = diag_.p;
        // (a sparse session's two setup products are always timed: profiling
        // cannot be switched on before the session exists)
        const bool pon = prof.on;
        prof.on = pon || sparse_;
        {
            ProfScope ps(prof, "diag_cols", s);
            col_product<EPI_SELF>(ca);
        }
        prof.on = pon;
        if (sparse_) {
            k_sp_norm_check<real><<<grid_for(V), kBlock, 0, s>>>(V_, diag_.p, sp_.m.word.p);
            PFDR_HIP(hipGetLastError());
            if (sp_.m.verdict(s))
                throw std::runtime_error("sparse A: a column has squared norm 0 (the reference "
                                         "divides by it)");
        }
    } else {
        k_diag<real><<<grid_for(V), kBlock, 0, s>>>(V_, mode_, A_.p, Vglob_, v0_, diag_.p);
    }
    PFDR_HIP(hipGetLastError());
    zs_ = tiled_ ? E_ : 0;
    load_values(Values{p->mem, p->X, p->Y, p->La_d1, p->La_l1, p->L});
    if (halo_) {  // Z-direct on every rank or on none (see zdirect)
        Transport &tr = *halo_->tr;
        DevBuf<real> l0(1);
        DevBuf<int64_t> nbad(1);
        PFDR_HIP(hipMemcpyAsync(l0.p, &la0_, sizeof(real), hipMemcpyHostToDevice, s));
        tr.broadcast(l0.p, sizeof(real), 0, s);
        real la0r0 = real(0);
        PFDR_HIP(hipMemcpyAsync(&la0r0, l0.p, sizeof(real), hipMemcpyDeviceToHost, s));
        tr.wait(s);
        const int64_t mine = (tiled_ && la_uniform_ && la0_ == la0r0) ? 0 : 1;
        PFDR_HIP(hipMemcpyAsync(nbad.p, &mine, sizeof(int64_t), hipMemcpyHostToDevice, s));
        tr.allreduce_sum(nbad.p, 1, 2, s);
        int64_t all = 1;
        PFDR_HIP(hipMemcpyAsync(&all, nbad.p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        tr.wait(s);
        zd_ranks_ = all == 0;
    }
    interior_edges = E_;

    device_bytes = 0;
    auto acc = [&](size_t b) { device_bytes += (int64_t)b; };
    acc(Eu_.n * 4 + Ev_.n * 4);
    for (DevBuf<real> *b : {&La_d1_, &La_l1_, &Y_, &A_, &L_, &diag_, &Ga_, &invAux_, &Th_l1_, &absval_,
                            &pre_, &Z2_, &A1_, &wz_, &R_,
                            &vpart_, &opart_, &Obj_, &Dif_, &xout_, &Rsum_, &xfull_, &spart_})
        acc(b->n * sizeof(real));
    acc(Rpart_.n * sizeof(double));
    acc(sp_.bytes());
    acc((xp_.n + gi_.n) * sizeof(R2<real>) + inc_.ptr.n * 4 + inc_.idx.n * 4);
    acc(split_.bytes() + tile_.bytes());
    if (halo_) {
        plan_overlap();
        // RCCL partitions replay captured chunks too (pull, sweeps, push and
        // the all-reduces of a chunk of iterations in one hipGraph launch:
        // the host's ~30 API calls per iteration otherwise approach a rank's
        // GPU time at N = 8); the loopback transport rendezvous on the host
        capturable_ = halo_->tr->capturable() && !rec_obj_;
        graphs_ok_ = itMax_ >= 2 * chunk_ && capturable_;
    } else if (!tiny_) {
        // (a lane's bodies are launched by its batch, in lock step: no graph)
        capturable_ = !share;
        graphs_ok_ = capturable_ && itMax_ >= 2 * chunk_;
        // (an edgeless graph has no edge sweep to carry the decision)
        fuse_ = track_ && !rec_obj_ && (mode_ == A_IDENT || mode_ == A_DIAG) &&
                nbv_ <= kFuseBlocks && E_ > 0 && !want_seq;
        if (fuse_) ctrl2_.alloc(1);
        fused = fuse_ ? 1 : 0;
        if (fuse_) plan_pad();
    }
    // sequential evolution statistic: the plain multi-launch loop on one GPU;
    // a partition sums in the caller's order across the ranks (seq_evolution)
    seqdif_ = track_ && !tiny_ && !fuse_ &&
              (want_seq || (evo_ == PFDR_EVOLUTION_AUTO && Vglob_ >= kSeqDifMin));
    if (seqdif_) {
        const long nt = V_;  // terms per sum, in this rank's vertex order
        tstride_ = (nt + 3) / 4 * 4;  // 16-byte aligned second array
        terms_.alloc(2 * (size_t)tstride_);
        if (!halo_) {
            dws_.alloc(mono_ws_bytes<real>(nt, 2));
        } else if (lab_.p) {  // routed to caller-order slices, then chained
            std::vector<int> hl(V_);
            PFDR_HIP(hipMemcpy(hl.data(), lab_.p, sizeof(int) * V_, hipMemcpyDeviceToHost));
            route_.init(hl, Vglob_, 2, 1, *halo_->tr, s);
        } else {
            chain_.init(V_, 2, *halo_->tr);
        }
        seqdif = 1;
        const int smode = spec_mode(p);
        spec_ = difRcd2_ == real(0) && !rec_obj_ && (mode_ == A_IDENT || mode_ == A_DIAG) &&
                smode != PFDR_SPEC_OFF;
        if (spec_) {
            this->spec_setup(smode == PFDR_SPEC_SERIAL);
            // the halo exchanges stay on the session stream: a third stream
            // for them (overlap_) shared a hardware queue with the evolution
            // stream, so the next pull waited behind the whole evolution chain
            // (1-rank RCCL headline_conv 0.686 ms/iter against 0.557 on one GPU)
            if (evtr_) overlap_ = false;
            DevBuf<real> t2((size_t)sd_ * 2 * tstride_);  // terms of D iterations
            std::swap(terms_.p, t2.p);
            std::swap(terms_.n, t2.n);
            DevBuf<real> p2((size_t)sd_ * 2 * nbv_);  // and their block sums
            std::swap(vpart_.p, p2.p);
            std::swap(vpart_.n, p2.n);
            for (int k = 0; k + 1 < sd_; k++) xpx_[k].alloc(Vg_ + 2);  // (+2 as xp_)
        }
    }
    {
        // the ratio edge sweep where it pays: not beside an overlapped
        // evolution chain, whose kernels the faster sweep (eight waves per
        // SIMD against the pair sweep's seven) leaves no room to run in --
        // converged headline 0.570 ms/iter against 0.524 (f6d).
        // PFDR_EDGE_RATIO=0 / 1: never / wherever it applies.
        const char *e = getenv("PFDR_EDGE_RATIO");
        rat_on_ = e && *e ? e[0] != '0' : speculative != 1;
    }
    // the inputs are in the internal order now: only a reusable session
    // needs the maps again (the sequential evolution of a relabelled session
    // keeps order_, a sparse session's sequential objective emap_)
    if ((!seqdif_ || !reordered_) && !reusable_) order_.release();
    if (!reusable_) {
        if (!keep_oemap()) emap_.release();
        stg_e_.release();
        for (DevBuf<real> &b : stg_v_) b.release();
    } else {
        staging_bytes = stage_bytes();
        acc(emap_.n * 4 + (size_t)staging_bytes);
    }
    acc(where_.n * 4 + amp_orig_.n * sizeof(real) + order_.n * 4 + terms_.n * sizeof(real) + dws_.n);
    acc(route_.slice.n * sizeof(real) + route_.chain.ws.n + chain_.ws.n + ampg_.n * sizeof(real) +
        (xpx_[0].n + xpx_[1].n + xpx_[2].n) * sizeof(R2<real>));
    acc(sl_.n * 4 + wzp_.n * sizeof(real) + pidx_.n * 4 + (xpe_.n + gie_.n) * sizeof(R2<real>));
    finish_values();
    this->instantiate_setup_graph();
}

// rho, condMin, the evolution thresholds and the prox (ref l1 :499-512,
// bounds :472-490) of a problem
template <typename real>
void QuadSession<real>::set_params(double rho, double condMin, double difRcd, double difTol,
                                   double mn, double mx) {
    rho_ = (real)rho;
    condMin_ = (real)condMin;
    difTol_ = (real)difTol;
    const real rcd = (real)difRcd;
    difRcd2_ = rcd * rcd;
    lo_ = hi_ = real(0);
    if (flavour_ == 0) {
        prox_ = has_l1_ ? PROX_L1 : (positivity_ ? PROX_POS : PROX_NONE);
    } else {
        lo_ = (real)mn;
        hi_ = (real)mx;
        const real inf = Lim<real>::huge;
        const bool haslo = -inf < lo_, hashi = hi_ < inf;
        prox_ = (haslo && hashi) ? PROX_BOX : haslo ? PROX_LO : hashi ? PROX_HI : PROX_NONE;
    }
}

template <typename real>
const real *QuadSession<real>::device_source(DevBuf<real> &st, const void *src, size_t n, int mem,
                                             real *dst, bool mapped) {
    if (!src || !n) return nullptr;
    if (mem == PFDR_MEM_DEVICE) return static_cast<const real *>(src);
    if (!mapped && dst) {  // nothing to reorder: straight into the session's copy
        pins_.copy(dst, src, n * sizeof(real), hipMemcpyHostToDevice);
        return nullptr;
    }
    if (st.n < n) st.alloc(n);
    pins_.copy(st.p, src, n * sizeof(real), hipMemcpyHostToDevice);
    return st.p;
}

// The values `in` (null: the session's own) into the internal order and the
// solve at iteration 0: the control block, the iterate and Z = X at both
// ends, the weights' uniformity, the first preconditioning and forward
// step, Obj[0].  What depends on the graph or on A alone is not touched.
template <typename real>
void QuadSession<real>::load_values(const Values &in) {
    hipStream_t s = stream;
    const size_t V = V_, E = E_;
    const int mem = in.mem;
    it_ = it0_ = next_print_ = 0;
    reconditionings = 0;
    stopped_ = (itMax_ <= 0);
    // control block
    this->reset_ctrl();
    const real difTol2 = difTol_ * difTol_;
    hctrl_->dif = difTol2 > difRcd2_ ? difTol2 : difRcd2_;  // ref :342
    hctrl_->difTol = difTol2;
    hctrl_->difRcd = difRcd2_;
    hctrl_->eps = (real(0) < difTol_ && difTol_ < Lim<real>::eps) ? difTol_ : Lim<real>::eps;
    push_ctrl();
    // scalar cap of the metric (ref :225-229), in `real` arithmetic like the reference
    real cap = real(1.9) * (real(2) - rho_);
    if (hasL_ && !Ldiag_) {
        if (in.L) {
            PFDR_HIP(hipMemcpyAsync(&L0_, in.L, sizeof(real),
                                    mem == PFDR_MEM_DEVICE ? hipMemcpyDeviceToHost
                                                           : hipMemcpyHostToHost, s));
            PFDR_HIP(hipStreamSynchronize(s));
        }
        cap /= L0_;
    }
    cap_ = cap;
    // the arrays into the internal order, the iterate's (X, 0) pairs
    const int *ord = reordered_ ? order_.p : nullptr;
    const bool vlen = mode_ != A_DIRECT;  // Y of length V
    if (!vlen && in.Y) {
        if (mem == PFDR_MEM_DEVICE)
            PFDR_HIP(hipMemcpyAsync(Y_.p, in.Y, sizeof(real) * N_, hipMemcpyDeviceToDevice, s));
        else
            pins_.copy(Y_.p, in.Y, sizeof(real) * N_, hipMemcpyHostToDevice);
    }
    VLoad<real> va{};
    va.V = V_;
    va.order = ord;
    va.Yd = vlen ? Y_.p : nullptr;
    va.l1d = La_l1_.p;
    va.Ld = Ldiag_ ? L_.p : nullptr;
    va.Y = vlen ? device_source(stg_v_[0], in.Y, V, mem, Y_.p, ord != nullptr) : nullptr;
    va.l1 = La_l1_.p ? device_source(stg_v_[1], in.La_l1, V, mem, La_l1_.p, ord != nullptr)
                     : nullptr;
    va.L = Ldiag_ ? device_source(stg_v_[2], in.L, V, mem, L_.p, ord != nullptr) : nullptr;
    va.X = device_source(stg_v_[3], in.X, V, mem, nullptr, ord != nullptr);
    va.xcur = xpb(it_prev_);
    va.xp = xp_.p;
    va.flags = flags_.p;
    PFDR_HIP(hipMemsetAsync(flags_.p, 0, 4 * sizeof(int), s));
    k_load_vertex<real><<<grid_for(V, Vec<real>::kPer16B), kBlock, 0, s>>>(va);
    PFDR_HIP(hipGetLastError());
    pull(xp_.p, sizeof(R2<real>));
    // the edge weights, Z = X at both ends
    if (E_) {
        const real *la = device_source(stg_e_, in.La_d1, E, mem, La_d1_.p, emap_.p != nullptr);
        k_load_edge<real><<<grid_for(E, Vec<real>::kPer16B), kBlock, 0, s>>>(
            E_, emap_.p, la, La_d1_.p, Eu_.p, Ev_.p, xp_.p, Z2_.p, zs_, flags_.p);
        PFDR_HIP(hipGetLastError());
    }
    // the splitting weights are cw La_d1 again, whatever a reconditioning left
    A1_.release();
    // first preconditioning, first forward step
    precondition(true);
    if (mode_ == A_IDENT || mode_ == A_DIAG) {
        if (grad_.n < V) grad_.alloc(V);
        k_grad_vertex<real><<<grid_for(V), kBlock, 0, s>>>(V_, mode_, A_.p, Y_.p, xp_.p, grad_.p);
        k_forward_grad<real><<<grid_for(V), kBlock, 0, s>>>(V_, Ga_.p, grad_.p, xp_.p);
        PFDR_HIP(hipGetLastError());
        if (!reusable_) grad_.release();
    } else {
        forward_dense(GATE_NONE);
    }
    int hf[4] = {1, 1, 1, 1};
    seqobj_ = false;
    if (rec_obj_ && !halo_ &&
        ((mode_ == A_DIRECT && (exact_ || (sparse_ && sp_.exact))) || (mode_ == A_ATA && exact_))) {
        PFDR_HIP(hipMemcpyAsync(hf, flags_.p, sizeof(hf), hipMemcpyDeviceToHost, s));
        PFDR_HIP(hipStreamSynchronize(s));
        seqobj_ = !hf[VF_D1_NEG] && !hf[VF_L1_NEG];
        if (seqobj_ && !oterms_.p) {
            ot_e_ = mode_ == A_DIRECT ? ((long)N_ + 3) / 4 * 4 : 0;  // (A^tA: no row terms)
            ot_v_ = ot_e_ + (E_ + 3) / 4 * 4;
            oterms_.alloc((size_t)ot_v_ + V);
            ows_.alloc(mono_ws_bytes<real>(std::max<long>(std::max<long>(N_, E_), V_)));
        }
    }
    if (rec_obj_) objective();  // Obj[0]
    PFDR_HIP(hipStreamSynchronize(s));
    // c of the first conditioning: a_e = cw_ La_d1[e] in the edge sweeps
    PFDR_HIP(hipMemcpy(&cw_, &ctrl_.p->c, sizeof(real), hipMemcpyDeviceToHost));
    PFDR_HIP(hipMemcpy(hf, flags_.p, sizeof(hf), hipMemcpyDeviceToHost));
    if (E_) {
        PFDR_HIP(hipMemcpy(&la0_, La_d1_.p, sizeof(real), hipMemcpyDeviceToHost));
        la_uniform_ = hf[VF_D1_VARIES] == 0;
        la_uniform = la_uniform_ ? 1 : 0;
    }
    if (La_l1_.p) {
        PFDR_HIP(hipMemcpy(&l1u_, La_l1_.p, sizeof(real), hipMemcpyDeviceToHost));
        l1_uniform_ = hf[VF_L1_VARIES] == 0;
    }
    pins_.release();
    it_prev_ = 0;
}

// what the session's loop variant keeps beside the iterate: the per-edge
// endpoint copies of a padded session, the speculative iterate buffers, the
// formed ratios of the ratio edge sweep (cw_ and la0_ are known here)
template <typename real>
void QuadSession<real>::finish_values() {
    hipStream_t s = stream;
    refresh_ends();
    if (spec_)
        for (int k = 0; k + 1 < sd_; k++)
            PFDR_HIP(hipMemcpyAsync(xpx_[k].p, xp_.p, sizeof(R2<real>) * (Vg_ + 2),
                                    hipMemcpyDeviceToDevice, s));
    if (rat()) {  // (owned and ghost ends)
        if (!rr_.p) {
            rr_.alloc(Vg_ + 2);  // (+2: the tiled edge sweep stages vertex pairs)
            PFDR_HIP(hipMemsetAsync(rr_.p, 0, (Vg_ + 2) * sizeof(real), s));
        }
        k_ratio_vertex<real><<<grid_for(Vg_), kBlock, 0, s>>>(Vg_, cw_, la0_, Ga_.p, invAux_.p,
                                                              rr_.p);
        PFDR_HIP(hipGetLastError());
    } else {
        rr_.release();
    }
    edge_ratio = rr_.p ? 1 : 0;
    device_bytes += (int64_t)(rr_.n * sizeof(real)) - rr_counted_;
    rr_counted_ = (int64_t)(rr_.n * sizeof(real));
    xr_ = xw_ = xp_.p;
}

// pfdr_session_reload: the checks, all before any device work, then the
// constructor's own load
template <typename real>
void QuadSession<real>::reload(const pfdr_reload *r) {
    if (!reusable_)
        throw std::runtime_error("the session was not created reusable "
                                 "(pfdr_session_create_reusable)");
    if (halo_) throw std::runtime_error("a partitioned session cannot be reloaded");
    if (r->mem != PFDR_MEM_HOST && r->mem != PFDR_MEM_DEVICE)
        throw std::runtime_error("mem must be PFDR_MEM_HOST or PFDR_MEM_DEVICE");
    if (r->La_l1 && !has_l1_)
        throw std::runtime_error("La_l1 given, but the session was created without it");
    if (r->L && !hasL_)
        throw std::runtime_error("L given, but the session was created without it");
    if (flavour_ == 1 && !(r->min <= r->max))
        throw std::runtime_error("bounds: min > max or NaN");
    if (r->itMax > itMax0_)
        throw std::runtime_error("itMax above the one the session was created with (the "
                                 "records are sized by it)");
    const real rcd = (real)r->difRcd, tol = (real)r->difTol;
    if (tracked(rcd, tol) != track_)
        throw std::runtime_error("difTol / difRcd would switch the tracking of the iterate "
                                 "evolution, chosen at creation");
    if ((r->difRcd == 0.0) != rcd_zero_)
        throw std::runtime_error("difRcd cannot change between zero and non-zero");
    if ((rcd * rcd == real(0)) != rcd0_)
        throw std::runtime_error("difRcd would move the session to another loop variant "
                                 "(speculative or not), chosen at creation");
    hipStream_t s = stream;
    PFDR_HIP(hipStreamSynchronize(s));  // (no control-block copy in flight)
    it_prev_ = it_;
    itMax_ = r->itMax;
    set_params(r->rho, r->condMin, r->difRcd, r->difTol, r->min, r->max);
    drop_graphs();  // cw_ and la0_ are kernel arguments of the captured bodies
    if (capturable_) graphs_ok_ = itMax_ >= 2 * chunk_;
    load_values(Values{r->mem, r->X, r->Y, r->La_d1, r->La_l1, r->L});
    finish_values();
    device_bytes += stage_bytes() - staging_bytes;
    staging_bytes = stage_bytes();
    this->instantiate_setup_graph();
}

template <typename real>
void QuadSession<real>::plan_pad() {
    // up to kPadBlocks vertex blocks: at 1024 blocks (512^2 grid, f32) the
    // scattered contribution stores cost more than the round trips they save
    // (profiles/r2/r2zp_exp_pad.log, r2zq_exp_pad.log)
    if (halo_ || !E_ || nbv_ > kPadBlocks) return;
    hipStream_t s = stream;
    PinnedSmall pin(s);
    int *hm = static_cast<int *>(pin.p);
    DevBuf<int> dm(1);
    PFDR_HIP(hipMemsetAsync(dm.p, 0, sizeof(int), s));
    k_pad_nmax<<<grid_for(nbv_), kBlock, 0, s>>>(V_, nbv_, inc_.ptr.p, dm.p);
    PFDR_HIP(hipGetLastError());
    PFDR_HIP(hipMemcpyAsync(hm, dm.p, sizeof(int), hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
    const int nmax = std::max(kBlock, (*hm + kBlock - 1) / kBlock * kBlock);
    if (nmax > kPadPer * kBlock) return;
    sl_.alloc(2 * (size_t)E_);
    wzp_.alloc((size_t)nbv_ * nmax);
    PFDR_HIP(hipMemsetAsync(wzp_.p, 0, wzp_.n * sizeof(real), s));
    // f32 up to kEndsBlocks (f32 us/iter 11.2 -> 9.6 at 9 blocks, 11.5 ->
    // 10.5 at 256, 12.7 -> 12.2 at 507; f64 slower: 10.4 -> 11.0 at 9 blocks,
    // 12.5 -> 26 at 256; profiles/r2/r2zz_exp_ends.log, r2zz2)
    ends_ = sizeof(real) == 4 && nbv_ <= kEndsBlocks;
    if (ends_) {
        pidx_.alloc((size_t)nbv_ * nmax);
        PFDR_HIP(hipMemsetAsync(pidx_.p, 0, pidx_.n * sizeof(int), s));
        xpe_.alloc(2 * (size_t)E_);
        gie_.alloc(2 * (size_t)E_);
    }
    k_pad_slots<<<nbv_, kBlock, 0, s>>>(V_, E_, inc_.ptr.p, inc_.idx.p, nmax, sl_.p,
                                        ends_ ? pidx_.p : nullptr);
    PFDR_HIP(hipGetLastError());
    pad_nmax_ = nmax;
    pad_ = true;
    padded = 1;  // (finish_values fills the endpoint copies)
}

template <typename real>
void QuadSession<real>::refresh_ends() {
    if (!ends_) return;
    k_pad_ends<real><<<grid_for(E_), kBlock, 0, stream>>>(E_, Eu_.p, Ev_.p, xp_.p, gi_.p, xpe_.p,
                                                          gie_.p);
    PFDR_HIP(hipGetLastError());
}

// endpoints (local ids), partition plan, incidence CSR keyed by global edge id
template <typename real>
void QuadSession<real>::setup_graph(const pfdr_problem *p) {
    hipStream_t s = stream;
    const size_t E = E_;
    const auto kind = p->mem == PFDR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    Eu_.alloc(E ? E : 1);
    Ev_.alloc(E ? E : 1);
    DevBuf<unsigned> eg;
    const unsigned *eg_ptr = nullptr;  // original edge ids of a relabelled graph
    long e_offset = 0;
    if (p->nranks > 1 || p->comm) {
        partition_setup(p, V_, E_, halo_, Eu_, Ev_, eg, &e_offset, s);
        Vg_ = V_ + halo_->G;
        ghosts = halo_->G;
    } else {
        Vg_ = V_;
        if (E && kind == hipMemcpyHostToDevice) {
            pins_.copy(Eu_.p, p->Eu, E * 4, kind);
            pins_.copy(Ev_.p, p->Ev, E * 4, kind);
        } else if (E) {
            PFDR_HIP(hipMemcpyAsync(Eu_.p, p->Eu, E * 4, kind, s));
            PFDR_HIP(hipMemcpyAsync(Ev_.p, p->Ev, E * 4, kind, s));
        }
    }
    check_endpoints(Eu_.p, Ev_.p, E_, Vg_, s);
    if (!halo_ && E_ && (mode_ == A_IDENT || mode_ == A_DIAG) && p->reorder != PFDR_REORDER_OFF &&
        (p->reorder == PFDR_REORDER_ON || labels_scattered(Eu_.p, Ev_.p, E_, V_, s)) &&
        bfs_order(Eu_.p, Ev_.p, E_, V_, order_, where_, s)) {
        // relabel the vertices and sort the edges by their new u end; the
        // incidence keys keep the original edge ids (summation order)
        reordered_ = true;
        reordered = 1;
        DevBuf<unsigned long long> k(E), ks(E);
        DevBuf<unsigned> v(E);
        eorig_.alloc(E);
        k_edge_order_keys<<<grid_for(E), kBlock, 0, s>>>(E_, Eu_.p, where_.p, k.p, v.p);
        PFDR_HIP(hipGetLastError());
        radix_sort_pairs_stable<unsigned long long>(k.p, ks.p, v.p, eorig_.p, (long)E, 64, s);
        DevBuf<int> nu(E), nv(E);
        emap_.alloc(E);
        k_edge_relabel<<<grid_for(E), kBlock, 0, s>>>(E_, eorig_.p, Eu_.p, Ev_.p, where_.p, nu.p,
                                                      nv.p, emap_.p);
        PFDR_HIP(hipGetLastError());
        PFDR_HIP(hipStreamSynchronize(s));
        std::swap(Eu_.p, nu.p);
        std::swap(Ev_.p, nv.p);
        eg_ptr = eorig_.p;
    }
    // tile order of large graphs (pfdr_layout.hpp); the incidence keys keep
    // the original edge ids (summation order)
    tiled_ = !tiny_ && E_ > 0 && (long)V_ > (long)kFuseBlocks * kBlock;
    if (tiled_) {
        tile_.order(E_, V_, Vg_, Eu_, Ev_, halo_ ? eg.p : eorig_.p, e_offset, eorig_, emap_,
                    halo_.get(), s);
        eg_ptr = eorig_.p;
        e_offset = 0;  // (a partitioned rank's keys are global ids now)
    }
    // contributions: local side-major [u ends | v ends] then the received tail
    const long R = halo_ ? halo_->R : 0;
    wz_.alloc(2 * E_ + R + kSlotGroup);  // (+kSlotGroup: tile_sum's whole groups)
    contribution_incidence(Eu_.p, Ev_.p, E_, V_, eg_ptr ? eg_ptr : eg.p, e_offset, halo_.get(),
                           inc_, s);
    eorig_.release();
    if (tiled_) {
        tile_.build(E_, V_, Eu_.p, Ev_.p, inc_, halo_.get(), sizeof(real), s);
        tiled_blocks = tile_.tiled_blocks;
        record_blocks = tile_.record_blocks;
        slot_patterns = tile_.slot_patterns;
        vertex_pair = tile_.vpair_cap;
    } else if (!tiny_) {
        split_.build(E_, V_, Eu_.p, inc_, GatherCap<real>::v / 2, s);
        split_blocks = split_.split_blocks;
        if (split_.uptr.p) ustaged = us_ ? 1 : 0;
    }
}

// R = Y - A X (direct mode), gated
template <typename real>
void QuadSession<real>::gemv_rows(int gate) {
    hipStream_t s = stream;
    ProfScope ps(prof, "gemv_rows", s);
    if (sparse_) {
        sp_.rows(xp_.p, Y_.p, R_.p, gate ? ctrl_.p : nullptr, gate, s);
        return;
    }
    if (exact_) {
        k_rows_seq<real><<<grid_for(N_), kBlock, 0, s>>>(N_, V_, A_.p, xp_.p, Y_.p, R_.p,
                                                        gate ? ctrl_.p : nullptr, gate);
        PFDR_HIP(hipGetLastError());
        return;
    }
    k_rows_partial<real><<<rows_nb_, kBlock, 0, s>>>(N_, V_, A_.p, xp_.p, rows_cpb_, Rpart_.p,
                                                    gate ? ctrl_.p : nullptr, gate);
    const Ctrl<real> *c = gate ? ctrl_.p : nullptr;
    if (!halo_) {
        k_rows_finish<real><<<grid_for(N_), kBlock, 0, s>>>(N_, rows_nb_, Rpart_.p, Y_.p, R_.p,
                                                           c, gate);
    } else {  // partial A X of this rank's columns, summed over the ranks
        k_rows_finish<real><<<grid_for(N_), kBlock, 0, s>>>(N_, rows_nb_, Rpart_.p, nullptr,
                                                           Rsum_.p, c, gate);
        halo_->tr->allreduce_sum(Rsum_.p, N_, dtype_of<real>(), s);
        k_rows_residual<real><<<grid_for(N_), kBlock, 0, s>>>(N_, Y_.p, Rsum_.p, R_.p, c, gate);
    }
    PFDR_HIP(hipGetLastError());
}

// forward step of the dense modes: P = 2X - Ga (A^t A X - A^t Y)
template <typename real>
void QuadSession<real>::forward_dense(int gate) {
    hipStream_t s = stream;
    ColArgs<real> ca{};
    ca.A = A_.p; ca.ncols = V_; ca.xp = xp_.p; ca.Ga = Ga_.p; ca.Y = Y_.p;
    ca.ctrl = gate ? ctrl_.p : nullptr;
    ca.gate = gate;
    if (mode_ == A_DIRECT) {
        // the residual is also what the objective needs
        gemv_rows(gate == GATE_NONE ? GATE_NONE : (rec_obj_ ? GATE_ACTIVE_OR_OBJ : GATE_ACTIVE));
        ca.len = N_; ca.w = R_.p;
        ProfScope ps(prof, "gemv_cols", s);
        col_product<EPI_FWD_DIRECT>(ca);
    } else {
        ca.w = full_x();
        ProfScope ps(prof, "symv", s);
        ata_product<EPI_FWD_ATA>(ca);
    }
    PFDR_HIP(hipGetLastError());
}

template <typename real>
const real *QuadSession<real>::full_x() {
    hipStream_t s = stream;
    k_x_extract<real><<<grid_for(V_), kBlock, 0, s>>>(V_, xp_.p, xfull_.p + v0_);
    PFDR_HIP(hipGetLastError());
    if (halo_) {  // all-gather of the owned blocks
        Transport &tr = *halo_->tr;
        const int n = tr.nranks;
        std::vector<const void *> sp(n, xfull_.p + v0_);
        std::vector<size_t> sb(n, (size_t)V_ * sizeof(real));
        std::vector<void *> rp(n);
        std::vector<size_t> rb(n);
        for (int q = 0; q < n; q++) {
            rp[q] = xfull_.p + halo_->off[q];
            rb[q] = (size_t)(halo_->off[q + 1] - halo_->off[q]) * sizeof(real);
        }
        tr.exchange(sp, sb, rp, rb, s);
    }
    return xfull_.p;
}

// (A^tA) w of the owned columns with epilogue EPI: block upper triangle when
// symv_ (one GPU, exactly symmetric matrix), else one wave per column
template <typename real>
template <int EPI>
void QuadSession<real>::ata_product(ColArgs<real> ca) {
    hipStream_t s = stream;
    ca.A = A_.p; ca.ncols = V_; ca.len = (int)Vglob_;
    if (exact_) {
        col_product<EPI>(ca);
    } else if (symv_) {
        const long nt = (long)snb_ * (snb_ + 1) / 2;
        k_symv_tiles<real><<<nt, kBlock, 0, s>>>(V_, A_.p, ca.w, spart_.p, ca.ctrl, ca.gate);
        k_symv_finish<real, EPI><<<(V_ + 63) / 64, kBlock, 0, s>>>(snb_, spart_.p, ca);
    } else {
        k_col_dot<real, EPI><<<grid_for((long)V_ * 64), kBlock, 0, s>>>(ca);
    }
    PFDR_HIP(hipGetLastError());
}

// column dots with epilogue EPI: sequential order (exact_) or one wave per column
template <typename real>
template <int EPI>
void QuadSession<real>::col_product(ColArgs<real> ca) {
    hipStream_t s = stream;
    if (sparse_) { sp_.template cols<EPI>(ca, s); return; }
    if (exact_)
        k_col_seq<real, EPI><<<grid_for(ca.ncols), kBlock, 0, s>>>(ca);
    else
        k_col_dot<real, EPI><<<grid_for((long)ca.ncols * 64), kBlock, 0, s>>>(ca);
    PFDR_HIP(hipGetLastError());
}

// symmetric products for V >= 4 T: one GPU, V a multiple of the 16-byte
// vector, A 16-byte aligned, and the caller's matrix exactly symmetric
// (k_sym_check, one pass at setup; a matrix that is not keeps the column
// dots, which read it as given)
template <typename real>
void QuadSession<real>::plan_symv(int known) {
    using S = SymT<real>;
    if (halo_ || exact_ || V_ < 4 * S::T) return;
    if (V_ % S::VW || ((uintptr_t)A_.p % 16)) return;
    hipStream_t s = stream;
    if (known >= 0) {  // (a lane: the first lane's verdict on the shared matrix)
        if (!known) return;
        symv_ = true;
        snb_ = (V_ + S::T - 1) / S::T;
        spart_.alloc((size_t)snb_ * V_);
        symv = 1;
        return;
    }
    DevBuf<int> flag(1);
    PFDR_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), s));
    const long n64 = (V_ + 63) / 64;
    k_sym_check<real><<<n64 * (n64 + 1) / 2, kBlock, 0, s>>>(V_, A_.p, flag.p);
    PFDR_HIP(hipGetLastError());
    int f = 1;
    PFDR_HIP(hipMemcpyAsync(&f, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    PFDR_HIP(hipStreamSynchronize(s));
    if (f) return;
    symv_ = true;
    snb_ = (V_ + S::T - 1) / S::T;
    spart_.alloc((size_t)snb_ * V_);
    symv = 1;
}

// gradient of the smooth part at the current X into grad_ (reconditioning)
template <typename real>
void QuadSession<real>::gradient() {
    hipStream_t s = stream;
    grad_.alloc(Vg_);
    if (mode_ == A_IDENT || mode_ == A_DIAG) {
        k_grad_vertex<real><<<grid_for(V_), kBlock, 0, s>>>(V_, mode_, A_.p, Y_.p, xp_.p, grad_.p);
    } else {
        ColArgs<real> ca{};
        ca.A = A_.p; ca.ncols = V_; ca.out = grad_.p; ca.Y = Y_.p;
        if (mode_ == A_DIRECT) {
            gemv_rows(GATE_NONE);
            ca.len = N_; ca.w = R_.p;
            col_product<EPI_GRAD_DIRECT>(ca);
        } else {
            ca.w = full_x();
            ata_product<EPI_GRAD_ATA>(ca);
        }
    }
    PFDR_HIP(hipGetLastError());
}

// amplitude scale c of the preconditioner (ref :124-154): the sum of |a| is
// sequential in global vertex order across the ranks (chain)
template <typename real>
void QuadSession<real>::amplitude(bool init) {
    hipStream_t s = stream;
    if (init && mode_ == A_DIRECT) {
        ColArgs<real> ca{};
        ca.A = A_.p; ca.ncols = V_; ca.len = N_; ca.w = Y_.p; ca.out = pre_.p; ca.div = diag_.p;
        const bool pon = prof.on;
        prof.on = pon || sparse_;  // (as the diagonal's product)
        {
            ProfScope ps(prof, "pinv_cols", s);
            col_product<EPI_DIV>(ca);
        }
        prof.on = pon;
    }
    k_amp<real><<<nbv_, kBlock, 0, s>>>(V_, init ? (mode_ == A_DIRECT ? 1 : 0) : 2, Y_.p, diag_.p,
                                        pre_.p, xp_.p, absval_.p, cnt_part_.p);
    PFDR_HIP(hipGetLastError());
    if (halo_ && lab_.p) {
        // relabelled partition: every rank holds the amplitudes of all
        // vertices at the caller's labels (one writer per position, so the
        // all-reduce adds zeros only) and sums them in that order
        Transport &tr = *halo_->tr;
        if (ampg_.n < (size_t)Vglob_) ampg_.alloc(Vglob_);
        PFDR_HIP(hipMemsetAsync(ampg_.p, 0, sizeof(real) * Vglob_, s));
        k_scatter<real><<<nbv_, kBlock, 0, s>>>(V_, absval_.p, lab_.p, ampg_.p);
        PFDR_HIP(hipGetLastError());
        tr.allreduce_sum(ampg_.p, (int)Vglob_, dtype_of<real>(), s);
        if (mono_ws_.n < mono_ws_bytes<real>(Vglob_)) mono_ws_.alloc(mono_ws_bytes<real>(Vglob_));
        mono_sum<real>(Vglob_, ampg_.p, nullptr, nbv_, cnt_part_.p, csum_.p, ccnt_.p, mono_ws_.p,
                       s);
        tr.allreduce_sum(ccnt_.p, 1, 2, s);
        k_set_c<real><<<1, 64, 0, s>>>(csum_.p, ccnt_.p, init ? 1 : 0, ctrl_.p);
        PFDR_HIP(hipGetLastError());
        return;
    }
    const bool seeded = halo_ && halo_->tr->rank > 0;
    if (halo_) halo_->tr->chain_recv(red_.p + 3, sizeof(real), s);
    const real *amp = absval_.p;
    if (reordered_) {  // the reference's sequential sum runs in the caller's labels
        k_gather<real><<<nbv_, kBlock, 0, s>>>(V_, absval_.p, where_.p, amp_orig_.p);
        amp = amp_orig_.p;
    }
    if (mono_ws_.n < mono_ws_bytes<real>(V_)) mono_ws_.alloc(mono_ws_bytes<real>(V_));
    mono_sum<real>(V_, amp, seeded ? red_.p + 3 : nullptr, nbv_, cnt_part_.p, csum_.p, ccnt_.p,
                   mono_ws_.p, s);
    PFDR_HIP(hipGetLastError());
    if (halo_) {
        Transport &tr = *halo_->tr;
        tr.chain_send(csum_.p, sizeof(real), s);
        tr.broadcast(csum_.p, sizeof(real), tr.nranks - 1, s);
        tr.allreduce_sum(ccnt_.p, 1, 2, s);
    }
    k_set_c<real><<<1, 64, 0, s>>>(csum_.p, ccnt_.p, init ? 1 : 0, ctrl_.p);
    PFDR_HIP(hipGetLastError());
}

// ref :57-268 (l1) / bounds :58-242
template <typename real>
void QuadSession<real>::precondition(bool init) {
    hipStream_t s = stream;
    const size_t V = V_;
    ProfScope ps(prof, init ? "precondition" : "recondition", s);
    amplitude(init);
    if (!init) {
        gradient();
        pull(xp_.p, sizeof(R2<real>));  // X at the ghosts
        pull(grad_.p, sizeof(real));
    }
    const bool first_recond = !init && !A1_.p;
    if (first_recond) A1_.alloc(E_ ? E_ : 1);  // a_e leave cw La_d1 for good
    if (E_) {
        k_d1_weights<real><<<nbe_, kBlock, 0, s>>>(E_, Eu_.p, Ev_.p, La_d1_.p, ctrl_.p, init ? 1 : 0,
                                                   condMin_, xp_.p, first_recond ? nullptr : A1_.p,
                                                   cw_, invAux_.p, A1_.p, wz_.p, Ga_.p, grad_.p,
                                                   Z2_.p, zs_);
        PFDR_HIP(hipGetLastError());
    }
    if (halo_) halo_->push(wz_.p, wz_.p + 2 * E_, sizeof(real), s);
    k_precond_vertex<real><<<nbv_, kBlock, 0, s>>>(V_, inc_.ptr.p, inc_.idx.p, wz_.p, diag_.p,
                                                   La_l1_.p, xp_.p, ctrl_.p, init ? 1 : 0, condMin_,
                                                   cap_, Ldiag_ ? L_.p : nullptr, Ga_.p,
                                                   invAux_.p, Th_l1_.p);
    PFDR_HIP(hipGetLastError());
    pull(Ga_.p, sizeof(real));
    pull(invAux_.p, sizeof(real));
    if (E_ && !init) {
        k_recond_edge<real><<<nbe_, kBlock, 0, s>>>(E_, Eu_.p, Ev_.p, A1_.p, invAux_.p, Ga_.p,
                                                    xp_.p, grad_.p, Z2_.p, zs_);
    }
    k_gi_pack<real><<<grid_for(Vg_), kBlock, 0, s>>>(Vg_, Ga_.p, invAux_.p, gi_.p);
    PFDR_HIP(hipGetLastError());
    if (!init && !rat() && rr_.p) {  // (A1 from the first reconditioning on)
        rr_.release();
        edge_ratio = 0;
    }
    if (!init) {
        // forward step with the new metric from the gradient taken before
        // reconditioning (ref :448-464)
        k_forward_grad<real><<<grid_for(V), kBlock, 0, s>>>(V_, Ga_.p, grad_.p, xp_.p);
        PFDR_HIP(hipGetLastError());
        grad_.release();
    }
}

// objective at the current iterate (ref :387-422), written at Obj[it]
template <typename real>
void QuadSession<real>::objective() {
    hipStream_t s = stream;
    const Ctrl<real> *c = ctrl_.p;
    if (seqobj_) {  // the three sums term by term, as the reference adds them
        real *tn = oterms_.p, *te = oterms_.p + ot_e_, *tv = oterms_.p + ot_v_;
        const bool direct = mode_ == A_DIRECT;
        const int nrow = direct ? N_ : 0;
        if (!direct) {  // (A^tA X) in the reference's order (exact_: k_col_seq)
            ColArgs<real> ca{};
            ca.out = pre_.p;
            ca.ctrl = c; ca.gate = GATE_OBJ;
            ca.w = full_x();
            ata_product<EPI_STORE>(ca);
        }
        const long nmax = std::max<long>(std::max<long>(nrow, E_), V_);
        k_obj_terms<real><<<grid_for(nmax), kBlock, 0, s>>>(
            nrow, E_, V_, R_.p, Eu_.p, Ev_.p, oemap(), xp_.p, La_d1_.p,
            flavour_ == 0 ? La_l1_.p : nullptr, tn, te, tv, c);
        PFDR_HIP(hipGetLastError());
        PFDR_HIP(hipMemsetAsync(red_.p, 0, 3 * sizeof(real), s));
        if (direct)
            mono_sum<real>(N_, tn, nullptr, 0, nullptr, red_.p, nullptr, ows_.p, s);
        else
            k_obj_data_seq<real><<<1, kBlock, 0, s>>>(V_, xp_.p, pre_.p, Y_.p, red_.p, c);
        if (E_) mono_sum<real>(E_, te, nullptr, 0, nullptr, red_.p + 2, nullptr, ows_.p, s);
        if (flavour_ == 0 && La_l1_.p)
            mono_sum<real>(V_, tv, nullptr, 0, nullptr, red_.p + 1, nullptr, ows_.p, s);
        k_obj_write<real><<<1, 64, 0, s>>>(red_.p, direct ? 1 : 0,
                                           flavour_ == 0 && La_l1_.p != nullptr, ctrl_.p, Obj_.p);
        PFDR_HIP(hipGetLastError());
        return;
    }
    const real *papp = nullptr;
    pull(xp_.p, sizeof(R2<real>));  // TV of boundary edges needs the ghosts' X
    if (mode_ == A_ATA) {
        ColArgs<real> ca{};
        ca.out = pre_.p;
        ca.ctrl = c; ca.gate = GATE_OBJ;
        ca.w = full_x();
        ata_product<EPI_STORE>(ca);
        papp = pre_.p;
    }
    k_obj_vertex<real><<<nbv_, kBlock, 0, s>>>(V_, mode_, xp_.p, A_.p, papp, Y_.p,
                                               flavour_ == 0 ? La_l1_.p : nullptr, opart_.p, nbv_, c);
    if (E_) k_obj_edge<real><<<nbe_, kBlock, 0, s>>>(E_, Eu_.p, Ev_.p, xp_.p, La_d1_.p, opart_.p + 2 * nbv_, c);
    // the residual is replicated on every rank: its norm counts once (rank 0)
    const int nbn = (halo_ && halo_->tr->rank != 0) ? 0 : nbn_;
    if (mode_ == A_DIRECT && nbn)
        k_obj_rsq<real><<<nbn, kBlock, 0, s>>>(N_, R_.p, opart_.p + 2 * nbv_ + nbe_, c);
    k_obj_reduce<real><<<1, kBlock, 0, s>>>(opart_.p, nbv_, E_ ? nbe_ : 0, nbn, mode_ == A_DIRECT,
                                            c, red_.p);
    if (halo_) halo_->tr->allreduce_sum(red_.p, 3, dtype_of<real>(), s);
    k_obj_write<real><<<1, 64, 0, s>>>(red_.p, mode_ == A_DIRECT,
                                       flavour_ == 0 && La_l1_.p != nullptr, ctrl_.p, Obj_.p);
    PFDR_HIP(hipGetLastError());
}

template <typename real>
void QuadSession<real>::edge_sweep(long ebeg, long eend, const Ctrl<real> *c, const char *name,
                                   long ebeg2, long eend2, const FuseDecide<real> *fd) {
    constexpr int EPT = Vec<real>::kPer16B;
    if (eend <= ebeg) { ebeg = ebeg2; eend = eend2; ebeg2 = eend2 = 0; }
    if (eend <= ebeg) return;
    hipStream_t s = stream;
    ProfScope ps(prof, name, s);
    ERange rg{ebeg, eend, ebeg2, eend2, grid_for(eend - ebeg, EPT)};
    const int nb = rg.nb0 + (eend2 > ebeg2 ? grid_for(eend2 - ebeg2, EPT) : 0);
    const int xm = xcd_fit(nb, xcd_e_), g = xcd_grid(nb, xm);
    const FuseDecide<real> f = fd ? *fd : FuseDecide<real>{};
    if (ends_ && fuse_) {  // the whole edge range (fused sessions sweep [0, E) in one launch)
        k_edge_sweep_ends<real><<<g, kBlock, 0, s>>>(E_, xpe_.p, gie_.p, Z2_.p, A1_.p, cw_,
                                                     la_it(), la0_, rho_, c, nb, xm, f, pad_out());
        return;
    }
    constexpr long EB = kBlock * EPT;  // edges per tiled edge-sweep block
    if (tiled_ && !fuse_ && rg.nb0 == nb && ebeg % EB == 0 && (eend % EB == 0 || eend == E_)) {
        // edge blocks [ebeg / EB, ...) of the tile order (a partitioned rank
        // sweeps its interior blocks and the rest in two launches)
        auto k = rr_.p ? k_edge_sweep_tl<real, true, true>
                 : (!la_it() && !A1_.p) ? k_edge_sweep_tl<real, true>
                                        : k_edge_sweep_tl<real, false>;
        k<<<g, kBlock, 0, s>>>(E_, V_, Eu_.p, tile_.luv.p, tile_.erec.p, Ev_.p, xr_, Z2_.p, A1_.p,
                               cw_, gi_.p, la_it(), la0_, zdirect() ? nullptr : wz_.p, rho_, c,
                               (int)(ebeg / EB), nb, xm, rr_.p);
        return;
    }
    if (tiled_) throw std::logic_error("tiled edge sweep: range not on edge blocks");
    if (us_ && split_.uptr.p) {
        auto k = fuse_ ? k_edge_sweep_us<real, true> : k_edge_sweep_us<real, false>;
        k<<<g, kBlock, 0, s>>>(E_, Eu_.p, Ev_.p, split_.uptr.p, xr_, Z2_.p, A1_.p, cw_, gi_.p,
                               la_it(), la0_, wz_.p, rho_, c, nb, xm, rg, f, pad_out());
    } else {
        auto k = fuse_ ? k_edge_sweep<real, true> : k_edge_sweep<real, false>;
        k<<<g, kBlock, 0, s>>>(E_, Eu_.p, Ev_.p, xr_, Z2_.p, A1_.p, cw_, gi_.p, la_it(), la0_,
                               wz_.p, rho_, c, nb, xm, rg, f, pad_out());
    }
}

template <typename real>
void QuadSession<real>::tiny_chunk(int n) {
    const bool gated = track_ || rec_obj_;
    TinyArgs<real> t{};
    t.E = E_; t.Eu = Eu_.p; t.Ev = Ev_.p; t.Z2 = Z2_.p; t.A1 = A1_.p; t.La_d1 = la_it();
    t.la0 = la0_; t.cw = cw_; t.rho = rho_; t.gi = gi_.p; t.wz = wz_.p;
    t.va = vargs(0, nbv_, nullptr);
    t.red = red_.p; t.ctrl = gated ? ctrl_.p : nullptr; t.Dif = rec_dif_ ? Dif_.p : nullptr;
    t.track = track_ ? 1 : 0; t.iters = n;
    ProfScope ps(prof, "tiny_iterate", stream);
    k_tiny_iterate<real><<<1, kTiny, 0, stream>>>(t);
    PFDR_HIP(hipGetLastError());
}

template <typename real>
VArgs<real> QuadSession<real>::vargs(int bbeg, int bend, const Ctrl<real> *c) {
    VArgs<real> a{};
    a.V = V_; a.ptr = inc_.ptr.p; a.idx = inc_.idx.p; a.xp = xr_; a.wz = wz_.p;
    a.xpo = xw_ == xr_ ? nullptr : xw_;
    a.uptr = split_.uptr.p; a.mask = split_.mask.p; a.oidx = split_.oidx.p;
    a.blkok = split_.blkok.p;
    a.Y = Y_.p; a.A = A_.p; a.Ga = Ga_.p; a.Th_l1 = Th_l1_.p;
    a.prox = prox_; a.positivity = positivity_; a.lo = lo_; a.hi = hi_;
    a.fwd = mode_ == A_IDENT ? 1 : (mode_ == A_DIAG ? 2 : 0);
    a.track = track_ ? 1 : 0; a.part = vpart_.p; a.ctrl = c;
    a.late = fuse_ ? 1 : 0;
    a.E = E_;
    if (tiled_) {
        const TileLayout &t = tile_;
        a.slots = t.slots.p; a.trec = t.trec.p; a.ptab = t.ptab.p; a.prec = t.prec.p;
        a.deg8 = t.deg8.p; a.ustart = t.ustart.p; a.tptr = t.tptr.p; a.tstart = t.tstart.p;
        a.tlen = t.tlen.p; a.tok = t.tok.p;
        a.zs = Z2_.p; a.invAux = invAux_.p; a.a0 = cw_ * la0_;
        a.gi = gi_.p;  // (Ga, 1/Aux) in one load
    }
    a.l1uni = l1_uniform_ ? 1 : 0;
    a.l1u = l1u_;
    a.terms = seqdif_ ? terms_.p : nullptr;
    a.tmap = seqdif_ && reordered_ ? order_.p : nullptr;
    a.tstride = tstride_;
    a.bbeg = bbeg; a.nb = bend - bbeg; a.xcd = xcd_fit(a.nb, xcd_v_);
    a.bsplit = a.nb; a.bjump = 0;
    return a;
}

template <typename real>
void QuadSession<real>::vertex_sweep(int bbeg, int bend, const Ctrl<real> *c, const char *name,
                                     int bbeg2, int bend2) {
    if (bend <= bbeg) { bbeg = bbeg2; bend = bend2; bbeg2 = bend2 = 0; }
    if (bend <= bbeg) return;
    hipStream_t s = stream;
    VArgs<real> a = vargs(bbeg, bend, c);
    if (bend2 > bbeg2) {  // second range: logical blocks past the first jump to it
        a.bsplit = bend - bbeg;
        a.bjump = bbeg2 - bend;
        a.nb += bend2 - bbeg2;
        a.xcd = xcd_fit(a.nb, xcd_v_);
    }
    ProfScope ps(prof, name, s);
    if (pad_ && bend2 <= bbeg2) {
        k_vertex_sweep_pad<real><<<xcd_grid(a.nb, a.xcd), kBlock, 0, s>>>(
            a, wzp_.p, pad_nmax_, ends_ ? pidx_.p : nullptr, ends_ ? xpe_.p : nullptr);
        return;
    }
    if (tile_.vpair_cap && bend2 <= bbeg2 && a.nb >= 2) {  // pairs of record blocks, one range
        const int np = a.nb / 2;
        const size_t lb = 2 * (size_t)tile_.vpair_cap * sizeof(real);
        if (a.nb & 1) {  // the odd last block first, on its own
            VArgs<real> a1 = a;
            a1.bbeg = a.bbeg + a.nb - 1;
            a1.nb = 1;
            a1.bsplit = 1;
            a1.xcd = 0;
            if (zdirect()) k_vertex_sweep<real, 8, true><<<1, kBlock, 0, s>>>(a1);
            else k_vertex_sweep<real, 8><<<1, kBlock, 0, s>>>(a1);
        }
        a.xcd = xcd_fit(np, xcd_v_);
        const int g = xcd_grid(np, a.xcd);
        if (zdirect()) k_vertex_sweep_pair<real, true><<<g, kBlock, lb, s>>>(a, tile_.vpair_cap);
        else k_vertex_sweep_pair<real><<<g, kBlock, lb, s>>>(a, tile_.vpair_cap);
        return;
    }
    if (zdirect())
        k_vertex_sweep<real, 8, true><<<xcd_grid(a.nb, a.xcd), kBlock, 0, s>>>(a);
    else
        k_vertex_sweep<real, 8><<<xcd_grid(a.nb, a.xcd), kBlock, 0, s>>>(a);
}

// the sweeps of one iteration: (partitions) the ghosts' (X, P) pulled into
// the buffer the edge sweep reads (xr_), the edge sweep, the ghost ends'
// contributions pushed to their owners, the vertex sweep (into xw_)
template <typename real>
void QuadSession<real>::sweeps(const Ctrl<real> *c) {
    hipStream_t s = stream;
    if (overlap_) {
        // pull ghosts (comm) || interior edges; boundary edges; push (comm)
        // || interior vertices; boundary vertices
        PFDR_HIP(hipEventRecord(ev_[0], s));
        PFDR_HIP(hipStreamWaitEvent(comm_, ev_[0], 0));
        {
            ProfScope ps(prof, "halo_pull", comm_);
            halo_->pull(xr_, sizeof(R2<real>), comm_);
        }
        PFDR_HIP(hipEventRecord(ev_[1], comm_));
        edge_sweep(elo_, ehi_, c, "edge_sweep");
        PFDR_HIP(hipStreamWaitEvent(s, ev_[1], 0));
        edge_sweep(0, elo_, c, "edge_sweep_b", ehi_, E_);  // both boundary ranges, one launch
        PFDR_HIP(hipEventRecord(ev_[2], s));
        PFDR_HIP(hipStreamWaitEvent(comm_, ev_[2], 0));
        {
            ProfScope ps(prof, "halo_push", comm_);
            real *src = zdirect() ? Z2_.p : wz_.p;  // Z-direct ranks push Z
            halo_->push(src, src + 2 * E_, sizeof(real), comm_);
        }
        PFDR_HIP(hipEventRecord(ev_[3], comm_));
        vertex_sweep(blo_, bhi_, c, "vertex_sweep");
        PFDR_HIP(hipStreamWaitEvent(s, ev_[3], 0));
        vertex_sweep(0, blo_, c, "vertex_sweep_b", bhi_, nbv_);
    } else {
        if (halo_) {
            ProfScope ps(prof, "halo_pull", s);
            halo_->pull(xr_, sizeof(R2<real>), s);
        }
        edge_sweep(0, E_, c, "edge_sweep");
        if (halo_) {
            ProfScope ps(prof, "halo_push", s);
            real *src = zdirect() ? Z2_.p : wz_.p;  // Z-direct ranks push Z
            halo_->push(src, src + 2 * E_, sizeof(real), s);
        }
        vertex_sweep(0, nbv_, c, "vertex_sweep");
    }
}

// the sweeps of speculative iteration t, on its buffers (b = t mod D)
template <typename real>
void QuadSession<real>::spec_sweeps(int t, int b) {
    xr_ = xpb(t - 1);
    xw_ = xpb(t);
    real *const keep = terms_.p, *const keepp = vpart_.p;
    terms_.p += (long)b * 2 * tstride_;  // vargs() hands the sweep this iteration's terms
    vpart_.p += (long)b * 2 * nbv_;
    sweeps(ctrl_.p);
    terms_.p = keep;
    vpart_.p = keepp;
    xr_ = xw_ = xp_.p;
}

template <typename real>
void QuadSession<real>::spec_decide(int b, hipStream_t s) {
    seq_evolution(terms_.p + (long)b * 2 * tstride_, vpart_.p + (long)b * 2 * nbv_, s);
    k_decide<real><<<1, 64, 0, s>>>(ctrl_.p, red_.p, rec_dif_ ? Dif_.p : nullptr, 1);
}

template <typename real>
void QuadSession<real>::body(int i, int n) {
    hipStream_t s = stream;
    const bool gated = track_ || rec_obj_;
    if (fuse_) {
        // E(i) decides iteration i - 1 (from cb[(i-1)&1] into cb[i&1]), V(i)
        // reads cb[i&1]; the last body closes the chunk with k_reduce_decide's
        // arithmetic, its decision into ctrl_
        Ctrl<real> *cb[2] = {ctrl_.p, ctrl2_.p};
        FuseDecide<real> fd{};
        if (i > 0) {
            fd.src = cb[(i - 1) & 1]; fd.dst = cb[i & 1]; fd.part = vpart_.p;
            fd.red = red_.p; fd.Dif = rec_dif_ ? Dif_.p : nullptr; fd.nparts = nbv_;
        }
        edge_sweep(0, E_, cb[0], "edge_sweep", 0, 0, &fd);
        vertex_sweep(0, nbv_, cb[i & 1], "vertex_sweep");
        if (i == n - 1) {
            FuseDecide<real> fl{cb[i & 1], cb[0], vpart_.p, red_.p, rec_dif_ ? Dif_.p : nullptr,
                                nbv_};
            k_decide_fused<real><<<1, kBlock, 0, s>>>(fl);
        }
        PFDR_HIP(hipGetLastError());
        return;
    }
    head();
    if (mode_ == A_DIRECT || mode_ == A_ATA) forward_dense(gated ? GATE_ACTIVE : GATE_NONE);
    if (rec_obj_) objective();
}

template <typename real>
void QuadSession<real>::lane_settle(int n) {
    const bool g = gated();
    if (g) {
        it_ = hctrl_->it;
    } else {
        it_ += n;
        if (it_ >= itMax_) stopped_ = true;
    }
    if (g && hctrl_->stop) {
        stopped_ = true;
    } else if (g && hctrl_->recond) {
        recondition();
        reconditionings++;
        hctrl_->recond = 0;
        hctrl_->halt = 0;
        push_ctrl();
        if (verbose_) { printf("done.\n"); fflush(stdout); }
    }
    if (verbose_ && (it_ >= next_print_ || stopped_)) {
        print_progress();
        next_print_ = it_ + verbose_;
    }
}

// the sweeps of one iteration and the loop decision on it (every variant but
// the fused one, whose decision rides in the next edge sweep)
template <typename real>
void QuadSession<real>::head() {
    hipStream_t s = stream;
    const bool gated = track_ || rec_obj_;
    const Ctrl<real> *c = gated ? ctrl_.p : nullptr;
    sweeps(c);
    if (seqdif_) {
        // the reference's two sequential sums (ref :518-526), then its decision
        ProfScope ps(prof, "seq_evolution", s);
        seq_evolution(terms_.p, vpart_.p, s);
        k_decide<real><<<1, 64, 0, s>>>(ctrl_.p, red_.p, rec_dif_ ? Dif_.p : nullptr, 1);
    } else if (gated && !halo_) {
        k_reduce_decide<real><<<1, kBlock, 0, s>>>(nbv_, vpart_.p, red_.p, ctrl_.p,
                                                   rec_dif_ ? Dif_.p : nullptr, track_ ? 1 : 0);
    } else if (gated) {  // the partial sums are all-reduced before the decision
        if (track_) {
            k_reduce_pairs<real><<<1, kBlock, 0, s>>>(nbv_, vpart_.p, red_.p, 1);
            halo_->tr->allreduce_sum(red_.p, 2, dtype_of<real>(), s);
        }
        k_decide<real><<<1, 64, 0, s>>>(ctrl_.p, red_.p, rec_dif_ ? Dif_.p : nullptr, track_ ? 1 : 0);
    }
    PFDR_HIP(hipGetLastError());
}

// red_[0..2) = the sums of (X_ - X)^2 and X^2 over every vertex in the
// caller's order, rounded as the reference's one-thread loop.  part: the
// vertex sweep's per-block sums of the same terms (their binades predicted
// from them when the terms lie in vertex order)
template <typename real>
void QuadSession<real>::seq_evolution(real *terms, const real *part, hipStream_t s) {
    evolution_sum(terms, V_, 2, tstride_, reordered_ ? nullptr : part, nbv_, s);
}

// interior edge range and vertex-block range of a partitioned session (the
// longest runs without ghost endpoints / received contributions); edges
// outside [elo_, ehi_) and blocks outside [blo_, bhi_) wait for the halo
template <typename real>
void QuadSession<real>::plan_overlap() {
    hipStream_t s = stream;
    constexpr int EPT = Vec<real>::kPer16B;
    // edges: a ghost endpoint (u is always owned; v may be a ghost)
    std::vector<int> hv(E_);
    if (E_) PFDR_HIP(hipMemcpy(hv.data(), Ev_.p, E_ * 4, hipMemcpyDeviceToHost));
    long best0 = 0, best1 = 0;
    for (long e = 0; e < E_;) {
        if (hv[e] >= V_) { e++; continue; }
        long f = e;
        while (f < E_ && hv[f] < V_) f++;
        if (f - e > best1 - best0) { best0 = e; best1 = f; }
        e = f;
    }
    // both cuts on the lane width: every launch starts vector-aligned
    elo_ = ((best0 + EPT - 1) / EPT) * EPT;
    ehi_ = std::max(elo_, (best1 / EPT) * EPT);
    if (tiled_) {  // tile order: the interior edges come first, cut on whole edge blocks
        constexpr long EB = kBlock * EPT;
        elo_ = 0;
        ehi_ = (tile_.Eint / EB) * EB;
    }
    // vertex blocks: any CSR entry from the received tail
    std::vector<int> ptr(V_ + 1);
    std::vector<unsigned> idx(inc_.n);
    PFDR_HIP(hipMemcpy(ptr.data(), inc_.ptr.p, (V_ + 1) * 4, hipMemcpyDeviceToHost));
    if (inc_.n) PFDR_HIP(hipMemcpy(idx.data(), inc_.idx.p, inc_.n * 4, hipMemcpyDeviceToHost));
    int b0 = 0, b1 = 0;
    for (int b = 0; b < nbv_;) {
        auto tailblk = [&](int q) {
            const int v0 = q * kBlock, v1 = std::min(V_, v0 + kBlock);
            for (int j = ptr[v0]; j < ptr[v1]; j++)
                if (idx[j] >= (unsigned)(2 * E_)) return true;
            return false;
        };
        if (tailblk(b)) { b++; continue; }
        int f = b;
        while (f < nbv_ && !tailblk(f)) f++;
        if (f - b > b1 - b0) { b0 = b; b1 = f; }
        b = f;
    }
    blo_ = b0;
    bhi_ = b1;
    PFDR_HIP(hipStreamCreateWithFlags(&comm_, hipStreamNonBlocking));
    for (hipEvent_t &e : ev_) PFDR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    overlap_ = true;
    interior_edges = ehi_ - elo_;
    (void)s;
}

// rank 0 of a partition reports
template <typename real>
void QuadSession<real>::print_progress() {
    hctrl_->it = it_;  // (an ungated run: the mirror is not read back)
    if (halo_ && halo_->tr->rank != 0) return;
    printf("iteration %d (max. %d)\n", it_, itMax_);
    if (track_) {
        printf("iterate evolution %g (recond. %g; tol. %g)\n", (double)hctrl_->dif,
               (double)hctrl_->difRcd, (double)hctrl_->difTol);
    }
    fflush(stdout);
}

template <typename real>
void QuadSession<real>::recondition() {
    if (verbose_) { print_progress(); printf("Reconditioning... "); fflush(stdout); }
    precondition(false);
    refresh_ends();  // (X, P) and (Ga, 1/Aux) rewritten
    drop_graphs();  // A1_ now holds the splitting weights' factors
    difRcd2_ *= real(0.01);  // ref :458
    hctrl_->difRcd = difRcd2_;
}

template <typename real>
void *QuadSession<real>::device_x() {
    if (xout_.n < (size_t)V_) xout_.alloc(V_);
    if (reordered_)
        k_x_extract_perm<real><<<grid_for(V_), kBlock, 0, stream>>>(V_, xpb(it_), where_.p,
                                                                    xout_.p);
    else
        k_x_extract<real><<<grid_for(V_), kBlock, 0, stream>>>(V_, xpb(it_), xout_.p);
    PFDR_HIP(hipGetLastError());
    PFDR_HIP(hipStreamSynchronize(stream));
    return xout_.p;
}

template <typename real>
void QuadSession<real>::result(void *X_host, int *it, void *Obj_host, void *Dif_host) {
    hipStream_t s = stream;
    HostPins hp(s);
    if (X_host) {
        void *dx = device_x();
        hp.copy(X_host, dx, sizeof(real) * V_, hipMemcpyDeviceToHost);
    }
    this->download_records(it, Obj_host, Dif_host, Obj_.p, Dif_.p, hp);
    hp.release();
    PFDR_HIP(hipStreamSynchronize(s));
}

SessionBase *create_quadratic_session(const pfdr_problem *p) {
    if (p->dtype == PFDR_F32) return new QuadSession<float>(p);
    if (p->dtype == PFDR_F64) return new QuadSession<double>(p);
    throw std::runtime_error("dtype must be PFDR_F32 or PFDR_F64");
}

// pfdr_session_create_reusable: A null for a dense (or no) matrix
SessionBase *create_quadratic_session_reusable(const pfdr_problem *p, const pfdr_csc *A) {
    if (p->dtype == PFDR_F32) return new QuadSession<float>(p, A, true);
    if (p->dtype == PFDR_F64) return new QuadSession<double>(p, A, true);
    throw std::runtime_error("dtype must be PFDR_F32 or PFDR_F64");
}

// a lane of a batch: a reusable session on the batch's matrix
template <typename real>
DenseLane<real> *create_quadratic_lane(const pfdr_problem *p, const LaneShare<real> &share) {
    return new QuadSession<real>(p, nullptr, true, &share);
}
template DenseLane<float> *create_quadratic_lane<float>(const pfdr_problem *,
                                                        const LaneShare<float> &);
template DenseLane<double> *create_quadratic_lane<double>(const pfdr_problem *,
                                                          const LaneShare<double> &);

SessionBase *create_quadratic_session_sparse(const pfdr_problem *p, const pfdr_csc *A) {
    if (!A) throw std::runtime_error("sparse A: null matrix");
    if (p->dtype == PFDR_F32) return new QuadSession<float>(p, A);
    if (p->dtype == PFDR_F64) return new QuadSession<double>(p, A);
    throw std::runtime_error("dtype must be PFDR_F32 or PFDR_F64");
}

// ------------------------------------------------ drop-in entry points --
template <typename real>
static int quadratic_host(const char *fn, int kind, int V, int E, int N, real *X,
                          const real *Y, const real *A, const int *Eu,
                          const int *Ev, const real *La_d1, const real *La_l1,
                          int positivity, real mn, real mx, int Ltype,
                          const real *L, real rho, real condMin, real difRcd,
                          real difTol, int itMax, int *it, real *Obj,
                          real *Dif, int verbose, const pfdr_csc *csc = nullptr) {
    pfdr_problem p{};
    p.kind = kind;
    p.dtype = dtype_of<real>();
    p.mem = PFDR_MEM_HOST;
    p.V = V; p.E = E; p.N = N;
    p.X = X; p.Y = Y; p.A = A; p.Eu = Eu; p.Ev = Ev;
    p.La_d1 = La_d1; p.La_l1 = La_l1; p.positivity = positivity;
    p.min = mn; p.max = mx; p.Ltype = Ltype; p.L = L;
    p.rho = rho; p.condMin = condMin; p.difRcd = difRcd; p.difTol = difTol;
    p.itMax = itMax; p.verbose = verbose;
    return solve_one_call<QuadSession<real>>(fn, p, X, it, Obj, Dif, N, 1, !csc, csc);
}

}  // namespace pfdr

using pfdr::quadratic_host;

extern "C" int pfdr_quadratic_d1_l1_f32(int V, int E, int N, float *X,
    const float *Y, const float *A, const int *Eu, const int *Ev,
    const float *La_d1, const float *La_l1, int positivity, int Ltype,
    const float *L, float rho, float condMin, float difRcd, float difTol,
    int itMax, int *it, float *Obj, float *Dif, int verbose) {
    return quadratic_host<float>("pfdr_quadratic_d1_l1_f32", PFDR_KIND_L1, V, E, N, X, Y, A, Eu,
                                 Ev, La_d1, La_l1, positivity, 0.f, 0.f, Ltype, L, rho, condMin,
                                 difRcd, difTol, itMax, it, Obj, Dif, verbose);
}
extern "C" int pfdr_quadratic_d1_l1_f64(int V, int E, int N, double *X,
    const double *Y, const double *A, const int *Eu, const int *Ev,
    const double *La_d1, const double *La_l1, int positivity, int Ltype,
    const double *L, double rho, double condMin, double difRcd,
    double difTol, int itMax, int *it, double *Obj, double *Dif,
    int verbose) {
    return quadratic_host<double>("pfdr_quadratic_d1_l1_f64", PFDR_KIND_L1, V, E, N, X, Y, A, Eu,
                                  Ev, La_d1, La_l1, positivity, 0.0, 0.0, Ltype, L, rho, condMin,
                                  difRcd, difTol, itMax, it, Obj, Dif, verbose);
}
extern "C" int pfdr_quadratic_d1_bounds_f32(int V, int E, int N, float *X,
    const float *Y, const float *A, const int *Eu, const int *Ev,
    const float *La_d1, float min, float max, int Ltype, const float *L,
    float rho, float condMin, float difRcd, float difTol, int itMax,
    int *it, float *Obj, float *Dif, int verbose) {
    return quadratic_host<float>("pfdr_quadratic_d1_bounds_f32", PFDR_KIND_BOUNDS, V, E, N, X, Y,
                                 A, Eu, Ev, La_d1, nullptr, 0, min, max, Ltype, L, rho, condMin,
                                 difRcd, difTol, itMax, it, Obj, Dif, verbose);
}
extern "C" int pfdr_quadratic_d1_bounds_f64(int V, int E, int N, double *X,
    const double *Y, const double *A, const int *Eu, const int *Ev,
    const double *La_d1, double min, double max, int Ltype, const double *L,
    double rho, double condMin, double difRcd, double difTol, int itMax,
    int *it, double *Obj, double *Dif, int verbose) {
    return quadratic_host<double>("pfdr_quadratic_d1_bounds_f64", PFDR_KIND_BOUNDS, V, E, N, X, Y,
                                  A, Eu, Ev, La_d1, nullptr, 0, min, max, Ltype, L, rho, condMin,
                                  difRcd, difTol, itMax, it, Obj, Dif, verbose);
}

// sparse A (CSC) in place of the dense matrix: pfdr_mi355x.h, "sparse A"
extern "C" int pfdr_quadratic_d1_l1_csc_f32(int V, int E, int N, float *X, const float *Y,
    int64_t nnz, const int64_t *colptr, const int32_t *rowidx, const float *val,
    const int *Eu, const int *Ev, const float *La_d1, const float *La_l1,
    int positivity, int Ltype, const float *L, float rho, float condMin,
    float difRcd, float difTol, int itMax, int *it, float *Obj, float *Dif,
    int verbose) {
    const pfdr_csc A{nnz, colptr, rowidx, val};
    return quadratic_host<float>("pfdr_quadratic_d1_l1_csc_f32", PFDR_KIND_L1, V, E, N, X, Y,
                                 nullptr, Eu, Ev, La_d1, La_l1, positivity, 0.f, 0.f, Ltype, L,
                                 rho, condMin, difRcd, difTol, itMax, it, Obj, Dif, verbose, &A);
}
extern "C" int pfdr_quadratic_d1_l1_csc_f64(int V, int E, int N, double *X, const double *Y,
    int64_t nnz, const int64_t *colptr, const int32_t *rowidx, const double *val,
    const int *Eu, const int *Ev, const double *La_d1, const double *La_l1,
    int positivity, int Ltype, const double *L, double rho, double condMin,
    double difRcd, double difTol, int itMax, int *it, double *Obj, double *Dif,
    int verbose) {
    const pfdr_csc A{nnz, colptr, rowidx, val};
    return quadratic_host<double>("pfdr_quadratic_d1_l1_csc_f64", PFDR_KIND_L1, V, E, N, X, Y,
                                  nullptr, Eu, Ev, La_d1, La_l1, positivity, 0.0, 0.0, Ltype, L,
                                  rho, condMin, difRcd, difTol, itMax, it, Obj, Dif, verbose, &A);
}
extern "C" int pfdr_quadratic_d1_bounds_csc_f32(int V, int E, int N, float *X, const float *Y,
    int64_t nnz, const int64_t *colptr, const int32_t *rowidx, const float *val,
    const int *Eu, const int *Ev, const float *La_d1, float min, float max,
    int Ltype, const float *L, float rho, float condMin, float difRcd,
    float difTol, int itMax, int *it, float *Obj, float *Dif, int verbose) {
    const pfdr_csc A{nnz, colptr, rowidx, val};
    return quadratic_host<float>("pfdr_quadratic_d1_bounds_csc_f32", PFDR_KIND_BOUNDS, V, E, N, X,
                                 Y, nullptr, Eu, Ev, La_d1, nullptr, 0, min, max, Ltype, L, rho,
                                 condMin, difRcd, difTol, itMax, it, Obj, Dif, verbose, &A);
}
extern "C" int pfdr_quadratic_d1_bounds_csc_f64(int V, int E, int N, double *X, const double *Y,
    int64_t nnz, const int64_t *colptr, const int32_t *rowidx, const double *val,
    const int *Eu, const int *Ev, const double *La_d1, double min, double max,
    int Ltype, const double *L, double rho, double condMin, double difRcd,
    double difTol, int itMax, int *it, double *Obj, double *Dif, int verbose) {
    const pfdr_csc A{nnz, colptr, rowidx, val};
    return quadratic_host<double>("pfdr_quadratic_d1_bounds_csc_f64", PFDR_KIND_BOUNDS, V, E, N,
                                  X, Y, nullptr, Eu, Ev, La_d1, nullptr, 0, min, max, Ltype, L,
                                  rho, condMin, difRcd, difTol, itMax, it, Obj, Dif, verbose, &A);
}
