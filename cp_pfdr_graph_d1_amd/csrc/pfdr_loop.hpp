// The host side of a device-controlled PFDR loop, shared by the quadratic and
// simplex sessions: control block and its pinned mirror, chunks of iterations
// replayed as hipGraphs, the pipelined gated run, the speculative iteration's
// streams and events, the sequential evolution sum, and the frame of the
// one-call entries.  A session supplies what a body launches, what a
// reconditioning does, the progress line and the buffers a speculative
// iteration cycles through (the hooks below: one virtual call per body or per
// chunk, on the host).
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>

#include "pfdr_halo.hpp"
#include "pfdr_session.hpp"

namespace pfdr {

template <typename real>
class IterLoop : public SessionBase {
  public:
    ~IterLoop() override { close(); }
    int run(int iters) final;
    void prepare(int iters) final;

  protected:
    // ------------------------------------------------------------ hooks --
    virtual void body(int i, int n) = 0;  // i-th of n bodies of a chunk (not speculative)
    virtual void tiny_chunk(int n) = 0;   // n iterations in one workgroup launch (tiny_)
    // speculative iteration t: select its buffers (b = t mod D) and sweep on
    // `stream`; then its evolution sum and decision on s
    virtual void spec_sweeps(int t, int b) = 0;
    virtual void spec_decide(int b, hipStream_t s) = 0;
    // a reconditioning request was read into hctrl_: announce it (verbose_),
    // recondition, drop the graphs, set hctrl_->difRcd (the loop clears the
    // request, uploads the block and closes the line with "done.")
    virtual void recondition() = 0;
    virtual void print_progress() = 0;
    virtual bool gated() const = 0;  // the device decides when to stop

    // ------------------------------------------------------------ state --
    std::unique_ptr<Halo> halo_;  // partition plan (null on one GPU)
    // the transport of the evolution sums: a speculative partition's own
    // (Transport::split), so they run beside the next iteration's exchanges
    std::unique_ptr<Transport> evtr_;
    Transport &etr() { return evtr_ ? *evtr_ : *halo_->tr; }
    DevBuf<Ctrl<real>> ctrl_;
    Ctrl<real> *hctrl_ = nullptr;  // pinned mirror
    // run_pipelined: the control block's snapshots after two chunks in flight
    Ctrl<real> *snap_[2] = {};
    hipEvent_t snapev_[2] = {};
    int itMax_ = 0, verbose_ = 0;
    int it_ = 0;
    int it0_ = 0;  // completed iterations when the captured / launched bodies start
    bool stopped_ = false;
    int chunk_ = 32;
    int next_print_ = 0;
    bool tiny_ = false;  // small graph: a chunk of iterations in one workgroup launch
    // hipGraph of a chunk of iterations (unprofiled): a replayed kernel
    // boundary costs ~1.6 us of GPU time, a launched one ~2.8 us
    // (profiles/r2/r2d_launch_gap.log) -- a large share of an iteration of a
    // small graph, and cut pursuit's reduced problems are otherwise bound by
    // the host's launches.  Re-captured after a reconditioning (new kernel
    // arguments).
    bool graphs_ok_ = false;
    bool capturable_ = false;  // prepare(): graphs of any run length on request
    std::map<int, hipGraphExec_t> graphs_;
    // Speculative iteration (sequential evolution, no reconditioning, no
    // objective record): the evolution sum and the decision on iteration t
    // run on a second stream (evs_) while iterations t + 1 ... t + D - 1
    // sweep; iteration t + D waits for that decision (depth D = sd_: 2; 4 on
    // a partition of three or more ranks, whose rank-to-rank evolution chain,
    // run over evtr_ beside the halo exchanges, takes several of a rank's
    // iterations).  The iterate and the terms cycle through D buffers, so
    // when the decision on t stops the loop the iterate of t is intact and
    // the speculative iterations after it are simply discarded: iterate,
    // iteration count and Dif are the sequential loop's, bit for bit.
    static constexpr int kSpecMax = 4;
    bool spec_ = false;
    int sd_ = 2;
    hipStream_t evs_ = nullptr;  // the decisions' stream (null: PFDR_SPEC_SERIAL, the session's)
    hipEvent_t evv_[kSpecMax] = {}, evd_[kSpecMax] = {};
    // evolution sums with the reference's sequential rounding
    // (PFDR_EVOLUTION_*, include/pfdr_mi355x.h): one GPU sums with mono_sum
    // (scratch dws_); a partition sums rank to rank (ChainSum); a relabelled
    // partition first routes every vertex's terms to the rank whose
    // caller-order slice holds its label (TermRoute), then chains
    bool seqdif_ = false;
    ChainSum<real> chain_;
    TermRoute<real> route_;
    DevBuf<char> dws_;
    DevBuf<real> red_;  // the sums (all-reduced scalars on a partition)

    // ------------------------------------------------------------ setup --
    // the zeroed pinned mirror with obj_it and itMax set; the session fills
    // in dif, difTol, difRcd and eps, then push_ctrl()
    Ctrl<real> *alloc_ctrl() {
        ctrl_.alloc(1);
        static_assert(sizeof(Ctrl<real>) <= kPinnedSmall, "control block");
        hctrl_ = static_cast<Ctrl<real> *>(pinned_small_get());
        return reset_ctrl();
    }
    // the mirror back at iteration 0 (a reload; no copy of it in flight)
    Ctrl<real> *reset_ctrl() {
        std::memset(hctrl_, 0, sizeof(Ctrl<real>));
        hctrl_->obj_it = -1;
        hctrl_->itMax = itMax_;
        return hctrl_;
    }
    // a session that decided spec_: its depth, stream, events and, on a
    // partition, the split transport (a collective: every rank decides
    // alike).  It launches directly on its two streams: the decision's
    // kernels must run BESIDE the next sweeps, and a replayed graph ran its
    // branches one after the other (headline_conv 0.852 ms/iter with the
    // graph, r4h)
    void spec_setup(bool serial) {
        if (halo_ && !serial) evtr_ = halo_->tr->split(stream);
        sd_ = halo_ && halo_->tr->nranks >= 3 ? 4 : 2;
        if (!serial) PFDR_HIP(hipStreamCreateWithFlags(&evs_, hipStreamNonBlocking));
        for (int k = 0; k < sd_; k++) {
            PFDR_HIP(hipEventCreateWithFlags(&evv_[k], hipEventDisableTiming));
            PFDR_HIP(hipEventCreateWithFlags(&evd_[k], hipEventDisableTiming));
        }
        speculative = serial ? 2 : 1;
        graphs_ok_ = capturable_ = false;
    }
    // the chunk graph is part of the setup (instantiation costs ~0.1-1 ms,
    // which a small solve timed to tolerance would otherwise pay in its loop)
    void instantiate_setup_graph() {
        if (graphs_ok_) {
            try {
                (void)chunk_graph(chunk_);
            } catch (const std::exception &) {
                if (!halo_) throw;
                graphs_ok_ = capturable_ = false;  // this transport would not capture: launch directly
                (void)hipGetLastError();
            }
        }
        graphs = graphs_ok_ ? 1 : 0;
    }
    // release of the loop's host resources, before the session's buffers go
    // (a session's destructor calls it first; idempotent)
    void close() {
        if (hctrl_) {
            (void)hipStreamSynchronize(stream);  // no control-block copy in flight
            pinned_small_put(hctrl_);
            hctrl_ = nullptr;
        }
        for (Ctrl<real> *&c : snap_) if (c) { pinned_small_put(c); c = nullptr; }
        auto destroy = [](hipEvent_t &e) { if (e) (void)hipEventDestroy(e); e = nullptr; };
        for (hipEvent_t &e : snapev_) destroy(e);
        for (hipEvent_t &e : evv_) destroy(e);
        for (hipEvent_t &e : evd_) destroy(e);
        if (evs_) {
            (void)hipStreamSynchronize(evs_);
            (void)hipStreamDestroy(evs_);
            evs_ = nullptr;
        }
        drop_graphs();
    }

    // ------------------------------------------------------------- loop --
    void push_ctrl() {
        PFDR_HIP(hipMemcpyAsync(ctrl_.p, hctrl_, sizeof(Ctrl<real>), hipMemcpyHostToDevice, stream));
    }
    void pull_ctrl() {
        PFDR_HIP(hipMemcpyAsync(hctrl_, ctrl_.p, sizeof(Ctrl<real>), hipMemcpyDeviceToHost, stream));
        wait_stream();
    }
    // host wait for the session stream; partitioned sessions wait under the
    // transport's watchdog (a stalled halo exchange fails the call with the
    // rank, peers, bytes and iteration instead of hanging)
    void wait_stream() {
        if (!halo_) { PFDR_HIP(hipStreamSynchronize(stream)); return; }
        halo_->tr->phase = "iterations";
        halo_->tr->iteration = it_;
        halo_->tr->wait(stream);
    }
    void drop_graphs() {
        for (auto &kv : graphs_) (void)hipGraphExecDestroy(kv.second);
        graphs_.clear();
    }
    // red_[0 .. narr) = the sums of narr arrays of n terms (array y at terms +
    // y * stride) over every rank in the caller's order, rounded as the
    // reference's one-thread loop.  part / nparts: per-block sums of the same
    // terms when they lie in vertex order on one GPU (their binades predicted
    // from them), else null
    void evolution_sum(real *terms, long n, int narr, long stride, const real *part, int nparts,
                       hipStream_t s) {
        const int *halt = &ctrl_.p->halt;
        if (!halo_)
            mono_sum<real>(n, terms, nullptr, 0, nullptr, red_.p, nullptr, dws_.p, s, narr, stride,
                           halt, part, nparts);
        else if (!route_.ready())
            chain_.run(etr(), terms, stride, red_.p, halt, s);
        else
            route_.run(etr(), terms, stride, red_.p, halt, s);
    }
    // it and the records of the iterations so far (null: not recorded)
    void download_records(int *it, void *Obj_host, void *Dif_host, const real *Obj,
                          const real *Dif, HostPins &hp) {
        if (it) *it = it_;
        if (Obj_host && Obj) hp.copy(Obj_host, Obj, sizeof(real) * (it_ + 1), hipMemcpyDeviceToHost);
        if (Dif_host && Dif && it_ > 0)
            hp.copy(Dif_host, Dif, sizeof(real) * it_, hipMemcpyDeviceToHost);
    }

  private:
    int graph_key(int n) const { return kSpecMax * n + (spec_ ? it0_ % sd_ : 0); }
    void spec_body(int i, int n);
    void bodies(int n) {
        for (int i = 0; i < n; i++) spec_ ? spec_body(i, n) : body(i, n);
    }
    hipGraphExec_t chunk_graph(int n);
    void run_bodies(int n);
    bool settle(bool gated, bool drain);
    void run_pipelined(int target);
};

// iteration t = it0_ + 1 + i of a speculative session
template <typename real>
void IterLoop<real>::spec_body(int i, int n) {
    hipStream_t s = stream;
    const int t = it0_ + 1 + i;
    const int b = t % sd_;
    if (i >= sd_) PFDR_HIP(hipStreamWaitEvent(s, evd_[b], 0));  // the decision on t - D
    spec_sweeps(t, b);
    PFDR_HIP(hipEventRecord(evv_[b], s));
    const hipStream_t es = evs_ ? evs_ : s;
    PFDR_HIP(hipStreamWaitEvent(es, evv_[b], 0));
    spec_decide(b, es);  // overlaps the sweeps of t + 1 (not when serial)
    PFDR_HIP(hipGetLastError());
    PFDR_HIP(hipEventRecord(evd_[b], es));
    if (i == n - 1) PFDR_HIP(hipStreamWaitEvent(s, evd_[b], 0));  // join: the chunk's last
}

// the captured graph of n bodies (a whole chunk, or a run's tail after
// prepare()), instantiated once -- at the end of the setup for chunk_, and
// again after a reconditioning dropped them.  Speculative: keyed by t mod D
// too (the buffers its bodies cycle through)
template <typename real>
hipGraphExec_t IterLoop<real>::chunk_graph(int n) {
    const int key = graph_key(n);
    auto it = graphs_.find(key);
    if (it != graphs_.end()) return it->second;
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    PFDR_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    try {
        bodies(n);
    } catch (...) {
        (void)hipStreamEndCapture(stream, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
    }
    PFDR_HIP(hipStreamEndCapture(stream, &g));
    const hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    PFDR_HIP(e);
    // uploaded now, so that its first replay (a timed run's, after
    // prepare()) pays no upload: the driver's 20-step line 0.522 -> 0.517 ms
    PFDR_HIP(hipGraphUpload(ge, stream));
    graphs_.emplace(key, ge);
    return ge;
}

// whole chunks replay the captured graph; a partial chunk (the tail of a
// run) replays one only if prepare() built it, else it is launched directly
// rather than captured for one use
template <typename real>
void IterLoop<real>::run_bodies(int n) {
    if (tiny_) { tiny_chunk(n); return; }
    it0_ = it_;
    const int key = graph_key(n);
    if (!prof.on && capturable_ && graphs_.count(key)) {
        PFDR_HIP(hipGraphLaunch(graphs_[key], stream));
        return;
    }
    if (!graphs_ok_ || prof.on || n != chunk_) {
        bodies(n);
        return;
    }
    PFDR_HIP(hipGraphLaunch(chunk_graph(chunk_), stream));
}

// the graphs a run of `iters` iterations will replay (chunks of chunk_ and
// the tail), built now so that the run itself launches no capture
template <typename real>
void IterLoop<real>::prepare(int iters) {
    if (!capturable_ || iters <= 0) return;
    it0_ = it_;  // (the run starts here: its parity)
    if (iters >= chunk_) (void)chunk_graph(chunk_);
    if (iters % chunk_) (void)chunk_graph(iters % chunk_);
    PFDR_HIP(hipStreamSynchronize(stream));
}

// after a chunk: the stop or the reconditioning that the control block just
// read into hctrl_ asks for (stop first), then the progress line.  drain: a
// chunk is queued behind the one read (it ran halted).  true: reconditioned
template <typename real>
bool IterLoop<real>::settle(bool gated, bool drain) {
    bool reconditioned = false;
    if (gated && hctrl_->stop) {
        stopped_ = true;
    } else if (gated && hctrl_->recond) {
        if (drain) wait_stream();
        recondition();
        reconditionings++;
        hctrl_->recond = 0;
        hctrl_->halt = 0;
        push_ctrl();
        if (verbose_) { printf("done.\n"); fflush(stdout); }
        reconditioned = true;
    }
    if (verbose_ && (it_ >= next_print_ || stopped_)) {
        print_progress();
        next_print_ = it_ + verbose_;
    }
    return reconditioned;
}

template <typename real>
int IterLoop<real>::run(int iters) {
    const bool g = gated();
    const int target = (int)std::min<long>((long)it_ + std::max(iters, 0), (long)itMax_);
    const bool pipelined = g && !halo_ && !spec_;
    if (pipelined) run_pipelined(target);
    // every rank runs the same number of bodies: the decisions come from
    // all-reduced values, so the control blocks agree
    while (!pipelined && !stopped_ && it_ < target) {
        const int n = std::min(target - it_, chunk_);
        run_bodies(n);
        if (g) {
            pull_ctrl();
            it_ = hctrl_->it;
        } else {
            it_ += n;
            if (it_ >= itMax_) stopped_ = true;
        }
        settle(g, false);
    }
    wait_stream();
    if (prof.on) prof.resolve();
    return it_;
}

// Gated single-GPU runs: chunk k + 1 is launched before the host reads the
// control block chunk k left (a device-to-host snapshot ordered between the
// two chunks), so the host's round trip -- ≈35-45 us per chunk, a tenth of
// a 32-iteration chunk of C1 -- overlaps the GPU's work instead of idling
// it.  A chunk launched after a stop or a reconditioning request runs with
// the halt flag set: every kernel of it returns at once and changes nothing,
// so the iterates, the iteration count and Dif are those of the one-chunk-
// at-a-time loop.
template <typename real>
void IterLoop<real>::run_pipelined(int target) {
    for (int k = 0; k < 2; k++) {
        if (!snap_[k]) snap_[k] = static_cast<Ctrl<real> *>(pinned_small_get());
        if (!snapev_[k]) PFDR_HIP(hipEventCreateWithFlags(&snapev_[k], hipEventDisableTiming));
    }
    int k = 0, nq = 0;  // slot of the oldest unread snapshot, chunks in flight
    int ahead = it_;    // iterations launched so far, if none stops
    while (!stopped_) {
        while (nq < 2 && ahead < target) {
            const int n = std::min(target - ahead, chunk_);
            run_bodies(n);
            const int slot = (k + nq) & 1;
            PFDR_HIP(hipMemcpyAsync(snap_[slot], ctrl_.p, sizeof(Ctrl<real>),
                                    hipMemcpyDeviceToHost, stream));
            PFDR_HIP(hipEventRecord(snapev_[slot], stream));
            ahead += n;
            nq++;
        }
        if (nq == 0) break;
        PFDR_HIP(hipEventSynchronize(snapev_[k]));
        *hctrl_ = *snap_[k];
        k ^= 1;
        nq--;
        it_ = hctrl_->it;
        if (settle(true, true)) {
            nq = 0;
            ahead = it_;
        }
        if (!stopped_ && nq == 0 && ahead >= target) break;
    }
}

// The frame of a one-call entry on host arrays: the problem partitioned
// across the configured devices (multidev: not for a sparse A, which stays on
// one GPU whatever the device group), or one session set up, run to the end
// and read back; exceptions mapped to the C status.  N, K: for the call trace
template <typename Session, typename real, typename... Ctor>
int solve_one_call(const char *fn, pfdr_problem &p, real *X, int *it, real *Obj, real *Dif, int N,
                   int K, bool multidev, Ctor... ctor) {
    const int verbose = p.verbose;
    p.record_obj = Obj != nullptr;
    p.record_dif = Dif != nullptr;
    try {
        CallTrace tr(fn);
        if (verbose) { printf("Initializing constants and variables... "); fflush(stdout); }
        const std::vector<int> devs = multidev ? multidev_devices(&p) : std::vector<int>();
        int its = 0;
        if (!devs.empty()) {  // partitioned across the configured devices
            if (verbose) { printf("done (%d devices).\n", (int)devs.size()); fflush(stdout); }
            multidev_solve(&p, devs, &its, Obj, Dif);
        } else {
            std::unique_ptr<Session> s(new Session(&p, ctor...));
            if (verbose) { printf("done.\nPreconditioned forward-Douglas-Rachford algorithm\n"); fflush(stdout); }
            tr.setup_done();
            s->run(p.itMax);
            tr.run_done();
            s->result(X, &its, Obj, Dif);
            s.reset();
        }
        if (it) *it = its;
        tr.finish(p.V, p.E, N, K, its);
    } catch (const HipError &h) {
        return report_error(fn, h);
    } catch (const std::exception &ex) {
        return report_error(fn, ex.what());
    }
    return PFDR_OK;
}

}  // namespace pfdr
