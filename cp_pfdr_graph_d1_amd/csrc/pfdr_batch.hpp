// Batched dense-A PFDR sessions (include/pfdr_mi355x.h, "batched dense
// sessions"): B problems that share A, the graph and the penalties and differ
// in the observation and the iterate, iterated in lock step so that one
// stream of A serves every channel's products.
//
// A batch is B lanes.  A lane is a reusable QuadSession (pfdr_quadratic.hip)
// on a borrowed device matrix: its own iterate, edge variables, metric and
// control block, and the session's own kernels for everything but the forward
// step.  The batch (pfdr_batch.hip) uploads A once, drives the lanes through
// the seams below and launches the batched products on their buffers; each
// (row or column, channel) sum of those kernels is added in the order of the
// scalar kernel it replaces, so a lane's bytes are the scalar session's.
#pragma once
#include "pfdr_session.hpp"

namespace pfdr {

// what a lane borrows from its batch: the matrix, and from the first lane
// the diagonal of A^tA and the verdict of the symmetry check
template <typename real>
struct LaneShare {
    const real *A = nullptr;
    const real *diag = nullptr;  // null: the lane forms its own (the first lane)
    int symv = -1;               // -1: the lane checks the symmetry itself
};

// the buffers of a lane that the batched products read and write
template <typename real>
struct LaneView {
    typename Vec<real>::v2 *xp;  // (X, P) pairs
    real *R;                  // direct mode: the residual Y - A X
    const real *Y, *Ga;
    const Ctrl<real> *ctrl;   // null: an ungated session
    double *rpart;            // direct mode: the row partials (rows_nb x N)
    real *xfull;              // A^tA mode: X alone (V)
    real *spart;              // symmetric tiles: the partials (snb x V)
};

// facts that are equal over the lanes of a batch
struct LaneFacts {
    int V, N;            // N: the rows of A (direct) or V (A^tA)
    bool direct;         // N > 0
    bool exact, symv;    // the product path
    bool gated, rec_obj;
    int rows_nb, rows_cpb, snb;
};

template <typename real>
class DenseLane {
  public:
    virtual ~DenseLane() = default;
    virtual SessionBase &base() = 0;
    virtual LaneFacts facts() const = 0;
    virtual LaneView<real> view() = 0;
    virtual const real *diag() const = 0;
    // one iteration in three parts: the sweeps and the loop decision, the
    // forward step (scalar: the session's own launches), the objective
    virtual void lane_head() = 0;
    virtual void lane_forward() = 0;
    virtual void lane_objective() = 0;
    // the chunk boundary: the control block into the mirror, then what
    // IterLoop::run does after a chunk of n bodies
    virtual void lane_chunk_begin() = 0;
    virtual void lane_snapshot() = 0;
    virtual void lane_settle(int n) = 0;
    virtual int lane_it() const = 0;
    virtual int lane_itmax() const = 0;
    virtual bool lane_stopped() const = 0;
};

// a lane of the problem p (its X and Y: the channel's), defined beside the
// session (pfdr_quadratic.hip)
template <typename real>
DenseLane<real> *create_quadratic_lane(const pfdr_problem *p, const LaneShare<real> &share);

}  // namespace pfdr
