/* ==========================================================================
 * pfdr_mi355x.h — C ABI of the MI355X-native PFDR solvers (libpfdr_mi355x.so)
 *
 * Plain C, fixed-width scalars, plain pointers and sizes; no C++ or torch
 * types.  Two layers:
 *
 *  1. Drop-in entry points.  Same argument list and meaning as the reference
 *     C++ templates they replace, host pointers, synchronous (device work is
 *     finished and every output copied back before return), status return
 *     instead of void.  The C++ drop-in symbols
 *     (include/PFDR_graph_quadratic_d1_l1.hpp etc.) forward to these.
 *       pfdr_quadratic_d1_l1_{f32,f64}
 *           replaces PFDR_graph_quadratic_d1_l1<real>
 *           (reference include/PFDR_graph_quadratic_d1_l1.hpp:36-42,
 *            src/PFDR_graph_quadratic_d1_l1.cpp:270-553)
 *       pfdr_quadratic_d1_bounds_{f32,f64}
 *           replaces PFDR_graph_quadratic_d1_bounds<real>
 *           (reference include/PFDR_graph_quadratic_d1_bounds.hpp:34-40,
 *            src/PFDR_graph_quadratic_d1_bounds.cpp:244-530)
 *       pfdr_loss_d1_simplex_{f32,f64}
 *           replaces PFDR_graph_loss_d1_simplex<real>
 *           (reference include/PFDR_graph_loss_d1_simplex.hpp:24-30,
 *            src/PFDR_graph_loss_d1_simplex.cpp:372-715)
 *       pfdr_proj_simplex_metric_{f32,f64}
 *           replaces proj_simplex_metric<real>
 *           (reference include/proj_simplex.hpp:33-35,
 *            src/proj_simplex_metric.cpp:18-83)
 *
 *  2. Sessions: the same solvers with inputs that may already live in HBM,
 *     setup separated from iterations (benchmarks, repeated solves) and the
 *     1-D vertex-range partition across GPUs (RCCL halo exchange).
 *
 * Every entry returns PFDR_OK (0) or an error code; pfdr_last_error() gives
 * the message of the calling thread's last failure.  There is no CPU
 * fallback: without a usable gfx950 device every compute entry fails.
 * ======================================================================== */
#ifndef PFDR_MI355X_H
#define PFDR_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFDR_OK 0
#define PFDR_ERR_ARG 1    /* invalid argument */
#define PFDR_ERR_HIP 2    /* HIP runtime failure (no device, OOM, fault) */
#define PFDR_ERR_RCCL 3   /* collective failure */
#define PFDR_ERR_STATE 4  /* session used out of order */

/* Lipschitz information type, same values as the reference's
 * typedef enum {SCAL, DIAG} Lipschtype (include/PFDR_graph_quadratic_d1_l1.hpp:34) */
#define PFDR_LIPSCHITZ_SCAL 0
#define PFDR_LIPSCHITZ_DIAG 1

const char *pfdr_last_error(void);
int pfdr_abi_version(void);          /* 4 (pfdr_problem.spec added) */
int pfdr_device_count(void);         /* visible HIP devices, <0 on error */

/* ------------------------------------------------------------------ l1 -- */
int pfdr_quadratic_d1_l1_f32(int V, int E, int N, float *X, const float *Y,
    const float *A, const int *Eu, const int *Ev, const float *La_d1,
    const float *La_l1, int positivity, int Ltype, const float *L,
    float rho, float condMin, float difRcd, float difTol, int itMax,
    int *it, float *Obj, float *Dif, int verbose);
int pfdr_quadratic_d1_l1_f64(int V, int E, int N, double *X, const double *Y,
    const double *A, const int *Eu, const int *Ev, const double *La_d1,
    const double *La_l1, int positivity, int Ltype, const double *L,
    double rho, double condMin, double difRcd, double difTol, int itMax,
    int *it, double *Obj, double *Dif, int verbose);

/* -------------------------------------------------------------- bounds -- */
int pfdr_quadratic_d1_bounds_f32(int V, int E, int N, float *X,
    const float *Y, const float *A, const int *Eu, const int *Ev,
    const float *La_d1, float min, float max, int Ltype, const float *L,
    float rho, float condMin, float difRcd, float difTol, int itMax,
    int *it, float *Obj, float *Dif, int verbose);
int pfdr_quadratic_d1_bounds_f64(int V, int E, int N, double *X,
    const double *Y, const double *A, const int *Eu, const int *Ev,
    const double *La_d1, double min, double max, int Ltype, const double *L,
    double rho, double condMin, double difRcd, double difTol, int itMax,
    int *it, double *Obj, double *Dif, int verbose);

/* ------------------------------------------------------------- simplex -- */
int pfdr_loss_d1_simplex_f32(int K, int V, int E, float al,
    const float *La_f, float *P, const float *Q, const int *Eu,
    const int *Ev, const float *La_d1, float rho, float condMin,
    float difRcd, float difTol, int itMax, int *it, float *Obj, float *Dif,
    int verbose);
int pfdr_loss_d1_simplex_f64(int K, int V, int E, double al,
    const double *La_f, double *P, const double *Q, const int *Eu,
    const int *Ev, const double *La_d1, double rho, double condMin,
    double difRcd, double difTol, int itMax, int *it, double *Obj,
    double *Dif, int verbose);

int pfdr_proj_simplex_metric_f32(float *X, const float *M, int D, int N,
    int nm, const float *A, int na);
int pfdr_proj_simplex_metric_f64(double *X, const double *M, int D, int N,
    int nm, const double *A, int na);

/* ------------------------------------------------------------ sessions -- */
#define PFDR_KIND_L1 0
#define PFDR_KIND_BOUNDS 1
#define PFDR_KIND_SIMPLEX 2

#define PFDR_F32 0
#define PFDR_F64 1

#define PFDR_MEM_HOST 0    /* pointers are host memory (copied in) */
#define PFDR_MEM_DEVICE 1  /* pointers are device memory of the current device */
/* Ordering of device inputs: the library reads (and, for the session's
 * lifetime, keeps reading nothing but its own copies of) the caller's
 * device arrays on its own non-blocking stream, which does not wait for the
 * caller's streams.  Every write into those arrays must be complete before
 * the call (e.g. synchronise the producing stream; the Python front-end
 * synchronises torch's current stream).  Outputs are complete on return. */

/* Internal vertex relabelling for cache locality (breadth-first order,
 * pfdr_order.hip): AUTO applies it when the labels look random (V >= 2^20 and
 * over a quarter of the edges span more than V/64 labels).  Inputs and
 * outputs stay in the caller's labels; the reference's summation orders are
 * kept, so results do not change. */
#define PFDR_REORDER_AUTO 0
#define PFDR_REORDER_ON 1
#define PFDR_REORDER_OFF 2

/* Iterate-evolution statistic (the stopping / reconditioning test and Dif;
 * reference src/PFDR_graph_quadratic_d1_l1.cpp:514-529, simplex
 * src/PFDR_graph_loss_d1_simplex.cpp:653-691).  The reference adds its terms
 * one by one in `real`, and over millions of f32 terms that sum drifts by
 * percents from the exact value -- enough to move the stopping iteration.
 * SEQUENTIAL reproduces that rounding exactly (parallel binade scan,
 * pfdr_monosum.hpp): Dif, the stopping iteration and the iterate are then
 * the reference's bit for bit.  TREE sums in a fixed tree (faster; the
 * decision may land an iteration or so away on huge f32 problems).  AUTO:
 * SEQUENTIAL on one GPU for sums of at least 2^17 terms, except on the
 * small-graph paths that decide inside a sweep (quadratic: identity /
 * diagonal A, no objective record, <= 1,024 vertex blocks of 256; both
 * solvers' one-workgroup paths), which keep TREE.  A partitioned session
 * applies the same rule to its global term count: SEQUENTIAL sums the terms
 * rank to rank in the caller's order (ChainSum, pfdr_halo.hpp; a relabelled
 * split first routes every term to the rank owning that caller-order
 * slice), bit-identical to one GPU; the simplex's label counts (0 / 1 terms,
 * exact in any order) keep TREE there.  SEQUENTIAL forced on a small graph
 * takes the multi-launch loop instead of those paths. */
#define PFDR_EVOLUTION_AUTO 0
#define PFDR_EVOLUTION_SEQUENTIAL 1
#define PFDR_EVOLUTION_TREE 2
/* speculative decisions (pfdr_problem.spec; env PFDR_SPEC = auto | serial |
 * off overrides): sessions with a sequential evolution statistic, difRcd = 0
 * and no objective record decide on iteration t while t + 1 sweeps.
 *   AUTO   the evolution sums and the decision run on a second stream; a
 *          partition runs them over a communicator split from its own
 *          (ncclCommSplit) beside the next iteration's halo exchanges --
 *          concurrent operations on two communicators, which NCCL/RCCL do
 *          not guarantee to co-schedule;
 *   SERIAL the same buffers and decisions on the session stream over the one
 *          communicator: no split, no second stream, no concurrency; results
 *          identical bit for bit, the decision no longer overlapped;
 *   OFF    the plain sequential loop (identical results). */
#define PFDR_SPEC_AUTO 0
#define PFDR_SPEC_SERIAL 1
#define PFDR_SPEC_OFF 2

typedef struct pfdr_problem {
    int kind;             /* PFDR_KIND_* */
    int dtype;            /* PFDR_F32 / PFDR_F64: type of every real array */
    int mem;              /* PFDR_MEM_*: location of every array below */
    int V, E, N, K;       /* as the reference (K only for simplex) */
    void *X;              /* X (quadratic) or P (simplex), initial value */
    const void *Y;        /* Y / A^tY (quadratic) or Q (simplex) */
    const void *A;        /* quadratic only, NULL for identity */
    const int *Eu, *Ev;   /* endpoints (global vertex ids when distributed) */
    const void *La_d1;    /* length E */
    const void *La_l1;    /* l1 weights (V) or La_f (simplex, V); may be NULL */
    int positivity;       /* l1 only */
    double min, max;      /* bounds only (+-HUGE_VAL for none) */
    double al;            /* simplex only */
    int Ltype;            /* PFDR_LIPSCHITZ_* */
    const void *L;        /* NULL, scalar or length V */
    double rho, condMin, difRcd, difTol;
    int itMax;
    int verbose;
    int record_obj;       /* keep Obj[0..itMax] on the device */
    int record_dif;       /* keep Dif[0..itMax-1] on the device */
    /* --- 1-D vertex-range partition (leave zero for one GPU) ------------ */
    int nranks, rank;     /* rank r owns global vertices [vtx_begin, vtx_begin+V) */
    void *comm;           /* ncclComm_t (pfdr_comm_init) or loopback hub */
    int comm_kind;        /* PFDR_COMM_RCCL or PFDR_COMM_LOOPBACK */
    int64_t vtx_begin;    /* first owned global vertex */
    int64_t V_global;     /* total vertices over all ranks */
    const int64_t *e_global; /* global id of each local edge; NULL: e_offset + e */
    int64_t e_offset;
    /* --- internal locality reordering (quadratic solvers, one GPU) -------- */
    int reorder;          /* PFDR_REORDER_*; results are identical either way */
    /* --- iterate-evolution statistic -------------------------------------- */
    int evolution;        /* PFDR_EVOLUTION_* */
    /* --- relabelled partition (pfdr_locality_order) ----------------------- */
    const int64_t *vtx_label; /* caller's label of each owned vertex (V of them,
                             host or device per mem); NULL: vtx_begin + v.  Set
                             when the ranks own ranges of a RELABELLED graph:
                             the preconditioner's amplitude sum then runs in
                             the caller's label order (all-reduced, then summed
                             in that order on every rank), as the reference's
                             one-thread loop does (quadratic solvers). */
    /* --- speculative decisions ---------------------------------------------- */
    int spec;             /* PFDR_SPEC_* (0: AUTO) */
} pfdr_problem;

typedef struct pfdr_session pfdr_session;

/* Locality order of a graph's vertices for a vertex-range partition
 * (randomly labelled k-NN graphs must be reordered before
 * partitioning, or every edge becomes a halo edge): the deterministic
 * breadth-first order of pfdr_order.hip, computed on the current device.
 * order_out[new] = old label (V entries, host or device per mem).  *applied
 * = 0 when the graph is path-like (too many levels) and the identity was
 * returned.  Use: rank r owns new labels [off[r], off[r+1]), its edges are
 * those whose relabelled Eu it owns (original edge ids as e_global), and
 * vtx_label = order_out[off[r] .. off[r+1]) (see partition.py). */
int pfdr_locality_order(int V, int64_t E, const int *Eu, const int *Ev, int mem,
                        int *order_out, int *applied);

int pfdr_session_create(pfdr_session **out, const pfdr_problem *p);
/* Run up to `iters` more iterations (stopping early on difTol / itMax as the
 * reference does).  *it_total receives the total iteration count so far. */
int pfdr_session_run(pfdr_session *s, int iters, int *it_total);
/* Capture now the hipGraphs that a later pfdr_session_run(s, iters) replays
 * (chunks of 32 iterations and the run's tail), so that the run itself
 * instantiates nothing; no iteration runs.  A no-op where the session
 * launches directly (small one-workgroup graphs, objective record, loopback
 * partitions). */
int pfdr_session_prepare(pfdr_session *s, int iters);
/* Copy X (or P) back to host memory, and the iteration count; Obj/Dif copy
 * it+1 / it values when recorded (may be NULL). */
int pfdr_session_result(pfdr_session *s, void *X_host, int *it, void *Obj_host,
                        void *Dif_host);
/* Device pointer of the current iterate (valid until destroy). */
void *pfdr_session_device_x(pfdr_session *s);
/* Kernel timing: when enabled, HIP events bracket the launches of the named
 * kernels on the session stream; stats give timed launches and mean
 * duration.  on = 0 off, 1 every launch, P >= 2 every P-th launch of each
 * kernel (an event pair costs ~6-9 us of GPU time: sampling keeps it out of
 * short iterations).  The filter restricts timing to a comma-separated list
 * of kernel names (NULL or "" = all). */
int pfdr_session_set_profiling(pfdr_session *s, int on);
int pfdr_session_profile_filter(pfdr_session *s, const char *names);
int pfdr_session_kernel_stats(pfdr_session *s, const char *kernel,
                              int *launches, double *mean_ms);
/* Synchronise the session stream. */
int pfdr_session_sync(pfdr_session *s);
/* Bytes of device memory held by the session. */
int64_t pfdr_session_device_bytes(pfdr_session *s);
/* Session facts by name: "reordered" (1 when the internal locality
 * relabelling is active), "device_bytes", "split_blocks", "ustaged",
 * "symv", "tiny", "coop" (workgroups of the persistent mid-size-graph
 * launch, 0 when off), "fused" (1: the loop decision of a small graph is
 * taken inside the next edge sweep, two launches per iteration), "padded"
 * (1: such a graph's contributions are stored in per-vertex-block lists, so
 * its vertex sweep stages them without dependent address loads),
 * "dense_exact" (1: the dense products run in the reference's sequential
 * order, bit-exact; small single-GPU problems; with weights >= 0 a recorded
 * Obj is added in that order as well, in direct and in A^tA mode),
 * "tiled_blocks" (vertex
 * blocks staging tile-ordered contributions) and "record_blocks" (of those,
 * the blocks whose runs fit one per-block record), "slot_patterns" (distinct
 * slot sequences of those records' runs, 0: per-entry slots), "speculative"
 * (1: the evolution sums run beside the next iteration's sweeps on a second
 * stream, 2: after them on the session stream), "edge_ratio" (1: the tiled
 * edge sweep reads each end's (c La_d1 / Aux) / Ga formed once per vertex;
 * until the first reconditioning), "vertex_pair" (> 0: the vertex sweep takes
 * two record blocks per workgroup, the value the largest block's entries).
 * Sparse sessions add "sparse_nnz" (stored entries; 0 for any other session),
 * "sparse_exact" (1: the four products add the stored entries in the
 * reference's order, bit-exact on the densified matrix; 0: the parallel
 * kernels), "sparse_seg_col" / "sparse_seg_row" (lanes per column / row of
 * the parallel kernels) and "sparse_csr_us" (wall time of the CSR build).
 * "reusable" (1: created by pfdr_session_create_reusable), "staging_bytes"
 * (the device staging such a session keeps for host arrays) and
 * "reconditionings" (their count since the creation or the last reload). */
int pfdr_session_query(pfdr_session *s, const char *what, int64_t *value);
void pfdr_session_destroy(pfdr_session *s);

/* ------------------------------------------------------------ sparse A -- */
/* A (N-by-V, N > 0) in compressed sparse columns, the sparse twin of the
 * reference's column-major layout: column v holds the entries
 * colptr[v] .. colptr[v+1] - 1.
 *   colptr[V+1]  non-decreasing, colptr[0] = 0, colptr[V] = nnz;
 *   rowidx[nnz]  in [0, N), strictly ascending inside each column;
 *   val[nnz]     of the problem's real type; stored zeros are allowed and
 *                behave as the dense zero would.
 * 1 <= nnz < 2^31 - 256.  The arrays are host or device memory per
 * pfdr_problem.mem (the one-call entries: host) and are copied in.
 *
 * The session is the direct-mode one (Y of length N, Obj with 1/2 ||R||^2)
 * whose four products with A -- diag(A^tA), the pseudo-inverse, R = Y - A X
 * and -A^t R -- walk the stored entries.  While the longest column and the
 * longest row have at most 8,192 entries, each product adds its entries in
 * ascending index order in the real type, which gives the bytes of the
 * reference's loops on the densified matrix as long as the iterates are
 * finite ("sparse_exact" = 1; a recorded Obj as well, its three sums added
 * term by term, unless a La_d1 / La_l1 is negative); longer ones take the
 * parallel kernels (a segment of lanes per column / row, sums in double),
 * within the dense modes' tolerances of it.  The environment variable
 * PFDR_SPARSE_EXACT = 1 | 0 | auto, read when the session is created, forces
 * one or the other.
 *
 * PFDR_ERR_ARG, with the offence named by the last-error string and before
 * any iteration runs: N <= 0; p->A set as well; the simplex kind; nranks > 1
 * or a communicator; a NULL array; colptr not as above; a row index out of
 * range or not strictly ascending; a column of squared norm 0 (the reference
 * divides by it).  Cut pursuit takes the same pfdr_csc through
 * pfdr_cp_solver_create_sparse, pfdr_cp_reduce_csc_* and
 * pfdr_cpgraph_gradient_csc below. */
typedef struct pfdr_csc {
    int64_t nnz;
    const int64_t *colptr;
    const int32_t *rowidx;
    const void *val;
} pfdr_csc;
int pfdr_session_create_sparse(pfdr_session **out, const pfdr_problem *p, const pfdr_csc *A);
/* The one-call solvers above with A replaced by nnz, colptr, rowidx, val. */
int pfdr_quadratic_d1_l1_csc_f32(int V, int E, int N, float *X, const float *Y,
    int64_t nnz, const int64_t *colptr, const int32_t *rowidx, const float *val,
    const int *Eu, const int *Ev, const float *La_d1, const float *La_l1,
    int positivity, int Ltype, const float *L, float rho, float condMin,
    float difRcd, float difTol, int itMax, int *it, float *Obj, float *Dif,
    int verbose);
int pfdr_quadratic_d1_l1_csc_f64(int V, int E, int N, double *X, const double *Y,
    int64_t nnz, const int64_t *colptr, const int32_t *rowidx, const double *val,
    const int *Eu, const int *Ev, const double *La_d1, const double *La_l1,
    int positivity, int Ltype, const double *L, double rho, double condMin,
    double difRcd, double difTol, int itMax, int *it, double *Obj, double *Dif,
    int verbose);
int pfdr_quadratic_d1_bounds_csc_f32(int V, int E, int N, float *X, const float *Y,
    int64_t nnz, const int64_t *colptr, const int32_t *rowidx, const float *val,
    const int *Eu, const int *Ev, const float *La_d1, float min, float max,
    int Ltype, const float *L, float rho, float condMin, float difRcd,
    float difTol, int itMax, int *it, float *Obj, float *Dif, int verbose);
int pfdr_quadratic_d1_bounds_csc_f64(int V, int E, int N, double *X, const double *Y,
    int64_t nnz, const int64_t *colptr, const int32_t *rowidx, const double *val,
    const int *Eu, const int *Ev, const double *La_d1, double min, double max,
    int Ltype, const double *L, double rho, double condMin, double difRcd,
    double difTol, int itMax, int *it, double *Obj, double *Dif, int verbose);
/* Debug: the CSR view a sparse session built (rowptr[N+1], colidx[nnz],
 * rval[nnz] of the session's real type; host arrays, any may be NULL). */
int pfdr_debug_session_csr(pfdr_session *s, int64_t *rowptr, int32_t *colidx, void *rval);

/* ---------------------------------------------------- reusable sessions -- */
/* A quadratic session (PFDR_KIND_L1 / _BOUNDS, one GPU) that solves problem
 * after problem on the graph and the matrix it was created with.
 * pfdr_session_create_reusable is pfdr_session_create (A NULL) or
 * pfdr_session_create_sparse (A given) and behaves and runs exactly as they
 * do; it only keeps what a reload needs and they release: the map from the
 * internal edge order to the caller's (4 bytes per edge, tile-ordered or
 * relabelled sessions), the relabelling (4 bytes per vertex, relabelled
 * sessions) and the device staging of host arrays that go through either.
 * "device_bytes" counts them ("staging_bytes": the staging alone).  The
 * simplex kind and partitioned problems (nranks > 1 or a communicator) are
 * PFDR_ERR_ARG.
 *
 * pfdr_session_reload replaces values and restarts the solve at iteration 0,
 * as if a session had just been created on the new problem: the result of the
 * runs that follow (X, it, Obj, Dif) and the session's path queries equal a
 * fresh session's bit for bit.  X, Y, La_d1, La_l1, L: in the caller's vertex
 * / edge order and the session's real type, host or device memory per mem; a
 * NULL pointer keeps the session's copy, and for X that is the current
 * iterate (a warm start).  L has the form it had at creation (one value or V
 * of them).  The scalars are always read: min and max (bounds kind only),
 * rho, condMin, difRcd, difTol, itMax.  Everything that depends on the graph
 * or on A alone is kept (orders, incidence, tile tables, the diagonal of A^tA,
 * a sparse A's CSR view); the loop variant chosen at creation is kept too.
 * The captured graphs are dropped and the chunk graph is instantiated again.
 * The cost is a few streaming passes over the value arrays and the first
 * preconditioning.
 *
 * PFDR_ERR_ARG, naming the offence and before any device work (the session
 * then still holds its problem and can go on running): a session not created
 * reusable; the simplex kind; a partitioned session; La_l1 or L given where
 * the session was created without it (a NULL La_l1 keeps the session's, so
 * the weights cannot be taken away either); min > max or a NaN bound; itMax
 * above the creation's (the records are sized by it); difTol / difRcd that
 * would switch the tracking of the iterate evolution (difTol > 0 || difRcd >
 * 0 || record_dif) on or off, move difRcd between zero and non-zero, or in
 * any other way change the loop variant chosen at creation. */
typedef struct pfdr_reload {
    int mem;              /* PFDR_MEM_*: location of every array below */
    const void *X;        /* initial iterate (V); NULL: the current iterate */
    const void *Y;        /* as pfdr_problem.Y; NULL: kept */
    const void *La_d1;    /* length E; NULL: kept */
    const void *La_l1;    /* length V (l1 kind); NULL: kept */
    const void *L;        /* one value or V, as at creation; NULL: kept */
    double min, max;      /* bounds kind */
    double rho, condMin, difRcd, difTol;
    int itMax;            /* <= the creation's */
} pfdr_reload;
int pfdr_session_create_reusable(pfdr_session **out, const pfdr_problem *p, const pfdr_csc *A);
int pfdr_session_reload(pfdr_session *s, const pfdr_reload *r);

/* ------------------------------------------------ batched dense sessions -- */
/* B problems of kind l1 or bounds with a dense A (direct, N > 0, or
 * premultiplied, N = -V) that share A, the graph, La_d1, La_l1, L, the bounds
 * and every scalar, and differ in the observation and in the iterate -- a time
 * series of sensor vectors through one lead field.  The iterations of the
 * dense modes are the stream of A; a batch iterates its channels in lock step
 * and one pass over A serves a group of G channels ("channel_group", 8), so B
 * channels cost ceil(B / G) passes per product, not B.
 *
 * Layout: every array is channel-major and contiguous.  p->X is B x V
 * (channel b at X + b V), p->Y is B x len (len = N in direct mode, V in A^tA
 * mode); the outputs X (B x V), it (B), Obj (B x (itMax + 1)) and Dif (B x
 * itMax, itMax the creation's) follow the same rule; any output may be NULL.
 * mem covers all arrays, as for a session.  1 <= B <= 64.  A is copied to the
 * device once.
 *
 * Channel equality: channel b is the session pfdr_session_create would make
 * on (X_b, Y_b, the shared rest); after any sequence of pfdr_batch_run calls
 * its X, it, Obj and Dif are that session's bytes after the same sequence of
 * pfdr_session_run calls -- in f32 and f64, on every product path (the
 * sequential-order one of small problems, "dense_exact", the column dots,
 * the row partials, the symmetric tiles, "symv"), with difTol > 0 (each
 * channel stops at its own iteration and is not written again while the
 * others go on) and with difRcd > 0 (each channel reconditions at its own
 * iterations and decays its own difRcd^2).  The batched kernels add every
 * (row or column, channel) sum in the order and precision of the scalar
 * kernel they replace.  On the sequential-order path the products stay the
 * scalar kernels, one launch per channel.
 *
 * pfdr_batch_run returns when every channel has stopped or has run `iters`
 * more iterations; it[b] (it may be NULL) is channel b's total.
 * pfdr_batch_reload is pfdr_session_reload for every channel at once: r->Y
 * (B x len) and r->X (B x V) are per channel, NULL Y keeps the current
 * observations and NULL X warm-starts every channel from its own iterate;
 * La_d1, La_l1 and L are one shared array each, or NULL; the scalars are read
 * and the refusals are those of pfdr_session_reload (the batch stays
 * runnable).  What follows equals a fresh batch on the new values, byte for
 * byte; A, diag(A^tA), the symmetric-product plan and the graph tables are
 * kept.  pfdr_batch_query answers "channels" (B), "channel_group" (G),
 * "active" (channels not yet stopped), "shared_products" (batched product
 * launches so far), "device_bytes" (A counted once), "symv" and "dense_exact"
 * (as a session).
 *
 * PFDR_ERR_ARG, with the offence named by pfdr_last_error, before any device
 * work and without a handle: B outside [1, 64]; N == 0 (an identity or
 * diagonal A has no product to share: use one reusable session and
 * pfdr_session_reload); the simplex kind; A == NULL; nranks > 1 or a
 * communicator (a device group, pfdr_set_devices, does not apply either);
 * anything pfdr_session_create refuses for one channel.  A sparse A is not
 * offered here: there is no pfdr_csc argument. */
typedef struct pfdr_batch pfdr_batch;
int pfdr_batch_create(pfdr_batch **out, const pfdr_problem *p, int B);
int pfdr_batch_run(pfdr_batch *b, int iters, int *it /* B, may be NULL */);
int pfdr_batch_result(pfdr_batch *b, void *X, int *it, void *Obj, void *Dif);
int pfdr_batch_reload(pfdr_batch *b, const pfdr_reload *r);
int pfdr_batch_query(pfdr_batch *b, const char *what, int64_t *value);
void pfdr_batch_destroy(pfdr_batch *b);

/* ------------------------------------------- dense matrices (CP builder) -- */
/* Gram matrix on the matrix cores (exact-f32 / f64 MFMA, fixed-order
 * reductions): which = 0 -> G = A^t A (N-by-N), 1 -> G = A A^t (M-by-M); A
 * is M-by-N column major; mem = PFDR_MEM_HOST or _DEVICE for A and G.
 * *ms (may be NULL) receives the kernel time.  Replaces the reference's
 * symmetrisation loops (src/operator_norm_matrix.cpp:112-165,
 * src/CP_PFDR_graph_quadratic_d1_l1.cpp:688-702). */
int pfdr_gram_f32(int which, int M, int N, const float *A, int mem, float *G, double *ms);
int pfdr_gram_f64(int which, int M, int N, const double *A, int mem, double *G, double *ms);
/* Strictly sequential sum seed + a[0] + ... + a[n-1] of NONNEGATIVE terms,
 * rounded exactly as the one-thread loop: the preconditioner's amplitude sum
 * (src/PFDR_graph_quadratic_d1_l1.cpp:146-152, _bounds.cpp:143-149).  method 0:
 * workgroup binade scan (what the solvers use), 1: one-lane loop.  mem =
 * PFDR_MEM_HOST / _DEVICE for a; *ms (may be NULL) receives the kernel time.
 * Negative terms give an unspecified result. */
int pfdr_sequential_sum_f32(int64_t n, const float *a, int mem, float seed, int method,
                            float *out, double *ms);
int pfdr_sequential_sum_f64(int64_t n, const double *a, int mem, double seed, int method,
                            double *out, double *ms);
/* The stable LSD radix sort the library builds its incidence lists with
 * (pairs sorted by the low `bits` bits of the key, equal keys in input
 * order), on host arrays, in place; *ms (may be NULL) receives the sort's
 * GPU time.  n < 2^31.  Exposed for its tests. */
int pfdr_radix_sort_pairs_u32(int64_t n, uint32_t *keys, uint32_t *vals, int bits, double *ms);
int pfdr_radix_sort_pairs_u64(int64_t n, uint64_t *keys, uint32_t *vals, int bits, double *ms);
/* Squared operator norm ||A||^2 by the power method (reference
 * operator_norm_matrix<real>, include/operator_norm_matrix.hpp:12-14, same
 * argument meaning; deterministic starts, numbered across the batches of 64
 * that nbInit > 64 takes).  *gram_ms (may be NULL): time of
 * the Gram step when the matrix was symmetrised first. */
int pfdr_operator_norm_f32(int M, int N, const float *A, int mem, float nTol, int itMax,
                           int nbInit, int verbose, float *norm2, double *gram_ms);
int pfdr_operator_norm_f64(int M, int N, const double *A, int mem, double nTol, int itMax,
                           int nbInit, int verbose, double *norm2, double *gram_ms);
/* The same for A (N-by-V) in CSC (pfdr_csc above; its arrays host or device
 * per mem, copied in and checked as pfdr_session_create_sparse checks them,
 * except that an empty column is accepted): ||A||^2 by the power method on
 * A^tA, two sparse products per iteration, never densified and never
 * symmetrised.  All starts run at once in a batch of 16, 32 or 64, each with
 * the reference's stopping rule (a - b)/b < nTol; the result is the largest b
 * over the first nbInit starts (nbInit <= 0 counts as 1; a NaN never wins; a
 * matrix whose stored values are all zero gives 0).  Start c, coordinate r,
 * takes the dense entry's starting value number r + c V, c counting across
 * batches.  Every sum adds its terms in a fixed order that depends on neither
 * the batch size nor the other starts, and there are no floating-point
 * atomics: a start's result does not depend on nbInit, and two calls give the
 * same bytes.  A negative itMax runs no iteration after the first product, as
 * in the dense entry.  ms (may be NULL) receives two values: the wall time of
 * the CSR build and of the power method.
 *
 * PFDR_ERR_ARG, naming the offence and before any device work: N <= 0,
 * V <= 0, mem neither PFDR_MEM_HOST nor _DEVICE, a NULL pfdr_csc or array in
 * it, nnz outside [1, 2^31 - 256), a NULL norm2; after the one-pass device
 * check and before any product: a malformed colptr or rowidx. */
int pfdr_operator_norm_csc_f32(int N, int V, const pfdr_csc *A, int mem, float nTol, int itMax,
                               int nbInit, int verbose, float *norm2, double *ms);
int pfdr_operator_norm_csc_f64(int N, int V, const pfdr_csc *A, int mem, double nTol, int itMax,
                               int nbInit, int verbose, double *norm2, double *ms);
/* The diagonal Lipschitz majorant of a CSC: L[v] = sum_i |A_iv| r_i with
 * r_i = sum_j |A_ij| (V values, host or device per mem).  By Cauchy-Schwarz
 * A^tA <= diag(L), so L is valid PFDR_LIPSCHITZ_DIAG input, and max_v L[v] <=
 * ||A||_1 ||A||_inf.  *bound (a host value, may be NULL) receives that scalar
 * bound, max_v sum_i |A_iv| times max_i r_i.  Every sum runs over the stored
 * entries in stored order, in double, and is rounded once to the real type.
 * An empty column gives L[v] = 0 (the sessions refuse such a column anyway:
 * its squared norm is 0).  Arguments and errors as above (L for norm2). */
int pfdr_lipschitz_diag_csc_f32(int N, int V, const pfdr_csc *A, int mem, float *L, float *bound);
int pfdr_lipschitz_diag_csc_f64(int N, int V, const pfdr_csc *A, int mem, double *L,
                                double *bound);

/* Cut-pursuit reduced-problem builder (reference
 * src/CP_PFDR_graph_quadratic_d1_l1.cpp:663-841).
 * Components: rVc[rV + 1] offsets into the vertex list Vc[V].  A, Y as the
 * CP caller's (N > 0: A N-by-V, Y length N; N = -V: A = A^tA, Y = A^tY;
 * N = 0: A diagonal or NULL).  preAt (N > 0): also form rAA = rA^t rA and
 * rY = rA^t Y (forced for N <= 0).  Outputs (host or device per mem): rA
 * (N-by-rV, N > 0), rAA (rV-by-rV, or rV for N = 0), rY (rV; not formed
 * for N > 0 without preAt: CP then passes the whole Y), L (rV: the
 * Lipschitz metric l^2 c after Jacobi equilibration, c = squared norm of
 * the equilibrated matrix by the power method with normTol / normItMax /
 * normNbInit — CP uses 1e-3, 100, 10), Leq (rV, may be NULL: l).  All sums
 * sequential in the reference's order (bit-identical to the restatement);
 * only c depends on the (deterministic) starts. */
int pfdr_cp_reduce_f32(int N, int V, const float *A, const float *Y, int rV, const int *rVc,
                       const int *Vc, int preAt, int mem, float normTol, int normItMax,
                       int normNbInit, float *rA, float *rAA, float *rY, float *L, float *Leq);
int pfdr_cp_reduce_f64(int N, int V, const double *A, const double *Y, int rV, const int *rVc,
                       const int *Vc, int preAt, int mem, double normTol, int normItMax,
                       int normNbInit, double *rA, double *rAA, double *rY, double *L,
                       double *Leq);
/* pfdr_cp_reduce_* for N > 0 with A in CSC (pfdr_csc above; its arrays host
 * or device per mem, copied in and checked as pfdr_session_create_sparse
 * checks them, except that a column of squared norm 0 is accepted, as the
 * dense entry accepts it).  rA stays dense (N-by-rV reals must fit in device
 * memory; failing that is PFDR_ERR_HIP as for the dense entry): each element
 * is the sum of the stored entries A[n, Vc[i]] over the component's range of
 * Vc, i ascending, from +0, which is the dense entry's sum without its +-0
 * terms.  Every output therefore has the bytes pfdr_cp_reduce_* gives on the
 * densified matrix, for any partition and either preAt.  No floating atomics:
 * the same bytes on every run.  N <= 0, a NULL pfdr_csc or array in it, nnz
 * outside [1, 2^31 - 256): PFDR_ERR_ARG before any device work; a malformed
 * colptr or rowidx: PFDR_ERR_ARG naming the offence. */
int pfdr_cp_reduce_csc_f32(int N, int V, const pfdr_csc *A, const float *Y, int rV,
                           const int *rVc, const int *Vc, int preAt, int mem, float normTol,
                           int normItMax, int normNbInit, float *rA, float *rAA, float *rY,
                           float *L, float *Leq);
int pfdr_cp_reduce_csc_f64(int N, int V, const pfdr_csc *A, const double *Y, int rV,
                           const int *rVc, const int *Vc, int preAt, int mem, double normTol,
                           int normItMax, int normNbInit, double *rA, double *rAA, double *rY,
                           double *L, double *Leq);
/* pfdr_cp_reduce_csc_* at preAt = 0 with the reduced operator rA returned as
 * a CSC and never densified: *rnnz entries (host scalar), rcolptr[rV + 1],
 * rrowidx and rval (capacity A->nnz each; host or device per mem, allocated
 * by the caller), columns = components, rows strictly ascending inside a
 * column.  A pair (n, rv) is stored iff A stores some entry A[n, v] with v in
 * component rv, whatever the sum comes to (a sum that cancels is a stored
 * zero), so *rnnz <= A->nnz and the structure depends on A's structure and the
 * partition only.  Every value is the sum of the stored entries A[n, Vc[i]]
 * over the component's range of Vc, i ascending, from +0: the bytes of the
 * dense rA's element, also after the equilibration's divide-and-multiply
 * round trip, which the values go through element by element.  Leq = l, the
 * column norms over the stored entries in ascending row order, has the dense
 * entry's bytes as well.  L = l (l c), where c is the squared norm of rA with
 * every column divided by its l, by the power method of
 * pfdr_operator_norm_csc_* on those entries (normTol, normItMax, normNbInit
 * as passed); the dense entry's c comes from its own power method, so the two
 * L agree to the power methods' tolerance, not to the bit.  A reduced column
 * of norm 0 (or not finite) is PFDR_ERR_ARG naming rv: a sparse session
 * refuses such a column.  The argument checks are pfdr_cp_reduce_csc_*'s, and
 * rnnz, rcolptr, rrowidx and rval are required.  No floating atomics: the same
 * bytes on every run. */
int pfdr_cp_reduce_csc_sparse_f32(int N, int V, const pfdr_csc *A, const float *Y, int rV,
                                  const int *rVc, const int *Vc, int mem, float normTol,
                                  int normItMax, int normNbInit, int64_t *rnnz,
                                  int64_t *rcolptr, int32_t *rrowidx, float *rval, float *L,
                                  float *Leq);
int pfdr_cp_reduce_csc_sparse_f64(int N, int V, const pfdr_csc *A, const double *Y, int rV,
                                  const int *rVc, const int *Vc, int mem, double normTol,
                                  int normItMax, int normNbInit, int64_t *rnnz,
                                  int64_t *rcolptr, int32_t *rrowidx, double *rval, double *L,
                                  double *Leq);
/* pfdr_cp_reduce_csc_* at preAt = 1 without the dense rA: rA is the CSC of
 * pfdr_cp_reduce_csc_sparse_* (not scaled: the premultiplied branch leaves rA
 * as summed), and rAA = rA^t rA (rV * rV, both triangles) and rY = rA^t Y (rV)
 * are summed over its stored entries.  rAA[rv + rV ru] adds, for the rows
 * stored in both columns in ascending order, the products rounded one by one,
 * from +0, and is +0 where the columns share no row; rY[rv] adds val * Y[row]
 * over column rv's entries in the same way.  The terms left out are +-0 added
 * to sums that started at +0, so while the values are finite rAA, rY, Leq
 * (the roots of rAA's diagonal) and L (the power method of pfdr_cp_reduce_* on
 * the equilibrated rAA, then the same revert) have the bytes of
 * pfdr_cp_reduce_csc_* at preAt = 1.  This holds up to rV * rV * N / 2 = 2^34
 * multiply-adds: above it the dense entry forms rAA on the matrix cores and
 * the two agree to that Gram's tolerance only; this entry keeps the
 * reference's order at every size.  Device memory: the entries and rV * rV
 * reals, never N * rV; no floating atomics, the same bytes on every run.
 * PFDR_CP_GRAM_WINDOW (rows, >= 1; read at every call) shortens the window of
 * rows that the Gram kernel holds in LDS, for tests; it changes no byte.
 * rAA and rY are required, L and Leq may be NULL; rnnz, rcolptr, rrowidx and
 * rval are all NULL or all set, with the capacities of
 * pfdr_cp_reduce_csc_sparse_*.  A column of norm 0 is accepted, as the dense
 * entry accepts it.  The argument and CSC checks are pfdr_cp_reduce_csc_*'s;
 * arrays host or device per mem. */
int pfdr_cp_reduce_csc_sparse_preAt_f32(int N, int V, const pfdr_csc *A, const float *Y, int rV,
                                        const int *rVc, const int *Vc, int mem, float normTol,
                                        int normItMax, int normNbInit, float *rAA, float *rY,
                                        float *L, float *Leq, int64_t *rnnz, int64_t *rcolptr,
                                        int32_t *rrowidx, float *rval);
int pfdr_cp_reduce_csc_sparse_preAt_f64(int N, int V, const pfdr_csc *A, const double *Y, int rV,
                                        const int *rVc, const int *Vc, int mem, double normTol,
                                        int normItMax, int normNbInit, double *rAA, double *rY,
                                        double *L, double *Leq, int64_t *rnnz, int64_t *rcolptr,
                                        int32_t *rrowidx, double *rval);

/* ------------------------------------------- cut-pursuit graph steps -- */
/* The full-graph work of every cut-pursuit iteration around the reduced
 * PFDR solve, on a device-resident graph
 * (reference src/CP_PFDR_graph_quadratic_d1_l1.cpp; the cut is
 * pfdr_cpgraph_mincut below, or the caller's own maxflow: capacities out,
 * segments 0 = SOURCE / 1 = SINK back).  The
 * graph holds the endpoints, TV weights La_d1[E], l1 weights La_l1[V] (or
 * NULL), the activity of every edge (CP's is_active, initially none), the
 * components (Cv[V], Vc[V], rVc[rV + 1], initially one) and the component
 * values rX[rV].  Every result equals the reference's, including its
 * orders (queue order of Vc, visiting order of the reduced edges) and its
 * floating sums.  dtype PFDR_F32 / PFDR_F64 fixes the real type of every
 * void* below; mem = PFDR_MEM_HOST / _DEVICE for the caller's arrays. */
typedef struct pfdr_cpgraph pfdr_cpgraph;
int pfdr_cpgraph_create(pfdr_cpgraph **out, int dtype, int V, int E,
    const int *Eu, const int *Ev, const void *La_d1, const void *La_l1, int mem);
void pfdr_cpgraph_destroy(pfdr_cpgraph *g);
int pfdr_cpgraph_set_active(pfdr_cpgraph *g, const uint8_t *active, int mem);
int pfdr_cpgraph_get_active(pfdr_cpgraph *g, uint8_t *active, int mem);
int pfdr_cpgraph_set_components(pfdr_cpgraph *g, int rV, const int *Cv,
    const int *Vc, const int *rVc, int mem);
/* any output may be NULL */
int pfdr_cpgraph_get_components(pfdr_cpgraph *g, int *rV, int *Cv, int *Vc,
    int *rVc, int mem);
/* rX[rV]: the values of the current components */
int pfdr_cpgraph_set_values(pfdr_cpgraph *g, const void *rX, int mem);
/* connected components of the graph minus its active edges (:566-597) */
int pfdr_cpgraph_components(pfdr_cpgraph *g, int *rV);
/* reduced edges and weights of the current components (:599-661); eps is
 * CP's (:236-251), the weight of an isolated component's self-loop */
int pfdr_cpgraph_reduced_graph(pfdr_cpgraph *g, double eps, int *rE);
/* rEu, rEv, rLa_d1 [rE], rLa_l1 [rV] (when La_l1); any may be NULL */
int pfdr_cpgraph_get_reduced(pfdr_cpgraph *g, int *rEu, int *rEv,
    void *rLa_d1, void *rLa_l1, int mem);
/* deactivate the active edges whose components' values differ by at most
 * CP_difTol relatively (:863-886) */
int pfdr_cpgraph_merge(pfdr_cpgraph *g, double eps, double CP_difTol, int *deactivated);
/* DfS[V] (kept on the device; copied out when DfS != NULL) at the current
 * values (:339-413): N > 0: A N-by-V, R[N] the residual Y - A X; N = -V:
 * A = A^tA, Y = A^tY; N = 0: A diagonal or NULL, Y = A^tY */
int pfdr_cpgraph_gradient(pfdr_cpgraph *g, int N, const void *A, const void *Y,
    const void *R, int mem, void *DfS);
/* The N > 0 case with A in CSC (val of the graph's real type; A and R host or
 * device per mem; checked as pfdr_cp_reduce_csc_* checks it): -A^t R adds each
 * column's products val[e] R[rowidx[e]] in stored order, the dense call's sum
 * without its +-0 terms, so DfS has the dense call's bytes on the densified
 * matrix while R is finite. */
int pfdr_cpgraph_gradient_csc(pfdr_cpgraph *g, int N, const pfdr_csc *A, const void *R,
    int mem, void *DfS);
/* cut 0: the single cut of the differentiable case (La_l1 NULL, no
 * positivity); 1 / 2: directions +1_U / -1_U (:402-535).  tr_cap[V]
 * (source > 0 / sink < 0), r_cap[E] (both arcs of an edge), from the
 * activity BEFORE this cut's activations; either may be NULL */
int pfdr_cpgraph_capacities(pfdr_cpgraph *g, int cut, int positivity,
    void *tr_cap, void *r_cap, int mem);
/* the same for CP_PFDR_graph_quadratic_d1_bounds (graph created without
 * La_l1): cut 0 when min = -inf and max = inf; cut 1 (+1_U): +inf on the
 * components at max, else DfS; cut 2 (-1_U): +inf on the components at min,
 * else -DfS (src/CP_PFDR_graph_quadratic_d1_bounds.cpp:386-534) */
int pfdr_cpgraph_capacities_bounds(pfdr_cpgraph *g, int cut, double min, double max,
    void *tr_cap, void *r_cap, int mem);
/* activate the inactive edges whose ends lie in different segments[V] */
int pfdr_cpgraph_activate(pfdr_cpgraph *g, const uint8_t *segment, int mem,
    int *activated);

/* The cut of capacities tr_cap[V] (> 0 source, < 0 sink, may be infinite)
 * and r_cap[E] (finite, >= 0) as the capacities entries above and the
 * simplex driver's produce them, real type the graph's, host or device per
 * mem.  segment[V] (in mem): 0 = SOURCE exactly for the vertices reachable
 * from the source in the residual graph of a maximum flow, the set the
 * reference's Boykov-Kolmogorov maxflow returns; 1 = SINK.  Synchronous
 * push-relabel on the device, no floating atomics: the same inputs give the
 * same bytes on every run.  flow (may be NULL): the value of the cut, summed
 * in f64; rounds (may be NULL): push/relabel rounds run.  Uses the endpoints
 * and the incidence lists only: activity, components and values are neither
 * read nor changed.  NaN in tr_cap, negative, NaN or infinite r_cap:
 * PFDR_ERR_ARG. */
#define PFDR_ARCS_BOTH 0      /* r_cap[e] is the capacity of both arcs of edge e (l1, bounds drivers) */
#define PFDR_ARCS_FORWARD 1   /* r_cap[e] is arc Eu[e] -> Ev[e]; the reverse arc has none (simplex driver) */
int pfdr_cpgraph_mincut(pfdr_cpgraph *g, int arcs, const void *tr_cap, const void *r_cap,
                        int mem, uint8_t *segment, double *flow, int64_t *rounds);
/* global relabels (breadth-first labellings) of the last cut on g */
int pfdr_cpgraph_mincut_relabels(pfdr_cpgraph *g, int64_t *relabels);

/* The duplex driver, CP_PFDR_graph_quadratic_d1_l1_duplex, in its
 * non-differentiable case (graph created with La_l1; positivity optional):
 * one cut per iteration on a two-layer maxflow graph, node v (v1) and node
 * V + v (v2) per vertex (src/CP_PFDR_graph_quadratic_d1_l1_duplex.cpp:101-116).
 * The gradient is pfdr_cpgraph_gradient's.  tr_cap[2V] (v1 nodes, then v2),
 * r_link[V] (arc v1 -> v2; v2 -> v1 has none), r_cap[E] (every arc of edge
 * e, both layers) from the activity before the cut (:469-527); any may be
 * NULL.  Activation: edges separated in either layer, segment[2V]
 * (:531-545).  The components, reduced graph and merge are the l1 driver's.
 * (Its differentiable case indexes La_d1 as if its one-layer graph had four
 * arcs per edge, :407 / :628 -- not reproduced.) */
int pfdr_cpgraph_capacities_duplex(pfdr_cpgraph *g, int positivity, void *tr_cap,
    void *r_link, void *r_cap, int mem);
int pfdr_cpgraph_activate_duplex(pfdr_cpgraph *g, const uint8_t *segment, int mem,
    int *activated);
/* The duplex driver's cut.  Node v (v1) and node V + v (v2) per vertex;
 * tr_cap[2V] (> 0 source, < 0 sink, may be infinite), r_link[V]: arc v1 -> v2
 * (v2 -> v1 has none), r_cap[E]: both arcs of edge e in both layers; finite,
 * >= 0.  segment[2V]: 0 = SOURCE exactly for the nodes reachable from the
 * source in the residual graph of a maximum flow (the reference's BK answer
 * on the graph of :101-116), 1 = SINK.  pfdr_cpgraph_mincut's contract
 * otherwise: host or device memory per mem, the same bytes on every run, flow
 * (the cut's value: terminals, r_cap once per layer, links) summed in f64 in
 * a fixed order, flow and rounds optional, only the endpoints are read.  The
 * rounds are pfdr_cpgraph_mincut's own kernels over a CSR of 2V nodes and
 * 2E + V edges, built by the graph's first two-layer cut and kept with it.
 * A NaN terminal, a negative, NaN or infinite r_cap or r_link, or
 * 2 (2E + V) > INT_MAX (the CSR's offsets are int): PFDR_ERR_ARG.
 * pfdr_cpgraph_mincut_relabels reports the last cut of either kind. */
int pfdr_cpgraph_mincut_duplex(pfdr_cpgraph *g, const void *tr_cap, const void *r_link,
                               const void *r_cap, int mem, uint8_t *segment,
                               double *flow, int64_t *rounds);

/* The simplex driver, CP_PFDR_graph_loss_d1_simplex (graph created
 * without La_l1): K >= 2 labels, Q[V*K] and the component label vectors
 * rP[rV*K] vertex-major like the reference (P[v*K + k]); al = 0 linear,
 * 1 quadratic, (0, 1) smoothed-KL loss.  One CP iteration: gradient ->
 * for n = 1 .. K-1 { capacities(n) -> mincut (PFDR_ARCS_FORWARD) -> expand(n,
 * segments) } -> activate -> pfdr_cpgraph_components -> reduced_graph ->
 * observations (the reduced problem's rQ, rLa_f and warm start rP) ->
 * PFDR_graph_loss_d1_simplex -> set_values -> merge.  eps: the driver's
 * finite-difference precision (src/CP_PFDR_graph_loss_d1_simplex.cpp:214-231).
 * Replaces :327-376 (gradient), :525-536 (most confident labels),
 * :542-604 (alpha-expansion capacities and labels), :608-618 (activation),
 * :733-766 (reduced observations) and :782-803 (merge). */
int pfdr_cpgraph_simplex_setup(pfdr_cpgraph *g, int K, double al, const void *Q, int mem);
/* per component the sums of Q in Vc order; linear: rQ = sums, rP = corner
 * of the first largest; else rQ = rP = sums / size, rLa_f[rV] = size.  The
 * component values become rP.  Any output may be NULL; also gives the
 * initial values of the one-component state (:96-108) */
int pfdr_cpgraph_simplex_observations(pfdr_cpgraph *g, void *rP, void *rQ, void *rLa_f,
    int mem);
/* rP[rV*K]: the label vectors of the current components (PFDR's output) */
int pfdr_cpgraph_simplex_set_values(pfdr_cpgraph *g, const void *rP, int mem);
/* DfS[V*K] and rDi[rV] (most confident label per component), kept on the
 * device (copied out when not NULL); resets every vertex's alternative */
int pfdr_cpgraph_simplex_gradient(pfdr_cpgraph *g, double eps, void *DfS, int *rDi, int mem);
/* alpha-expansion n in [1, K): tr_cap[V] and r_cap[E], the capacity of arc
 * 2e (Eu -> Ev); arc 2e + 1 has none (:563-595) */
int pfdr_cpgraph_simplex_capacities(pfdr_cpgraph *g, int n, void *tr_cap, void *r_cap,
    int mem);
/* the SINK side of expansion n's maxflow takes alternative n (:600-604) */
int pfdr_cpgraph_simplex_expand(pfdr_cpgraph *g, int n, const uint8_t *segment, int mem);
int pfdr_cpgraph_simplex_activate(pfdr_cpgraph *g, int *activated);
/* deactivate the active edges whose components' label vectors differ by
 * at most eps in every label */
int pfdr_cpgraph_simplex_merge(pfdr_cpgraph *g, double eps, int *deactivated);
/* Djv[V]: every vertex's alternative after the expansions so far */
int pfdr_cpgraph_simplex_labels(pfdr_cpgraph *g, int *Djv, int mem);

/* -------------------------------------------------- whole cut pursuit -- */
/* CP_PFDR_graph_quadratic_d1_l1<real> of the reference (arguments as
 * include/CP_PFDR_graph_quadratic_d1_l1.hpp:52-61; the restart record is
 * pfdr_cp_solver_* below), the loop above with pfdr_cpgraph_mincut and the
 * PFDR solver,
 * everything resident on the current device: host arrays come in once, Cv[V]
 * and rX[*rV] (capacity V) go out once.  N > 0: A N-by-V column major, Y[N];
 * N = -V: A = A^tA, Y = A^tY; N = 0: A diagonal or NULL, Y = A^tY.  La_l1
 * may be NULL.  Time[CP_itMax + 1] (seconds), Obj[CP_itMax + 1],
 * Dif[CP_itMax] and CP_it may be NULL.  The iterate evolution and the
 * stopping rule (dif < CP_difTol^2) are the reference's. */
int pfdr_cp_quadratic_d1_l1_f32(int V, int E, int N, int *rV, int *Cv, float *rX,
    const float *Y, const float *A, const int *Eu, const int *Ev, const float *La_d1,
    const float *La_l1, int positivity, float CP_difTol, int CP_itMax, int *CP_it,
    float rho, float condMin, float difRcd, float difTol, int itMax,
    double *Time, float *Obj, float *Dif, int verbose);
int pfdr_cp_quadratic_d1_l1_f64(int V, int E, int N, int *rV, int *Cv, double *rX,
    const double *Y, const double *A, const int *Eu, const int *Ev, const double *La_d1,
    const double *La_l1, int positivity, double CP_difTol, int CP_itMax, int *CP_it,
    double rho, double condMin, double difRcd, double difTol, int itMax,
    double *Time, double *Obj, double *Dif, int verbose);

/* CP_PFDR_graph_quadratic_d1_l1_duplex<real> of the reference (arguments as
 * include/CP_PFDR_graph_quadratic_d1_l1.hpp:133-142; the restart record is
 * pfdr_cp_solver_* below): pfdr_cp_quadratic_d1_l1's loop with one two-layer
 * cut per
 * iteration in place of its two cuts -- gradient,
 * pfdr_cpgraph_capacities_duplex, pfdr_cpgraph_mincut_duplex,
 * pfdr_cpgraph_activate_duplex -- and everything else (initialisation, eps,
 * the iteration that activates nothing, the reduced problem, PFDR from zero,
 * merge, residual, iterate evolution, objective, stopping rule, argument
 * checks, NULL outputs) that entry's, resident on the device in the same way.
 * Two corners the reference leaves undefined:
 *  - differentiable case (no La_l1, no positivity): the reference builds the
 *    one-layer graph but indexes it as if it had four arcs per edge (:407,
 *    :628, :869); not reproduced.  The entry runs the l1 driver's single-cut
 *    path: the result equals pfdr_cp_quadratic_d1_l1's byte for byte.
 *  - positivity without La_l1: the reference reads the up / down directional
 *    derivatives from uninitialised memory (:470-502); here both are the
 *    gradient (pfdr_cpgraph_capacities_duplex).
 * verbose prints what pfdr_cp_quadratic_d1_l1 prints. */
int pfdr_cp_quadratic_d1_l1_duplex_f32(int V, int E, int N, int *rV, int *Cv, float *rX,
    const float *Y, const float *A, const int *Eu, const int *Ev, const float *La_d1,
    const float *La_l1, int positivity, float CP_difTol, int CP_itMax, int *CP_it,
    float rho, float condMin, float difRcd, float difTol, int itMax,
    double *Time, float *Obj, float *Dif, int verbose);
int pfdr_cp_quadratic_d1_l1_duplex_f64(int V, int E, int N, int *rV, int *Cv, double *rX,
    const double *Y, const double *A, const int *Eu, const int *Ev, const double *La_d1,
    const double *La_l1, int positivity, double CP_difTol, int CP_itMax, int *CP_it,
    double rho, double condMin, double difRcd, double difTol, int itMax,
    double *Time, double *Obj, double *Dif, int verbose);
/* Where the calling thread's last pfdr_cp_quadratic_d1_l1_duplex_* call spent
 * its time; the layout of pfdr_cp_quadratic_d1_bounds_stats: seconds[6] =
 * gradient, the cuts (capacities, cut, activation), the other graph steps and
 * the reduction, PFDR, the evolution / objective sums, the whole call;
 * counts[4] = cuts, push/relabel rounds, global relabels, PFDR iterations.
 * Either output may be NULL. */
int pfdr_cp_quadratic_d1_l1_duplex_stats(double *seconds, int64_t *counts);

/* CP_PFDR_graph_quadratic_d1_bounds<real> of the reference (arguments as
 * include/CP_PFDR_graph_quadratic_d1_bounds.hpp; the restart record is
 * pfdr_cp_solver_* below):
 * the same loop for the box min <= x <= max (+-HUGE_VAL: no bound) -- the
 * one-component least-squares value projected onto the box, one cut when
 * there is no bound and two otherwise (pfdr_cpgraph_capacities_bounds,
 * pfdr_cpgraph_mincut with PFDR_ARCS_BOTH), the reduced problem solved by the
 * bounds PFDR from zero -- everything resident on the current device: host
 * arrays come in once, Cv[V] and rX[*rV] (the caller's, capacity V) go out
 * once, and in between only scalars cross to the host.  N, A, Y, Time, Obj,
 * Dif and CP_it as pfdr_cp_quadratic_d1_l1; every scalar sum is added one by
 * one in the reference's order.  One departure: min > max or a NaN bound is
 * PFDR_ERR_ARG (the reference clamps to min and hands PFDR an empty box).
 * V <= 0, E < 0, CP_itMax < 0, a missing required pointer, N != 0 without A or
 * N < 0 with -N != V: PFDR_ERR_ARG before any device work.  min == max, E = 0
 * and V = 1 are valid. */
int pfdr_cp_quadratic_d1_bounds_f32(int V, int E, int N, int *rV, int *Cv, float *rX,
    const float *Y, const float *A, const int *Eu, const int *Ev, const float *La_d1,
    float min, float max, float CP_difTol, int CP_itMax, int *CP_it,
    float rho, float condMin, float difRcd, float difTol, int itMax,
    double *Time, float *Obj, float *Dif, int verbose);
int pfdr_cp_quadratic_d1_bounds_f64(int V, int E, int N, int *rV, int *Cv, double *rX,
    const double *Y, const double *A, const int *Eu, const int *Ev, const double *La_d1,
    double min, double max, double CP_difTol, int CP_itMax, int *CP_it,
    double rho, double condMin, double difRcd, double difTol, int itMax,
    double *Time, double *Obj, double *Dif, int verbose);
/* Where the calling thread's last pfdr_cp_quadratic_d1_bounds_* call spent
 * its time (host clock around synchronous steps; either output may be NULL):
 * seconds[6] = gradient, the cuts (capacities, cut, activation), the other
 * graph steps and the reduction, PFDR, the evolution / objective sums, the
 * whole call; counts[4] = cuts, push/relabel rounds and global relabels over
 * all of them, PFDR iterations over all reduced problems. */
int pfdr_cp_quadratic_d1_bounds_stats(double *seconds, int64_t *counts);

/* CP_PFDR_graph_loss_d1_simplex<real> of the reference (arguments as
 * include/CP_PFDR_graph_loss_d1_simplex.hpp:41-48; the restart record is
 * pfdr_cp_solver_* below): the simplex driver's loop above -- gradient, K - 1
 * alpha-expansions
 * with pfdr_cpgraph_mincut (PFDR_ARCS_FORWARD), activation, components,
 * reduced graph, observations, the simplex PFDR solver from the components'
 * own optima, merge -- everything resident on the current device: host arrays
 * come in once, Cv[V] and rP go out once, and in between only scalars cross
 * to the host.  Q[V*K] and rP vertex-major like the reference (Q[v*K + k],
 * rP[rv*K + k]); rP is the caller's, capacity K*V, and receives K * (*rV)
 * values.  al = 0 linear, 1 quadratic, (0, 1) smoothed-KL loss.
 * Time[CP_itMax + 1] (seconds), Obj[CP_itMax + 1], Dif[CP_itMax] and CP_it may
 * be NULL.  The iterate evolution (mean l1 change of the label vectors for
 * CP_difTol < 1, the count of vertices whose first-largest label changed for
 * CP_difTol >= 1), the stopping rule (dif < CP_difTol) and the driver's eps
 * (:214-231 as compiled) are the reference's, every sum in its order.
 * Two departures: Obj[0] is the functional at the one-component solution, by
 * the formulas of every later Obj[k] (the reference's initialize() :119-146
 * does not evaluate the functional for al != 0; for al = 0 the values agree);
 * al < 0 or al > 1 is PFDR_ERR_ARG (the reference then reads constants it
 * never set).  K < 2, V <= 0, E < 0, CP_itMax < 0 or a missing required
 * pointer: PFDR_ERR_ARG before any device work.  E = 0 and V = 1 are valid. */
int pfdr_cp_loss_d1_simplex_f32(int K, int V, int E, float al, int *rV, int *Cv, float *rP,
    const float *Q, const int *Eu, const int *Ev, const float *La_d1,
    float CP_difTol, int CP_itMax, int *CP_it,
    float rho, float condMin, float difRcd, float difTol, int itMax,
    double *Time, float *Obj, float *Dif, int verbose);
int pfdr_cp_loss_d1_simplex_f64(int K, int V, int E, double al, int *rV, int *Cv, double *rP,
    const double *Q, const int *Eu, const int *Ev, const double *La_d1,
    double CP_difTol, int CP_itMax, int *CP_it,
    double rho, double condMin, double difRcd, double difTol, int itMax,
    double *Time, double *Obj, double *Dif, int verbose);
/* Where the calling thread's last pfdr_cp_loss_d1_simplex_* call spent its
 * time (host clock around synchronous steps; any output may be NULL):
 * seconds[6] = gradient, the K - 1 cuts (capacities, cut, expansion), the
 * other graph steps, PFDR, the evolution / objective sums, the whole call;
 * counts[4] = expansions, push/relabel rounds and global relabels over all of
 * them, PFDR iterations over all reduced problems; exp_rounds / exp_relabels
 * [n_exp]: the same per expansion in call order, for the first 64 (-1 past
 * the last one run or kept). */
int pfdr_cp_loss_d1_simplex_stats(double *seconds, int64_t *counts, int64_t *exp_rounds,
    int64_t *exp_relabels, int n_exp);

/* ------------------------------------------- resumable cut pursuit -- */
/* The restart record of the reference's drivers (CP_restart, their last
 * argument) as a handle: the problem, its pfdr_cpgraph and the cut-pursuit
 * state stay on the device between calls.  create is the setup of the matching
 * one-call entry (upload, graph, the reference's initialize()) and leaves the
 * one-component state; the first run equals that entry byte for byte, Obj[0]
 * included.  Every later run, and every run after set_state / set_partition /
 * set_penalties, is the reference's warm restart
 * (src/CP_PFDR_graph_quadratic_d1_l1.cpp:293-319): the iteration counter starts
 * at 0, dif at max(CP_difTol^2, 1) (simplex: max(CP_difTol, 1)), the first
 * preAt decision of N > 0 is taken with PFDR_itMax, the state is its own
 * previous iterate, Time counts from the call.  So a resumed run iterates
 * again even when the last one stopped on dif.  Obj[0] of a resumed run is the
 * last Obj this handle computed (the reference leaves it unwritten); after
 * set_state, set_partition, set_penalties, or a run without Obj, it is NaN. */
typedef struct pfdr_cp_problem {
    int kind;             /* PFDR_KIND_L1 / PFDR_KIND_BOUNDS / PFDR_KIND_SIMPLEX */
    int duplex;           /* PFDR_KIND_L1 only: the duplex driver */
    int dtype;            /* PFDR_F32 / PFDR_F64: type of every real array */
    int mem;              /* PFDR_MEM_*: location of every array below.  Device
                             arrays are copied, except A, which is borrowed: it
                             must stay valid and unchanged until destroy */
    int V, E, N, K;       /* as the entries (K only for the simplex, N not) */
    const void *Y;        /* Y / A^tY, or Q[V*K] for the simplex */
    const void *A;        /* as the entries; NULL for identity */
    const int *Eu, *Ev;
    const void *La_d1;    /* length E */
    const void *La_l1;    /* length V or NULL (PFDR_KIND_L1 only) */
    int positivity;       /* PFDR_KIND_L1 only */
    double min, max;      /* PFDR_KIND_BOUNDS only (+-HUGE_VAL for none) */
    double al;            /* simplex only */
} pfdr_cp_problem;

typedef struct pfdr_cp_params {
    double CP_difTol;
    int CP_itMax;
    double rho, condMin, difRcd, difTol;
    int itMax;
    int verbose;
} pfdr_cp_params;

typedef struct pfdr_cp_solver pfdr_cp_solver;

/* Argument errors are the matching entry's, before any device work. */
int pfdr_cp_solver_create(pfdr_cp_solver **out, const pfdr_cp_problem *p);
/* The same with the observation operator A (p->N-by-p->V, p->N > 0) in CSC;
 * kinds PFDR_KIND_L1 (duplex or not) and PFDR_KIND_BOUNDS.  A's arrays are
 * host or device per p->mem and are copied (the dense p->A is borrowed).  Cut
 * pursuit reads the full-size A in three places -- initialize()'s column sum,
 * pfdr_cp_reduce's component column sums and the gradient -A^t R -- and those
 * walk the stored entries in the dense loops' order; the reduced matrix stays
 * dense (p->N * rV reals; pfdr_cp_solver_set_reduced below keeps it sparse
 * instead) and the rest of the loop is the dense solver's code.
 * Every run, state and statistic therefore equals, byte for byte, those of
 * pfdr_cp_solver_create on the densified matrix, and every other
 * pfdr_cp_solver_* call works on the handle unchanged.  PFDR_ERR_ARG before
 * any device work: p->N <= 0; p->A set as well; the simplex kind; a NULL A or
 * array in it; nnz outside [1, 2^31 - 256).  A malformed colptr or rowidx
 * (as for pfdr_session_create_sparse; a column of squared norm 0 is accepted,
 * as the dense solver accepts it) is PFDR_ERR_ARG naming the offence, and no
 * handle is created. */
int pfdr_cp_solver_create_sparse(pfdr_cp_solver **out, const pfdr_cp_problem *p,
                                 const pfdr_csc *A);
/* How a solver created by pfdr_cp_solver_create_sparse keeps the reduced
 * operator rA of an iteration that works on rA directly (the reference's
 * branch without premultiplication, taken when rV >= 2 N pit / (N + pit), pit
 * the previous PFDR iteration count).  PFDR_REDUCED_DENSE, the default: N * rV
 * reals, every byte as documented above.  PFDR_REDUCED_SPARSE: rA is the CSC
 * of pfdr_cp_reduce_csc_sparse_* with its CSR view, built on the device; the
 * N * rV array is never allocated, PFDR runs as a sparse session on it
 * (pfdr_session_create_sparse, device arrays) and the residual walks its
 * rows.  rA's values, l and the residual keep the dense mode's bytes; L and
 * the PFDR iterates follow another power method's estimate of c and another
 * session, so a run agrees with the dense mode's to the solvers' tolerances
 * and equals, byte for byte, the same steps composed through the public
 * entries.  An iteration whose rA has a column of norm 0 (or not finite)
 * takes the dense branch, and premultiplied iterations are the dense mode's
 * in either mode.  With R = NULL, pfdr_cp_solver_set_state and
 * pfdr_cp_solver_set_partition recompute R over the stored entries: the same
 * bytes.  May be called between runs; the state is kept.  PFDR_ERR_ARG naming
 * the offence: a solver not created by pfdr_cp_solver_create_sparse, the
 * simplex kind, an unknown mode.
 * PFDR_REDUCED_SPARSE_ALL: direct iterations as under PFDR_REDUCED_SPARSE (the
 * dense fallback for a column of norm 0 included), and the premultiplied
 * iterations (p->N > 0) keep rA sparse as well: rAA = rA^t rA and rY = rA^t Y
 * are summed over its stored entries (pfdr_cp_reduce_csc_sparse_preAt_*), PFDR
 * runs on (rAA, rY) as in the dense mode and the residual walks rA's rows.
 * The N * rV array is then allocated by the zero-norm fallback only.  A
 * premultiplied iteration keeps the dense mode's bytes -- L, the iterates and
 * the residual -- while rV * rV * N / 2 <= 2^34 (above it the dense mode's
 * Gram leaves the reference's order and this one does not), so a run whose
 * iterations are all premultiplied equals the dense mode's byte for byte. */
#define PFDR_REDUCED_DENSE 0
#define PFDR_REDUCED_SPARSE 1
#define PFDR_REDUCED_SPARSE_ALL 2
int pfdr_cp_solver_set_reduced(pfdr_cp_solver *s, int mode);
/* Of the last run, any may be NULL: the iterations solved on a sparse rA, the
 * direct iterations solved on a dense one (all of them in the dense mode, the
 * zero-norm fallbacks in the sparse mode), the most entries a sparse rA held. */
int pfdr_cp_solver_reduced_stats(pfdr_cp_solver *s, int64_t *sparse_iterations,
                                 int64_t *dense_direct_iterations, int64_t *max_rnnz);
/* The same of the last run's premultiplied iterations with p->N > 0 (the
 * counts above are of the direct ones only), any may be NULL: those solved
 * from the stored entries of a sparse rA (PFDR_REDUCED_SPARSE_ALL), those that
 * formed the dense N * rV array (every one in the other two modes), the most
 * entries such a sparse rA held. */
int pfdr_cp_solver_premultiplied_stats(pfdr_cp_solver *s, int64_t *sparse_iterations,
                                       int64_t *dense_iterations, int64_t *max_rnnz);
void pfdr_cp_solver_destroy(pfdr_cp_solver *s);
/* Host outputs, any may be NULL: Time[CP_itMax + 1], Obj[CP_itMax + 1],
 * Dif[CP_itMax] of the solver's real type. */
int pfdr_cp_solver_run(pfdr_cp_solver *s, const pfdr_cp_params *q, int *CP_it,
                       double *Time, void *Obj, void *Dif);
/* The state, any output may be NULL, host or device per mem: Cv[V], Vc[V],
 * rVc[*rV + 1] (capacity V + 1), active[E], rX[*rV] (capacity V; simplex
 * rP[*rV * K] vertex-major, capacity K V), R[N] = Y - A X (N > 0 only). */
int pfdr_cp_solver_get_state(pfdr_cp_solver *s, int *rV, int *Cv, int *Vc, int *rVc,
                             uint8_t *active, void *rX, void *R, int mem);
/* Replaces the state after checking it on the device (only a flag word comes
 * back): 1 <= rV <= V; rVc[0] = 0, rVc[rV] = V, strictly increasing; Vc a
 * permutation of [0, V); Cv[Vc[i]] the component whose range holds i;
 * active[e] 0 or 1; no NaN in rX or R; bounds: rX within [min, max].  A failed
 * check is PFDR_ERR_ARG naming it, and the solver is left as it was.
 * R = NULL (N > 0): recomputed in the reference's order (:889-901) by the
 * loop's own kernels, pfdr_cp_reduce's component column sums without
 * premultiplication and the loop's residual kernel: the bytes the loop holds
 * after an iteration that worked on rA directly.  (After a premultiplied
 * iteration the loop's R comes from column sums that were never scaled and
 * scaled back by the equilibration, and may differ in the last bit.) */
int pfdr_cp_solver_set_state(pfdr_cp_solver *s, int rV, const int *Cv, const int *Vc,
                             const int *rVc, const uint8_t *active, const void *rX,
                             const void *R, int mem);
/* A state from what the drivers return: label[V] in [0, nlabels) and
 * values[nlabels] (simplex nlabels K).  Edge e becomes active iff its ends'
 * labels differ; the components are pfdr_cpgraph_components of that activity
 * (a label class that is not connected becomes several); each takes the value
 * of the label of the first vertex of its range; R is recomputed. */
int pfdr_cp_solver_set_partition(pfdr_cp_solver *s, int nlabels, const int *label,
                                 const void *values, int mem);
/* Overwrites La_d1[E] and / or La_l1[V] (NULL: unchanged; La_l1 only if the
 * solver was created with one); negative or NaN weights are PFDR_ERR_ARG.
 * The state is kept and the next run is a restart. */
int pfdr_cp_solver_set_penalties(pfdr_cp_solver *s, const void *La_d1,
                                 const void *La_l1, int mem);
/* seconds[6] / counts[4] of the last run in pfdr_cp_quadratic_d1_bounds_stats'
 * layout (simplex: counts[0] = expansions), and the seconds create spent.
 * Any may be NULL. */
int pfdr_cp_solver_stats(pfdr_cp_solver *s, double *seconds, int64_t *counts,
                         double *setup_seconds);
/* La_d1[E] / La_l1[V] of a graph, in place (NULL: unchanged).  The graph
 * caches topology only (incidence lists, the cut's CSRs), never weights. */
int pfdr_cpgraph_set_weights(pfdr_cpgraph *g, const void *La_d1, const void *La_l1, int mem);
/* active[e] = (label[Eu[e]] != label[Ev[e]]), label[V] any ints */
int pfdr_cpgraph_set_active_by_labels(pfdr_cpgraph *g, const int *label, int mem);

/* ------------------------------------------------------ multi-GPU comm -- */
/* Partitioned sessions (quadratic solvers, identity or diagonal A): every
 * rank passes its owned vertices (V of them, global ids [vtx_begin,
 * vtx_begin + V), ranks in vertex order) and its edges (global endpoint ids,
 * global edge ids e_global or e_offset + e).  Creation and every run() are
 * collective.  The result equals the unpartitioned solve bit for bit. */
#define PFDR_COMM_RCCL 0      /* one process per GPU, ncclComm_t */
#define PFDR_COMM_LOOPBACK 1  /* k ranks as k threads of one process, one GPU */
#define PFDR_COMM_ID_BYTES 128
/* rank 0 creates the id, the caller broadcasts it, every rank inits */
int pfdr_comm_unique_id(void *id_out /* PFDR_COMM_ID_BYTES */);
int pfdr_comm_init(void **comm_out, int nranks, int rank, const void *id);
int pfdr_comm_destroy(void *comm);
int pfdr_comm_allreduce_max_f64(void *comm, double *value);
int pfdr_loopback_create(void **hub_out, int nranks);
/* a failing rank wakes the others: their pending and later exchanges fail */
int pfdr_loopback_abort(void *hub, const char *reason);
int pfdr_loopback_destroy(void *hub);
/* Watchdog: a rank whose collective does not complete within
 * PFDR_COMM_TIMEOUT seconds (default 120) prints
 * "[pfdr watchdog] ... rank r of n, <phase>, iteration i, last collective:
 * <op, peers, bytes>" to stderr, aborts the communicator (RCCL) or the hub
 * (loopback) and fails the call with that message (no retry). */

/* Several GPUs behind the drop-in entry points (one synchronous call, one
 * host thread per device, RCCL communicators from ncclCommInitAll, created
 * once and cached across calls): the drop-in calls of this process with at
 * least min_vertices vertices (< 0: the default 2^20) are vertex-range
 * partitioned across devices[0 .. n) -- bit-identical to the one-GPU solve.
 * n = 0 returns to one GPU.  The devices must be all distinct (RCCL), or one
 * device repeated, which runs the ranks as threads on it (loopback transport;
 * for tests); a mixed list is refused and leaves the configuration as it was.
 * Without this call the PFDR_DEVICES environment variable (N or "all")
 * selects devices 0 .. N-1. */
int pfdr_set_devices(int n, const int *devices, int64_t min_vertices);

/* Host-only partition planner (what the partitioned session runs at setup;
 * exposed so the partition logic can be driven by any transport, e.g. the
 * CPU tests).  Rank `rank` owns global vertices [offsets[rank],
 * offsets[rank+1]); its E edges have global endpoints Eu/Ev and global ids
 * e_global (or e_offset + e).  Flow: create -> get PULL_REQUEST/PUSH_ITEMS
 * for every peer -> send them -> set_incoming what every peer sent ->
 * finish -> get the results.  pfdr_plan_get returns the element count and
 * copies the elements when out != NULL. */
typedef struct pfdr_plan pfdr_plan;
#define PFDR_PLAN_GHOSTS 0          /* int64 global ids of the ghost vertices */
#define PFDR_PLAN_EU_LOCAL 1        /* int32 local endpoint ids (ghosts >= V) */
#define PFDR_PLAN_EV_LOCAL 2
#define PFDR_PLAN_PULL_REQUEST 3    /* int64 ghost ids owned by `peer` */
#define PFDR_PLAN_PUSH_ITEMS 4      /* int64 (vertex, 2 e_global + side) pairs for `peer` */
#define PFDR_PLAN_PUSH_ADDR 5       /* uint32 contribution address of every item sent */
#define PFDR_PLAN_PULL_INDEX 6      /* int32 owned local ids to send, per peer */
#define PFDR_PLAN_RECV_KEYS 7       /* uint64 (local vertex << 32 | order) of items received */
#define PFDR_PLAN_GHOST_OFFSETS 8   /* int32 nranks + 1 */
#define PFDR_PLAN_PULL_OFFSETS 9    /* int32 nranks + 1, into PULL_INDEX */
#define PFDR_PLAN_PUSH_OFFSETS 10   /* int32 nranks + 1, into PUSH_ADDR */
#define PFDR_PLAN_RECV_OFFSETS 11   /* int32 nranks + 1, into RECV_KEYS */
int pfdr_plan_create(pfdr_plan **out, int nranks, int rank,
    const int64_t *offsets, int E, const int *Eu, const int *Ev,
    const int64_t *e_global, int64_t e_offset);
int64_t pfdr_plan_get(pfdr_plan *plan, int what, int peer, void *out);
int pfdr_plan_set_incoming(pfdr_plan *plan, int peer, int what, int64_t n,
    const int64_t *data);
int pfdr_plan_finish(pfdr_plan *plan);
void pfdr_plan_destroy(pfdr_plan *plan);

/* ---------------------------------------------------------- test hooks -- */
/* The per-edge-block records of the tiled edge sweep (k_edge_sweep_tl), built
 * on the device from host endpoint arrays already in tile order: blocks
 * [blk_begin, blk_begin + blk_count) of 1,024 (f32) / 512 (f64) edges are
 * written, every other record of rec (rec_ints = blocks * ints per record)
 * keeps what the caller put there -- so a test can check that building one
 * block's record touches nothing else.  Layout: pfdr_debug_erec_layout. */
int pfdr_debug_tile_erec(int64_t E, int dtype, const int *Eu, const int *Ev,
    int blk_begin, int blk_count, int *rec, int64_t rec_ints);
int pfdr_debug_erec_layout(int *ints, int *runs, int *nostage);
/* out[i] = log(x[i]) on the device, the function (and compile flags) the
 * smoothed-KL objective of pfdr_cp_loss_d1_simplex_* uses; host arrays of n
 * reals of dtype PFDR_F32 / PFDR_F64.  For the test that measures its error. */
int pfdr_debug_device_log(int dtype, int64_t n, const void *x, void *out);

/* -------------------------------------------------- synthetic inputs -- */
/* Host-side deterministic generators (no device needed), identical laws to
 * cp_pfdr_graph_d1_amd/graphs.py.  Edges are written for emitters
 * [v_begin, v_end); the k-NN graph writes exactly k*(v_end-v_begin). */
int64_t pfdr_gen_knn_jitter_grid(int nx, int ny, int nz, int k, uint64_t seed,
    double jitter, int64_t v_begin, int64_t v_end, int *Eu, int *Ev);
int64_t pfdr_gen_grid_edges(int nx, int ny, int nz, int conn,
    int64_t v_begin, int64_t v_end, int *Eu, int *Ev);
int pfdr_gen_piecewise_f32(int nx, uint64_t seed, double noise,
    int64_t v_begin, int64_t v_end, float *Y);
int pfdr_gen_piecewise_f64(int nx, uint64_t seed, double noise,
    int64_t v_begin, int64_t v_end, double *Y);
/* Dense inputs (C3): out[i] = lo + (hi-lo) U(seed, i0+i); y = A x with each
 * row accumulated in double in increasing column order (host- and
 * thread-count independent); a symmetric diagonally dominant V-by-V matrix
 * (off-diagonal s (2U - 1), diagonal d). */
int pfdr_gen_uniform_f32(uint64_t seed, int64_t i0, int64_t n, double lo, double hi,
    float *out);
int pfdr_gen_uniform_f64(uint64_t seed, int64_t i0, int64_t n, double lo, double hi,
    double *out);
int pfdr_gen_matvec_f32(int64_t N, int64_t V, const float *A, const float *x, float *y);
int pfdr_gen_matvec_f64(int64_t N, int64_t V, const double *A, const double *x, double *y);
int pfdr_gen_symmetric_f32(int64_t V, uint64_t seed, double s, double d, float *G);
int pfdr_gen_symmetric_f64(int64_t V, uint64_t seed, double s, double d, double *G);

#ifdef __cplusplus
}
#endif
#endif /* PFDR_MI355X_H */
