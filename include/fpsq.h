/*
 * fpsq.h -- C ABI of libfpsq.so: the MI355X (gfx950) back-end for the two regularised KKT saddle-point
 * solves  [I A'; A -delta I]  that FletcherPenaltySolver.jl performs on every obj/grad of FletcherPenaltyNLP.
 *
 * This is the drop-in boundary: what a `struct HIPQDSolver <: QDSolver` on the Julia side binds with `ccall`
 * (see INTEGRATION.md).  Plain C, opaque handle, plain pointers and sizes; no C++/torch types.
 * Reference = JuliaSmoothOptimizers/FletcherPenaltySolver.jl v0.3.0; citations are file:line in that repo.
 *
 * Conventions
 *   n = nvar, m = number of penalised constraints, A = constraint Jacobian (m x n), fp64 throughout.
 *   Every `double*` / index pointer argument may point to HOST or DEVICE memory; the library inspects it
 *   (hipPointerGetAttributes) and stages host data itself.  Output buffers are CALLER-owned (the reference hands
 *   out aliases of solver-owned buffers, src/solve_linear_system.jl:139; callers copy out immediately,
 *   src/model-Fletcherpenaltynlp.jl:244-248, so caller-owned outputs are equivalent and remove the aliasing).
 *   All calls are synchronous: on return the outputs are complete (the solver's stream has been synchronised).
 *   INPUT READINESS: the library works on its own non-blocking HIP stream and reads DEVICE-resident arguments in place.
 *   Device data handed to a call must therefore be complete when the call is made -- either the caller has
 *   synchronised the stream that produced it, or it has registered that stream once with fpsq_set_input_stream(): every
 *   call then first makes the solver's stream wait (event, no host block) for all work queued on the registered
 *   stream so far, which orders both the reads of device inputs and the overwriting of device output buffers that
 *   earlier kernels of that stream may still be reading.  Host-resident arguments need nothing.
 *   Since round 5 a single-GPU handle (or one whose communicator has ONE rank) does more with a registered stream: it ENQUEUES
 *   ON IT, instead of on a stream of its own (FPSQ_ADOPT_STREAM=0 keeps the own stream and the event pair) -- the inputs and the
 *   outputs are then ordered by the stream itself, and the two hops between queues that lay between the last kernel of an
 *   evaluation and the first of the next (the caller's stream waits for the tail, the library's for the caller's) are gone:
 *   ~28 us per evaluation at the headline size.  The registered stream must outlive its registration; registering another
 *   stream (or none: enabled = 0) first drains the one in use.  Handles sharded over several ranks keep their own stream.
 *   One handle is non-re-entrant, exactly like one reference QDSolver (shared mutable workspaces).
 *
 * Return codes
 *   0            success
 *   > 0          soft numerical failure, bit 0: first system `solved == false`, bit 1: second system.  The
 *                reference only `@warn`s in that case and returns what was computed
 *                (src/solve_linear_system.jl:54-56,73-75,92-94,101-103,128-130,136-138); so does this library.
 *   < 0          hard error (bad handle/argument, HIP/RCCL failure); message via fpsq_last_error().
 */
#ifndef FPSQ_H
#define FPSQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fpsq_solver_s *fpsq_handle;

enum {
  FPSQ_OK = 0,
  FPSQ_ERR_ARG = -1,
  FPSQ_ERR_HIP = -2,
  FPSQ_ERR_STATE = -3, /* e.g. solve before the Jacobian was set */
  FPSQ_ERR_COMM = -4,
  FPSQ_ERR_TIMEOUT = -5
};

/* Krylov termination status (Krylov.jl `stats.status` strings, as an enum) */
enum {
  FPSQ_ST_UNKNOWN = 0,
  FPSQ_ST_ZERO_RHS = 1,     /* "x = 0 is a zero-residual solution" */
  FPSQ_ST_ZERO_ATB = 2,     /* "x = 0 is a minimum least-squares solution" */
  FPSQ_ST_SOLVED = 3,       /* tolerances met */
  FPSQ_ST_ZERO_RESID = 4,   /* "found approximate zero-residual solution" */
  FPSQ_ST_FWD_ERR = 5,      /* "truncated forward error small enough" */
  FPSQ_ST_ILL_COND = 6,     /* condition number limit */
  FPSQ_ST_MAXITER = 7,      /* "maximum number of iterations exceeded" */
  FPSQ_ST_INCONSISTENT = 8, /* "system may be inconsistent" (CRAIG) */
  FPSQ_ST_SOLVED_LQ = 9     /* LNLQ: "solutions xL and yL good enough" (FPSQ_ST_SOLVED: the CRAIG point xC, yC) */
};

/* how the two saddle-point systems of a call are solved (fpsq_options.kkt_method) */
enum {
  FPSQ_KKT_LSQR_CRAIG = 0, /* the reference's iterative path: LSQR on A' + CRAIG / LNLQ on A (solve_linear_system.jl:107-140)
                              for solve_two_mixed, two LSQR for solve_two_least_squares (:79-105).  Default. */
  FPSQ_KKT_MINRES_K = 1    /* MINRES on K = [I A'; A -delta I] itself, order n + m, both systems in lock-step.  NOT a path
                              of the reference: BASELINE.json north_star / configs[1] ("MINRES matrix-free") and SURVEY
                              8(b)'s method enum name it.  Stops on the reference's MINRES tolerances (ne_atol, ne_rtol,
                              ne_etol, ne_conlim; ne_itmax = 0 -> 2 (n + m)); stats are MINRES's.  Serves
                              fpsq_solve_two_mixed, fpsq_solve_two_least_squares and fpsq_ys_gs on a single-GPU handle;
                              the fused fpsq_qp_* entries and sharded handles return FPSQ_ERR_STATE with it. */
};

/* least-norm method of solve_two_mixed / ys_gs / qp_objgrad (fpsq_options.ln_method) */
enum {
  FPSQ_LN_CRAIG = 0, /* craig! with sqd and M = (1/delta) I: the reference's default workspace (struct.jl:121, :210-244) */
  FPSQ_LN_LNLQ = 1   /* lnlq! through the generic solve_least_norm (struct.jl:251-281; the commented alternative of
                        :121): M = (1/delta) I WITHOUT sqd, i.e. the minimum-norm solution of A x = -c for every delta */
};

/* The fields of Krylov.jl's `stats` that the reference reads
 * (src/solve_two_systems_struct.jl:183,242,279; src/solve_linear_system.jl:71). */
typedef struct {
  int32_t solved;
  int32_t inconsistent;
  int32_t niter;
  int32_t status;
  double rnorm;  /* last residual-norm estimate */
  double arnorm; /* last ||A'r|| estimate (LSQR, MINRES), 0 for CRAIG */
} fpsq_stats;

/* Replaces the keyword arguments of `IterativeSolver(nlp, ::T; ...)`, src/solve_two_systems_struct.jl:94-131.
 * Same names, same defaults (fpsq_default_options). */
typedef struct {
  double ls_atol, ls_rtol; /* LSQR, :99-100 */
  int64_t ls_itmax;        /* 5 (m + n), :101-103 */
  double ln_atol, ln_rtol, ln_btol, ln_conlim; /* CRAIG, :104-107 */
  int64_t ln_itmax;                            /* 5 (m + n), :108-110 */
  double ne_atol, ne_rtol, ne_etol;            /* MINRES on A A' + tau I, :111-113 */
  int64_t ne_itmax;                            /* 0 => 2 m, :114 */
  double ne_conlim;                            /* :115 */
  /* Krylov.jl lsqr! keywords the reference leaves at their defaults (sqrt(eps), 1/sqrt(eps)) */
  double ls_axtol, ls_btol, ls_etol, ls_conlim;
  /* execution knobs (no reference counterpart) */
  int32_t fuse_two_rhs;  /* 1: run the two recurrences of a solve_two_* call in lock-step, one SpMM(k=2) per
                            product instead of two SpMVs; results per system are identical to the unfused run */
  int32_t lookahead;     /* Krylov iterations the host may enqueue ahead of the device's progress word */
  int32_t device;        /* HIP device ordinal */
  int32_t jac_format;    /* storage of A for the A product: 0 = auto (column-sorted row groups when every group spans
                            < 2^21 columns, else CSR), 1 = CSR only */
  int32_t ln_method;     /* FPSQ_LN_CRAIG (default) or FPSQ_LN_LNLQ: which Krylov.jl workspace `solver_struct_least_norm`
                            would be (src/solve_two_systems_struct.jl:121) */
  int32_t kkt_method;    /* FPSQ_KKT_LSQR_CRAIG (default, the reference's path) or FPSQ_KKT_MINRES_K */
} fpsq_options;

/* defaults of src/solve_two_systems_struct.jl:99-115 for an (n, m) problem; fuse_two_rhs = 1 */
void fpsq_default_options(int64_t n, int64_t m, fpsq_options *opts);

/* Replaces the constructor contract `QDS(nlp, ::T; kwargs...)` (src/solve_two_systems_struct.jl:94-98;
 * call site src/parameters.jl:299).  `opts == NULL` => defaults. */
int fpsq_create(fpsq_handle *out, int64_t n, int64_t m, const fpsq_options *opts);
int fpsq_destroy(fpsq_handle h);
const char *fpsq_last_error(fpsq_handle h); /* h may be NULL: error of the last failed fpsq_create */

/* Jacobian sparsity, once per model.  Replaces `jac_structure!(nlp, rows, cols)` at
 * src/solve_two_systems_struct.jl:331-337: COO triplets in the model's fixed order, `index_base` 1 for
 * Julia.  Duplicates are allowed and are summed, as in SparseArrays.sparse (src/solve_linear_system.jl:233).
 * Builds CSR(A), CSR(A') and the value permutations on the device. */
int fpsq_set_jacobian_structure_coo(fpsq_handle h, int64_t nnz, const int64_t *rows, const int64_t *cols,
                                    int32_t index_base);
/* Same for a caller that already holds 0-based CSR (rowptr: m+1, colind: rowptr[m]); values then come in
 * CSR order. */
int fpsq_set_jacobian_structure_csr(fpsq_handle h, const int32_t *rowptr, const int32_t *colind);

/* Jacobian values at the current x, in the order of the structure call.  Replaces `jac_coord!(nlp, x, vals)`
 * at src/solve_linear_system.jl:223-228 and the per-x operator rebuild `jac_op!` at :118-122. */
int fpsq_set_jacobian_values(fpsq_handle h, const double *vals);

/* Registers (enabled != 0) or clears the caller's producer stream for device-resident arguments, see "INPUT
 * READINESS" above.  `hip_stream` is a hipStream_t (NULL = the legacy default stream). */
int fpsq_set_input_stream(fpsq_handle h, int32_t enabled, void *hip_stream);

/* STREAM-ORDERED OUTPUTS (optional; needs a stream registered with fpsq_set_input_stream).  By default every call returns
 * with all outputs complete.  With stream_ordered != 0, fpsq_qp_objgrad on a single-GPU handle whose vector arguments
 * (x, gx, ys, gs) all reside on the handle's GPU returns as soon as its HOST-visible results -- the return code, *fx and
 * the statistics -- are final, while the last kernels that write the DEVICE-resident outputs may still be running: the
 * registered stream has been made to wait for them (event, no host block), so work queued there afterwards -- the caller's
 * next kernels reading gx, its updates of x -- is ordered behind the evaluation, exactly as a stream-ordered library call.
 * A caller that touches the outputs from the host or from another stream must synchronise the registered stream first.
 * The host turn-around between dependent evaluations (return, the caller's decision, the next call's set-up) then overlaps
 * the GPU's tail instead of leaving it idle.  Every other case (host-resident arguments, sharded handles, profiling) keeps
 * the synchronous behaviour. */
int fpsq_set_output_ordering(fpsq_handle h, int32_t stream_ordered);

/* `nlp.delta`, mutated by the outer loop (src/algo.jl:389-393). */
int fpsq_set_delta(fpsq_handle h, double delta);

/* solve_two_mixed (src/solve_linear_system.jl:28-43, iterative method :107-140):
 *   K [p1; q1] = [rhs1; 0],  K [p2; q2] = [0; rhs2];   rhs1: n, rhs2: m;  p*: n, q*: m.
 * st[0] = LSQR stats, st[1] = CRAIG stats. */
int fpsq_solve_two_mixed(fpsq_handle h, const double *rhs1, const double *rhs2, double *p1, double *q1,
                         double *p2, double *q2, fpsq_stats st[2]);

/* solve_two_least_squares (src/solve_linear_system.jl:12-25, :79-105):
 *   K [p1; q1] = [rhs1; 0],  K [p2; q2] = [rhs2; 0];   rhs1, rhs2: n.  Uses the Jacobian of the last
 *   fpsq_set_jacobian_values (the reference does not refresh `nlp.Aop` either, :85-86). */
int fpsq_solve_two_least_squares(fpsq_handle h, const double *rhs1, const double *rhs2, double *p1, double *q1,
                                 double *p2, double *q2, fpsq_stats st[2]);

/* solve_two_extras (src/solve_linear_system.jl:2-9, :45-77), tau = max(delta, 1e-14):
 *   out1 = argmin ||A'q - rhs1||^2 + tau ||q||^2  (LSQR, lambda = sqrt(tau)),  out2 = (A A' + tau I)^-1 rhs2 (MINRES).
 *   rhs1: n, rhs2: m; out1, out2: m. */
int fpsq_solve_two_extras(fpsq_handle h, const double *rhs1, const double *rhs2, double *out1, double *out2,
                          fpsq_stats st[2]);

/* Fused convenience for `_compute_ys_gs!` after the user-model evaluations
 * (src/model-Fletcherpenaltynlp.jl:242-248): solve_two_mixed(g, c) then
 *   gs = p1 + sigma p2, ys = q1 + sigma q2, v = p2, w = q2  in one epilogue kernel. */
int fpsq_ys_gs(fpsq_handle h, const double *g, const double *c, double sigma, double *gs, double *ys, double *v,
               double *w, fpsq_stats st[2]);

/* y = alpha * op(A) x + beta * y with the handle's Jacobian; trans = 0: A (x: n, y: m), 1: A' (x: m, y: n).
 * The device `jprod!` / `jtprod!` (e.g. the rho A'c term, src/model-Fletcherpenaltynlp.jl:388-395). */
int fpsq_jac_mul(fpsq_handle h, int32_t trans, double alpha, const double *x, double beta, double *y);

/* ---- device-resident equality-QP user model (the synthetic workloads of BASELINE.json):
 *        f(x) = 1/2 x' diag(q) x + d'x,   c(x) = A x - b,   A = the handle's Jacobian.
 * fpsq_qp_objgrad is one `objgrad!(::FletcherPenaltyNLP, x, gx)` at a fresh x
 * (src/model-Fletcherpenaltynlp.jl:403-437) run entirely on the device: g, c, the two solves, the ys/gs
 * epilogue, Hsv = q .* v (constraints are linear, so S(x,w) gs = 0), + rho A'c, + eta (x - xk).
 * Any of gx, ys, gs may be NULL.  xk may be NULL when eta == 0. */
typedef struct fpsq_qp_s *fpsq_qp;
int fpsq_qp_create(fpsq_handle h, const double *qdiag, const double *d, const double *b, fpsq_qp *out);
int fpsq_qp_destroy(fpsq_qp qp);
int fpsq_qp_objgrad(fpsq_handle h, fpsq_qp qp, const double *x, double sigma, double rho, double eta,
                    const double *xk, double *fx, double *gx, double *ys, double *gs, fpsq_stats st[2]);
/* One `hprod!(::FletcherPenaltyNLP, x, v, Hv)` on the same model, entirely on the device.
 * hessian_approx = 2, Val(2) (src/model-Fletcherpenaltynlp.jl:521-570):
 *   Hsv = q .* v;  (p1, _, p2, _) = solve_two_least_squares(v, Hsv);  Ptv = v - p1;
 *   Hv = p2 - q .* Ptv + 2 sigma Ptv (+ rho A'(A v)) (+ eta v)      (the constraint Hessians vanish: c is linear).
 *   st[0], st[1] = the two LSQR recurrences.
 * hessian_approx = 1, Val(1) (:572-634): the same, then Ssv = ghjvprod(x, gs, v) (= 0 for linear constraints),
 *   (invJtJJv, invJtJSsv) = solve_two_extras(v, Ssv) and Hv -= A' invJtJSsv (- hprod_nln(x, invJtJJv, gs; obj_weight = 0) = 0):
 *   the LSQR + MINRES lanes of fpsq_solve_two_extras and one more A' product; st must then hold FOUR entries, st[2], st[3] =
 *   the statistics of those two recurrences, and bits 2, 3 of a positive return code flag their `solved == false`.
 * The Hessian-free sub-solvers call this once per inner CG iteration. */
int fpsq_qp_hprod(fpsq_handle h, fpsq_qp qp, const double *v, double sigma, double rho, double eta, int32_t hessian_approx,
                  double *Hv, fpsq_stats *st);
/* The same model with a SPARSE SYMMETRIC objective Hessian, f(x) = 1/2 x'Q x + d'x (a mass or stiffness matrix), on the
 * iterative handle -- the contract of fpsq_band_qp_create_csr (below): Q is n x n in CSR, 0-based, FULL symmetric storage
 * (both triangles), columns in any order, the diagonal may be absent (= 0); host or device pointers.  The constraints are
 * linear, so the Lagrangian Hessian is Q and the two evaluations become (:403-437, :521-570)
 *   objgrad: g = Q x + d, gx = gs - Q p2 + sigma p2 + rho A'c + eta (x - xk), *fx with f = 1/2 x'Q x + d'x;
 *   hprod:   (p1, _, p2, _) = solve_two_least_squares(v, Q v), Hv = p2 - Q Ptv + 2 sigma Ptv + rho A'(A v) + eta v;
 *            hessian_approx = 1 runs its solve_two_extras lanes on (v, 0) as above (nothing in them involves Q).
 * Checked once, on the host: an index out of range, a duplicate entry, a pattern or values that are not symmetric
 * (Q_ij != Q_ji) give FPSQ_ERR_ARG and a message in fpsq_last_error(h) that starts with "qp_create_csr:" and names the
 * range / duplicate / pattern / values -- the kernels read rows only, so an unsymmetric Q would otherwise give a wrong
 * Hessian silently.  *out is written on success only.
 * fpsq_qp_objgrad / fpsq_qp_hprod / fpsq_qp_destroy take the object unchanged.  Q = diag(q) + R: the kernels of the Krylov
 * loop and of its tail run as on the diagonal model, with the diagonal part; R enters in launches of its own -- an objgrad
 * is two launches longer (d + R x and the -1/2 x'R x partials in front, gx -= R p2 behind the tail), an hprod one
 * (Q v in front instead of q .* v, Hv -= R (v - p1) behind the tail); every sum in a fixed order, so two calls with the
 * same arguments return the same bits, and the stream-ordered return (fpsq_set_output_ordering) applies unchanged.  Hv must
 * not alias v.  Models of either kind may share a handle and do not disturb each other.
 * SCOPE: single-GPU handles with kkt_method = FPSQ_KKT_LSQR_CRAIG (ln_method CRAIG or LNLQ).  On a handle with a
 * communicator, or with FPSQ_KKT_MINRES_K, this entry and an evaluation of such a model return FPSQ_ERR_STATE with a
 * message (in halo mode the n-vectors are column windows: R would need an exchange of its own). */
int fpsq_qp_create_csr(fpsq_handle h, const int32_t *q_rowptr, const int32_t *q_colind, const double *q_vals,
                       const double *d, const double *b, fpsq_qp *out);

/* ---- multi-GPU: 1-D row sharding of A across ranks.  Each rank creates its handle with
 * the GLOBAL n and its LOCAL m (its block of constraints), passes its local rows to set_jacobian_*, and
 * m-vectors (rhs2, q1, q2, ys, w, c, b) are the rank's slices.  n-vectors are replicated.  Partial A'u
 * products and m-vector dot products are all-reduced with RCCL on the solver's stream.
 * fpsq_comm_unique_id fills a 128-byte id on rank 0; the caller broadcasts it and every rank calls
 * fpsq_comm_init.  Without fpsq_comm_init the handle is single-GPU. */
int fpsq_comm_unique_id(uint8_t id[128]);
int fpsq_comm_init(fpsq_handle h, int32_t nranks, int32_t rank, const uint8_t id[128]);
/* How the exchanges of the halo-sharded Krylov loop travel between the ranks of a node (fpsq_info.comm_route reports what
 * a handle ended up with):
 *   FPSQ_ROUTE_P2P   peer to peer, no collective call inside the loop: every rank exports its gather buffers, halo slots
 *                    and flag words (hipIpcGetMemHandle), maps its peers' (hipIpcOpenMemHandle, peer access over xGMI) and
 *                    from then on WRITES its records -- the norm partials of a product, the raw A'u sums of its two overlap
 *                    regions, the four sums of phi -- straight into the peers' buffers, announces them with sequence
 *                    numbers and waits (a bounded number of polls: FPSQ_ERR_TIMEOUT, never a hang) for theirs, one
 *                    one-workgroup kernel per exchange.  Per joint Krylov iteration: 2 product launches + 3 exchange kernels --
 *                    or, when every rank has a device of its own (round 5), NO exchange kernel for the sums: the leader
 *                    workgroups of the product launches write their rank's local sums into the peers' mapped receive
 *                    areas and add the ranks' rows up in rank order themselves (fpsq_info.comm_in_launch_sums = 1:
 *                    2 product launches + the halo launch; one launch per iteration when no row is shared with a neighbour).
 *   FPSQ_ROUTE_RCCL  ncclAllGather / grouped ncclSend + ncclRecv on the solver's stream (3 RCCL operations per iteration:
 *                    latency-bound at the headline size); also what the replicated (non-halo) layout always uses.
 * fpsq_comm_set_route(h, route), after fpsq_comm_init and BEFORE fpsq_comm_set_halo: FPSQ_ROUTE_AUTO (default) = P2P when
 * every rank can export and map, else RCCL -- decided unanimously at the first solve (the handles travel through one RCCL
 * all-gather); FPSQ_ROUTE_RCCL = never try; FPSQ_ROUTE_P2P = fail the first solve with FPSQ_ERR_COMM when it cannot be
 * set up.  The reference has nothing to mirror here (no parallelism at all). */
enum { FPSQ_ROUTE_AUTO = 0, FPSQ_ROUTE_RCCL = 1, FPSQ_ROUTE_P2P = 2, FPSQ_ROUTE_LOCAL = 3, FPSQ_ROUTE_LOCAL_P2P = 4 };
int fpsq_comm_set_route(fpsq_handle h, int32_t route);
/* HALO MODE (banded Jacobians; SURVEY.md 8e "contract path").  When the rows of a rank touch only a column window
 * [w_lo(r), w_hi(r)) of the n columns, windows tile [0, n) and only overlap between neighbouring ranks, the n-vectors
 * need not be replicated: the rank's handle is created with n = its WINDOW length (column indices relative to
 * w_lo(r)), every n-vector argument is the rank's window of the global vector (identical on overlaps), and per
 * Krylov iteration the ranks exchange the partial A'u products of the overlap regions with their neighbours
 * (overlap_left = w_hi(r-1) - w_lo(r) entries at the head of the window, overlap_right = w_hi(r) - w_lo(r+1) at its
 * tail; <= 2 x 8192 x 2 doubles at the headline size) instead of all-reducing an n x 2 vector, plus one 4-double
 * all-reduce per reduction (sums over n-vectors run over the owned prefix [0, n - overlap_right)).  Call after
 * fpsq_comm_init / fpsq_comm_init_local; overlaps must be 0 at the outer ends (rank 0 left, last rank right). */
int fpsq_comm_set_halo(fpsq_handle h, int64_t overlap_left, int64_t overlap_right);
/* In-process stand-in for RCCL: `nshards` (<= 8) row-shard handles living in ONE process on ONE GPU, each driven
 * by its own host thread; the all-reduce is a summation kernel.  Lets the sharded numerics be parity-tested on a
 * one-GPU box.  Create the group, attach every shard handle, run the same call on all shards concurrently. */
int fpsq_local_group_create(int32_t nshards, void **group);
int fpsq_local_group_destroy(void *group);
int fpsq_comm_init_local(fpsq_handle h, void *group, int32_t shard);
/* on != 0 (before the shards attach): the shards of the group exchange their halo records and norm partials PEER TO PEER --
 * every rank writes its record straight into its peers' buffers, announces it with a sequence number and waits (bounded)
 * for theirs, one small kernel per exchange and no collective call inside the Krylov loop.  This is the protocol of the
 * xGMI route between the GPUs of a node (peers' buffers mapped with hipIpcOpenMemHandle instead of living on the same
 * device); it is exercised here between logical shards of one GPU (<= 3: every shard needs a hardware queue of its own while
 * it waits), not measured on a multi-GPU node.  Halo mode only. */
int fpsq_local_group_set_p2p(void *group, int32_t on);


/* ---- dense-block Jacobian variant (BASELINE configs[2]; the DIRECT back-end of the seam for small / dense problems).
 * Replaces the reference's factorisation path: LDLtSolver (src/solve_two_systems_struct.jl:308-353),
 * solve_two_mixed / solve_two_least_squares with `ldl_factorize!` + `ldiv!` (src/solve_linear_system.jl:161-252) and
 * the dense A A' + tau I contraction of src/model-Fletcherpenaltynlp.jl:478-484.  Here: M = A A' + delta I on the fp64
 * matrix cores (v_mfma_f64_16x16x4_f64), blocked Cholesky M = L L', two right-hand sides per solve:
 *   q1 = M^-1 A rhs1, p1 = rhs1 - A'q1;   mixed: q2 = -M^-1 rhs2, p2 = -A'q2;   least squares: q2 = M^-1 A rhs2, p2 = rhs2 - A'q2.
 * fpsq_dense_factorize returns 1 (soft) with *info = first non-positive pivot row (1-based) when M is not positive
 * definite -- the counterpart of `factorized(str) == false` (src/solve_linear_system.jl:242-246). */
typedef struct fpsq_dense_s *fpsq_dense;
typedef struct {
  int64_t n, m;
  double last_syrk_ms; /* device time of M = A A' + delta I */
  double last_chol_ms; /* device time of the blocked Cholesky */
  double last_solve_ms;
  int64_t regularized_pivots; /* pivots replaced by the dynamic regularisation in the last factorisation */
} fpsq_dense_info;
int fpsq_dense_create(fpsq_dense *out, int64_t n, int64_t m, int32_t device);
int fpsq_dense_destroy(fpsq_dense d);
const char *fpsq_dense_last_error(fpsq_dense d);
int fpsq_dense_set_jacobian(fpsq_dense d, const double *a_rowmajor); /* m x n, the Jacobian at the current x */
/* The reference's hand-over instead of a dense array: `jac_structure!` once (src/solve_two_systems_struct.jl:331-337: COO
 * triplets in the model's order, index_base 1 for Julia, duplicates allowed), then per x the output of `jac_coord!`
 * (src/solve_linear_system.jl:223-228) -- nnz values in that order, HOST or DEVICE memory; one scatter kernel puts them into
 * the dense storage, duplicates summed in a fixed order like `sparse(rows, cols, vals)` (:233). */
int fpsq_dense_set_structure_coo(fpsq_dense d, int64_t nnz, const int64_t *rows, const int64_t *cols, int32_t index_base);
int fpsq_dense_set_jacobian_coo(fpsq_dense d, const double *vals);
int fpsq_dense_factorize(fpsq_dense d, double delta, int32_t *info);
/* Dynamic regularisation of LDLFactorizations.jl as the reference's LDLtSolver configures it
 * (src/solve_two_systems_struct.jl:345-348: tol = r1 = sqrt(eps), r2 = -sqrt(eps)).  A pivot d of M = A A' + delta I with
 * d <= tol -- minus d is the pivot of the (2,2) block of K = [I A'; A -delta I] once the identity block is eliminated
 * (its pivots are 1: r1 never fires) -- is replaced by `reg` = -r2 and counted (fpsq_dense_info.regularized_pivots); the
 * factorisation then succeeds on rank-deficient Jacobians (test/rank-deficient.jl) instead of reporting a non-positive
 * pivot.  reg <= 0 switches it off (the default).  `tol` is absolute, like the scaled threshold the reference uses.
 * reg = FPSQ_REG_DROP drops the pivot instead: the row counts as linearly dependent on the earlier ones, its multiplier comes
 * out as (numerically) zero and the other rows solve the consistent part of the normal equations -- multiplier estimates
 * stay bounded on rank-deficient Jacobians (test/test-2.jl:264-287 FLT), where a pivot of sqrt(eps) makes them ~ 1/sqrt(eps).
 * The host bindings default to the reference's ldlt_r2 = -sqrt(eps) (reg = sqrt(eps)); the drop rule is their explicit option. */
#define FPSQ_REG_DROP 1e200
int fpsq_dense_set_regularization(fpsq_dense d, double tol, double reg);
int fpsq_dense_solve_two_mixed(fpsq_dense d, const double *rhs1, const double *rhs2, double *p1, double *q1, double *p2,
                               double *q2);
int fpsq_dense_solve_two_least_squares(fpsq_dense d, const double *rhs1, const double *rhs2, double *p1, double *q1,
                                       double *p2, double *q2);
/* m x m row-major copy of the factor storage: lower triangle = L with M = L L' (upper triangle unspecified) */
int fpsq_dense_get_factor(fpsq_dense d, double *l_out);
int fpsq_dense_get_info(fpsq_dense d, fpsq_dense_info *info);

/* ---- sparse direct back-end: the reference's LDLtSolver path for SPARSE Jacobians whose
 * normal-equations matrix is banded (PDE-like Jacobians: row i only touches a column window that moves with i).
 *   fpsq_band_create      = the constructor's symbolic work (src/solve_two_systems_struct.jl:326-344: the COO pattern of
 *                           triu(K) and `ldl_analyze`): here the block band structure of M = A A' + delta I -- the Schur
 *                           complement of the identity block of K = [I A'; A -delta I] -- from the CSR pattern of A
 *                           (half bandwidth = the largest row distance of two entries of one column).  When the
 *                           natural band is wide (> 1/8 of the matrix) the rows are first reordered by reverse
 *                           Cuthill-McKee on the graph of A A' -- the bandwidth-reducing counterpart of the fill-reducing
 *                           ordering `ldl_analyze` computes -- and the ordering is kept if it narrows the band.  A long
 *                           narrow band is further ordered from BOTH ends towards the middle (blocks alternately from
 *                           the top and from the bottom), which makes its elimination two independent chains that
 *                           fpsq_band_factorize and the solves run side by side on two streams.  All permutations are
 *                           internal (right-hand sides, solutions and reported pivot rows stay in the caller's order).
 *                           Environment switches for A/B runs: FPSQ_BAND_REORDER, FPSQ_BAND_TWOCHAIN (0 = off).
 *   fpsq_band_factorize   = `jac_coord!` + `sparse(...)` + `ldl_factorize!` (src/solve_linear_system.jl:223-234): forms M
 *                           into 128 x 128 blocks of the band on the device and factors it with a right-looking
 *                           block-banded Cholesky (the dense back-end's MFMA block kernels); returns 1 (soft) with *info
 *                           = first non-positive pivot row when M is not positive definite and no regularisation is set.
 *                           "First" is by the elimination order, never by time: of several such rows the one at the lowest
 *                           STORED position is reported (in the caller's numbering), the same one in every factorisation.
 *                           Without reordering that is the lowest row index.  With two elimination chains the stored order
 *                           is: rows 0 .. 127, then rows m-1 .. m-128 (descending), then rows 128 .. 255, then rows m-129 ..
 *                           m-256, ... and the rows left in the middle last -- so of one such row in each chain the one in
 *                           the block nearer to ITS end of the matrix wins, and at equal block distance the top chain's.
 *   fpsq_band_set_regularization = the dynamic regularisation of :345-348, as for the dense back-end.
 *   fpsq_band_solve_two_*  = `ldiv!` with two right-hand sides (:189-203, :236-251) on the cached factor.
 * Storage is (m / 128) x (half bandwidth in blocks + 1) blocks; create fails with FPSQ_ERR_STATE when that does not fit
 * the device (or the half bandwidth exceeds 143 blocks AND a row spans more than 9600 columns), with FPSQ_ERR_ARG when
 * the pattern holds duplicate entries.  Arguments may be host or device pointers; calls are synchronous.
 *
 * BORDERED BAND (fpsq_band_create_bordered, _create_coo_bordered, _analyze_bordered: the entries above plus max_border, 0 ..
 * 16, anything else FPSQ_ERR_ARG; the entries above ARE these with max_border = 0).  A few constraint rows that touch columns
 * all over the range -- a mean-value, volume or mass-conservation constraint, the wrap-around rows of a periodic boundary --
 * couple with every row of M, and no ordering narrows such a band.  Up to max_border of them are eliminated LAST instead: in
 * the stored order (band rows first, the s border rows last)
 *     M = [B C; C' D],   B = A_b A_b' + delta I (the band that is factored),   C = A_b A_s',   D = A_s A_s' + delta I,
 * a factorisation also forms Z = B^-1 C (one tile of the block sweeps) and the s x s Cholesky of S = D - C'Z, and every
 * M-solve of every entry below is  y = B^-1 r (the sweeps),  w = S^-1 (t - C'y),  u = y - Z w  (two launches more).
 * SELECTION, deterministic: the candidates are the max_border rows of widest column span (last - first column + 1; ties: the
 * lower row index first), taken widest first; the border is the SHORTEST such prefix after whose removal the remaining rows,
 * put through the ordering described above (reverse Cuthill-McKee when wide, then the two-ended order), have a half
 * bandwidth in blocks of at most a quarter of the half bandwidth the ordering of ALL rows gives.  No such prefix (more long
 * rows than max_border, or nothing to gain): the border is empty and the handle is the one max_border = 0 gives, bit for
 * bit.  Border rows are stored last, in ascending order of the caller's index; fpsq_band_analyze_bordered lists them at the
 * end of row_perm.  nblocks, bandwidth_blocks, factor_bytes and chains describe the band part.  The dynamic regularisation
 * applies to the pivots of S by the rule of the pivots of B; without it a non-positive pivot of S gives the soft code 1 with
 * *info = that border row (1-based, the caller's numbering), and regularized_pivots counts the pivots of S too.  All sums
 * of the correction have a fixed order: calls are repeatable and the block entries keep their DETERMINISM contract.
 *
 * LONG COLUMNS (fpsq_band_create_bordered_cols, _create_coo_bordered_cols, _analyze_bordered_cols: the bordered entries plus
 * max_cols, 0 .. 16, anything else FPSQ_ERR_ARG; the bordered entries ARE these with max_cols = 0).  The transposed case: a
 * variable that appears in constraints all over the row range -- a global parameter, a free final time or step length, a
 * scalar control, a shared design or inflow variable -- is a long COLUMN of A, and one such column makes M structurally
 * dense whatever the row order.  Up to max_cols of them are taken out of the band instead: with A = [A_b | U] as a column
 * partition (U: m x s, the long columns)
 *     M = A A' + delta I = B + U U',   B = A_b A_b' + delta I (the band that is factored),
 *     M^-1 r = y - Z w,   y = B^-1 r (the sweeps),   Z = B^-1 U,   S = I + U'Z (s x s, S >= I),   w = S^-1 (U'y).
 * A factorisation also forms U ([m][16] in the stored row order), Z (one tile of the block sweeps) and the Cholesky of S;
 * every M-solve of every entry below takes the correction behind its sweeps (two launches more).  SCOPE: through THESE entries
 * (and the older ones above) a handle takes ONE kind of border, max_border > 0 together with max_cols > 0 is FPSQ_ERR_ARG --
 * both kinds on one handle are the ARROW BAND entries below; at most 16 columns.
 * SELECTION, deterministic, the row border's rule transposed: the candidates are the max_cols columns with the most entries
 * (ties: the lower column index first), taken most first; the long columns are the SHORTEST such prefix after whose removal
 * (a) no row of A is left without an entry (B would be structurally singular at delta = 0) and (b) the remaining columns,
 * put through the ordering described above, have a half bandwidth in blocks of at most a quarter of the half bandwidth
 * ALL columns give.  No such prefix: border_cols = 0 and the handle is the one max_cols = 0 gives, bit for bit.  Columns
 * are not renumbered: every n-vector stays in the caller's order.  nblocks, bandwidth_blocks, factor_bytes and chains
 * describe B; row_perm is the ordering of the rows on the remaining columns.
 * PRODUCTS: A x reads a long column's entries where they are, in the rows.  In A'q no lane group walks a long column: the
 * transposed structure holds, for long column i, one entry of value 1 per chunk of rows, pointing at a slot behind the
 * padded rows of the vector, and a grid-wide reduction in a fixed order leaves the chunk sums of U[.][i] q[.] in those slots
 * (fpsq_band_jac_mul(trans = 1) and the A'c / A'(A v) terms).  For the SOLUTIONS of the M-solves the slots receive w itself:
 * U'(y - Z w) = w exactly, so the rows of A'q1 / A'q2 (hence of p1, p2, gs, Hv ...) that belong to long columns equal the
 * products only to rounding.
 * NUMERICS: the low-rank form is as accurate as a Cholesky of M while U is moderate against B; where the long columns
 * dominate it loses digits roughly like cond(B) cond(S) (a numpy model of the scheme against a dense LU of K: 2e-15 .. 6e-14
 * on the shapes of the tests where the Cholesky of M gives 1e-15 .. 7e-15; 1e-10 against 1.4e-13 on aug2dc_like(51), delta =
 * 0, with 4 all-row columns scaled by 30, cond(B) = 1e3, cond(M) = 2e5, cond(S) = 9e3).  That loss belongs to the scheme;
 * border_pivot_ratio reports it per factorisation.  A pivot of S that fails the rule of the pivots of B (S >= I, so only behind a
 * failing pivot of B, which keeps *info) is regularised or reported as the last stored row; regularized_pivots counts it.
 *
 * ARROW BAND (fpsq_band_create_arrow, _create_coo_arrow, _analyze_arrow: the arguments of the _bordered_cols entries, both
 * maxima 0 .. 16 INDEPENDENTLY, anything else FPSQ_ERR_ARG).  Border rows and long columns on one handle: a model with a free
 * final time or a global parameter (a long column) and an integral, mean-value or mass constraint (a long row).  Stored row
 * order: the mb band rows, then the s_r border rows; columns are not renumbered; L = the s_c long columns, "o" = restricted to
 * the other columns:
 *     A = [A_b,o U_b; A_s,o U_s],   M = A A' + delta I = M_r + U U',   U = [U_b; U_s] (m x s_c, ALL rows, the border's included),
 *     M_r = [B C; C' D],   B = A_b,o A_b,o' + delta I,   C = A_b,o A_s,o',   D = A_s,o A_s,o' + delta I.
 * M_r^-1 is the bordered band's solve (sweeps on B, w_r = S_r^-1 (t - C'y), u = y - Z_r w_r, Z_r = B^-1 C, S_r = D - C'Z_r) and
 * the long columns' correction is wrapped around it: M^-1 r = y - Z_c w_c, y = M_r^-1 r, Z_c = M_r^-1 U, S_c = I + U'Z_c >= I,
 * w_c = S_c^-1 U'y.  A factorisation forms C, D, Z_r, S_r as a bordered handle does (on the other columns), then U, Z_c (the
 * block sweeps followed by the rows' correction), S_c and G = U_s' - U_b'Z_r (s_c x s_r).  COST of an M-solve behind the
 * sweeps: FOUR launches in the nested form (the two corrections one after the other); the default FUSED form takes TWO: since
 * U'M_r^-1 r = U_b'y + G w_r with y the sweeps' output, one reduction forms the partials of C'y and U_b'y in one pass over y
 * and one update solves with S_r, then S_c, and corrects every row once (u = y - Z_r w_r - Z_c,b w_c on the band rows, w_r -
 * Z_c,s w_c on the border rows).  FPSQ_ARROW_FUSED=0 (read at create) selects the nested form; the two agree to rounding, not
 * bitwise.  Everything else is as on the two kinds alone: the border rows' right-hand sides travel in the last stored rows,
 * the long columns' rows of A'q in the slots behind the padded rows, all sums in a fixed order (DETERMINISM as below).
 * last_border_ms spans both shares, border_pivot_ratio is S_c's; a failing pivot of S_r follows the row border's rule (*info =
 * that border row), one of S_c the long columns'; regularized_pivots counts both.
 * SELECTION, deterministic:  (1) the column candidates Cc are the max_cols columns with the most entries (ties: the lower
 * index), the row candidates Rc the max_border rows of widest column span measured over the columns NOT in Cc, widest first
 * (ties: the lower index) -- otherwise a parameter column at the end of the column order makes every row look wide.  (2)
 * COLUMNS: the rule of LONG COLUMNS (the shortest prefix of Cc meeting (a) and (b)) on the pattern with the rows Rc set aside,
 * in the baseline ordering and in the trial orderings alike; (a) is checked over ALL rows.  That is L.  (3) ROWS: the rule of
 * BORDERED BAND on the pattern with the columns L masked: spans, candidates and orderings use the remaining columns, the
 * quarter is measured against the ordering of all rows on the remaining columns.  That is R.  (4) REDUCTIONS, bit for bit: L
 * empty -> what the _bordered entries give with max_border; R empty -> the columns are decided again by the plain column rule
 * and the result is what _bordered_cols(0, max_cols) gives; max_border = 0 resp. max_cols = 0 -> the corresponding older
 * entry; both empty -> the plain handle.  Each phase costs at most one ordering per candidate prefix.  row_perm lists the
 * border rows last (ascending), long_cols is as in _analyze_bordered_cols; nblocks, bandwidth_blocks, factor_bytes and
 * chains describe B. */
typedef struct fpsq_band_s *fpsq_band;
typedef struct {
  int64_t n, m, nnz;
  int64_t nblocks;           /* 128-row blocks of M */
  int64_t bandwidth_blocks;  /* half bandwidth of M in blocks */
  int64_t factor_bytes;      /* storage of the banded factor */
  double last_form_ms, last_chol_ms, last_solve_ms;
  int64_t regularized_pivots;
  int64_t reordered;         /* 1: the symbolic phase reordered the rows of A (reverse Cuthill-McKee and / or the two-ended
                                order of the two elimination chains) */
  int64_t chains;            /* 2: the band is eliminated from both ends at once (two streams), 1: one chain */
  int64_t border_rows;       /* rows eliminated last as a border (0 unless created with max_border > 0 and rows were taken) */
  double last_border_ms;     /* device time of C, D, Z, S (long columns: U, Z, S; arrow: both) and its Cholesky in the last
                                factorisation (not in last_chol_ms) */
  int64_t border_cols;       /* long columns taken out of the band (0 unless created with max_cols > 0 and columns were taken) */
  double border_pivot_ratio; /* long columns: (largest / smallest pivot of the Cholesky factor of S)^2 in the last
                                factorisation, an estimate of cond(S); 1 without long columns */
} fpsq_band_info;
int fpsq_band_create(fpsq_band *out, int64_t n, int64_t m, const int32_t *rowptr, const int32_t *colind, int32_t device);
int fpsq_band_create_bordered(fpsq_band *out, int64_t n, int64_t m, const int32_t *rowptr, const int32_t *colind,
                              int32_t max_border, int32_t device);
/* The same from the model's COO structure (`jac_structure!`, struct.jl:331-337; index_base 1 for Julia; duplicates allowed
 * and summed) -- with fpsq_band_factorize_coo taking the output of `jac_coord!` (nnz values in that order, HOST or DEVICE
 * memory): the sorted order is kept on the device and one gather(-sum) kernel fills the CSR slots, so neither the caller nor
 * the binding re-orders anything per x (src/solve_linear_system.jl:223-234). */
int fpsq_band_create_coo(fpsq_band *out, int64_t n, int64_t m, int64_t nnz, const int64_t *rows, const int64_t *cols,
                         int32_t index_base, int32_t device);
int fpsq_band_create_coo_bordered(fpsq_band *out, int64_t n, int64_t m, int64_t nnz, const int64_t *rows, const int64_t *cols,
                                  int32_t index_base, int32_t max_border, int32_t device);
int fpsq_band_create_bordered_cols(fpsq_band *out, int64_t n, int64_t m, const int32_t *rowptr, const int32_t *colind,
                                   int32_t max_border, int32_t max_cols, int32_t device);
int fpsq_band_create_coo_bordered_cols(fpsq_band *out, int64_t n, int64_t m, int64_t nnz, const int64_t *rows,
                                       const int64_t *cols, int32_t index_base, int32_t max_border, int32_t max_cols,
                                       int32_t device);
int fpsq_band_create_arrow(fpsq_band *out, int64_t n, int64_t m, const int32_t *rowptr, const int32_t *colind,
                           int32_t max_border, int32_t max_cols, int32_t device);
int fpsq_band_create_coo_arrow(fpsq_band *out, int64_t n, int64_t m, int64_t nnz, const int64_t *rows, const int64_t *cols,
                               int32_t index_base, int32_t max_border, int32_t max_cols, int32_t device);
int fpsq_band_factorize_coo(fpsq_band b, const double *vals, double delta, int32_t *info);
/* the ordering decisions of fpsq_band_create alone, on the host (no device needed; rowptr / colind in HOST memory): row_perm
 * (m entries, may be null) = the caller's row stored at each position, info = blocks / half bandwidth / factor bytes /
 * reordered / chains of the structure fpsq_band_create would set up. */
int fpsq_band_analyze(int64_t n, int64_t m, const int32_t *rowptr, const int32_t *colind, int32_t *row_perm,
                      fpsq_band_info *info);
int fpsq_band_analyze_bordered(int64_t n, int64_t m, const int32_t *rowptr, const int32_t *colind, int32_t max_border,
                               int32_t *row_perm, fpsq_band_info *info);
/* long_cols (16 entries, may be null): the columns taken, ascending, -1 beyond border_cols */
int fpsq_band_analyze_bordered_cols(int64_t n, int64_t m, const int32_t *rowptr, const int32_t *colind, int32_t max_border,
                                    int32_t max_cols, int32_t *row_perm, int32_t *long_cols, fpsq_band_info *info);
int fpsq_band_analyze_arrow(int64_t n, int64_t m, const int32_t *rowptr, const int32_t *colind, int32_t max_border,
                            int32_t max_cols, int32_t *row_perm, int32_t *long_cols, fpsq_band_info *info);
int fpsq_band_destroy(fpsq_band b);
const char *fpsq_band_last_error(fpsq_band b);
int fpsq_band_set_regularization(fpsq_band b, double tol, double reg);
int fpsq_band_factorize(fpsq_band b, const double *vals, double delta, int32_t *info);
int fpsq_band_solve_two_mixed(fpsq_band b, const double *rhs1, const double *rhs2, double *p1, double *q1, double *p2,
                              double *q2);
int fpsq_band_solve_two_least_squares(fpsq_band b, const double *rhs1, const double *rhs2, double *p1, double *q1,
                                      double *p2, double *q2);
int fpsq_band_get_info(fpsq_band b, fpsq_band_info *info);

/* ---- the device-resident equality-QP user model on the banded handle: the fpsq_qp_* group of the iterative handle on the
 * DIRECT back-end.   f(x) = 1/2 x' diag(q) x + d'x,   c(x) = A x - b,   A = the Jacobian the handle was last factorised with.
 * These entries use the CACHED factor: the caller factorises (fpsq_band_factorize[_coo]) when the Jacobian's values or delta
 * change -- the counterpart of fpsq_set_jacobian_values on the iterative handle -- and an evaluation costs no
 * factorisation.  Without a valid factor they return FPSQ_ERR_STATE like the solve entries.  Vectors are host or device
 * pointers; device-resident ones are read and written in place (no staging copy), and an evaluation then moves nothing
 * between host and device but its scalars, once.  Row permutation, padding and the two elimination chains stay internal.
 *   fpsq_band_qp_objgrad  one `objgrad!(::FletcherPenaltyNLP, x, gx)` (src/model-Fletcherpenaltynlp.jl:403-437) on this model
 *                         (the constraint Hessians vanish: Sstw = 0, Hsv = q .* v):  (p1, q1, p2, q2) = solve_two_mixed(g, c),
 *                         ys = q1 + sigma q2, gs = p1 + sigma p2, gx = gs + (sigma - q) .* p2 + rho A'c + eta (x - xk),
 *                         *fx = f - c'ys + rho/2 c'c + eta/2 |x - xk|^2 (a HOST double).  gx, ys, gs may be NULL; xk NULL
 *                         with eta > 0 means xk = 0.  The rho / eta terms are added when the parameter is positive.
 *                         Sums are formed in a fixed order: two calls with the same arguments return the same bits.
 *   fpsq_band_qp_hprod    one `hprod!` with hessian_approx = 2 (:521-570): (p1, _, p2, _) = solve_two_least_squares(v, q .* v),
 *                         Ptv = v - p1, Hv = p2 - q .* Ptv + 2 sigma Ptv + rho A'(A v) + eta v.  hessian_approx = 1 (:572-634)
 *                         returns the SAME vector and launches nothing more: its extra terms vanish identically on this model
 *                         (Ssv = ghjvprod = 0 for linear constraints, the exact solve of a zero right-hand side is zero, and
 *                         hprod with obj_weight = 0 is zero).  Any other value: FPSQ_ERR_ARG.
 *   fpsq_band_jac_mul     y = alpha op(A) x + beta y, trans = 0: A (x: n, y: m), 1: A' (x: m, y: n), in the caller's row order.
 *   fpsq_band_set_input_stream  as fpsq_set_input_stream ("INPUT READINESS" above): once a stream is registered (enabled != 0;
 *                         NULL = the legacy default stream), each of the calls above and fpsq_band_factorize[_coo] first makes
 *                         the handle's stream wait (event, no host block) for everything enqueued on that stream so far.
 *                         Outputs are complete when a call returns, so there is no output-ordering switch.
 *   fpsq_band_qp_create_csr  the same model with a SPARSE SYMMETRIC objective Hessian, f(x) = 1/2 x'Q x + d'x (a mass or
 *                         stiffness matrix): Q is n x n in CSR, 0-based, FULL symmetric storage (both triangles), columns in
 *                         any order, the diagonal may be absent (= 0); host or device pointers.  The constraints are linear, so
 *                         the Lagrangian Hessian is Q and the two evaluations become (:403-437, :521-570)
 *                           objgrad: g = Q x + d, gx = gs - Q p2 + sigma p2 + rho A'c + eta (x - xk), *fx with f = 1/2 x'Q x + d'x;
 *                           hprod:   (p1, _, p2, _) = solve_two_least_squares(v, Q v), Hv = p2 - Q Ptv + 2 sigma Ptv
 *                                    + rho A'(A v) + eta v   (hessian_approx = 1 again the same vector),
 *                         everything else as above.  Checked once, on the host: an index out of range, a duplicate entry, a
 *                         pattern or values that are not symmetric (Q_ij != Q_ji) give FPSQ_ERR_ARG with a message in
 *                         fpsq_band_last_error(b) -- the kernels read rows only, so an unsymmetric Q would otherwise give a
 *                         wrong Hessian silently.  fpsq_band_qp_objgrad / _hprod / _destroy take the object unchanged; an
 *                         evaluation is two launches longer than on the diagonal model (Q = diag + R: R x resp. R v in front,
 *                         R p2 resp. R Ptv behind the A' product) and as repeatable.  FPSQ_BAND_QP_G is ignored here.
 * Destroy a model before the handle it was created on.  FPSQ_BAND_QP_G=1 (read by fpsq_band_qp_create; A/B runs) forms g at
 * gather time in the A product instead of writing it first. */
typedef struct fpsq_band_qp_s *fpsq_band_qp;
int fpsq_band_qp_create(fpsq_band b, const double *qdiag, const double *d, const double *bvec, fpsq_band_qp *out);
int fpsq_band_qp_create_csr(fpsq_band b, const int32_t *q_rowptr, const int32_t *q_colind, const double *q_vals,
                            const double *d, const double *bvec, fpsq_band_qp *out);
int fpsq_band_qp_destroy(fpsq_band_qp qp);
int fpsq_band_qp_objgrad(fpsq_band b, fpsq_band_qp qp, const double *x, double sigma, double rho, double eta,
                         const double *xk, double *fx, double *gx, double *ys, double *gs);
int fpsq_band_qp_hprod(fpsq_band b, fpsq_band_qp qp, const double *v, double sigma, double rho, double eta,
                       int32_t hessian_approx, double *Hv);
int fpsq_band_jac_mul(fpsq_band b, int32_t trans, double alpha, const double *x, double beta, double *y);
int fpsq_band_set_input_stream(fpsq_band b, int32_t enabled, void *hip_stream);

/* ---- the device-resident model with NONLINEAR equality constraints on the banded handle: a QP objective with
 * separable-quadratic constraints on the pattern of A,
 *     f(x) = 1/2 x' diag(q) x + d'x,    c_i(x) = sum_j (A_ij + 1/2 H_ij x_j) x_j - b_i,    H has exactly the sparsity of A,
 * so that J(x)_ij = A_ij + H_ij x_j keeps the handle's pattern for every x, sum_i y_i Hess c_i = diag(H'y) and
 * ghjvprod(x, g, v) = H (g .* v).  Unlike the fpsq_band_qp_* group, whose Jacobian is constant and whose factor is the caller's
 * to keep, this model's Jacobian moves with x: an objgrad REFACTORISES, as the reference's LDLtSolver does per solve_two_mixed
 * (src/solve_linear_system.jl:223-251).  The multiplier-weighted curvature in Hsv, Sstw, ghjvprod and the separate hprod! Val(1)
 * (src/model-Fletcherpenaltynlp.jl:382-399, :572-634), which vanish on the fpsq_band_qp_* model, are live here.  Pointers are
 * host or device pointers, calls are synchronous and honour fpsq_band_set_input_stream; sums are formed in a fixed order (same
 * arguments, same bits).
 *   fpsq_band_nlp_create  a_vals, h_vals: the values of A and H in the order fpsq_band_factorize takes its values (the CSR the
 *                         handle was created with); bvec in the caller's row order.  All are copied.  Handles without border rows
 *                         or long columns are accepted, reordered and two-chain ones included; a handle with border rows, with
 *                         long columns (they change the transposed structure) or created by a fpsq_band_create_coo* entry (its
 *                         callers do not know the slot order) gives FPSQ_ERR_STATE and a message that names which.
 *   fpsq_band_nlp_create_arrow  the same parameter list for a handle of ANY kind but the last: border rows, long columns, both
 *                         (fpsq_band_create_bordered, _create_bordered_cols, _create_arrow) or neither (then the model gives
 *                         the bits of fpsq_band_nlp_create's); only a handle of a fpsq_band_create_coo* entry is refused
 *                         (FPSQ_ERR_STATE, the same message).  Every entry below takes the model whichever entry made it, with
 *                         the same state rules and soft codes; a failing border pivot in an objgrad's factorisation is reported
 *                         or regularised exactly as fpsq_band_factorize does on that handle.  Border rows cost nothing beyond
 *                         the handle's own correction of an M-solve.  With long columns the transposed value arrays gain the
 *                         virtual entries of "LONG COLUMNS" (J': 1, H': 0), and an objgrad / an hprod Val(1) adds two launches: the chunk
 *                         sums of U'c resp. U'(J v) into the virtual rows (as fpsq_band_qp_objgrad has them), and one workgroup
 *                         per long column that forms (H'q1)_j, (H'q2)_j, (H'c)_j from the column's own entries in a fixed order
 *                         and completes gx_j, (q - H'ys)_j, (H'c)_j resp. Hv_j -- the transposed rows of a long column are
 *                         virtual and carry no curvature.  An objgrad adds a third when the band is formed by row pairs
 *                         (FPSQ_BAND_FORM=1: the gather of the other columns' values).  hprod Val(2) adds none.
 *   fpsq_band_nlp_objgrad one `objgrad!` at a fresh x: (1) J(x) is written into the handle's value arrays; (2) the numeric
 *                         factorisation of J J' + delta I runs on them -- the return value is the soft code 1 with *info (may be
 *                         NULL) as fpsq_band_factorize gives them, and with it nothing is evaluated and no output is written;
 *                         (3) (p1, q1, p2, q2) = solve_two_mixed(g, c), g = q .* x + d; (4) ys = q1 + sigma q2,
 *                         gs = p1 + sigma p2,
 *                           gx = gs - (q - H'ys) .* p2 + sigma p2 + (H'q2) .* gs + rho J'c + eta (x - xk);
 *                         (5) *fx = f - c'ys + rho/2 c'c + eta/2 |x - xk|^2 (a HOST double).  The rho and eta terms enter only
 *                         when the parameter is positive; xk NULL means 0; gx, ys, gs may be NULL.  gx is the gradient of the
 *                         function *fx is a value of: Hsv is formed with -ys, as `hprod!` and `hess_coord!` form it (:477, :538,
 *                         :590), not with +ys as `grad!` has it (:382, :415) -- the two agree only when the constraints are
 *                         linear.  AFTERWARDS THE HANDLE'S VALUES ARE J(x): fpsq_band_jac_mul multiplies with J(x), and
 *                         a fpsq_band_qp_* model on this handle would evaluate on J(x) until the handle is factorised again.
 *   fpsq_band_nlp_hprod   one `hprod!` at the point of the LAST SUCCESSFUL objgrad of this model, on its factor.  The model
 *                         keeps qe = q - H'ys, hc = H'c and gs from that evaluation.
 *                         hessian_approx = 2 (:521-570): (p1, _, p2, _) = solve_two_least_squares(v, qe .* v), Ptv = v - p1,
 *                           Hv = p2 - qe .* Ptv + 2 sigma Ptv [+ hc .* v + rho J'(J v)] [+ eta v]
 *                         (the brackets enter when rho > 0 resp. eta > 0; Hcv is NOT scaled by rho, :562).
 *                         hessian_approx = 1 (:572-634): the same with rho (hc .* v + J'(J v)) (:626), and additionally
 *                           Hv -= J'z + (H'q1) .* gs,   z = M^-1 H (gs .* v),  q1 = M^-1 J v (the first solve's own multipliers).
 *                         z comes from the cached factor, M = J J' + delta I: the reference's tau = max(delta, 1e-14) (:148 of
 *                         solve_linear_system.jl) differs only for delta < 1e-14, by O(1e-14 |M^-1|).  Any other value:
 *                         FPSQ_ERR_ARG.  Without a prior successful objgrad of THIS model, or when anyone has factorised the
 *                         handle since (fpsq_band_factorize[_coo], another model's objgrad): FPSQ_ERR_STATE with a message -- the
 *                         handle counts its factorisations and the model remembers the count it saw.
 *   fpsq_band_nlp_cons    c(x) in the caller's row order: one launch on the model's own arrays, no factor needed.
 *   fpsq_band_nlp_create_coupled  the same model with COUPLING TERMS: nterms terms t = (t_row, t_j, t_k, t_w), each adding
 *                         t_w x_tj x_tk to c_trow, so that with "t in i" for t_row = i
 *                           c_i(x)  = sum_j (A_ij + 1/2 H_ij x_j) x_j + sum_{t in i} w_t x_jt x_kt - b_i,
 *                           J(x)_ij = A_ij + H_ij x_j + sum_{t in i, jt = j} w_t x_kt + sum_{t in i, kt = j} w_t x_jt,
 *                           sum_i y_i Hess c_i = diag(H'y) + Wo(y),  Wo(y)_jk = Wo(y)_kj = sum_{t: {jt, kt} = {j, k}} w_t y_trow,
 *                           ghjvprod(x, g, v)_i = sum_j H_ij g_j v_j + sum_{t in i} w_t (g_jt v_kt + g_kt v_jt).
 *                         t_row: 0-based rows in the caller's order; t_j, t_k: 0-based columns, BOTH entries of row t_row of the
 *                         handle's pattern (store an explicit A_ij = 0 where need be), so J(x) keeps the pattern and the symbolic
 *                         phase, the orderings and the factorisation are those of the handle.  Host or device pointers; all are
 *                         copied.  The terms are checked once, on the host: an index out of range, jt = kt (a square belongs to
 *                         h_vals), a pair {j, k} listed twice in a row (in either order), a (row, j) or (row, k) that is not an
 *                         entry of the pattern give FPSQ_ERR_ARG with a message.  Handles as fpsq_band_nlp_create takes them
 *                         (border rows, long columns, _coo: FPSQ_ERR_STATE with its messages).  The entries above take the model,
 *                         with the same state rules and soft codes, and compute fpsq_band_nlp_objgrad's / _hprod's formulas with
 *                         diag(H'y) + Wo(y) in the place of diag(H'y) everywhere: with E = diag(q - H'ys) - Wo(ys),
 *                           gx = gs - E p2 + sigma p2 + (diag(H'q2) + Wo(q2)) gs + rho J'c + eta (x - xk),
 *                           Val(2): (p1, _, p2, _) = solve_two_least_squares(v, E v), Hv = p2 - E Ptv + 2 sigma Ptv
 *                                   [+ (diag(H'c) + Wo(c)) v + rho J'(J v)] [+ eta v],
 *                           Val(1): the same with rho ((diag(H'c) + Wo(c)) v + J'(J v)), and
 *                                   Hv -= J'z + (diag(H'q1) + Wo(q1)) gs,  z = M^-1 ghjvprod(x, gs, v).
 *                         With nterms = 0 (the term pointers may be NULL) the model IS fpsq_band_nlp_create's: the same launches,
 *                         the same bits.  With terms an objgrad is 8 launches besides the factorisation and the sweeps (the
 *                         separable model: 6), hprod Val(2) 4 or 5 (3 or 4), Val(1) 6 (5); S = the pattern of Wo, its contributor
 *                         lists and the per-entry partner lists are built at create.
 *   fpsq_band_nlp_create_coupled_arrow  fpsq_band_nlp_create_coupled's parameter list, checks, messages and formulas for a
 *                         handle of ANY kind but a fpsq_band_create_coo* one (FPSQ_ERR_STATE, fpsq_band_nlp_create's message), as
 *                         fpsq_band_nlp_create_arrow takes them: a free final time or a global parameter that multiplies the
 *                         dynamics is a coupling term whose second column is a long column.  Terms may lie in band rows and in
 *                         border rows, between two band columns, a band column and a long column, or two long columns.  The
 *                         state rules and soft codes are unchanged; a failing border pivot is reported or regularised as on
 *                         fpsq_band_nlp_create_arrow.  With nterms = 0 the model IS fpsq_band_nlp_create_arrow's on that handle,
 *                         on a handle without border rows and long columns it IS fpsq_band_nlp_create_coupled's: the same
 *                         launches, the same bits.  A long column coupled to the states owns a row of S with up to m entries:
 *                         those rows are kept out of the CSR the lane-group kernels walk (there they are empty) and summed by
 *                         one workgroup per long column, in a fixed order and without atomics.  Launches besides the
 *                         factorisation and the sweeps, on a handle with long columns: an objgrad 11 (fpsq_band_nlp_create_arrow:
 *                         8; one more each when the band is formed by row pairs), hprod Val(2) 7 or 8 (the separable model on
 *                         that handle: 4 or 5), Val(1) 10 (7).  FPSQ_BAND_NLP_LONG_ROWS=0, read at create, leaves the long rows
 *                         inside S for the lane-group kernels (one launch fewer per objgrad, two per hprod): the independent form
 *                         the split one is measured and cross-checked against (profiles/band_coupled_arrow_nlp.md).
 *   fpsq_band_nlp_create_fn  the model with ELEMENTWISE FUNCTION TERMS: one code byte per entry (fn_codes, in the order of
 *                         a_vals; host or device pointer, copied) names phi from the table FPSQ_FN_* below, and
 *                           c_i(x)  = sum_j (A_ij x_j + H_ij phi_kij(x_j)) - b_i,
 *                           J(x)_ij = A_ij + H_ij phi'(x_j),     sum_i y_i Hess c_i = diag(G(x)'y),  G(x)_ij = H_ij phi''(x_j),
 *                           ghjvprod(x, g, v) = G(x) (g .* v):
 *                         sin theta of a rotating body, a reaction rate exp, a cubic spring, a saturating tanh.  J(x) keeps the
 *                         pattern, so the handle, its orderings and the factorisation are untouched.  Handles as
 *                         fpsq_band_nlp_create_arrow takes them (plain, reordered, two-chain, border rows, long columns, arrow;
 *                         a fpsq_band_create_coo* handle: FPSQ_ERR_STATE, its message under this entry's name).  A code >= 6
 *                         gives FPSQ_ERR_ARG and a message that names the first such entry.  With fn_codes NULL or every code 0
 *                         (phi = 1/2 x^2) the model IS fpsq_band_nlp_create_arrow's on that handle: the same launches, the same
 *                         bits.  The entries above take the model with the same state rules, soft codes and formulas, H' read
 *                         as G(x)': the curvature coefficient is an array that every objgrad rewrites next to J(x) (both in
 *                         the stored and in the transposed order, by the same device function: the same bits), and an hprod
 *                         runs on the G of the last successful objgrad, which the model keeps.  c(x) inside an objgrad is
 *                         sum_k (J_k x_c - rem_k) - b with the remainder rem = H (phi'(x) x - phi(x)) written next to J;
 *                         fpsq_band_nlp_cons evaluates phi itself.  The model adds NO launch to any evaluation -- the two value
 *                         launches of an objgrad are replaced by their function forms --, one 4-byte readback per objgrad and
 *                         nnz + t_nnz + nnz doubles.  NON-FINITE J(x) (exp overflows above 709; every entry is evaluated
 *                         whatever its H_ij): the value launch raises a word the objgrad reads BEFORE it factorises; it then
 *                         returns the soft code 1 with *fx = nan, *info = -1 (no pivot row), nothing factorised, nothing
 *                         evaluated and no output written -- what a failed factorisation returns, and the state an hprod
 *                         refuses.  Function terms TOGETHER with coupling terms are not offered.
 *   fpsq_band_nlp_set_objective_terms  ELEMENTWISE FUNCTION TERMS IN THE OBJECTIVE of a model made by ANY of the five create
 *                         entries: one weight w_j and one code byte per VARIABLE (n doubles, n bytes; host or device pointers,
 *                         copied; codes NULL: every code 0) name psi from the same table, and
 *                           f(x) = 1/2 x' diag(q) x + d'x + sum_j w_j psi_kj(x_j),
 *                           grad f = q .* x + d + w .* psi'(x),     Hess f = diag(q_x),  q_x = q + w .* psi''(x):
 *                         a pendulum's potential energy sum (1 - cos theta_k), an exponential control cost, a saturating tanh
 *                         tracking term, a cubic regulariser.  The constraints, J(x), the pattern and the factorisation are
 *                         untouched.  In the formulas of fpsq_band_nlp_objgrad / _hprod above, g is grad f(x) and every q is q_x:
 *                         qe = q_x - H'ys (with coupling terms E = diag(q_x - H'ys) - Wo(ys)), and f gains sum_j w_j psi(x_j).
 *                         An entry with w_j = 0 contributes exactly nothing and is NOT evaluated (exp at x_j = 800 under
 *                         w_j = 0 is harmless, and its code byte may hold anything); a code >= 6 under w_j != 0 gives
 *                         FPSQ_ERR_ARG and a message that names the first such j; a model of another handle: FPSQ_ERR_ARG.
 *                         w NULL REMOVES the terms: the model is then the one it was before, with the same launches and the
 *                         same bits.  The call may come at any time and any number of times; it clears the model's point, so
 *                         an hprod after it gives FPSQ_ERR_STATE ("no successful objgrad") until the next objgrad.  An objgrad
 *                         with terms adds ONE elementwise launch behind the value launches of J(x) and before the factorisation:
 *                         it rewrites the effective vectors q_x and d_e = d + w .* (psi'(x) - psi''(x) .* x) -- so that
 *                         q_x .* x + d_e = grad f(x) and the kernels that take (q, d) take (q_x, d_e) unchanged -- and sums f in
 *                         a fixed order into one partial per workgroup (no atomics on doubles), from which *fx is finished.
 *                         A Hessian product and fpsq_band_nlp_cons add none: they run on what the objgrad left.  NON-FINITE
 *                         OBJECTIVE: a non-finite w_j psi, w_j psi' or w_j psi'' raises the word a non-finite J(x) raises, read
 *                         once per objgrad BEFORE it factorises (a model with both kinds of terms reads once); the objgrad
 *                         returns what fpsq_band_nlp_create_fn describes -- soft code 1, *fx = nan, *info = -1, nothing
 *                         factorised or evaluated, no output written, the word cleared -- and the message says whether J(x),
 *                         the objective or both raised it.  Memory with terms: 3 n doubles (w, q_x, d_e), n code bytes and
 *                         one double per workgroup of the A-side grid; it stays with the model after the terms are removed.
 * Destroy a model before the handle it was created on. */
enum { /* phi, phi', phi'' of a function code (one byte per entry) */
  FPSQ_FN_HALFSQ = 0, /* 1/2 x^2,  x,         1                  */
  FPSQ_FN_CUBE6 = 1,  /* x^3 / 6,  1/2 x^2,   x                  */
  FPSQ_FN_SIN = 2,    /* sin x,    cos x,     -sin x             */
  FPSQ_FN_COS = 3,    /* cos x,    -sin x,    -cos x             */
  FPSQ_FN_EXP = 4,    /* exp x,    exp x,     exp x              */
  FPSQ_FN_TANH = 5,   /* t = tanh x,  1 - t^2,  -2 t (1 - t^2)   */
  FPSQ_FN_COUNT = 6
};
typedef struct fpsq_band_nlp_s *fpsq_band_nlp;
int fpsq_band_nlp_create(fpsq_band b, const double *qdiag, const double *d, const double *bvec, const double *a_vals,
                         const double *h_vals, fpsq_band_nlp *out);
int fpsq_band_nlp_create_arrow(fpsq_band b, const double *qdiag, const double *d, const double *bvec, const double *a_vals,
                               const double *h_vals, fpsq_band_nlp *out);
int fpsq_band_nlp_create_fn(fpsq_band b, const double *qdiag, const double *d, const double *bvec, const double *a_vals,
                            const double *h_vals, const uint8_t *fn_codes, fpsq_band_nlp *out);
int fpsq_band_nlp_create_coupled(fpsq_band b, const double *qdiag, const double *d, const double *bvec,
                                 const double *a_vals, const double *h_vals,
                                 int64_t nterms, const int32_t *t_row, const int32_t *t_j, const int32_t *t_k,
                                 const double *t_w, fpsq_band_nlp *out);
int fpsq_band_nlp_create_coupled_arrow(fpsq_band b, const double *qdiag, const double *d, const double *bvec,
                                       const double *a_vals, const double *h_vals,
                                       int64_t nterms, const int32_t *t_row, const int32_t *t_j, const int32_t *t_k,
                                       const double *t_w, fpsq_band_nlp *out);
int fpsq_band_nlp_set_objective_terms(fpsq_band b, fpsq_band_nlp nlp, const double *w, const uint8_t *codes);
int fpsq_band_nlp_destroy(fpsq_band_nlp nlp);
int fpsq_band_nlp_objgrad(fpsq_band b, fpsq_band_nlp nlp, const double *x, double sigma, double rho, double eta, double delta,
                          const double *xk, double *fx, double *gx, double *ys, double *gs, int32_t *info);
int fpsq_band_nlp_hprod(fpsq_band b, fpsq_band_nlp nlp, const double *v, double sigma, double rho, double eta,
                        int32_t hessian_approx, double *Hv);
int fpsq_band_nlp_cons(fpsq_band b, fpsq_band_nlp nlp, const double *x, double *c);

/* ---- block entries on the cached banded factor: k vectors per call.  A triangular sweep streams the whole factor whether it
 * carries one vector or several, so these entries carry a TILE of 8 vectors (16 right-hand-side columns: the two M-solves of
 * each) through one pair of sweeps on the fp64 matrix cores; k > 8 is processed in successive tiles of 8.
 * A block is k vectors stored one after the other: vector j of an n-block starts at base + j * n (a C-contiguous (k, n) array);
 * q1 / q2 are (k, m).  Pointers are host or device; device-resident blocks are read and written in place.  Calls are
 * synchronous (outputs complete on return), honour fpsq_band_set_input_stream, update last_solve_ms and return
 * FPSQ_ERR_STATE without a valid factor.  Work buffers (16 (n + 2 mpad) + 8 mpad doubles, the publication buffer, 8 n more for
 * a sparse Q, staging for host-resident blocks) are allocated at the first block call and freed with the handle.
 *   fpsq_band_solve_two_least_squares_block  column j = fpsq_band_solve_two_least_squares(rhs1[j], rhs2[j]); any of p1, q1, p2, q2
 *                         may be NULL and is then not produced.  k < 1 or a NULL right-hand side: FPSQ_ERR_ARG.
 *   fpsq_band_qp_hprod_block  column j = fpsq_band_qp_hprod on V[j], for both models (fpsq_band_qp_create, _create_csr);
 *                         hessian_approx 1 and 2 give the same bits, any other value FPSQ_ERR_ARG, as do k < 1, a NULL block
 *                         and V / HV ranges that overlap (message in fpsq_band_last_error).
 *   fpsq_band_qp_objgrad_block  column j = fpsq_band_qp_objgrad at X[j], on the model qp (either kind) with its linear term
 *                         replaced by D[j] and its right-hand side by Bv[j]: a family of QPs that share A and Q -- and so the
 *                         factor -- but differ in d and b, or k points of one QP.  D: (k, n), NULL = the model's d for every
 *                         column; Bv: (k, m) in the caller's row order, NULL = the model's b.  So g_j = Q X[j] + d_j,
 *                         c_j = A X[j] - b_j, and the formulas of fpsq_band_qp_objgrad from there on (the rho and eta terms
 *                         only when the parameter is positive; XK: (k, n), NULL with eta > 0 means xk = 0).  fx: k doubles
 *                         on the HOST, required; GX, GS (k, n) and YS (k, m) may be NULL and are then not produced.
 *                         FPSQ_ERR_ARG (message in fpsq_band_last_error): k < 1, a NULL X or fx, a model of another handle,
 *                         an output block whose range overlaps an input block or another output block.  The partial sums
 *                         of the scalars (5 x 2048 x 8 doubles) are allocated at the first call of this entry.
 * DETERMINISM: a column's result -- fx[j] included -- is bitwise independent of k, of the column's position in the block and
 * of what the other columns hold (short tiles are padded with zero columns; every column's sums have a fixed order: the
 * grids depend on the shape alone, per-column partial sums are laid out [workgroup][column] and summed in index order, no
 * floating-point atomics), and repeatable from call to call.  It is NOT bitwise the single-vector entry's -- the matrix-core
 * sweep sums in another order than the vector-unit sweep --; both meet the same bar against the exact solve. */
int fpsq_band_solve_two_least_squares_block(fpsq_band b, int32_t k, const double *rhs1, const double *rhs2, double *p1,
                                            double *q1, double *p2, double *q2);
int fpsq_band_qp_hprod_block(fpsq_band b, fpsq_band_qp qp, int32_t k, const double *V, double sigma, double rho, double eta,
                             int32_t hessian_approx, double *HV);
int fpsq_band_qp_objgrad_block(fpsq_band b, fpsq_band_qp qp, int32_t k, const double *X, const double *D, const double *Bv,
                               double sigma, double rho, double eta, const double *XK, double *fx, double *GX, double *YS,
                               double *GS);

/* ---- introspection for benchmarks / profiling */
typedef struct {
  int64_t n, m, nnz;
  int64_t spmv_a_blocks, spmv_at_blocks; /* workgroups per A / A' product */
  double last_solve_ms;                  /* device time of the last solve_two_* / qp_objgrad (HIP events) */
  double last_spmv_ms;                   /* device time inside SpMV/SpMM kernels during that call */
  int64_t last_spmv_launches;
  int64_t last_kernel_launches;
  int64_t last_prod_a[2];  /* launches of the A  product during that call with 1 and with 2 right-hand sides */
  int64_t last_prod_at[2]; /* same for the A' product */
  int64_t at_sorted;       /* 1: the row blocks of A' are stored column-sorted (coalesced gathers, see k_spmv<.., CSORT>) */
  int64_t comm_route;      /* 0: single GPU; else FPSQ_ROUTE_RCCL / _P2P (decided at the first solve of a halo-sharded handle)
                              / _LOCAL / _LOCAL_P2P (in-process groups) */
  int64_t last_fused_launches; /* of the launches counted in last_prod_a[1] AND last_prod_at[1]: those that carried both products of a
                                  joint iteration in one grid (k_iter_fused; FPSQ_FUSE_ITER=0 disables) */
  /* CUMULATIVE over the life of the handle -- all three are 0 on a healthy run; a test or a benchmark asserts so:
   *   fuse_fallbacks  calls that ran into a bounded wait of a one-launch iteration and were REPEATED on two launches per
   *                   iteration (the caller saw a delay and rc = the repeated call's; the handle stays on two launches);
   *   wait_timeouts   calls in which a bounded wait inside a product launch expired (leaders' record, block flags, tagged
   *                   partials) -- every fuse_fallback is one of them, the others ended in FPSQ_ERR_TIMEOUT;
   *   p2p_timeouts    calls in which a bounded wait for a PEER's record expired (peer-to-peer route): FPSQ_ERR_TIMEOUT. */
  int64_t fuse_fallbacks, wait_timeouts, p2p_timeouts;
  /* the Krylov loop of the last call: joint iterations enqueued and kernel launches enqueued for them (exchanges and stand-alone
   * steps included; start-up and epilogue excluded): launches / iterations = launches per joint iteration */
  int64_t last_loop_iterations, last_loop_launches;
  int64_t last_multi_launches, last_multi_iterations; /* of last_fused_launches: joint iterations that shared a launch with others
                                  (k_iter_multi: several iterations per launch, FPSQ_MULTI_ITER=1 disables), and how many launches
                                  carried them: launches of the call = last_prod_a + last_prod_at - last_fused_launches
                                  - (last_multi_iterations - last_multi_launches) */
  int64_t comm_in_launch_sums; /* 1: a sharded handle whose sums over the ranks need no launch of their own -- formed inside the
                                  launches that need them (peer-to-peer route, every rank on a device of its own: csrc
                                  fpsq_krylov.hip.h xch_sum), or a communicator of one rank; 0: gather / collective launches */
} fpsq_info;
int fpsq_get_info(fpsq_handle h, fpsq_info *info);
/* on != 0: bracket every SpMV/SpMM launch with HIP events on the solver's stream so that last_spmv_ms is filled
 * (adds event records between kernels; leave off when timing whole evaluations) */
int fpsq_set_profiling(fpsq_handle h, int32_t on);

/* Test hook for the run-ahead heuristics of the Krylov loop.  A solve normally enqueues the iterations of the PREVIOUS call
 * of the same kind without looking at the device and, right behind them, its final vector update and the caller's epilogue
 * kernels gated on the recurrences' `done` flags (csrc/fpsq_run.hip.h run_krylov).  This call overrides that expected count for
 * the NEXT solve call of the handle only (expect >= 0; 0 = "unknown": no speculation), so that tests can place the
 * speculation before, at and behind the true iteration count deterministically.  Results never depend on it. */
int fpsq_debug_expect_iterations(fpsq_handle h, int64_t expect);

const char *fpsq_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FPSQ_H */
