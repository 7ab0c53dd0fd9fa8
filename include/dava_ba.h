/*
 * dava_ba.h -- C ABI of the MI355X (gfx950) batched BFGS bundle-adjustment solver.
 *
 * This is the drop-in boundary for the one hot path of
 * jskinn/deep-attention-visual-odometry that this project replaces: the
 * `autograd_solvers/` BFGS loop + strong-Wolfe line search evaluated on a
 * multi-view pinhole (+ Brown-Conrady) reprojection objective.  The reference
 * is pure PyTorch (no FFI exists there); each entry point below names the
 * reference interface it replaces.  The Python mirror of the reference API
 * (deep_attention_visual_odometry_amd.autograd_solvers) binds these symbols
 * through ctypes; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer (HBM) unless stated otherwise.
 *    Struct arguments themselves are host memory.
 *  - `stream` is a hipStream_t (NULL = default stream); all work is
 *    enqueued asynchronously on it, nothing synchronises the host, and no
 *    entry point allocates memory (caller supplies the workspace), so every
 *    call is graph-capturable.
 *  - Functional ownership, like the reference (`bfgs_solver.py:197`):
 *    inputs are never written; outputs may not alias inputs unless stated.
 *  - Return value: DAVA_OK or a DAVA_ERR_* code; nothing throws across the ABI.
 *    dava_status_string() turns a code into text.
 *  - fp32 throughout the fused solver (the reference's dtype for the BA path),
 *    with an opt-in float64 flavour of the objective evaluation and of the
 *    one-launch COMPACT solve, its second derivatives and its adjoint (the
 *    `_f64` entry points on DavaSceneF64: the
 *    reference's training entry point and its solver / geometry tests run in
 *    float64); the generic BFGS building blocks come in _f32 and _f64 flavours
 *    because the reference's own unit tests drive them in float64.
 */
#ifndef DAVA_BA_H
#define DAVA_BA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAVA_ABI_VERSION 4

enum DavaStatus {
  DAVA_OK = 0,
  DAVA_ERR_INVALID_ARGUMENT = 1, /* bad sizes / null pointers / P mismatch  */
  DAVA_ERR_WORKSPACE = 2,        /* workspace missing or too small          */
  DAVA_ERR_LAUNCH = 3,           /* HIP launch failure                      */
  DAVA_ERR_UNSUPPORTED = 4       /* shape outside what this build supports  */
};

/* Representation of the inverse Hessian inside the fused solver. */
enum DavaHessianMode {
  DAVA_HESSIAN_DENSE = 0,  /* dense P x P fp32 per problem in HBM (the reference's data structure) */
  DAVA_HESSIAN_COMPACT = 1 /* exact rank-2 update history (s_j, H_{j-1} y_j): same math, O(kP) bytes;
                            * past 1024 updates (iterations > 1025) a problem that is still running
                            * folds its history into the dense matrix once and continues DENSE */
};

/* Why a problem stopped (bfgs_solver.py:143-145, :203-207). */
enum DavaStopReason {
  DAVA_STOP_ITERATIONS = 0, /* ran `iterations` steps                 */
  DAVA_STOP_ERROR = 1,      /* error <= error_threshold (or NaN)      */
  DAVA_STOP_STEP = 2,       /* ||step|| <= minimum_step (or NaN)      */
  DAVA_STOP_DROP = 3        /* training-mode drop path (drop_path_p)  */
};

/* Per-(view, point) residual summed into the objective.
 *  SQUARED_REPROJECTION: vis * |pi(X) - obs|^2  -- the benchmark objective.
 *  RAY_ANGLE: vis * angle(ray(obs), p) with ray(obs) = (u - cx, v - cy, elu(f) + 1) and p the
 *    camera-relative point: the error CalibrationNetwork minimises (calibration_network.py:58-67,
 *    geometry/homogeneous_projection.py:21-44, geometry/projective_plane_angle_distance.py:20-64).
 *    Pinhole only (distortion must be 0).                                                      */
enum DavaResidual {
  DAVA_RESIDUAL_SQUARED_REPROJECTION = 0,
  DAVA_RESIDUAL_RAY_ANGLE = 1
};

/* A batch of independent calibration problems.
 * Parameter layout per problem (calibration_pinhole_camera_model.py:33-75):
 *   [f, cx, cy | X_0..X_{N-1} (xyz) | t_1..t_{M-1} | w_1..w_{M-1} | k1 k2 k3 p1 p2 (if distortion)]
 * num_parameters must equal 3 + 3N + 6(M-1) + 5*distortion.                     */
typedef struct DavaScene {
  int32_t batch;               /* B >= 0                               */
  int32_t num_views;           /* M >= 2                               */
  int32_t num_points;          /* N >= 1                               */
  int32_t distortion;          /* 0 = pinhole, 1 = + Brown-Conrady     */
  int32_t num_parameters;      /* P                                    */
  const float* observations;   /* (B, M, N, 2) fp32                    */
  const uint8_t* visibility;   /* (B, M, N) 0/1                        */
  int32_t residual;            /* DavaResidual                         */
} DavaScene;

/* Mirrors the eval-mode BFGSSolver constructor (bfgs_solver.py:49-78). */
typedef struct DavaSolverConfig {
  float sufficient_decrease;      /* c1, default 1e-4                          */
  float curvature;                /* c2, default 0.9                           */
  float error_threshold;          /* default 1e-4                              */
  float minimum_step;             /* default 1e-8                              */
  int32_t iterations;             /* default 1000                              */
  int32_t max_line_search_trials; /* 1000 in wolfe_conditions.py:116           */
  int32_t strong_wolfe;           /* 1 (bfgs_solver.py:189)                    */
  int32_t hessian_mode;           /* DavaHessianMode                           */
  /* Training mode's drop path (bfgs_solver.py:121-125): at the top of every iteration a problem
   * keeps updating only if a uniform draw in [0, 1) exceeds drop_path_p, else it stops for good
   * (DAVA_STOP_DROP).  Draws are counter-based (seed, problem, iteration): the same seed gives the
   * same schedule on any launch shape.  0 = eval mode (the default).                           */
  float drop_path_p;
  uint32_t drop_seed_lo, drop_seed_hi;
  /* Training mode's return_second_last (bfgs_solver.py:196-212): a problem that stops by the
   * minimum-step rule returns the parameters BEFORE its last step (x_k, not x_{k+1}); every other
   * stop returns the current ones, as without it.  0 = off (the default).  The reference's own
   * masked_scatter also moves rows between problems when a problem stops this way while a later
   * problem of the batch continues; the caller detects that case from the status words (the Python
   * module then runs the reference's loop instead).                                */
  int32_t return_second_last;
} DavaSolverConfig;

/* Per-problem status written by dava_ba_solve: int32 (B, 4) =
 * {steps taken, DavaStopReason, objective evaluations, line-search trials}. */
#define DAVA_STATUS_WORDS 4

/* Bytes of device workspace dava_ba_solve needs for this scene/config: the solve's state
 * (inverse-Hessian representation; O(P) vectors for large P) followed by a 256-byte
 * work-queue counter.  A workspace of this size lets the launch run one workgroup per
 * resident slot, each taking the next problem when it finishes one (problems that stop
 * early free their slot); a workspace without the counter's 256 bytes still works, one
 * workgroup per problem. */
size_t dava_ba_solve_workspace_bytes(const DavaScene* scene, const DavaSolverConfig* config);

/* How dava_ba_solve runs a scene/config (host-only query, no device needed): lets a caller
 * account for the HBM traffic of the launch (benchmarks, roofline) without re-deriving it. */
typedef struct DavaSolvePlan {
  int32_t global_vectors;      /* 1: the O(P) state lives in the workspace (large P), 0: in LDS  */
  int32_t workgroup_threads;   /* threads of the one workgroup that solves a problem            */
  int32_t lds_bytes;           /* dynamic LDS per workgroup                                     */
  int32_t lds_history_entries; /* COMPACT: the oldest history entries kept on-chip, never in HBM */
} DavaSolvePlan;
int dava_ba_solve_plan(const DavaScene* scene, const DavaSolverConfig* config, DavaSolvePlan* plan_out);

/* The whole eval-mode solve, one launch.
 * Replaces BFGSSolver.forward(parameters, error_function)
 * (autograd_solvers/bfgs_solver.py:80-215) with error_function = the objective
 * over `scene` (its `residual`), including line_search_wolfe_conditions
 * (autograd_solvers/line_search/wolfe_conditions.py:23-239, strong=True).
 *   x0        (B, P) fp32 initial guess
 *   x_out     (B, P) fp32 result (may alias x0)
 *   error_out (B)    fp32 objective at x_out, or NULL
 *   status_out(B, 4) int32, or NULL                                         */
int dava_ba_solve(const DavaScene* scene, const DavaSolverConfig* config, const float* x0, float* x_out,
                  float* error_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                  void* stream);

/* ---- differentiating THROUGH the fused solve (the reference's create_graph mode,
 * bfgs_solver.py:85, :133-135, :213-215: every iteration's gradient kept in the graph, the
 * line search's step size a constant) without a dense (B, P, P) inverse Hessian per iteration.
 * A recording solve keeps a tape in HBM (x_k, g_k, the compact history rows, step sizes; see
 * csrc/dava_tape.hpp); the adjoint replays it backwards, one workgroup per problem.
 * COMPACT mode only, iterations <= 1025 and P <= 14336: shapes whose O(P) state fits the LDS
 * (C1-C3) keep it there, larger ones (the forward's global-vector mode, e.g. C5 with P = 12381)
 * keep it in the adjoint's workspace.  Otherwise the size queries return 0 and the calls
 * DAVA_ERR_UNSUPPORTED. */

/* Bytes of the tape (including the work-queue counter's 256 bytes), or 0 if unsupported. */
size_t dava_ba_solve_tape_bytes(const DavaScene* scene, const DavaSolverConfig* config);

/* dava_ba_solve (bitwise the same x_out, error_out and status_out) that also writes the tape.
 * status_out is required (the adjoint reads the steps each problem took). */
int dava_ba_solve_record(const DavaScene* scene, const DavaSolverConfig* config, const float* x0, float* x_out,
                         float* error_out, int32_t* status_out, void* tape, size_t tape_bytes, void* stream);

/* Device workspace of dava_ba_solve_backward, or 0 if unsupported. */
size_t dava_ba_solve_backward_workspace_bytes(const DavaScene* scene, const DavaSolverConfig* config);

/* History entries (s_j, w_j) the adjoint keeps in LDS for its whole reverse sweep (the oldest
 * ones, as many as one workgroup's LDS leaves room for, at most iterations - 1).  The library
 * reads no environment; only the test/A-B override dava_debug_set_override("ADJ_LDS_ENTRIES", n)
 * caps it.  Informational: for byte models. */
int dava_ba_solve_backward_lds_entries(const DavaScene* scene, const DavaSolverConfig* config);

/* Vector-Jacobian product of the recorded solve: given x_out_grad = dL/dx_out (B, P), writes
 *   x0_grad            (B, P)        dL/dx0
 *   observations_grad  (B, M, N, 2)  dL/dobs (or NULL)
 * scene/config/status must be those of the recording call, the tape unmodified. */
int dava_ba_solve_backward(const DavaScene* scene, const DavaSolverConfig* config, const void* tape,
                           size_t tape_bytes, const int32_t* status, const float* x_out_grad, float* x0_grad,
                           float* observations_grad, void* workspace, size_t workspace_bytes, void* stream);

/* One objective evaluation per problem at x + alpha[b] * direction.
 * Replaces one call of the reference-composed error function plus
 * torch.autograd.grad (bfgs_solver.py:131-135 / wolfe_conditions.py:134-143):
 *   direction (B, P) or NULL (then alpha is ignored and the point is x)
 *   alpha     (B)    or NULL (= 0)
 *   error_out (B)    E
 *   grad_out  (B, P) dE/dx at the point, or NULL
 *   slope_out (B)    d . dE/dx at the point (forward mode), or NULL (needs direction) */
int dava_ba_evaluate(const DavaScene* scene, const float* x, const float* direction, const float* alpha,
                     float* error_out, float* grad_out, float* slope_out, void* stream);

/* ---- float64 flavour of the evaluation and of the fused solve (additive to ABI 4) ----
 * The same objectives and the same algorithm with every value a double: parameters, observations,
 * thresholds (1e-4 as a double is the reference's 1e-4), history rows.  COMPACT inverse Hessian only;
 * dava_ba_solve_f64 / dava_ba_solve_record_f64 run eval mode, training mode's drop path and
 * return_second_last go through dava_ba_solve_train_f64 / dava_ba_solve_record_train_f64 (DavaTrainingF64,
 * below).  One 256-thread workgroup per problem with its whole state in LDS: these entry points support a
 * shape when that image fits 160 KiB (C1-C3 do; C5 does not) and 1 <= iterations <= 1025.  Anything else:
 * DAVA_ERR_UNSUPPORTED, and 0 from the size query.  Scenes beyond the LDS image evaluate and solve through
 * the `_large_f64` entry points further down; the recording solve, the adjoint and the second derivatives
 * keep the limit. */
typedef struct DavaSceneF64 {
  int32_t batch;               /* B >= 0                               */
  int32_t num_views;           /* M >= 2                               */
  int32_t num_points;          /* N >= 1                               */
  int32_t distortion;          /* 0 = pinhole, 1 = + Brown-Conrady     */
  int32_t num_parameters;      /* P                                    */
  const double* observations;  /* (B, M, N, 2) fp64                    */
  const uint8_t* visibility;   /* (B, M, N) 0/1                        */
  int32_t residual;            /* DavaResidual                         */
} DavaSceneF64;

typedef struct DavaSolverConfigF64 {
  double sufficient_decrease;     /* c1, default 1e-4                          */
  double curvature;               /* c2, default 0.9                           */
  double error_threshold;         /* default 1e-4                              */
  double minimum_step;            /* default 1e-8                              */
  int32_t iterations;             /* 1 .. 1025                                 */
  int32_t max_line_search_trials; /* 1000 in wolfe_conditions.py:116           */
  int32_t strong_wolfe;           /* 1 (bfgs_solver.py:189)                    */
} DavaSolverConfigF64;

/* Bytes of device workspace dava_ba_solve_f64 needs: the history rows,
 * B * 2 * max(iterations - 1, 1) * round_up(P, 4) * 8, followed by a 256-byte tail kept for a
 * work-queue counter (this version launches one workgroup per problem and leaves it unused).
 * 0 if the scene / config is invalid or unsupported.  dava_ba_solve_f64 requires a workspace of at
 * least this size (tail included) whenever iterations > 1, else DAVA_ERR_WORKSPACE. */
size_t dava_ba_solve_workspace_bytes_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config);

/* dava_ba_solve in float64: x0, x_out (B, P) fp64 (may alias), error_out (B) fp64 or NULL,
 * status_out (B, 4) int32 or NULL (the same four words). */
int dava_ba_solve_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config, const double* x0, double* x_out,
                      double* error_out, int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream);

/* dava_ba_evaluate in float64 (same NULL conventions). */
int dava_ba_evaluate_f64(const DavaSceneF64* scene, const double* x, const double* direction, const double* alpha,
                         double* error_out, double* grad_out, double* slope_out, void* stream);

/* ---- float64 second derivatives and the float64 adjoint of the fused solve (additive to ABI 4) ----
 * dava_ba_second_order_obs in float64: forward-over-reverse with dual numbers over double, one 256-thread
 * workgroup per problem, the dual image in LDS (DAVA_ERR_UNSUPPORTED past 160 KiB).  Per problem, with a
 * parameter direction v and an observation direction u (either NULL = 0):
 *   error_out (B) E, grad_out (B, P) dE/dx, hv_out (B, P) H v + (d2E/dx dobs) u,
 *   obs_grad_out (B, M, N, 2) dE/dobs, obs_hv_out (B, M, N, 2) (d2E/dobs dx) v + (d2E/dobs2) u.
 * Every output may be NULL. */
int dava_ba_second_order_f64(const DavaSceneF64* scene, const double* x, const double* direction,
                             const double* obs_direction, double* error_out, double* grad_out, double* hv_out,
                             double* obs_grad_out, double* obs_hv_out, void* stream);

/* Bytes of the float64 tape: csrc/dava_tape.hpp's blocks with every element a double,
 *   8 * B * (2 kcap Pv + 2 K Pv + round_up(3 K + 1, 4)) + 256,  K = iterations, kcap = max(K - 1, 1),
 *   Pv = round_up(P, 4).
 * > 0 exactly where dava_ba_solve_workspace_bytes_f64 is. */
size_t dava_ba_solve_tape_bytes_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config);

/* dava_ba_solve_f64 (bitwise the same x_out, error_out and status_out) that also writes the tape: x_k and g_k
 * at the start of every iteration, alpha_k, rho_j, c_j and gamma; the tape's history block is the solve's
 * workspace.  Slots the solve does not reach are zeroed.  status_out is required. */
int dava_ba_solve_record_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config, const double* x0,
                             double* x_out, double* error_out, int32_t* status_out, void* tape, size_t tape_bytes,
                             void* stream);

/* Device workspace of dava_ba_solve_backward_f64 (the adjoint's rows, 8 * B * K * Pv, and a 256-byte tail),
 * or 0 where it does not run: its LDS image (14 vectors of Pv doubles, the scene) must fit 160 KiB. */
size_t dava_ba_solve_backward_workspace_bytes_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config);

/* dava_ba_solve_backward in float64: x_out_grad (B, P) -> x0_grad (B, P), observations_grad (B, M, N, 2) or
 * NULL.  One workgroup per problem, deterministic (two launches give bitwise the same gradients). */
int dava_ba_solve_backward_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config, const void* tape,
                               size_t tape_bytes, const int32_t* status, const double* x_out_grad, double* x0_grad,
                               double* observations_grad, void* workspace, size_t workspace_bytes, void* stream);

/* ---- training mode of the float64 fused solve (additive to ABI 4) ----
 * DavaSolverConfig's training fields for the float64 entry points, with the float32 solve's semantics:
 *   drop_path_p > 0     before its first iteration a problem draws the iteration at which the drop path
 *                       stops it (bfgs_solver.py:121-125) from the counter-based generator of
 *                       (drop_seed, problem, iteration); the draw and its comparison with drop_path_p
 *                       are the float32 solve's, so one seed gives one schedule in both precisions.
 *                       A problem stopped this way reports DAVA_STOP_DROP; one stopped at iteration 0
 *                       returns x0 with 0 steps.
 *   return_second_last  a problem stopped by the minimum-step rule returns x before its last step
 *                       (bfgs_solver.py:196-212).  Its status words are the eval solve's: steps counts
 *                       the failed step.  A caller that differentiates such a solve therefore hands
 *                       dava_ba_solve_backward_f64 (as dava_ba_solve_backward in float32) a status whose
 *                       step count is one lower for every problem that stopped with DAVA_STOP_STEP: the
 *                       adjoint replays status[b][0] steps.
 * training == NULL, or a struct whose fields are all zero, is eval mode: the very launch of
 * dava_ba_solve_f64 / dava_ba_solve_record_f64.  drop_path_p outside [0, 1] (or NaN):
 * DAVA_ERR_INVALID_ARGUMENT, checked on the host before anything else.  Neither size query depends on
 * the training fields, and dava_ba_solve_backward_f64 takes tapes of either mode. */
typedef struct DavaTrainingF64 {
  float drop_path_p;                    /* [0, 1]; 0 = eval mode */
  uint32_t drop_seed_lo, drop_seed_hi;
  int32_t return_second_last;
} DavaTrainingF64;

int dava_ba_solve_train_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                            const DavaTrainingF64* training, const double* x0, double* x_out, double* error_out,
                            int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream);
int dava_ba_solve_record_train_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                   const DavaTrainingF64* training, const double* x0, double* x_out,
                                   double* error_out, int32_t* status_out, void* tape, size_t tape_bytes,
                                   void* stream);

/* Second derivatives of the objective, for differentiating THROUGH a solve whose error
 * function is a fused objective (the reference's create_graph double backward,
 * bfgs_solver.py:133-135).  Per problem, at x with direction v (per problem, NULL = 0):
 *   error_out (B)         E
 *   grad_out  (B, P)      dE/dx
 *   hv_out    (B, P)      (d^2E/dx^2) v
 *   obs_grad_out (B,M,N,2)  dE/dobs
 *   obs_hv_out   (B,M,N,2)  (d^2E/dobs dx) v
 * Every output may be NULL.  Forward-over-reverse of the same objective code (dual numbers).
 * Shapes whose dual LDS image exceeds 160 KiB return DAVA_ERR_UNSUPPORTED.                 */
int dava_ba_second_order(const DavaScene* scene, const float* x, const float* direction, float* error_out,
                         float* grad_out, float* hv_out, float* obs_grad_out, float* obs_hv_out, void* stream);
/* The same with an observation direction u (B, M, N, 2) as well (NULL = 0; r06, additive to ABI 4): the
 * observations carry tangent u, so
 *   hv_out     = (d^2E/dx^2) v + (d^2E/dx dobs) u
 *   obs_hv_out = (d^2E/dobs dx) v + (d^2E/dobs^2) u
 * -- what differentiating dE/dobs again needs (PyTorch double backward of the fused objectives). */
int dava_ba_second_order_obs(const DavaScene* scene, const float* x, const float* direction, const float* obs_direction,
                             float* error_out, float* grad_out, float* hv_out, float* obs_grad_out, float* obs_hv_out,
                             void* stream);

/* ---- fused gradient descent (additive to ABI 4) ----
 * Replaces SGDSolver.forward(parameters, error_function) (autograd_solvers/sgd_solver.py:29-44) with
 * error_function = the objective over `scene`:
 *   for k in 0 .. iterations-1:  x_{k+1} = x_k - learning_rate * dE/dx(x_k)
 * fp32; the update rounds the product, then the difference, as torch does.  No stopping rule, no mask.  One
 * launch, one workgroup per problem: the scene, x and the gradient in LDS (C1-C3), or x and the gradient in
 * LDS and the scene read in place (C5).  A scene whose image fits neither form: DAVA_ERR_UNSUPPORTED, and 0
 * from the size query.  iterations == 0 copies x0.  The FORCE_GV override asks for the second form. */
typedef struct DavaSgdConfig {
  float learning_rate;
  int32_t iterations; /* K >= 0 */
} DavaSgdConfig;

/*   x0 (B, P), x_out (B, P) (may alias x0), error_trace_out (B, K) E(x_k) for k = 0 .. K-1, or NULL */
int dava_ba_sgd_solve(const DavaScene* scene, const DavaSgdConfig* config, const float* x0, float* x_out,
                      float* error_trace_out, void* stream);

/* Bytes of the tape of a recording solve: x_k for k = 0 .. K-1 in rows of Pv = round_up(P, 4) floats, laid out
 * (B, K, Pv), no header: B * K * Pv * 4.  0 if the scene / config is invalid or unsupported (and for K = 0,
 * where no tape is needed and `tape` may be NULL). */
size_t dava_ba_sgd_tape_bytes(const DavaScene* scene, const DavaSgdConfig* config);

/* dava_ba_sgd_solve (bitwise the same x_out and error trace) that also writes the tape.  A tape below the
 * query's figure: DAVA_ERR_WORKSPACE. */
int dava_ba_sgd_solve_record(const DavaScene* scene, const DavaSgdConfig* config, const float* x0, float* x_out,
                             float* error_trace_out, void* tape, size_t tape_bytes, void* stream);

/* Host-only: 1 where dava_ba_sgd_backward runs this scene / config, else 0.  Its LDS image is the second
 * derivatives' dual image (dava_ba_second_order) plus a float accumulator for dL/dobs, and must fit 160 KiB
 * (C1-C3 do; C5 does not). */
int dava_ba_sgd_backward_supported(const DavaScene* scene, const DavaSgdConfig* config);

/* Vector-Jacobian product of the recorded descent: given x_out_grad = dL/dx_K (B, P), writes
 *   x0_grad            (B, P)        dL/dx_0
 *   observations_grad  (B, M, N, 2)  dL/dobs (or NULL: not formed; x0_grad is bitwise the same)
 * replaying the tape backwards with one dual-number pass of the objective per step:
 *   lambda <- lambda - lr H(x_k) lambda,  dL/dobs <- dL/dobs - lr (d2E/dobs dx)(x_k) lambda.
 * scene / config must be those of the recording call, the tape unmodified.  One workgroup per problem,
 * deterministic.  DAVA_ERR_UNSUPPORTED where dava_ba_sgd_backward_supported is 0. */
int dava_ba_sgd_backward(const DavaScene* scene, const DavaSgdConfig* config, const void* tape, size_t tape_bytes,
                         const float* x_out_grad, float* x0_grad, float* observations_grad, void* stream);

/* ---- generic BFGS building blocks (drive an arbitrary error closure) ----
 * batch = number of problems (all leading dims flattened), n = P.          */

/* BFGSSolver.update_inverse_hessian (bfgs_solver.py:235-303): h, h_out (batch,n,n); s, y (batch,n). */
int dava_bfgs_update_inverse_hessian_f32(int64_t batch, int64_t n, const float* h, const float* s,
                                         const float* y, float* h_out, void* stream);
int dava_bfgs_update_inverse_hessian_f64(int64_t batch, int64_t n, const double* h, const double* s,
                                         const double* y, double* h_out, void* stream);

/* BFGSSolver.scale_initial_inverse_hessian (bfgs_solver.py:217-233): scale_out (batch). */
int dava_bfgs_initial_scale_f32(int64_t batch, int64_t n, const float* s, const float* y, float* scale_out,
                                void* stream);
int dava_bfgs_initial_scale_f64(int64_t batch, int64_t n, const double* s, const double* y,
                                double* scale_out, void* stream);

/* h_out = scale[b] * h (batch,n,n): the k==1 rescale (bfgs_solver.py:159-167). May alias. */
int dava_bfgs_scale_matrix_f32(int64_t batch, int64_t n, const float* scale, const float* h, float* h_out,
                               void* stream);
int dava_bfgs_scale_matrix_f64(int64_t batch, int64_t n, const double* scale, const double* h,
                               double* h_out, void* stream);

/* d_out = -H g (bfgs_solver.py:173-176). */
int dava_bfgs_search_direction_f32(int64_t batch, int64_t n, const float* h, const float* g, float* d_out,
                                   void* stream);
int dava_bfgs_search_direction_f64(int64_t batch, int64_t n, const double* h, const double* g,
                                   double* d_out, void* stream);

/* The generic loop's update + direction WITHOUT the dense matrix (bfgs_solver.py:157-180, the
 * reference's gather / update / scatter of a (B, P, P) inverse Hessian): the inverse Hessian is kept
 * as compact history rows, exact BFGS in product form (the fused solve's COMPACT mode).
 *   S, W   (B_all, capacity, row_stride) history rows s_j and w_j = H_{j-1} y_j of every problem;
 *   rho, c (B_all, capacity); gamma (B_all): per-problem scalars (gamma written when count == 0);
 *   problem_index (n_active) int64: the history slot of each active row of g, y, s, d_out (n_active, n);
 *   count: entries stored so far (the same for every active problem: the loop's step index - 1).
 * For each active problem: H' = gamma I + the `count` stored rank-2 terms; appends entry `count`
 * = (s, H'y, 1/(s.y) or 0 if s.y <= 0, 1 + rho y.H'y) and writes d_out = -H g for
 * H = H' + the new term.  Needs count < capacity and row_stride >= n. */
int dava_bfgs_compact_direction_f32(int64_t n_active, int64_t n, int64_t row_stride, int64_t capacity,
                                    int64_t count, const int64_t* problem_index, const float* g, const float* y,
                                    const float* s, float* S, float* W, float* rho, float* c, float* gamma,
                                    float* d_out, void* stream);
int dava_bfgs_compact_direction_f64(int64_t n_active, int64_t n, int64_t row_stride, int64_t capacity,
                                    int64_t count, const int64_t* problem_index, const double* g, const double* y,
                                    const double* s, double* S, double* W, double* rho, double* c,
                                    double* gamma, double* d_out, void* stream);

/* Strong/weak Wolfe line-search state machine (wolfe_conditions.py:23-239),
 * batched, for an error function evaluated by the caller between calls.
 * state (batch, 9): {a_lo, a_hi, a, f_lo, f_hi, f_a, dphi_a, f0, dphi0}
 * flags (batch, 2) uint8: {widening, zooming}
 *   init:    dphi0 = direction . g0, a = 1, brackets 0, errors f0; widening.
 *   propose: (trial > 0) widening: a_hi = a, f_hi = f_a, a *= 2;
 *            zooming: a = (a_lo + a_hi) / 2.
 *   update:  after the caller wrote f(a) into column 5 and phi'(a) into
 *            column 6 for the active rows, apply N&W 3.5/3.6.
 * The search result is column 1 (a_hi).                                    */
int dava_wolfe_init_f32(int64_t batch, int64_t n, const float* direction, const float* f0, const float* g0,
                        float* state, uint8_t* flags, void* stream);
int dava_wolfe_init_f64(int64_t batch, int64_t n, const double* direction, const double* f0,
                        const double* g0, double* state, uint8_t* flags, void* stream);
int dava_wolfe_propose_f32(int64_t batch, float* state, const uint8_t* flags, void* stream);
int dava_wolfe_propose_f64(int64_t batch, double* state, const uint8_t* flags, void* stream);
int dava_wolfe_update_f32(int64_t batch, int32_t trial, float c1, float c2, int32_t strong, float* state,
                          uint8_t* flags, void* stream);
int dava_wolfe_update_f64(int64_t batch, int32_t trial, double c1, double c2, int32_t strong, double* state,
                          uint8_t* flags, void* stream);

/* ---- reverse mode of the building blocks (differentiating THROUGH the solve) ----
 * The reference's create_graph mode (bfgs_solver.py:85, :134, :213-215) back-propagates
 * through every op of the loop.  These are the vector-Jacobian products of the ops above;
 * grad_out is dL/d(output), every grad_* output may be NULL (not formed).  All (batch,n,n)
 * matrices are row-major and general (H is not assumed symmetric).                      */

/* VJP of update_inverse_hessian, including InverseCurvature's custom backward
 * (utils/func_inverse_curvature.py:36-51).  n <= 150 KiB / (9 sizeof(T)).               */
int dava_bfgs_update_inverse_hessian_backward_f32(int64_t batch, int64_t n, const float* h, const float* s,
                                                  const float* y, const float* grad_out, float* grad_h,
                                                  float* grad_s, float* grad_y, void* stream);
int dava_bfgs_update_inverse_hessian_backward_f64(int64_t batch, int64_t n, const double* h, const double* s,
                                                  const double* y, const double* grad_out, double* grad_h,
                                                  double* grad_s, double* grad_y, void* stream);

/* VJP of initial_scale (clamp backward passes where the input >= the bound, as torch). */
int dava_bfgs_initial_scale_backward_f32(int64_t batch, int64_t n, const float* s, const float* y,
                                         const float* grad_out, float* grad_s, float* grad_y, void* stream);
int dava_bfgs_initial_scale_backward_f64(int64_t batch, int64_t n, const double* s, const double* y,
                                         const double* grad_out, double* grad_s, double* grad_y, void* stream);

/* VJP of scale_matrix: grad_scale (batch), grad_h (batch,n,n). */
int dava_bfgs_scale_matrix_backward_f32(int64_t batch, int64_t n, const float* scale, const float* h,
                                        const float* grad_out, float* grad_scale, float* grad_h, void* stream);
int dava_bfgs_scale_matrix_backward_f64(int64_t batch, int64_t n, const double* scale, const double* h,
                                        const double* grad_out, double* grad_scale, double* grad_h, void* stream);

/* VJP of search_direction (d = -H g): grad_h = -grad_d g^T, grad_g = -H^T grad_d. */
int dava_bfgs_search_direction_backward_f32(int64_t batch, int64_t n, const float* h, const float* g,
                                            const float* grad_d, float* grad_h, float* grad_g, void* stream);
int dava_bfgs_search_direction_backward_f64(int64_t batch, int64_t n, const double* h, const double* g,
                                            const double* grad_d, double* grad_h, double* grad_g, void* stream);

/* ---- the building blocks above on HOST memory (CPU tensors; csrc/bfgs_host.hip) ----
 * The reference's solver runs wherever its parameters live (bfgs_solver.py:94-117; BASELINE C1 is
 * "BFGS on PyTorch CPU").  Same arguments and semantics as the device entry points of the same name
 * without the `dava_cpu_` prefix, every pointer host memory, no stream, synchronous.           */
int dava_cpu_bfgs_update_inverse_hessian_f32(int64_t batch, int64_t n, const float* h, const float* s,
                                             const float* y, float* h_out);
int dava_cpu_bfgs_update_inverse_hessian_f64(int64_t batch, int64_t n, const double* h, const double* s,
                                             const double* y, double* h_out);
int dava_cpu_bfgs_initial_scale_f32(int64_t batch, int64_t n, const float* s, const float* y, float* scale_out);
int dava_cpu_bfgs_initial_scale_f64(int64_t batch, int64_t n, const double* s, const double* y, double* scale_out);
int dava_cpu_bfgs_scale_matrix_f32(int64_t batch, int64_t n, const float* scale, const float* h, float* h_out);
int dava_cpu_bfgs_scale_matrix_f64(int64_t batch, int64_t n, const double* scale, const double* h, double* h_out);
int dava_cpu_bfgs_search_direction_f32(int64_t batch, int64_t n, const float* h, const float* g, float* d_out);
int dava_cpu_bfgs_search_direction_f64(int64_t batch, int64_t n, const double* h, const double* g, double* d_out);
int dava_cpu_wolfe_init_f32(int64_t batch, int64_t n, const float* direction, const float* f0, const float* g0,
                            float* state, uint8_t* flags);
int dava_cpu_wolfe_init_f64(int64_t batch, int64_t n, const double* direction, const double* f0, const double* g0,
                            double* state, uint8_t* flags);
int dava_cpu_wolfe_propose_f32(int64_t batch, float* state, const uint8_t* flags);
int dava_cpu_wolfe_propose_f64(int64_t batch, double* state, const uint8_t* flags);
int dava_cpu_wolfe_update_f32(int64_t batch, int32_t trial, float c1, float c2, int32_t strong, float* state,
                              uint8_t* flags);
int dava_cpu_wolfe_update_f64(int64_t batch, int32_t trial, double c1, double c2, int32_t strong, double* state,
                              uint8_t* flags);
int dava_cpu_bfgs_update_inverse_hessian_backward_f32(int64_t batch, int64_t n, const float* h, const float* s,
                                                      const float* y, const float* grad_out, float* grad_h,
                                                      float* grad_s, float* grad_y);
int dava_cpu_bfgs_update_inverse_hessian_backward_f64(int64_t batch, int64_t n, const double* h, const double* s,
                                                      const double* y, const double* grad_out, double* grad_h,
                                                      double* grad_s, double* grad_y);
int dava_cpu_bfgs_initial_scale_backward_f32(int64_t batch, int64_t n, const float* s, const float* y,
                                             const float* grad_out, float* grad_s, float* grad_y);
int dava_cpu_bfgs_initial_scale_backward_f64(int64_t batch, int64_t n, const double* s, const double* y,
                                             const double* grad_out, double* grad_s, double* grad_y);
int dava_cpu_bfgs_scale_matrix_backward_f32(int64_t batch, int64_t n, const float* scale, const float* h,
                                            const float* grad_out, float* grad_scale, float* grad_h);
int dava_cpu_bfgs_scale_matrix_backward_f64(int64_t batch, int64_t n, const double* scale, const double* h,
                                            const double* grad_out, double* grad_scale, double* grad_h);
int dava_cpu_bfgs_search_direction_backward_f32(int64_t batch, int64_t n, const float* h, const float* g,
                                                const float* grad_d, float* grad_h, float* grad_g);
int dava_cpu_bfgs_search_direction_backward_f64(int64_t batch, int64_t n, const double* h, const double* g,
                                                const double* grad_d, double* grad_h, double* grad_g);

/* ---- legacy IOptimisableFunction camera model (camera_model/pinhole_camera_model_l1.py) ----
 * Error and/or the reference's hand-written gradient of PinholeCameraModelL1 for
 * batch x estimates independent estimates (one workgroup each).  Per estimate:
 *   focal, cx, cy (1)      translation, lie_vector (views, 3)     world_points (points-2, 3)
 * shared per batch item: true_points (views, points, 2), visibility (views, points) 0/1.
 * inverse_pixel_ratio = 1/|maximum_pixel_ratio|; error_scale = the reference's fp32
 * sqrt(1/(views*points)).  error_out (batch, estimates), gradient_out (batch, estimates, P)
 * with P = 3 + 6 views + 3 points - 7, either may be NULL.  points >= 3.                  */
int dava_l1_camera_evaluate_f32(int64_t batch, int32_t estimates, int32_t views, int32_t points, const float* focal,
                                const float* cx, const float* cy, const float* translation, const float* lie_vector,
                                const float* world_points, const float* true_points, const uint8_t* visibility,
                                float minimum_z_distance, float inverse_pixel_ratio, float max_gradient,
                                float error_scale, float* error_out, float* gradient_out, void* stream);
int dava_l1_camera_evaluate_f64(int64_t batch, int32_t estimates, int32_t views, int32_t points, const double* focal,
                                const double* cx, const double* cy, const double* translation,
                                const double* lie_vector, const double* world_points, const double* true_points,
                                const uint8_t* visibility, double minimum_z_distance, double inverse_pixel_ratio,
                                double max_gradient, double error_scale, double* error_out, double* gradient_out,
                                void* stream);

/* Reverse mode through the model above (the reference's autograd through get_error /
 * get_gradient when enable_error_gradients / enable_grad_gradients allow it,
 * pinhole_camera_model_l1.py:132-285).  For every estimate and every input element
 * d in [0, D), D = 3 + 6 views + 3 (points-2), ordered focal, cx, cy, translation (views, 3),
 * lie_vector (views, 3), world_points (points-2, 3):
 *   input_cotangent_out[b, e, d] = error_cotangent[b, e] d error/d x_d
 *                                + sum_q gradient_cotangent[b, e, q] d gradient_q/d x_d
 * (either cotangent may be NULL).  detach_points != 0 differentiates the gradient with the world
 * and camera-relative points held constant, as the reference's enable_grad_gradients = False
 * does (:185-198).  Branches, clamps and clips take the derivative of the branch taken;
 * sign() is flat.  One workgroup per (b, e, d); deterministic.                              */
int dava_l1_camera_vjp_f32(int64_t batch, int32_t estimates, int32_t views, int32_t points, const float* focal,
                           const float* cx, const float* cy, const float* translation, const float* lie_vector,
                           const float* world_points, const float* true_points, const uint8_t* visibility,
                           float minimum_z_distance, float inverse_pixel_ratio, float max_gradient, float error_scale,
                           const float* error_cotangent, const float* gradient_cotangent, int32_t detach_points,
                           float* input_cotangent_out, void* stream);
int dava_l1_camera_vjp_f64(int64_t batch, int32_t estimates, int32_t views, int32_t points, const double* focal,
                           const double* cx, const double* cy, const double* translation, const double* lie_vector,
                           const double* world_points, const double* true_points, const uint8_t* visibility,
                           double minimum_z_distance, double inverse_pixel_ratio, double max_gradient,
                           double error_scale, const double* error_cotangent, const double* gradient_cotangent,
                           int32_t detach_points, double* input_cotangent_out, void* stream);

/* ---- float64 evaluation and solve at any scene size (additive to ABI 4) ----
 * The same kernels in three forms, chosen by what fits one workgroup's 160 KiB of LDS:
 *   0  the whole image in LDS: the launch of dava_ba_solve[_train]_f64 / dava_ba_evaluate_f64;
 *   1  observations and visibility read in place from device memory, the six O(P) vectors in LDS;
 *   2  the scene in place and the vectors (x, d, g, g_prev / y, s, H'y) in a per-problem slice of the
 *      workspace (the evaluation: x and direction in place, the gradient formed in grad_out's rows).
 * Same algorithm, operation order, stopping rules, status words and training-mode semantics in every form;
 * one workgroup per problem, which touches only its own slice.  No result depends on the workspace's previous
 * contents.  Form 2 keeps its view constants and history scalars in LDS: more than 251 views at 1025
 * iterations (361 for the evaluation) are DAVA_ERR_UNSUPPORTED.
 *
 * dava_ba_solve_form_f64: the form dava_ba_solve_large_f64 takes for this scene / config (host-only, no data
 * pointers needed), or a negative value, minus the status dava_ba_solve_large_f64 would return, where none
 * runs (invalid scene or config, iterations outside 1 .. 1025, ray angle with distortion). */
int dava_ba_solve_form_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config);

/* Bytes of device workspace dava_ba_solve_large_f64 needs, with Pv = round_up(P, 4):
 *   the history rows   B * 2 * max(iterations - 1, 1) * Pv * 8
 *   form 2 only        B * 6 * Pv * 8 of vectors, after the history rows
 *   a 256-byte tail (unused, as in dava_ba_solve_workspace_bytes_f64).
 * In form 0 this is dava_ba_solve_workspace_bytes_f64's figure.  0 where the solve does not run. */
size_t dava_ba_solve_large_workspace_bytes_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config);

/* dava_ba_solve_train_f64's contract for every scene dava_ba_solve_form_f64 accepts (training NULL or all
 * zero: eval mode).  The host checks run in dava_ba_solve_f64's order; a workspace below the query's figure
 * (needed whenever iterations > 1, and always in form 2) is DAVA_ERR_WORKSPACE before any launch. */
int dava_ba_solve_large_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                            const DavaTrainingF64* training, const double* x0, double* x_out, double* error_out,
                            int32_t* status_out, void* workspace, size_t workspace_bytes, void* stream);

/* dava_ba_evaluate_f64's contract at any N; no workspace.  In form 2 grad_out must not alias x or direction. */
int dava_ba_evaluate_large_f64(const DavaSceneF64* scene, const double* x, const double* direction,
                               const double* alpha, double* error_out, double* grad_out, double* slope_out,
                               void* stream);

/* ---- float64 gradients at any scene size (additive to ABI 4) ----
 * The recording solve, the adjoint and the second derivatives in the same three forms: 0 is the launch of the
 * symbol without `_large`; 1 reads the scene in place; 2 also keeps the O(P) vectors in a per-problem slice of
 * a workspace.  Every form runs one text with the same reduction trees.  No result depends on the previous
 * contents of a tape or workspace.  The F64_FORM override raises each form as it raises the solve's.
 *
 * Recording: the tape layout (dava_ba_solve_tape_bytes_f64's) does not depend on the form; its history block
 * is the solve's history workspace.  dava_ba_solve_tape_bytes_large_f64 is > 0 exactly where
 * dava_ba_solve_large_workspace_bytes_f64 is, and equals dava_ba_solve_tape_bytes_f64 wherever that is > 0.
 * Form 2's six vectors live in a workspace of their own: dava_ba_solve_record_large_workspace_bytes_f64 is
 * B * 6 * Pv * 8 + 256 in form 2 and 0 in forms 0 and 1 (workspace may then be NULL).
 * dava_ba_solve_record_large_f64 has dava_ba_solve_record_train_f64's contract (training NULL or all zero:
 * eval mode) and, in form 0, makes its launch; x_out, error_out and status are bitwise those of
 * dava_ba_solve_large_f64, and every tape slot the solve did not reach is zeroed. */
size_t dava_ba_solve_tape_bytes_large_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config);
size_t dava_ba_solve_record_large_workspace_bytes_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config);
int dava_ba_solve_record_large_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                   const DavaTrainingF64* training, const double* x0, double* x_out,
                                   double* error_out, int32_t* status_out, void* tape, size_t tape_bytes,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* The adjoint.  Its form is chosen by the fit of ITS image (14 vectors of Pv doubles, the dual view constants
 * and partials, scratch, a chunk's coefficients, and in form 0 the scene), whatever form the recording took:
 *   0  dava_ba_solve_backward_f64's launch;
 *   1  the vectors in LDS, the scene in place, the observation cotangent accumulated in observations_grad
 *      (zeroed by the kernel; not formed when NULL);
 *   2  the 14 vectors in a per-problem workspace slice too.
 * dava_ba_solve_backward_form_f64 (host-only): 0, 1, 2, or minus the status where none runs (iterations outside
 * 1 .. 1025, or the dual view constants alone exceed LDS).  Workspace: the rows a_j, B * K * Pv * 8, in form 2
 * B * 14 * Pv * 8 after them, and a 256-byte tail.  dava_ba_solve_backward_large_f64 takes
 * dava_ba_solve_backward_f64's arguments. */
int dava_ba_solve_backward_form_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config);
size_t dava_ba_solve_backward_large_workspace_bytes_f64(const DavaSceneF64* scene,
                                                        const DavaSolverConfigF64* config);
int dava_ba_solve_backward_large_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config, const void* tape,
                                     size_t tape_bytes, const int32_t* status, const double* x_out_grad,
                                     double* x0_grad, double* observations_grad, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* The second derivatives (dava_ba_second_order_f64's contract and outputs):
 *   0  dava_ba_second_order_f64's launch;
 *   1  the dual x and gradient in LDS, the scene in place, the dual dE/dobs in a workspace of B * 4MN doubles
 *      (only when obs_grad_out or obs_hv_out is asked for);
 *   2  the dual x and gradient in a per-problem workspace slice of 4 Pv doubles too, after the dE/dobs block.
 * dava_ba_second_order_form_f64 (host-only): 0, 1, 2 or minus the status.  The workspace query takes whether an
 * observation output will be asked for; it includes a 256-byte tail and is 0 only where no form runs. */
int dava_ba_second_order_form_f64(const DavaSceneF64* scene);
size_t dava_ba_second_order_large_workspace_bytes_f64(const DavaSceneF64* scene, int obs_outputs);
int dava_ba_second_order_large_f64(const DavaSceneF64* scene, const double* x, const double* direction,
                                   const double* obs_direction, double* error_out, double* grad_out, double* hv_out,
                                   double* obs_grad_out, double* obs_hv_out, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* The backward of the dense inverse-Hessian update in float64 beyond its LDS image (the generic loop's graph on a
 * large float64 scene): dava_bfgs_update_inverse_hessian_backward_f64 keeps nine vectors of n doubles in LDS and
 * is DAVA_ERR_UNSUPPORTED for n > 2133; this entry keeps them in a workspace of batch * 9 * n * 8 bytes and a
 * 256-byte tail there (the query: 0 where the LDS launch is taken, which needs no workspace), the same arithmetic
 * in the same order.  The F64_FORM override (1 | 2) asks for the workspace at any n. */
size_t dava_bfgs_update_inverse_hessian_backward_large_workspace_bytes_f64(int64_t batch, int64_t n);
int dava_bfgs_update_inverse_hessian_backward_large_f64(int64_t batch, int64_t n, const double* h, const double* s,
                                                        const double* y, const double* grad_out, double* grad_h,
                                                        double* grad_s, double* grad_y, void* workspace,
                                                        size_t workspace_bytes, void* stream);

/* ---- float32 second derivatives and the descent's adjoint beyond the LDS image ----
 * dava_ba_second_order(_obs) and dava_ba_sgd_backward keep one problem's whole dual-number image in LDS and stay
 * DAVA_ERR_UNSUPPORTED past 160 KiB (at M = 2 from N of about 1,650; C5, 16 x 4096).  The entry points below run
 * the same kernel bodies in the forms of the float64 ones above:
 *   0  the launch of the old symbol (no workspace);
 *   1  the dual x and gradient in LDS (16 Pv bytes, Pv = round_up(P, 4)), the scene read in place, the dual dE/dobs
 *      in a workspace of B * 4MN floats -- formed only when an observation output is asked for;
 *   2  the dual x and gradient in a per-problem workspace slice of 4 Pv floats too (C5: 16 Pv = 198 KB does not
 *      fit LDS).
 * Workspace: [dual dE/dobs: B * 4MN floats, only with an observation output | form 2: B * 4 Pv floats | a 256-byte
 * tail], uninitialised device memory; nothing is read from it before it is written.  The form is the lowest whose
 * image fits; the F32_DUAL_FORM override (1 | 2) raises it, never lowers it.  Results are bitwise those of form 0
 * wherever more than one form runs.  No atomics: two launches give the same bits.
 *
 * dava_ba_second_order_form (host-only): 0, 1, 2 or minus the status.
 * dava_ba_second_order_large_workspace_bytes (host-only): obs_outputs != 0 when obs_grad_out or obs_hv_out will be
 *   asked for; includes the tail; 0 only where no form runs (or the scene is invalid).
 * dava_ba_second_order_large: dava_ba_second_order_obs's contract and outputs at any form.  Checks, all before a
 *   launch: the scene; an empty batch is DAVA_OK; NULL x is DAVA_ERR_INVALID_ARGUMENT; a shape no form runs is
 *   DAVA_ERR_UNSUPPORTED; a form that needs workspace with none or too little is DAVA_ERR_WORKSPACE. */
int dava_ba_second_order_form(const DavaScene* scene);
size_t dava_ba_second_order_large_workspace_bytes(const DavaScene* scene, int obs_outputs);
int dava_ba_second_order_large(const DavaScene* scene, const float* x, const float* direction,
                               const float* obs_direction, float* error_out, float* grad_out, float* hv_out,
                               float* obs_grad_out, float* obs_hv_out, void* workspace, size_t workspace_bytes,
                               void* stream);

/* The adjoint of the fused gradient descent (dava_ba_sgd_backward's contract, tape and outputs) at any form.  In
 * forms 1 and 2 the dual dE/dobs of one step lives in the workspace (only when observations_grad is non-NULL) and
 * the accumulator of dL/dobs is observations_grad itself, zeroed and updated once per step by the thread that owns
 * the element, in form 0's arithmetic and order.  The tape is dava_ba_sgd_solve_record's, which runs these scenes
 * already.  dava_ba_sgd_backward_form (host-only): 0, 1, 2 or minus the status (the adjoint's own fit, whatever
 * the forward takes).  The workspace query takes whether observations_grad will be asked for.  Checks of the
 * launch, in order: the scene; the config; an empty batch is DAVA_OK; NULL x_out_grad or x0_grad is
 * DAVA_ERR_INVALID_ARGUMENT; DAVA_ERR_UNSUPPORTED; a missing or short tape or workspace is DAVA_ERR_WORKSPACE. */
int dava_ba_sgd_backward_form(const DavaScene* scene, const DavaSgdConfig* config);
size_t dava_ba_sgd_backward_large_workspace_bytes(const DavaScene* scene, const DavaSgdConfig* config, int obs_grad);
int dava_ba_sgd_backward_large(const DavaScene* scene, const DavaSgdConfig* config, const void* tape,
                               size_t tape_bytes, const float* x_out_grad, float* x0_grad, float* observations_grad,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- float64 fused gradient descent and its adjoint (additive to ABI 4) ----
 * dava_ba_sgd_solve / _record / _backward on doubles: the same descent, x_{k+1} = x_k - learning_rate dE/dx(x_k)
 * with the product rounded first and then the difference (no FMA), as torch does in float64; the same tape layout
 * (B, K, Pv = round_up(P, 4)) in doubles; the same adjoint.  One entry point per operation, designed with the forms
 * of the float64 kernels above from the start (no separate *_large_* twin):
 *   descent  0  x, the gradient, the observations and the visibility in LDS (at M = 2 up to N = 1,962);
 *            1  x and the gradient in LDS, the scene read in place (up to N = 3,353);
 *            2  the scene in place, x and the gradient in a per-problem workspace slice of 2 Pv doubles (C5).
 *   adjoint  0  the whole dual image and the accumulator of dL/dobs (2MN doubles) in LDS (up to N = 707);
 *            1  the dual x and gradient in LDS, the scene in place, the step's dual dE/dobs in a workspace of
 *               B * 4MN doubles (only with an observation gradient), the accumulator observations_grad itself,
 *               zeroed and updated by the element's owner thread in form 0's arithmetic and order (up to
 *               N = 1,667);
 *            2  the dual x and gradient in a per-problem workspace slice of 4 Pv doubles too.
 * Each operation takes the lowest form whose image fits 160 KiB; the F64_FORM override (1 | 2) raises it, never
 * lowers it; DAVA_ERR_UNSUPPORTED (-DAVA_ERR_UNSUPPORTED from the form queries) where not even form 2's image fits.
 * The adjoint's form is its own: it does not depend on the form the descent took.  Results are bitwise those of
 * form 0 wherever more than one form runs.  No atomics: two launches give the same bits.
 *
 * Checks of the launches, in order and all before a device is touched: the scene; the config
 * (DAVA_ERR_INVALID_ARGUMENT for NULL or negative iterations); an empty batch is DAVA_OK; NULL x0 / x_out (backward:
 * NULL x_out_grad / x0_grad) is DAVA_ERR_INVALID_ARGUMENT; DAVA_ERR_UNSUPPORTED; a missing or short tape (K > 0) or
 * workspace is DAVA_ERR_WORKSPACE.  Workspaces are uninitialised device memory: nothing is read before it is
 * written.  A NULL workspace is accepted where the query says 0. */
typedef struct DavaSgdConfigF64 {
  double learning_rate;
  int32_t iterations; /* K >= 0 */
} DavaSgdConfigF64;

/*   x0 (B, P), x_out (B, P) (may alias x0), error_trace_out (B, K) E(x_k) for k = 0 .. K-1, or NULL.
 *   iterations == 0 is a device copy of x0 and no launch. */
int dava_ba_sgd_solve_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config, const double* x0, double* x_out,
                          double* error_trace_out, void* workspace, size_t workspace_bytes, void* stream);
/* The same launch (bitwise the same x_out and trace) that also writes x_k, k = 0 .. K-1, to the tape (pads zero). */
int dava_ba_sgd_solve_record_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config, const double* x0,
                                 double* x_out, double* error_trace_out, void* tape, size_t tape_bytes,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* Host-only: B * K * round_up(P, 4) * 8; 0 where the descent does not run the scene, and for K = 0. */
size_t dava_ba_sgd_tape_bytes_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config);
/* Host-only: 0, 1, 2 or minus the status. */
int dava_ba_sgd_solve_form_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config);
/* Host-only: exactly what the launch needs -- form 2: B * 2 Pv * 8 plus a 256-byte tail; forms 0 and 1: 0. */
size_t dava_ba_sgd_solve_workspace_bytes_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config);

/* dava_ba_sgd_backward's contract on doubles: x_out_grad (B, P) -> x0_grad (B, P) and observations_grad
 * (B, M, N, 2), or NULL: then the dual dE/dobs is not formed and x0_grad is bitwise the same. */
int dava_ba_sgd_backward_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config, const void* tape,
                             size_t tape_bytes, const double* x_out_grad, double* x0_grad, double* observations_grad,
                             void* workspace, size_t workspace_bytes, void* stream);
/* Host-only: 0, 1, 2 or minus the status (the adjoint's own fit). */
int dava_ba_sgd_backward_form_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config);
/* Host-only; observations_grad != 0 when the observation gradient will be asked for.  Layout: [dual dE/dobs
 * B * 4MN doubles, only in forms 1 and 2 with an observation gradient | form 2: B * 4 Pv doubles | a 256-byte tail];
 * 0 where both blocks are empty (form 0; form 1 without an observation gradient). */
size_t dava_ba_sgd_backward_workspace_bytes_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config,
                                                int observations_grad);

/* ---- the legacy solver fused: BFGSCameraSolver + LineSearchStrongWolfeConditions in one launch (additive to ABI 4) ----
 * Replaces BFGSCameraSolver.forward(function) (solvers/bfgs_camera_solver.py, with
 * solvers/line_search_strong_wolfe_conditions.py inside it) over a PinholeCameraModelL1: one workgroup per
 * (batch item, estimate) runs max_iterations of [gradient; d = -g, then -H g; the max/min step clamp; the widening
 * phase; the secant zoom; H0 = (s.y / max(y.y, 1e-5)) I on the first iteration; the rank-2 update; masked_update;
 * updating &= error > epsilon], every evaluation being the model of dava_l1_camera_evaluate.  An estimate whose
 * error is no longer above epsilon is frozen: its workgroup stops there.  No gradients flow through this entry.
 *
 * Scene and model arguments are dava_l1_camera_evaluate's (inverse_pixel_ratio is the INPUT model's; points >= 4:
 * the model's add() has no z block at 3 points).  The config:
 *   max_iterations, widen_iterations (the line search's ceil(log2(max_step_size))), zoom_iterations, constrain
 *   (add()'s clamps: focal to [inverse pixel ratio, 1e3], cx and cy to [-1, 1], each lie vector re-wrapped to
 *   [-pi, pi));
 *   epsilon, max_step_size, sufficient_decrease, curvature, slope_scale (the line search's sqrt(float32(1 / P))):
 *   float32 values, because the Python modules hold them as float32 tensors; float64 data widens them;
 *   max_step_distance, min_step_distance: doubles, because the Python modules hold them as Python floats (float64
 *   data compares and divides by the unrounded values; float32 data rounds them);
 *   derived_inverse_pixel_ratio: the ratio of every model add() / masked_update() makes (they do not pass
 *   maximum_pixel_ratio on, so it is the constructor default's 1/5 whatever the input model's is).
 * Outputs: the six parameter tensors in the inputs' shapes, error_out (batch, estimates): that point's error,
 * iterations_out (batch, estimates): the iterations during which the estimate was still updating.  Optional
 * traces, each (batch, estimates, max_iterations) or NULL: trace_error (the error after each iteration's
 * masked_update), trace_alpha (the returned step's alpha; the step is alpha d), trace_exit (0 estimate already
 * frozen, 1 accepted while widening, 2 accepted in zoom, 3 unfinished from widening, 4 unfinished from zoom).
 *
 * Two forms by what fits 150 KiB of one workgroup's LDS beside the evaluation's (views, points, 4) scratch and the
 * O(P) state: 0 the P x P inverse Hessian in LDS, 1 in a per-estimate slice of the workspace (batch estimates P^2
 * elements, uninitialised); dava_l1_camera_solve_form_* returns the form or -1 where even form 1 does not fit.  The
 * L1_SOLVE_FORM override (1) raises the form, never lowers it; results are bitwise the same in both forms.
 * Deterministic.  Checked on the host before any device call, in order: sizes (negative counts, views < 1,
 * points < 4, NULL config: DAVA_ERR_INVALID_ARGUMENT); an empty batch or max_iterations == 0 is DAVA_OK (nothing is
 * written); a NULL scene, model, parameter output, error_out or iterations_out pointer is
 * DAVA_ERR_INVALID_ARGUMENT; DAVA_ERR_UNSUPPORTED; a missing or short workspace is DAVA_ERR_WORKSPACE. */
typedef struct DavaL1SolveConfig {
  int32_t max_iterations;
  int32_t widen_iterations;
  int32_t zoom_iterations;
  int32_t constrain;
  double max_step_distance;
  double min_step_distance;
  double derived_inverse_pixel_ratio;
  float epsilon;
  float max_step_size;
  float sufficient_decrease;
  float curvature;
  float slope_scale;
} DavaL1SolveConfig;

int dava_l1_camera_solve_f32(int64_t batch, int32_t estimates, int32_t views, int32_t points, const float* focal,
                             const float* cx, const float* cy, const float* translation, const float* lie_vector,
                             const float* world_points, const float* true_points, const uint8_t* visibility,
                             float minimum_z_distance, float inverse_pixel_ratio, float max_gradient,
                             float error_scale, const DavaL1SolveConfig* config, float* focal_out, float* cx_out,
                             float* cy_out, float* translation_out, float* lie_vector_out, float* world_points_out,
                             float* error_out, int32_t* iterations_out, float* trace_error, float* trace_alpha,
                             int32_t* trace_exit, void* workspace, size_t workspace_bytes, void* stream);
int dava_l1_camera_solve_f64(int64_t batch, int32_t estimates, int32_t views, int32_t points, const double* focal,
                             const double* cx, const double* cy, const double* translation, const double* lie_vector,
                             const double* world_points, const double* true_points, const uint8_t* visibility,
                             double minimum_z_distance, double inverse_pixel_ratio, double max_gradient,
                             double error_scale, const DavaL1SolveConfig* config, double* focal_out, double* cx_out,
                             double* cy_out, double* translation_out, double* lie_vector_out,
                             double* world_points_out, double* error_out, int32_t* iterations_out,
                             double* trace_error, double* trace_alpha, int32_t* trace_exit, void* workspace,
                             size_t workspace_bytes, void* stream);
/* Host-only. */
int dava_l1_camera_solve_form_f32(int32_t views, int32_t points);
int dava_l1_camera_solve_form_f64(int32_t views, int32_t points);
size_t dava_l1_camera_solve_workspace_bytes_f32(int64_t batch, int32_t estimates, int32_t views, int32_t points);
size_t dava_l1_camera_solve_workspace_bytes_f64(int64_t batch, int32_t estimates, int32_t views, int32_t points);

/* ---- test and A/B hooks ----
 * The library makes its launch choices itself (LDS or global-vector mode, waves per workgroup,
 * on-chip history entries, work queue, ...) and reads NOTHING from the environment.  Tests and A/B
 * measurements override a choice by name (FORCE_GV, GV_NO_XL, SOLVE_WAVES, WG_PER_CU, LDS_HISTORY,
 * STAGGER, STAGGER_LEVELS, NO_PPT, NO_QUEUE, ADJ_GV_WAVES, ADJ_FORCE_GV, ADJ_LDS_ENTRIES, ADJ_GD_HBM,
 * COMPACT_SWITCH, GV_SCALAR_SLICE, ADJ_SC_GLOBAL, F64_FORM, F32_DUAL_FORM, L1_SOLVE_FORM; csrc/dava_debug.hpp); value < 0 restores the
 * library's choice.  Process-wide, not thread-safe, host-only.  DAVA_ERR_INVALID_ARGUMENT for an
 * unknown name.                                                                                   */
int dava_debug_set_override(const char* name, int64_t value);
void dava_debug_clear_overrides(void);

/* ---- misc ---- */
const char* dava_status_string(int status);
int dava_abi_version(void);
/* Compiled-in device architecture, e.g. "gfx950". */
const char* dava_device_arch(void);

#ifdef __cplusplus
}
#endif

#endif /* DAVA_BA_H */
