// The float64 flavour of the BA hot path on gfx950: objective evaluation (dava_ba_evaluate_f64) and the
// one-launch BFGS + strong-Wolfe solve (dava_ba_solve_f64; dava_ba_solve_train_f64 with training mode's semantics).
//
// The reference trains and tests its calibration path in float64 (CalibrationNetwork under
// float_precision="64"; tests/autograd_solvers, tests/geometry in float64).  This file runs the same
// objective code as the fp32 kernels (ba_objective.hpp, instantiated with S = double) and the same
// algorithm as bfgs_solve.hip, in a deliberately small first form:
//  * one 256-thread workgroup per problem for the whole solve; x, d, g, g_prev / y, s, H'y, the scene
//    (observations as doubles, visibility bytes), the view constants and the history scalars in LDS;
//  * the inverse Hessian in COMPACT form only: rows s_j, w_j = H_{j-1} y_j as doubles in the HBM
//    workspace, rho_j, c_j in LDS; product form and operation order of compact_direction_kernel<T>
//    (bfgs_ops.hip), which the generic loop already runs -- and tests -- in float64;
//  * the strong-Wolfe state machine of wolfe_update_kernel<T> / oracle/solver.py in-kernel; every trial
//    is a full one: E, the forward-mode slope and the reverse-mode gradient at x + alpha d, so an
//    accepted trial is the next iterate's evaluation;
//  * every loop bounded by `iterations` or `max_line_search_trials`; no queue, no spin-wait.
// The recording form (dava_ba_solve_record_f64) is the same kernel behind a RECORD template flag: it
// additionally writes dava_tape.hpp's layout in doubles (x_k, g_k at the start of every iteration, alpha_k,
// rho_j, c_j, gamma) for the float64 adjoint (bfgs_adjoint_f64.hip); the tape's history block is its workspace.
// Training mode (dava_ba_solve_train_f64, dava_ba_solve_record_train_f64) is the same kernel behind a TRAIN
// template flag, with bfgs_solve.hip's semantics: the drop path draws its stopping iteration once before the
// loop (drop_uniform, the float32 generator and comparison: one schedule per seed in both precisions) and a
// problem that leaves there reports DAVA_STOP_DROP; return_second_last moves x only after the step has passed
// the minimum-step test.  The tape needs nothing more: the adjoint replays status[:, 0] steps.
// The kernel templates, the plans (every host check, once for all forms) and the launchers are in solve_f64.hpp.
// This file instantiates form 0 (the whole image in LDS): its entry points plan with any_form = false, so a scene
// that needs another form is DAVA_ERR_UNSUPPORTED and the F64_FORM override is ignored.
// Not here: forms 1 and 2 for scenes beyond the LDS image (bfgs_solve_large_f64.hip:
// dava_ba_solve_form_f64, dava_ba_solve_large_workspace_bytes_f64, dava_ba_solve_large_f64,
// dava_ba_evaluate_large_f64); dense / hybrid modes, lean trials, no-move runs, on-chip history entries.
#include "solve_f64.hpp"

using namespace dava;

int dava::f64::solve_form0(const SolvePlan& p, void* stream) {
  return p.launch ? launch_solve<0>(p, stream) : p.status;
}

int dava::f64::eval_form0(const EvalPlan& p, void* stream) { return p.launch ? launch_eval<0>(p, stream) : p.status; }

extern "C" size_t dava_ba_solve_workspace_bytes_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config) {
  const f64::SolveShape s = f64::solve_query(scene, config, false);
  return s.status == DAVA_OK ? s.workspace_bytes() : 0;
}

extern "C" size_t dava_ba_solve_tape_bytes_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config) {
  const f64::SolveShape s = f64::solve_query(scene, config, false);
  return s.status == DAVA_OK ? s.tape.total_bytes : 0;
}

extern "C" int dava_ba_solve_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config, const double* x0,
                                 double* x_out, double* error_out, int32_t* status_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return f64::solve_form0(f64::plan_solve(scene, config, nullptr, x0, x_out, error_out, status_out, nullptr, 0,
                                          workspace, workspace_bytes, false, false), stream);
}

extern "C" int dava_ba_solve_train_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                       const DavaTrainingF64* training, const double* x0, double* x_out,
                                       double* error_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  return f64::solve_form0(f64::plan_solve(scene, config, training, x0, x_out, error_out, status_out, nullptr, 0,
                                          workspace, workspace_bytes, false, false), stream);
}

extern "C" int dava_ba_solve_record_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config, const double* x0,
                                        double* x_out, double* error_out, int32_t* status_out, void* tape,
                                        size_t tape_bytes, void* stream) {
  return f64::solve_form0(f64::plan_solve(scene, config, nullptr, x0, x_out, error_out, status_out, tape, tape_bytes,
                                          nullptr, 0, true, false), stream);
}

extern "C" int dava_ba_solve_record_train_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                              const DavaTrainingF64* training, const double* x0, double* x_out,
                                              double* error_out, int32_t* status_out, void* tape, size_t tape_bytes,
                                              void* stream) {
  return f64::solve_form0(f64::plan_solve(scene, config, training, x0, x_out, error_out, status_out, tape, tape_bytes,
                                          nullptr, 0, true, false), stream);
}

extern "C" int dava_ba_evaluate_f64(const DavaSceneF64* scene, const double* x, const double* direction,
                                    const double* alpha, double* error_out, double* grad_out, double* slope_out,
                                    void* stream) {
  return f64::eval_form0(f64::plan_eval(scene, x, direction, alpha, error_out, grad_out, slope_out, false), stream);
}
