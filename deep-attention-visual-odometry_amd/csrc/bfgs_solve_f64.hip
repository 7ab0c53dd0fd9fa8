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
// The kernel templates are in solve_f64.hpp; this file launches their form 0 (the whole image in LDS).
// Not here: forms 1 and 2 for scenes beyond the LDS image (bfgs_solve_large_f64.hip:
// dava_ba_solve_form_f64, dava_ba_solve_large_workspace_bytes_f64, dava_ba_solve_large_f64,
// dava_ba_evaluate_large_f64); dense / hybrid modes, lean trials, no-move runs, on-chip history entries.
#include "solve_f64.hpp"

using namespace dava;

extern "C" size_t dava_ba_solve_workspace_bytes_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config) {
  DavaScene sc;
  if (f64::check_scene_f64(scene, false, sc) != DAVA_OK) return 0;
  if (f64::solve_supported(sc, config) != DAVA_OK) return 0;
  return f64::history_bytes(sc, config->iterations) + f64::kTailBytes;
}

// dava_ba_solve[_train]_f64 (record == false: `workspace` holds the history rows) and
// dava_ba_solve_record[_train]_f64 (`workspace` is the tape, whose first block is the history rows).
// training: null or all zero = eval mode, the instantiations without TRAIN.
int dava::f64::solve_lds(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                         const DavaTrainingF64* training, const double* x0, double* x_out, double* error_out,
                         int32_t* status_out, void* workspace, size_t workspace_bytes, bool record, void* stream) {
  if (training && !(training->drop_path_p >= 0.f && training->drop_path_p <= 1.f)) return DAVA_ERR_INVALID_ARGUMENT;
  const bool train = training && (training->drop_path_p > 0.f || training->return_second_last);
  DavaScene sc;
  const int st = f64::check_scene_f64(scene, true, sc);
  if (st != DAVA_OK) return st;
  const int sup = f64::solve_supported(sc, config);
  if (sup == DAVA_ERR_INVALID_ARGUMENT) return sup;
  if (sc.batch == 0) return DAVA_OK;
  if (!x0 || !x_out) return DAVA_ERR_INVALID_ARGUMENT;
  if (sup != DAVA_OK) return sup;
  const bool uses_ws = record || config->iterations > 1;
  const TapeLayout tl = tape_layout_f64(sc.batch, sc.num_parameters, config->iterations);
  if (record) {
    if (!status_out) return DAVA_ERR_INVALID_ARGUMENT;
    if (!workspace || workspace_bytes < tl.total_bytes) return DAVA_ERR_WORKSPACE;
  } else if (uses_ws && (!workspace || workspace_bytes < f64::history_bytes(sc, config->iterations) + f64::kTailBytes)) {
    // (the size the query reports, tail included: a queue counter put there later finds its bytes)
    return DAVA_ERR_WORKSPACE;
  }
  f64::TrainArgs a;
  a.L = make_layout(&sc);
  a.B = sc.batch;
  a.Pv = round_up(sc.num_parameters, 4);
  a.kcap = f64::history_capacity(config->iterations);
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.x0 = x0;
  a.x_out = x_out;
  a.err_out = error_out;
  a.status = status_out;
  a.hist = uses_ws ? static_cast<double*>(workspace) : nullptr;
  a.c1 = config->sufficient_decrease;
  a.c2 = config->curvature;
  a.thr = config->error_threshold;
  a.min_step = config->minimum_step;
  a.iters = config->iterations;
  a.max_trials = config->max_line_search_trials;
  a.strong = config->strong_wolfe;
  a.tape_x = record ? static_cast<double*>(workspace) + tl.x : nullptr;
  a.tape_g = record ? static_cast<double*>(workspace) + tl.g : nullptr;
  a.tape_sc = record ? static_cast<double*>(workspace) + tl.scal : nullptr;
  a.tape_tail = record ? static_cast<double*>(workspace) + tl.vecs : nullptr;
  a.T = tl.T;
  a.drop_p = train ? training->drop_path_p : 0.f;
  a.drop_seed = train ? ((unsigned long long)training->drop_seed_hi << 32) | training->drop_seed_lo : 0ull;
  a.second_last = train && training->return_second_last ? 1 : 0;
  const int lds = (int)f64::carve(sc.num_views, sc.num_points, a.Pv, a.kcap).total_bytes;
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto go = [&](auto kernel, const auto& args) {
    set_dynamic_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, dim3(a.B), dim3(kBlock), lds, s, args);
  };
  const f64::SolveArgs& ev = a;  // the eval-mode kernels' argument
  const bool ray = sc.residual == DAVA_RESIDUAL_RAY_ANGLE;
  constexpr int kRay = DAVA_RESIDUAL_RAY_ANGLE, kSq = DAVA_RESIDUAL_SQUARED_REPROJECTION;
  if (train) {
    if (ray && record) go(f64::bfgs_ba_solve_f64_kernel<kRay, true, true>, a);
    else if (ray) go(f64::bfgs_ba_solve_f64_kernel<kRay, false, true>, a);
    else if (record) go(f64::bfgs_ba_solve_f64_kernel<kSq, true, true>, a);
    else go(f64::bfgs_ba_solve_f64_kernel<kSq, false, true>, a);
  } else {
    if (ray && record) go(f64::bfgs_ba_solve_f64_kernel<kRay, true, false>, ev);
    else if (ray) go(f64::bfgs_ba_solve_f64_kernel<kRay, false, false>, ev);
    else if (record) go(f64::bfgs_ba_solve_f64_kernel<kSq, true, false>, ev);
    else go(f64::bfgs_ba_solve_f64_kernel<kSq, false, false>, ev);
  }
  return hipGetLastError() == hipSuccess ? DAVA_OK : DAVA_ERR_LAUNCH;
}

extern "C" int dava_ba_solve_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config, const double* x0,
                                 double* x_out, double* error_out, int32_t* status_out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return f64::solve_lds(scene, config, nullptr, x0, x_out, error_out, status_out, workspace, workspace_bytes, false,
                   stream);
}

extern "C" int dava_ba_solve_train_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                       const DavaTrainingF64* training, const double* x0, double* x_out,
                                       double* error_out, int32_t* status_out, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  return f64::solve_lds(scene, config, training, x0, x_out, error_out, status_out, workspace, workspace_bytes, false,
                   stream);
}

extern "C" size_t dava_ba_solve_tape_bytes_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config) {
  DavaScene sc;
  if (f64::check_scene_f64(scene, false, sc) != DAVA_OK) return 0;
  if (f64::solve_supported(sc, config) != DAVA_OK) return 0;
  return tape_layout_f64(sc.batch, sc.num_parameters, config->iterations).total_bytes;
}

extern "C" int dava_ba_solve_record_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config, const double* x0,
                                        double* x_out, double* error_out, int32_t* status_out, void* tape,
                                        size_t tape_bytes, void* stream) {
  return f64::solve_lds(scene, config, nullptr, x0, x_out, error_out, status_out, tape, tape_bytes, true, stream);
}

extern "C" int dava_ba_solve_record_train_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                              const DavaTrainingF64* training, const double* x0, double* x_out,
                                              double* error_out, int32_t* status_out, void* tape, size_t tape_bytes,
                                              void* stream) {
  return f64::solve_lds(scene, config, training, x0, x_out, error_out, status_out, tape, tape_bytes, true, stream);
}

extern "C" int dava_ba_evaluate_f64(const DavaSceneF64* scene, const double* x, const double* direction,
                                    const double* alpha, double* error_out, double* grad_out, double* slope_out,
                                    void* stream) {
  DavaScene sc;
  const int st = f64::check_scene_f64(scene, true, sc);
  if (st != DAVA_OK) return st;
  if (sc.batch == 0) return DAVA_OK;
  if (!x || !error_out) return DAVA_ERR_INVALID_ARGUMENT;
  if (slope_out && !direction) return DAVA_ERR_INVALID_ARGUMENT;
  const int Pv = round_up(sc.num_parameters, 4);
  const f64::Carve cv = f64::carve(sc.num_views, sc.num_points, Pv, 0);
  if (cv.total_bytes > f64::kMaxLdsBytes) return DAVA_ERR_UNSUPPORTED;
  const int lds = (int)cv.total_bytes;
  f64::EvalArgs a;
  a.L = make_layout(&sc);
  a.Pv = Pv;
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.x = x;
  a.dir = direction;
  a.alpha = alpha;
  a.err = error_out;
  a.grad = grad_out;
  a.slope = slope_out;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool G = grad_out != nullptr, S = slope_out != nullptr, T = direction != nullptr && alpha != nullptr;
  const int B = sc.batch, res = sc.residual;
  f64::launch_eval_for<0>(a, B, lds, s, res, G, S, T);
  return hipGetLastError() == hipSuccess ? DAVA_OK : DAVA_ERR_LAUNCH;
}
