// The float64 BA hot path for scenes whose LDS image does not fit 160 KiB: dava_ba_solve_large_f64 and
// dava_ba_evaluate_large_f64, with the host-only queries dava_ba_solve_form_f64 and
// dava_ba_solve_large_workspace_bytes_f64.
//
// The kernels are bfgs_ba_solve_f64_kernel / ba_evaluate_f64_kernel (solve_f64.hpp) in their forms 1 and 2: the
// body of bfgs_solve_f64.hip's kernels with the scene read in place from HBM (form 1) and, beyond that, the six
// O(P) vectors in a per-problem slice of the workspace (form 2).  The form is chosen by fit (f64::choose_form); a
// scene whose whole image fits takes form 0, i.e. the launch of dava_ba_solve[_train]_f64 / dava_ba_evaluate_f64.
// Workspace of the solve: [history B x (S[kcap][Pv], W[kcap][Pv]) | form 2: vectors B x 6 x Pv | 256-byte tail],
// doubles.  The vector slices arrive uninitialised: the kernel writes all 6 x Pv doubles of its slice, pads
// included, before it reads any.
// The recording solve in forms 1 and 2 (dava_ba_solve_record_large_f64, dava_ba_solve_tape_bytes_large_f64,
// dava_ba_solve_record_large_workspace_bytes_f64) is the same kernel with RECORD: the tape (dava_tape.hpp in doubles,
// the layout of every form) is its history workspace, and form 2's vector slices come from a workspace of their own:
// [vectors B x 6 x Pv | 256-byte tail].
// Not here: no LDS copies of x or d for a form-2 problem, no lean trials, no on-chip history entries, no dense / hybrid mode.
#include "solve_f64.hpp"

using namespace dava;

namespace {

// DAVA_OK if some form runs this scene / config (host-only); `form` then holds it
int large_supported(const DavaScene& sc, const DavaSolverConfigF64* c, int& form) {
  if (!c || c->iterations < 0 || c->max_line_search_trials < 0) return DAVA_ERR_INVALID_ARGUMENT;
  if (c->iterations < 1 || c->iterations > f64::kMaxIterations) return DAVA_ERR_UNSUPPORTED;
  form = f64::choose_form(sc.num_views, sc.num_points, round_up(sc.num_parameters, 4),
                          f64::history_capacity(c->iterations));
  // (form 2's own image -- view constants, view partials, history scalars -- grows with the views: more than
  //  251 of them at 1025 iterations do not fit)
  return form < 0 ? DAVA_ERR_UNSUPPORTED : DAVA_OK;
}

size_t vector_bytes(const DavaScene& sc) {
  return (size_t)sc.batch * f64::kSolveVectors * round_up(sc.num_parameters, 4) * sizeof(double);
}

size_t large_workspace_bytes(const DavaScene& sc, int iterations, int form) {
  return f64::history_bytes(sc, iterations) + (form == 2 ? vector_bytes(sc) : 0) + f64::kTailBytes;
}

template <int FORM>
void launch_solve(const f64::LargeArgs& a, int lds, hipStream_t s, bool ray, bool train, bool record = false) {
  auto go = [&](auto kernel) {
    set_dynamic_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, dim3(a.B), dim3(kBlock), lds, s, a);
  };
  constexpr int kRay = DAVA_RESIDUAL_RAY_ANGLE, kSq = DAVA_RESIDUAL_SQUARED_REPROJECTION;
  if (record) {
    if (train) {
      if (ray) go(f64::bfgs_ba_solve_f64_kernel<kRay, true, true, FORM>);
      else go(f64::bfgs_ba_solve_f64_kernel<kSq, true, true, FORM>);
    } else {
      if (ray) go(f64::bfgs_ba_solve_f64_kernel<kRay, true, false, FORM>);
      else go(f64::bfgs_ba_solve_f64_kernel<kSq, true, false, FORM>);
    }
  } else if (train) {
    if (ray) go(f64::bfgs_ba_solve_f64_kernel<kRay, false, true, FORM>);
    else go(f64::bfgs_ba_solve_f64_kernel<kSq, false, true, FORM>);
  } else {
    if (ray) go(f64::bfgs_ba_solve_f64_kernel<kRay, false, false, FORM>);
    else go(f64::bfgs_ba_solve_f64_kernel<kSq, false, false, FORM>);
  }
}

}  // namespace

extern "C" int dava_ba_solve_form_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config) {
  DavaScene sc;
  int st = f64::check_scene_f64(scene, false, sc);
  int form = -1;
  if (st == DAVA_OK) st = large_supported(sc, config, form);
  return st == DAVA_OK ? form : -st;
}

extern "C" size_t dava_ba_solve_large_workspace_bytes_f64(const DavaSceneF64* scene,
                                                          const DavaSolverConfigF64* config) {
  DavaScene sc;
  int form = -1;
  if (f64::check_scene_f64(scene, false, sc) != DAVA_OK) return 0;
  if (large_supported(sc, config, form) != DAVA_OK) return 0;
  return large_workspace_bytes(sc, config->iterations, form);
}

namespace {

// dava_ba_solve_large_f64 (tape == null: `workspace` holds the history rows and form 2's vectors) and
// dava_ba_solve_record_large_f64 (the tape's first block is the history rows; `workspace` holds form 2's vectors).
// The host checks of f64::solve_lds in its order; training: null or all zero = eval mode.
int solve_large(const DavaSceneF64* scene, const DavaSolverConfigF64* config, const DavaTrainingF64* training,
                const double* x0, double* x_out, double* error_out, int32_t* status_out, void* tape,
                size_t tape_bytes, bool record, void* workspace, size_t workspace_bytes, void* stream) {
  if (training && !(training->drop_path_p >= 0.f && training->drop_path_p <= 1.f)) return DAVA_ERR_INVALID_ARGUMENT;
  const bool train = training && (training->drop_path_p > 0.f || training->return_second_last);
  DavaScene sc;
  const int st = f64::check_scene_f64(scene, true, sc);
  if (st != DAVA_OK) return st;
  int form = -1;
  const int sup = large_supported(sc, config, form);
  if (sup == DAVA_ERR_INVALID_ARGUMENT) return sup;
  if (sc.batch == 0) return DAVA_OK;
  if (!x0 || !x_out) return DAVA_ERR_INVALID_ARGUMENT;
  if (sup != DAVA_OK) return sup;
  if (form == 0)  // the whole image fits LDS: the launch of dava_ba_solve[_record][_train]_f64
    return record ? f64::solve_lds(scene, config, training, x0, x_out, error_out, status_out, tape, tape_bytes, true,
                                   stream)
                  : f64::solve_lds(scene, config, training, x0, x_out, error_out, status_out, workspace,
                                   workspace_bytes, false, stream);
  const TapeLayout tl = tape_layout_f64(sc.batch, sc.num_parameters, config->iterations);
  if (record) {
    if (!status_out) return DAVA_ERR_INVALID_ARGUMENT;
    if (!tape || tape_bytes < tl.total_bytes) return DAVA_ERR_WORKSPACE;
    if (form == 2 && (!workspace || workspace_bytes < vector_bytes(sc) + f64::kTailBytes)) return DAVA_ERR_WORKSPACE;
  } else {
    const bool uses_ws = form == 2 || config->iterations > 1;
    if (uses_ws && (!workspace || workspace_bytes < large_workspace_bytes(sc, config->iterations, form)))
      return DAVA_ERR_WORKSPACE;  // (the size the query reports, tail included)
  }
  f64::LargeArgs a;
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
  a.hist = record ? static_cast<double*>(tape) : config->iterations > 1 ? static_cast<double*>(workspace) : nullptr;
  a.c1 = config->sufficient_decrease;
  a.c2 = config->curvature;
  a.thr = config->error_threshold;
  a.min_step = config->minimum_step;
  a.iters = config->iterations;
  a.max_trials = config->max_line_search_trials;
  a.strong = config->strong_wolfe;
  a.tape_x = record ? static_cast<double*>(tape) + tl.x : nullptr;
  a.tape_g = record ? static_cast<double*>(tape) + tl.g : nullptr;
  a.tape_sc = record ? static_cast<double*>(tape) + tl.scal : nullptr;
  a.tape_tail = record ? static_cast<double*>(tape) + tl.vecs : nullptr;
  a.T = record ? tl.T : 0;
  a.drop_p = train ? training->drop_path_p : 0.f;
  a.drop_seed = train ? ((unsigned long long)training->drop_seed_hi << 32) | training->drop_seed_lo : 0ull;
  a.second_last = train && training->return_second_last ? 1 : 0;
  a.vecs = form != 2 ? nullptr
           : record  ? static_cast<double*>(workspace)
                     : reinterpret_cast<double*>(static_cast<char*>(workspace) + f64::history_bytes(sc, a.iters));
  const int lds = (int)f64::carve_large(sc.num_views, a.Pv, a.kcap, form).total_bytes;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool ray = sc.residual == DAVA_RESIDUAL_RAY_ANGLE;
  if (form == 1) launch_solve<1>(a, lds, s, ray, train, record);
  else launch_solve<2>(a, lds, s, ray, train, record);
  return hipGetLastError() == hipSuccess ? DAVA_OK : DAVA_ERR_LAUNCH;
}

}  // namespace

extern "C" int dava_ba_solve_large_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                       const DavaTrainingF64* training, const double* x0, double* x_out,
                                       double* error_out, int32_t* status_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return solve_large(scene, config, training, x0, x_out, error_out, status_out, nullptr, 0, false, workspace,
                     workspace_bytes, stream);
}

extern "C" size_t dava_ba_solve_tape_bytes_large_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config) {
  DavaScene sc;
  int form = -1;
  if (f64::check_scene_f64(scene, false, sc) != DAVA_OK) return 0;
  if (large_supported(sc, config, form) != DAVA_OK) return 0;
  return tape_layout_f64(sc.batch, sc.num_parameters, config->iterations).total_bytes;
}

extern "C" size_t dava_ba_solve_record_large_workspace_bytes_f64(const DavaSceneF64* scene,
                                                                 const DavaSolverConfigF64* config) {
  DavaScene sc;
  int form = -1;
  if (f64::check_scene_f64(scene, false, sc) != DAVA_OK) return 0;
  if (large_supported(sc, config, form) != DAVA_OK) return 0;
  return form == 2 ? vector_bytes(sc) + f64::kTailBytes : 0;
}

extern "C" int dava_ba_solve_record_large_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                              const DavaTrainingF64* training, const double* x0, double* x_out,
                                              double* error_out, int32_t* status_out, void* tape, size_t tape_bytes,
                                              void* workspace, size_t workspace_bytes, void* stream) {
  return solve_large(scene, config, training, x0, x_out, error_out, status_out, tape, tape_bytes, true, workspace,
                     workspace_bytes, stream);
}

extern "C" int dava_ba_evaluate_large_f64(const DavaSceneF64* scene, const double* x, const double* direction,
                                          const double* alpha, double* error_out, double* grad_out, double* slope_out,
                                          void* stream) {
  DavaScene sc;
  const int st = f64::check_scene_f64(scene, true, sc);
  if (st != DAVA_OK) return st;
  if (sc.batch == 0) return DAVA_OK;
  if (!x || !error_out) return DAVA_ERR_INVALID_ARGUMENT;
  if (slope_out && !direction) return DAVA_ERR_INVALID_ARGUMENT;
  const int Pv = round_up(sc.num_parameters, 4);
  const int form = f64::choose_form(sc.num_views, sc.num_points, Pv, 0);
  if (form < 0) return DAVA_ERR_UNSUPPORTED;  // (more than 361 views: form 2's view constants and partials alone)
  if (form == 0) return dava_ba_evaluate_f64(scene, x, direction, alpha, error_out, grad_out, slope_out, stream);
  const int lds = (int)f64::carve_large(sc.num_views, Pv, 0, form).total_bytes;
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
  if (form == 1) f64::launch_eval_for<1>(a, sc.batch, lds, s, sc.residual, G, S, T);
  else f64::launch_eval_for<2>(a, sc.batch, lds, s, sc.residual, G, S, T);
  return hipGetLastError() == hipSuccess ? DAVA_OK : DAVA_ERR_LAUNCH;
}
