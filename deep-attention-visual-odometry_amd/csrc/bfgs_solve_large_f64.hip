// The float64 BA hot path for scenes whose LDS image does not fit 160 KiB: dava_ba_solve_large_f64 and
// dava_ba_evaluate_large_f64, with the host-only queries dava_ba_solve_form_f64 and
// dava_ba_solve_large_workspace_bytes_f64.
//
// The kernels are bfgs_ba_solve_f64_kernel / ba_evaluate_f64_kernel (solve_f64.hpp) in their forms 1 and 2: the
// body of bfgs_solve_f64.hip's kernels with the scene read in place from HBM (form 1) and, beyond that, the six
// O(P) vectors in a per-problem slice of the workspace (form 2).  The entry points here plan with any_form = true
// (solve_f64.hpp: the same checks as the form-0 symbols, the form chosen by f64::choose_form); a scene whose whole
// image fits takes form 0, i.e. the launch bfgs_solve_f64.hip instantiates (f64::solve_form0, f64::eval_form0).
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

int run(const f64::SolvePlan& p, void* stream) {
  if (!p.launch || p.shape.form == 0) return f64::solve_form0(p, stream);
  return p.shape.form == 1 ? f64::launch_solve<1>(p, stream) : f64::launch_solve<2>(p, stream);
}

}  // namespace

extern "C" int dava_ba_solve_form_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config) {
  const f64::SolveShape s = f64::solve_query(scene, config, true);
  return s.status == DAVA_OK ? s.form : -s.status;
}

extern "C" size_t dava_ba_solve_large_workspace_bytes_f64(const DavaSceneF64* scene,
                                                          const DavaSolverConfigF64* config) {
  const f64::SolveShape s = f64::solve_query(scene, config, true);
  return s.status == DAVA_OK ? s.workspace_bytes() : 0;
}

extern "C" size_t dava_ba_solve_tape_bytes_large_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config) {
  const f64::SolveShape s = f64::solve_query(scene, config, true);
  return s.status == DAVA_OK ? s.tape.total_bytes : 0;
}

extern "C" size_t dava_ba_solve_record_large_workspace_bytes_f64(const DavaSceneF64* scene,
                                                                 const DavaSolverConfigF64* config) {
  const f64::SolveShape s = f64::solve_query(scene, config, true);
  return s.status == DAVA_OK ? s.record_workspace_bytes() : 0;
}

extern "C" int dava_ba_solve_large_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                       const DavaTrainingF64* training, const double* x0, double* x_out,
                                       double* error_out, int32_t* status_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return run(f64::plan_solve(scene, config, training, x0, x_out, error_out, status_out, nullptr, 0, workspace,
                             workspace_bytes, false, true), stream);
}

extern "C" int dava_ba_solve_record_large_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                              const DavaTrainingF64* training, const double* x0, double* x_out,
                                              double* error_out, int32_t* status_out, void* tape, size_t tape_bytes,
                                              void* workspace, size_t workspace_bytes, void* stream) {
  return run(f64::plan_solve(scene, config, training, x0, x_out, error_out, status_out, tape, tape_bytes, workspace,
                             workspace_bytes, true, true), stream);
}

extern "C" int dava_ba_evaluate_large_f64(const DavaSceneF64* scene, const double* x, const double* direction,
                                          const double* alpha, double* error_out, double* grad_out, double* slope_out,
                                          void* stream) {
  const f64::EvalPlan p = f64::plan_eval(scene, x, direction, alpha, error_out, grad_out, slope_out, true);
  if (!p.launch || p.form == 0) return f64::eval_form0(p, stream);
  return p.form == 1 ? f64::launch_eval<1>(p, stream) : f64::launch_eval<2>(p, stream);
}
