// The float64 adjoint for scenes whose adjoint image does not fit 160 KiB: dava_ba_solve_backward_large_f64, with
// the host-only queries dava_ba_solve_backward_form_f64 and dava_ba_solve_backward_large_workspace_bytes_f64.
//
// The kernel is bfgs_ba_adjoint_f64_kernel (adjoint_f64.hpp) in its forms 1 and 2: the body of the form-0 adjoint
// with the scene read in place and the observation cotangent accumulated in the output (form 1) and, beyond that,
// the 14 Pv vectors in a per-problem slice of the workspace (form 2).  The form is chosen by fit
// (f64::choose_adjoint_form), independently of the form the recording took; a scene whose whole image fits takes
// form 0, i.e. the launch of dava_ba_solve_backward_f64.
// Workspace: [rows a_j B x K x Pv | form 2: vectors B x 14 x Pv | 256-byte tail], doubles.  The vector slices
// arrive uninitialised: the kernel writes all 14 x Pv doubles of its slice, pads included, before it reads any
// (the staging loop covers the ten plain vectors; every step writes the four dual slots -- as s, w, y, g_k for
// k > 0, as the dual x and gradient for every k -- over all Pv elements before reading them).
// Not here: LDS copies of x for a form-2 problem, single-pass row products, on-chip tape rows.
#include "adjoint_f64.hpp"

using namespace dava;

namespace {

// DAVA_OK if some form runs this scene / config (host-only); `form` then holds it
int large_adjoint_supported(const DavaSceneF64* scene, const DavaSolverConfigF64* c, DavaScene& sc, int& form) {
  const int st = f64::check_scene_f64(scene, false, sc);
  if (st != DAVA_OK) return st;
  if (!c || c->iterations < 0) return DAVA_ERR_INVALID_ARGUMENT;
  if (c->iterations < 1 || c->iterations > f64::kMaxIterations) return DAVA_ERR_UNSUPPORTED;
  form = f64::choose_adjoint_form(sc.num_views, sc.num_points, round_up(sc.num_parameters, 4));
  return form < 0 ? DAVA_ERR_UNSUPPORTED : DAVA_OK;
}

size_t row_bytes(const DavaScene& sc, const TapeLayout& tl) {
  return (size_t)sc.batch * tl.K * tl.Pv * sizeof(double);
}

size_t vector_bytes(const DavaScene& sc, const TapeLayout& tl) {
  return (size_t)sc.batch * (f64::kAdjVectors + 4) * tl.Pv * sizeof(double);
}

template <int FORM>
void launch_adjoint(const f64::LargeAdjointArgs& a, int B, int lds, hipStream_t s, bool ray) {
  auto go = [&](auto kernel) {
    set_dynamic_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, dim3(B), dim3(kBlock), lds, s, a);
  };
  if (ray) go(f64::bfgs_ba_adjoint_f64_kernel<DAVA_RESIDUAL_RAY_ANGLE, FORM>);
  else go(f64::bfgs_ba_adjoint_f64_kernel<DAVA_RESIDUAL_SQUARED_REPROJECTION, FORM>);
}

}  // namespace

extern "C" int dava_ba_solve_backward_form_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config) {
  DavaScene sc;
  int form = -1;
  const int st = large_adjoint_supported(scene, config, sc, form);
  return st == DAVA_OK ? form : -st;
}

extern "C" size_t dava_ba_solve_backward_large_workspace_bytes_f64(const DavaSceneF64* scene,
                                                                   const DavaSolverConfigF64* config) {
  DavaScene sc;
  int form = -1;
  if (large_adjoint_supported(scene, config, sc, form) != DAVA_OK) return 0;
  const TapeLayout tl = tape_layout_f64(sc.batch, sc.num_parameters, config->iterations);
  return row_bytes(sc, tl) + (form == 2 ? vector_bytes(sc, tl) : 0) + f64::kTailBytes;
}

extern "C" int dava_ba_solve_backward_large_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                                const void* tape, size_t tape_bytes, const int32_t* status,
                                                const double* x_out_grad, double* x0_grad,
                                                double* observations_grad, void* workspace, size_t workspace_bytes,
                                                void* stream) {
  DavaScene sc;
  int form = -1;
  const int st = large_adjoint_supported(scene, config, sc, form);
  if (st != DAVA_OK) return st;
  if (form == 0)  // the whole image fits LDS: the launch of dava_ba_solve_backward_f64
    return dava_ba_solve_backward_f64(scene, config, tape, tape_bytes, status, x_out_grad, x0_grad, observations_grad,
                                      workspace, workspace_bytes, stream);
  if (sc.batch == 0) return DAVA_OK;
  if (!scene->observations || !scene->visibility || !tape || !status || !x_out_grad || !x0_grad)
    return DAVA_ERR_INVALID_ARGUMENT;
  const TapeLayout tl = tape_layout_f64(sc.batch, sc.num_parameters, config->iterations);
  if (tape_bytes < tl.queue_byte) return DAVA_ERR_WORKSPACE;
  const size_t need = row_bytes(sc, tl) + (form == 2 ? vector_bytes(sc, tl) : 0);
  if (!workspace || workspace_bytes < need) return DAVA_ERR_WORKSPACE;
  f64::LargeAdjointArgs a;
  a.L = make_layout(&sc);
  a.Pv = tl.Pv;
  a.K = tl.K;
  a.tl = tl;
  a.tape = static_cast<const double*>(tape);
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.status = status;
  a.xbar = x_out_grad;
  a.x0_grad = x0_grad;
  a.obs_grad = observations_grad;
  a.arows = static_cast<double*>(workspace);
  a.obs_lds = 0;
  a.vecs = form == 2 ? reinterpret_cast<double*>(static_cast<char*>(workspace) + row_bytes(sc, tl)) : nullptr;
  const int lds = (int)f64::carve_adjoint_large(sc.num_views, tl.Pv, form).total_bytes;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool ray = sc.residual == DAVA_RESIDUAL_RAY_ANGLE;
  if (form == 1) launch_adjoint<1>(a, sc.batch, lds, s, ray);
  else launch_adjoint<2>(a, sc.batch, lds, s, ray);
  return hipGetLastError() == hipSuccess ? DAVA_OK : DAVA_ERR_LAUNCH;
}
