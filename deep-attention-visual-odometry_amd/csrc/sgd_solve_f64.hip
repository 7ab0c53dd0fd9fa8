// Fused gradient descent on the BA objectives in float64: sgd_solve.hip's descent
//   for k in 0 .. K-1:  g = d/dx sum_b E(x_k);  x_{k+1} = x_k - learning_rate * g
// on doubles, ONE launch, one kBlock workgroup per problem for the whole descent on a plain grid of B workgroups.
// The body is written once; FORM, a compile-time parameter, only says where its pointers come from (solve_f64.hpp):
//   form 0  x, the gradient, the observations (as doubles) and the visibility in LDS
//   form 1  x and the gradient in LDS, the scene read in place
//   form 2  the scene in place, x and the gradient in a per-problem workspace slice of 2 Pv doubles (uninitialised)
// In every form the view constants, the per-wave view partials and the two reduction buffers are in LDS.
// A step is f64::eval<GRAD> (which ends on a barrier and overwrites every gradient entry), the update -- the
// product rounded, then the difference, as torch does in float64 -- and one barrier.  RECORD also writes x_k,
// k = 0 .. K-1, to the tape (B, K, Pv) the adjoint replays (sgd_adjoint.hpp); it changes no arithmetic.
// Host side: one plan and one launcher for the plain and the recording entry point (dava_f64.hpp's rule); both plan
// with any_form = true -- there is no symbol of the LDS image alone.
#include "sgd_f64.hpp"
#include "solve_f64.hpp"

namespace dava {
namespace f64 {

// The LDS image, offsets in doubles (vis: in bytes).  x and g are relative to the vectors' base (LDS, or form 2's
// slice), the others to the LDS base.
struct SgdCarve {
  int x, g, views, vpart, scratch, obs, vis_bytes_off;
  long long total_bytes;
};

__host__ __device__ inline SgdCarve carve_sgd(int M, int N, int Pv, int form) {
  SgdCarve c{};
  const long long MN = (long long)M * N;
  const long long doubles = (form != 2 ? 2LL * Pv : 0) + views_floats(M) + (long long)vpart_floats(M) +
                            2 * kWaves * 32 + (form == 0 ? 2 * MN : 0);
  c.total_bytes = doubles * 8 + (form == 0 ? round_up((int)(MN < (1 << 30) ? MN : (1 << 30)), 8) : 0);
  if (c.total_bytes > kMaxLdsBytes) return c;  // (offsets are meaningful only for an image that fits)
  int o = 0;
  c.x = o; o += Pv;
  c.g = o; o += Pv;
  if (form == 2) o = 0;
  c.views = o; o += views_floats(M);
  c.vpart = o; o += vpart_floats(M);
  c.scratch = o; o += 2 * kWaves * 32;
  c.obs = o; o += form == 0 ? 2 * (int)MN : 0;
  c.vis_bytes_off = o * 8;
  return c;
}

// The form a scene takes: the lowest whose image fits 160 KiB, raised (never lowered) by the F64_FORM override; -1
// where not even form 2's image (the view constants and partials) fits.
inline int choose_sgd_form(int M, int N, int Pv) {
  int form = 2;
  if (carve_sgd(M, N, Pv, 0).total_bytes <= kMaxLdsBytes) form = 0;
  else if (carve_sgd(M, N, Pv, 1).total_bytes <= kMaxLdsBytes) form = 1;
  const long long forced = debug_knob(kDbgF64Form);
  if ((forced == 1 || forced == 2) && forced > form) form = (int)forced;  // (an image that fits form 0 fits form 1)
  if (form == 2 && carve_sgd(M, N, Pv, 2).total_bytes > kMaxLdsBytes) return -1;
  return form;
}

struct SgdArgs {
  Layout L;
  int Pv, K;
  double lr;
  const double* obs;
  const uint8_t* vis;
  const double* x0;
  double* x_out;
  double* trace;  // (B, K) E(x_k), or nullptr
  double* tape;   // (B, K, Pv) x_k (RECORD)
  double* vecs;   // form 2: B x (x, g)[Pv], uninitialised
};

template <int RES, bool RECORD, int FORM>
__global__ __launch_bounds__(kBlock, 1) void sgd_ba_solve_f64_kernel(SgdArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, Pv = a.Pv, K = a.K, MN = M * N;
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const SgdCarve cv = carve_sgd(M, N, Pv, FORM);
  double* vec = lds64;  // x and the gradient: LDS, or (form 2) this problem's workspace slice, laid out alike
  if constexpr (FORM == 2) vec = a.vecs + b * 2 * Pv;
  double* x = vec + cv.x;
  double* g = vec + cv.g;
  double* views = lds64 + cv.views;
  double* vpart = lds64 + cv.vpart;
  double* scratch = lds64 + cv.scratch;
  double* obl = lds64 + cv.obs;  // form 0: the scene's LDS copy
  uint8_t* vil = reinterpret_cast<uint8_t*>(lds64) + cv.vis_bytes_off;
  const double* obs = obl;
  const uint8_t* vis = vil;
  for (int i = tid; i < Pv; i += kBlock) {
    x[i] = i < P ? a.x0[b * P + i] : 0.0;
    g[i] = 0.0;
  }
  if constexpr (FORM == 0) {
    for (int i = tid; i < 2 * MN; i += kBlock) obl[i] = a.obs[b * 2 * MN + i];
    for (int i = tid; i < MN; i += kBlock) vil[i] = a.vis[b * MN + i] ? 1 : 0;
  } else {  // the scene where the caller put it
    obs = a.obs + b * 2 * MN;
    vis = a.vis + b * MN;
  }
  __syncthreads();
  const double lr = a.lr;
  int buf = 0;
  double unused = 0.0;
  for (int k = 0; k < K; ++k) {
    if constexpr (RECORD) {
      double* t = a.tape + (b * K + k) * Pv;
      for (int i = tid; i < Pv; i += kBlock) t[i] = x[i];
    }
    double E = 0.0;
    eval<true, false, false, RES>(L, x, nullptr, 0.0, obs, vis, g, views, vpart, scratch, buf, E, unused);
    if (tid == 0 && a.trace) a.trace[b * K + k] = E;
    for (int i = tid; i < P; i += kBlock) x[i] = descend(x[i], lr, g[i]);
    __syncthreads();
  }
  for (int i = tid; i < P; i += kBlock) a.x_out[b * P + i] = x[i];
}

// ---- host side ----

// What a scene and a config need, from the shapes alone: the queries and the launch's checks read the same numbers.
struct SgdShape {
  int status;  // DAVA_OK: `form` runs this scene / config
  int form, Pv, lds;
  size_t tape_bytes;    // B x K x Pv doubles
  size_t vector_bytes;  // form 2: B x 2 x Pv doubles, else 0
  // [form 2: vectors | tail], else nothing
  size_t workspace_bytes() const { return vector_bytes ? vector_bytes + kTailBytes : 0; }
};

inline SgdShape sgd_shape(const DavaScene& sc, const DavaSgdConfigF64* c) {
  SgdShape s{};
  s.form = -1;
  s.status = sgd_config_status(c);
  if (s.status != DAVA_OK) return s;
  s.status = DAVA_ERR_UNSUPPORTED;
  if (!sizes_sane(sc)) return s;
  s.Pv = round_up(sc.num_parameters, 4);
  s.form = choose_sgd_form(sc.num_views, sc.num_points, s.Pv);
  if (s.form < 0) return s;
  s.status = DAVA_OK;
  s.lds = (int)carve_sgd(sc.num_views, sc.num_points, s.Pv, s.form).total_bytes;
  s.tape_bytes = sgd_tape_bytes(sc.batch, c->iterations, s.Pv);
  s.vector_bytes = s.form == 2 ? (size_t)sc.batch * 2 * s.Pv * sizeof(double) : 0;
  return s;
}

// the shape behind a host-only query (which looks at no data pointer)
inline SgdShape sgd_query(const DavaSceneF64* scene, const DavaSgdConfigF64* c) {
  DavaScene sc;
  SgdShape s{};
  s.form = -1;
  s.status = check_scene_f64(scene, false, sc);
  return s.status == DAVA_OK ? sgd_shape(sc, c) : s;
}

struct SgdPlan {
  int status;
  bool launch;  // false: return `status` (a refusal, or DAVA_OK for an empty batch)
  bool copy;    // K == 0: x_out = x0, a device copy and no launch
  bool ray, record;
  int batch;
  SgdShape shape;
  SgdArgs args;
};

// The checks of both entry points, in their order
inline SgdPlan plan_sgd(const DavaSceneF64* scene, const DavaSgdConfigF64* config, const double* x0, double* x_out,
                        double* error_trace_out, void* tape, size_t tape_bytes, void* workspace,
                        size_t workspace_bytes, bool record) {
  SgdPlan p{};
  const auto refuse = [&p](int st) {
    p.status = st;
    return p;
  };
  DavaScene sc;
  const int st = check_scene_f64(scene, true, sc);
  if (st != DAVA_OK) return refuse(st);
  const SgdShape& s = p.shape = sgd_shape(sc, config);
  if (s.status == DAVA_ERR_INVALID_ARGUMENT) return refuse(s.status);
  if (sc.batch == 0) return refuse(DAVA_OK);
  if (!x0 || !x_out) return refuse(DAVA_ERR_INVALID_ARGUMENT);
  if (s.status != DAVA_OK) return refuse(s.status);
  const int K = config->iterations;
  if (record && K > 0 && (!tape || tape_bytes < s.tape_bytes)) return refuse(DAVA_ERR_WORKSPACE);
  if (s.vector_bytes && (!workspace || workspace_bytes < s.workspace_bytes())) return refuse(DAVA_ERR_WORKSPACE);
  p.ray = sc.residual == DAVA_RESIDUAL_RAY_ANGLE;
  p.record = record;
  p.batch = sc.batch;
  p.copy = K == 0;
  SgdArgs& a = p.args;
  a.L = make_layout(&sc);
  a.Pv = s.Pv;
  a.K = K;
  a.lr = config->learning_rate;
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.x0 = x0;
  a.x_out = x_out;
  a.trace = error_trace_out;
  a.tape = record ? static_cast<double*>(tape) : nullptr;
  a.vecs = s.form == 2 ? static_cast<double*>(workspace) : nullptr;
  p.launch = true;
  return p;
}

template <int FORM>
int launch_sgd(const SgdPlan& p, hipStream_t s) {
  with_flag(p.ray, [&](auto ray) {
    with_flag(p.record, [&](auto record) {
      constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
      launch_lds(sgd_ba_solve_f64_kernel<kRes, decltype(record)::value, FORM>, p.batch, kBlock, p.shape.lds, s, p.args);
    });
  });
  return launched();
}

inline int run_sgd(const SgdPlan& p, void* stream) {
  if (!p.launch) return p.status;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (p.copy) {  // no step: x_out = x0
    const SgdArgs& a = p.args;
    if (a.x_out != a.x0 && hipMemcpyAsync(a.x_out, a.x0, (size_t)p.batch * a.L.P * sizeof(double),
                                          hipMemcpyDeviceToDevice, s) != hipSuccess)
      return DAVA_ERR_LAUNCH;
    return DAVA_OK;
  }
  if (p.shape.form == 0) return launch_sgd<0>(p, s);
  return p.shape.form == 1 ? launch_sgd<1>(p, s) : launch_sgd<2>(p, s);
}

}  // namespace f64
}  // namespace dava

using namespace dava;

extern "C" int dava_ba_sgd_solve_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config, const double* x0,
                                     double* x_out, double* error_trace_out, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  return f64::run_sgd(f64::plan_sgd(scene, config, x0, x_out, error_trace_out, nullptr, 0, workspace, workspace_bytes,
                                    false), stream);
}

extern "C" int dava_ba_sgd_solve_record_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config,
                                            const double* x0, double* x_out, double* error_trace_out, void* tape,
                                            size_t tape_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  return f64::run_sgd(f64::plan_sgd(scene, config, x0, x_out, error_trace_out, tape, tape_bytes, workspace,
                                    workspace_bytes, true), stream);
}

// host-only
extern "C" size_t dava_ba_sgd_tape_bytes_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config) {
  const f64::SgdShape s = f64::sgd_query(scene, config);
  return s.status == DAVA_OK ? s.tape_bytes : 0;
}

// host-only: 0, 1, 2, or minus the status
extern "C" int dava_ba_sgd_solve_form_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config) {
  const f64::SgdShape s = f64::sgd_query(scene, config);
  return s.status == DAVA_OK ? s.form : -s.status;
}

// host-only: exactly what the launch needs (0: none, a NULL workspace is accepted)
extern "C" size_t dava_ba_sgd_solve_workspace_bytes_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config) {
  const f64::SgdShape s = f64::sgd_query(scene, config);
  return s.status == DAVA_OK ? s.workspace_bytes() : 0;
}
