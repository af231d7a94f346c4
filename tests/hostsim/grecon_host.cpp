// TEST INFRASTRUCTURE: instantiates the per-scene optimiser algorithm (glamr_amd/csrc/grecon_algo.hpp) with a single-threaded
// host runtime so the CPU test-suite can check its gradients and control flow against the oracle without a GPU.
// Same argument structs as the C ABI, but every pointer is a HOST pointer.  Never loaded by the product.
#include "stage_plan_shim.hpp"      // (grecon_algo.hpp through grecon_launch.hpp, and the plan's own entry points)
#include <vector>
using namespace glamr::grecon;

struct HostRT {
  static constexpr bool one_thread_per_frame = false;
  float* arena_ = nullptr; float* ws_ = nullptr;      // only the constant-layout instances ask for them
  float* arena() const { return arena_; }
  float* workspace() const { return ws_; }
  int tid() const { return 0; }
  int nthreads() const { return 1; }
  void sync() const {}
  float reduce_sum(float v) const { return v; }
  template <int N> void reduce_sum_n(float (&)[N]) const {}
  template <bool LDS = false>
  void scan_multi(float* const* ch, int nch, int n, int stride, bool reverse, bool /*shuffle_order*/ = false) const {
    for (int c = 0; c < nch; ++c) scan(ch[c], n, stride, reverse);
  }
  void scan(float* a, int n, int stride, bool reverse) const {
    if (!reverse) { for (int i = 1; i < n; ++i) a[(size_t)i * stride] += a[(size_t)(i - 1) * stride]; }
    else { for (int i = n - 2; i >= 0; --i) a[(size_t)i * stride] += a[(size_t)(i + 1) * stride]; }
  }
};

// HostRT + a per-iteration record of the scene's parameter vector and gradient (scene 0): the trajectory tests/tools compare with
// the reference's Adam trajectory iteration by iteration
struct TraceRT : HostRT {
  float* params_out = nullptr;   // [niters][scene_stride]
  float* grads_out = nullptr;    // [niters][scene_stride] (needs store_grad) or null
  int stride = 0;
  void trace(int it, Scene& sc) {
    if (params_out) for (int i = 0; i < stride; ++i) params_out[(size_t)it * stride + i] = sc.cp[i];
    if (grads_out && sc.store_grad) for (int i = 0; i < stride; ++i) grads_out[(size_t)it * stride + i] = sc.cg[i];
  }
};

// absolute_heading is only compiled into the instances of csrc/grecon_wide.hip: this runtime would silently accumulate the headings -- every
// entry point that takes a stage descriptor refuses it (return code 2; the callers assert 0)
static bool unsupported(const glamr_stage_desc* st) { return (st->flags & GLAMR_FLAG_ABSOLUTE_HEADING) != 0; }

// Instances are chosen through the device launcher's list (grecon_launch.hpp: with_stage_instance), and this one: the single-person / camera-mode
// specialisations WITHOUT an arena (FAST = 0), which the device never launches and this runtime -- no arena unless an entry point lends one -- does.
using HostOnlyInstances = InstanceList<Inst<0, true, 1>, Inst<0, true, 2>, Inst<0, true, 0>, Inst<0, false, 1>, Inst<0, false, 2>, Inst<0, false, 3>>;

// One stage over the first `n_scenes` scenes of the batch, each on the specialisation <fast, ., ., tmc> for its own person count and the stage's
// camera mode (gt: on the instance that also writes dL/d traj_local_pred): the workspace, the Adam table and, for fast = 1 -- the full arena of
// single-person scenes -- the arena in host memory with room for two keypoint rows "on chip"; tmc > 0 = arena / workspace laid out for that many
// frames (the constant-layout instance).  -3: an instance neither list has, or an arena mode nobody lends this runtime an arena for.
template <class RT>
static int run_scenes(RT& rt, const glamr_scene_batch* b, const glamr_stage_desc* st, float* grads_out, int n_scenes, int fast = 0, int tmc = 0, bool gt = false) {
  const int lay_len = tmc > 0 ? tmc : b->max_len;
  const glamr_param_layout l = make_layout(b->max_persons, b->max_len);
  std::vector<float> ws(scene_workspace_floats(b->max_persons, lay_len)), arena(fast ? scene_fast_floats(1, lay_len, 1) + (size_t)2 * 6 * lay_len : 0);
  std::vector<float> tab(2 * (size_t)(st->niters > 0 ? st->niters : 1));
  for (size_t i = 0; 2 * i < tab.size(); ++i) adam_coef_host(st->lr, (int)i + 1, &tab[2 * i]);
  rt.arena_ = fast ? arena.data() : nullptr; rt.ws_ = ws.data();
  for (int si = 0; si < n_scenes; ++si) {
    Scene sc;
    assemble_scene(*b, l, st, si, b->n_persons[si], b->seq_len[si], ws.data(), grads_out, sc, rt.arena_, arena.size(), 1, tmc);
    sc.adam_tab = st->niters <= ADAM_TAB_MAX ? tab.data() : nullptr;
    const bool single = !gt && b->n_persons[si] == 1;
    const StageInstance inst{fast, single, gt ? 0 : instance_cam(single, camera_mode(*st)), tmc, gt};
    const TrajGradOut go{gt ? b->g_traj_local + (size_t)si * b->max_persons * b->max_len * 11 : nullptr, b->max_persons, b->max_len};
    bool ran = false;
    auto run = [&](auto tag) {
      constexpr StageInstance I = decltype(tag)::value;
      constexpr bool have = I.fast == 0 || (I.fast == 1 && I.single && !I.gt);      // (the other arena modes are not instantiated)
      if constexpr (have && I.gt) run_scene<I.fast, I.single, I.cam, I.tmc, true>(rt, sc, *st, l, go);
      else if constexpr (have) run_scene<I.fast, I.single, I.cam, I.tmc>(rt, sc, *st, l);
      ran = have;
    };
    if (!(with_stage_instance(inst, run) || with_instance(HostOnlyInstances{}, inst, run)) || !ran) return -3;
  }
  return 0;
}

// scene 0 only, with the trajectory recorded
extern "C" int hostsim_grecon_trace_stage(const glamr_scene_batch* b, const glamr_stage_desc* st, float* grads_scratch, float* params_trace, float* grads_trace) {
  if (unsupported(st)) return 2;
  TraceRT rt;
  rt.params_out = params_trace; rt.grads_out = grads_trace; rt.stride = make_layout(b->max_persons, b->max_len).scene_stride;
  return run_scenes(rt, b, st, grads_scratch, 1);
}

extern "C" int hostsim_grecon_param_layout(int max_persons, int max_len, glamr_param_layout* out) {
  param_layout(max_persons, max_len, *out);
  return 0;
}

extern "C" int hostsim_grecon_run_stage(const glamr_scene_batch* b, const glamr_stage_desc* st, float* grads_out) {
  if (unsupported(st)) return 2;
  HostRT rt;
  return run_scenes(rt, b, st, grads_out, b->n_scenes);
}

// The full-arena single-person instances (parameters + Adam moments in the arena) with the arena in host memory; const_layout = laid out for
// GLAMR_CONST_LAYOUT_FRAMES frames.  Must give the results of hostsim_grecon_run_stage to the bit: same arithmetic, different addresses.
extern "C" int hostsim_grecon_run_stage_arena(const glamr_scene_batch* b, const glamr_stage_desc* st, int const_layout) {
  if (unsupported(st)) return 2;
  if (b->max_persons != 1) return -1;
  if (const_layout && layout_frames(1, b->max_len) != CL) return -2;
  HostRT rt;
  return run_scenes(rt, b, st, nullptr, b->n_scenes, 1, const_layout ? CL : 0);
}

// The same instance WITH the gradient record: what a stage driven launch by launch from outside runs on the device for one-person scenes
// (latent-optimisation mode, GLAMR_FLAG_KEEP_CAM_PARAMS).
extern "C" int hostsim_grecon_run_stage_arena_grads(const glamr_scene_batch* b, const glamr_stage_desc* st, float* grads_out) {
  if (unsupported(st)) return 2;
  if (b->max_persons != 1) return -1;
  HostRT rt;
  return run_scenes(rt, b, st, grads_out, b->n_scenes, 1);
}

// the optimiser's Adam update on a flat vector (compared bit for bit with torch.optim.Adam in tests/test_adam_exact.py)
extern "C" void hostsim_adam_step(int n, float* p, float* m, float* v, const float* g, double lr, int step) {
  float tab[2];
  adam_coef_host(lr, step, tab);
  AdamCoef c{tab[0], tab[1], 0.0f};
  c.finish();
  for (int i = 0; i < n; ++i) adam(p[i], m[i], v[i], g[i], c);
}
