// gfx950 kernel + C ABI of the fused global optimiser (algorithm: grecon_algo.hpp).
//
// Launch geometry: ONE workgroup per scene (a sequence with its persons and camera), threads over frames.  A scene's whole
// optimisation state is ~0.1-0.2 MB and stays L2-resident; iterations are separated by workgroup barriers only, so a stage of
// 500 iterations is a single launch with no grid-wide synchronisation and no host round trip.  Many scenes run concurrently,
// one per CU (blockIdx -> scene; with >= 256 scenes every CU is busy; XCD placement is irrelevant because scenes never
// communicate).
#include "common.hpp"
#include "grecon_launch.hpp"
#include "block_rt.hpp"
#include <map>
#include <memory>
#include <set>
#include <mutex>
#include <tuple>
#include <utility>
#include <vector>

namespace glamr {
namespace GLAMR_GRECON_NS {

static_assert(MAX_THREADS <= 512, "DeviceRT::scan_multi / scan_regs fetch the wave totals of a workgroup as two float4 reads: at most 8 waves (block_rt.hpp)");
static_assert(STAGE_RED_FLOATS == RT_RED_FLOATS, "grecon_launch.hpp's estimate of the static LDS");

struct KernelArgs {
  glamr_scene_batch b;
  glamr_stage_desc st;
  glamr_param_layout lay;
  float* workspace;
  unsigned long long* stamps;          // {earliest workgroup start, latest workgroup end} of this launch, 100 MHz ticks
  size_t ws_floats_per_scene;
  float* grads_out;
  const float* adam_tab;               // per-iteration Adam scalars formed on the host (workspace header) or null
  int use_lds;
  unsigned fast_floats;
  int layout_len;      // frames the arena / workspace arrays are laid out for (0 = the batch's max_len)
};

template <int FAST, bool SINGLE, int CAM, int TMC = 0>
__global__ __launch_bounds__(MAX_THREADS, WAVES_PER_EU) void grecon_stage_kernel(KernelArgs a) {
  __shared__ __attribute__((aligned(16))) float red[RT_RED_FLOATS];
  __shared__ Scene sc;
  __shared__ glamr_stage_desc s_st;        // the scene keeps POINTERS to these: they must live in LDS, not in a thread's private copy
  __shared__ glamr_param_layout s_lay;
  extern __shared__ __attribute__((aligned(16))) float arena[];     // prefix-sum buffers and neighbour-read arrays, when they fit
  const int si = blockIdx.x;
  // The stage is the pipeline's critical path; the priors' co-schedulable kernels of the other stream (nn_free.hpp) share these SIMDs
  // and have slack: this kernel's waves win the issue arbitration against them (user priority 0..3, the others stay at 0)
  __builtin_amdgcn_s_setprio(3);
  if (threadIdx.x == 0) {
    atomicMin(a.stamps, (unsigned long long)wall_clock64());
    s_st = a.st;
    s_lay = a.lay;
    assemble_scene(a.b, s_lay, &s_st, si, a.b.n_persons[si], a.b.seq_len[si], a.workspace + (size_t)si * a.ws_floats_per_scene, a.grads_out, sc,
                   a.use_lds ? arena : nullptr, a.fast_floats, a.use_lds, a.layout_len);
    sc.adam_tab = a.adam_tab;
  }
  __syncthreads();
  glamr::DeviceRT rt{red, a.workspace + (size_t)si * a.ws_floats_per_scene};
  run_scene<FAST, SINGLE, CAM, TMC>(rt, sc, a.st, a.lay);
  if (threadIdx.x == 0) atomicMax(a.stamps + 1, (unsigned long long)wall_clock64());
}

// The instances of a launch that also asks for dL/d traj_local_pred (glamr_scene_batch.g_traj_local: the attached trajectory prior of the
// latent-optimisation mode).  A kernel of its own, so that the instances above -- their names included -- are what they were.
template <int FAST>
__global__ __launch_bounds__(MAX_THREADS, WAVES_PER_EU) void grecon_stage_traj_grad_kernel(KernelArgs a) {
  __shared__ __attribute__((aligned(16))) float red[RT_RED_FLOATS];
  __shared__ Scene sc;
  __shared__ glamr_stage_desc s_st;
  __shared__ glamr_param_layout s_lay;
  extern __shared__ __attribute__((aligned(16))) float arena[];
  const int si = blockIdx.x;
  __builtin_amdgcn_s_setprio(3);
  if (threadIdx.x == 0) {
    atomicMin(a.stamps, (unsigned long long)wall_clock64());
    s_st = a.st;
    s_lay = a.lay;
    assemble_scene(a.b, s_lay, &s_st, si, a.b.n_persons[si], a.b.seq_len[si], a.workspace + (size_t)si * a.ws_floats_per_scene, a.grads_out, sc,
                   a.use_lds ? arena : nullptr, a.fast_floats, a.use_lds, a.layout_len);
    sc.adam_tab = a.adam_tab;
  }
  __syncthreads();
  glamr::DeviceRT rt{red, a.workspace + (size_t)si * a.ws_floats_per_scene};
  const TrajGradOut gt{a.b.g_traj_local + (size_t)si * a.b.max_persons * a.b.max_len * 11, a.b.max_persons, a.b.max_len};
  run_scene<FAST, false, 0, 0, true>(rt, sc, a.st, a.lay, gt);
  if (threadIdx.x == 0) atomicMax(a.stamps + 1, (unsigned long long)wall_clock64());
}

#ifdef GLAMR_GRECON_WIDE
// The instances of a launch with the world-frame residuals (glamr_grecon_run_stage_ext: world_dxy, world_res and their regularisers).  Kernels of
// their own, in this compile only: every other instance, its argument block included, is what it was.
struct KernelArgsExt { KernelArgs a; glamr_stage_ext ext; };
template <int FAST>
__global__ __launch_bounds__(MAX_THREADS, WAVES_PER_EU) void grecon_stage_ext_kernel(KernelArgsExt ax) {
  __shared__ __attribute__((aligned(16))) float red[RT_RED_FLOATS];
  __shared__ Scene sc;
  __shared__ glamr_stage_desc s_st;
  __shared__ glamr_param_layout s_lay;
  __shared__ SceneExt s_x;
  extern __shared__ __attribute__((aligned(16))) float arena[];
  const KernelArgs& a = ax.a;
  const int si = blockIdx.x;
  __builtin_amdgcn_s_setprio(3);
  if (threadIdx.x == 0) {
    atomicMin(a.stamps, (unsigned long long)wall_clock64());
    s_st = a.st;
    s_lay = a.lay;
    assemble_scene(a.b, s_lay, &s_st, si, a.b.n_persons[si], a.b.seq_len[si], a.workspace + (size_t)si * a.ws_floats_per_scene, a.grads_out, sc,
                   a.use_lds ? arena : nullptr, a.fast_floats, a.use_lds, a.layout_len);
    sc.adam_tab = a.adam_tab;
    bind_ext(s_x, a.b, ax.ext, si, a.st.niters);
  }
  __syncthreads();
  glamr::DeviceRT rt{red, a.workspace + (size_t)si * a.ws_floats_per_scene};
  run_scene<FAST, false, 0, 0, false, true>(rt, sc, a.st, a.lay, TrajGradOut{nullptr, 0, 0}, &s_x);
  if (threadIdx.x == 0) atomicMax(a.stamps + 1, (unsigned long long)wall_clock64());
}
#endif

}  // namespace GLAMR_GRECON_NS
}  // namespace glamr

using namespace glamr;
using namespace glamr::GLAMR_GRECON_NS;

// Scenes of more than 8 persons (up to GLAMR_GRECON_MAX_PERSONS = 32) run on the instances of csrc/grecon_wide.hip: this file compiled a
// second time with the person arrays of the scene description four times as long (too large for the static LDS the 153 KB arena of the
// instances below leaves), parameters and exchange arrays in the workspace or the lite arena.
constexpr int WIDE_MAX_PERSONS = 32;
#ifdef GLAMR_GRECON_WIDE
#define glamr_grecon_workspace_bytes glamr_grecon_workspace_bytes_wide_
#define glamr_grecon_run_stage glamr_grecon_run_stage_wide_
#define GLAMR_STAGE_EXT_PARAM , const glamr_stage_ext* ext
static_assert(MAXP == WIDE_MAX_PERSONS, "grecon_wide.hip sets GLAMR_MAX_PERSONS");
#else
extern "C" size_t glamr_grecon_workspace_bytes_wide_(int n_scenes, int max_persons, int max_len);
extern "C" int glamr_grecon_run_stage_wide_(const glamr_scene_batch* batch, const glamr_stage_desc* stage, float* grads_out, void* workspace, void* stream_,
                                            const glamr_stage_ext* ext);
#define GLAMR_STAGE_EXT_PARAM

extern "C" int glamr_grecon_param_layout(int max_persons, int max_len, glamr_param_layout* out) {
  GLAMR_REQUIRE(out && max_persons >= 1 && max_persons <= WIDE_MAX_PERSONS && max_len >= 2, "bad arguments (1 <= max_persons <= %d, max_len >= 2)", WIDE_MAX_PERSONS);
  param_layout(max_persons, max_len, *out);
  return GLAMR_OK;
}
#endif

// workspace header: the launch's clock stamps
constexpr size_t GLAMR_GRECON_WS_HEADER = 256;

namespace {
#ifndef GLAMR_GRECON_WIDE
// completion event of the last stage launch per workspace: glamr_grecon_last_launch_ns waits for THAT launch only, not for the device
std::mutex g_ws_mu;
// (an EVENT, not the stream handle: the caller may destroy its stream; an event outlives it.  Shared ownership: a thread that waits for a launch
// holds a reference, NOT the table's mutex -- launches on other workspaces, streams and threads go on while it waits)
struct LaunchEvent {
  hipEvent_t ev = nullptr;
  ~LaunchEvent() { if (ev) (void)hipEventDestroy(ev); }
};
std::map<const void*, std::shared_ptr<LaunchEvent>> g_ws_event;
void forget_workspaces_locked() { g_ws_event.clear(); }
std::shared_ptr<LaunchEvent> new_launch_event() {
  auto e = std::make_shared<LaunchEvent>();
  if (hipEventCreateWithFlags(&e->ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); e->ev = nullptr; return nullptr; }
  return e;
}
void record_launch(const void* workspace, hipStream_t stream);
#endif
// CUs of a device (per device: a process may drive more than one GPU)
int device_cu_count(int dev) {
  static std::mutex mu; static std::map<int, int> cus;
  std::lock_guard<std::mutex> lock(mu);
  int& n = cus[dev];
  if (n <= 0 && (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)) n = 256;
  return n;
}
// Adam's step size and second-moment correction per iteration, in the reference's own arithmetic (Python doubles, libm pow): a running product on
// the device would differ in the last bit of the fp32 scalar now and then, and the update must not (rotmath.hpp).  One table per (device, lr, niters),
// uploaded the first time a stage with that schedule runs and kept for the life of the process: no per-launch host->device copy (a pageable copy on the launch stream would stall a pipelined host).
int adam_table(double lr, int niters, const float** out) {
  static std::mutex mu; static std::map<std::tuple<int, double, int>, float*> tables;
  int devid = 0;
  GLAMR_HIP_CHECK(hipGetDevice(&devid));
  std::lock_guard<std::mutex> lock(mu);
  float*& dtab = tables[std::make_tuple(devid, lr, niters)];
  if (!dtab) {
    std::vector<float> tab(2 * (size_t)niters);
    for (int i = 0; i < niters; ++i) adam_coef_host(lr, i + 1, &tab[2 * (size_t)i]);
    GLAMR_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dtab), tab.size() * sizeof(float)));
    GLAMR_HIP_CHECK(hipMemcpy(dtab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  *out = dtab;
  return GLAMR_OK;
}
// launches the plan's instance; its dynamic-LDS limit is raised once per (device, instance) and process (a driver call per launch is host time on every step)
template <class Args>
int launch_stage(void (*kern)(Args), const StagePlan& plan, int dev, hipStream_t stream, const Args& ka, int n_scenes) {
  if (plan.lds_bytes) {
    static std::mutex mu; static std::set<std::pair<int, const void*>> raised;
    std::lock_guard<std::mutex> lock(mu);
    if (raised.insert(std::make_pair(dev, reinterpret_cast<const void*>(kern))).second)
      GLAMR_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX));
  }
  hipLaunchKernelGGL(kern, dim3(n_scenes), dim3(plan.threads), plan.lds_bytes, stream, ka);
  return GLAMR_OK;
}
int current_device() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess ? dev : 0;
}
}  // namespace

extern "C" size_t glamr_grecon_workspace_bytes(int n_scenes, int max_persons, int max_len) {
  if (n_scenes <= 0 || max_persons < 1 || max_persons > WIDE_MAX_PERSONS || max_len < 2) return 0;
#ifndef GLAMR_GRECON_WIDE
  if (max_persons > MAXP) return glamr_grecon_workspace_bytes_wide_(n_scenes, max_persons, max_len);
  {      // a stage with a flag only the wide instances know (GLAMR_FLAG_ABSOLUTE_HEADING) runs there with ITS workspace layout: the larger of the two
    const size_t wide = glamr_grecon_workspace_bytes_wide_(n_scenes, max_persons, max_len);
    const size_t own = GLAMR_GRECON_WS_HEADER + (size_t)n_scenes * align_up(scene_workspace_floats(max_persons, layout_frames(max_persons, max_len)), 64) * sizeof(float);
    return wide > own ? wide : own;
  }
#endif
  return GLAMR_GRECON_WS_HEADER + (size_t)n_scenes * align_up(scene_workspace_floats(max_persons, layout_frames(max_persons, max_len)), 64) * sizeof(float);
}

#ifndef GLAMR_GRECON_WIDE
namespace { int run_stage_any(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const glamr_stage_ext* ext, float* grads_out, void* workspace, void* stream_); }
extern "C" int glamr_grecon_run_stage(const glamr_scene_batch* batch, const glamr_stage_desc* stage, float* grads_out, void* workspace, void* stream_) {
  return run_stage_any(batch, stage, nullptr, grads_out, workspace, stream_);
}
// per slot and frame: Adam's two moments of the 8 residual numbers and the rotation columns before the orientation residual (grecon_algo.hpp EXT_WS)
extern "C" size_t glamr_grecon_ext_workspace_bytes(int n_scenes, int max_persons, int max_len) {
  if (n_scenes <= 0 || max_persons < 1 || max_persons > WIDE_MAX_PERSONS || max_len < 2) return 0;
  return (size_t)n_scenes * max_persons * max_len * EXT_WS * sizeof(float);
}
// per slot and existing row: Adam's two moments of the two numbers of a heading vector (GLAMR_EXT_HV_WS)
extern "C" size_t glamr_grecon_heading_vec_workspace_bytes(int n_scenes, int max_persons, int max_len) {
  if (n_scenes <= 0 || max_persons < 1 || max_persons > WIDE_MAX_PERSONS || max_len < 2) return 0;
  return (size_t)n_scenes * max_persons * max_len * GLAMR_EXT_HV_WS * sizeof(float);
}
extern "C" int glamr_grecon_run_stage_ext(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const glamr_stage_ext* ext, float* grads_out,
                                          void* workspace, void* stream_) {
  if (ext) {
    GLAMR_REQUIRE(batch && stage && workspace, "null argument");
    GLAMR_REQUIRE(ext->residuals && ext->losses && ext->workspace, "a required array of glamr_stage_ext is NULL");
    GLAMR_REQUIRE(!(ext->var_mask & ~(GLAMR_EXT_VAR_WORLD_DXY | GLAMR_EXT_VAR_WORLD_RES)) && !(ext->flags & ~(GLAMR_EXT_HAS_WORLD_DXY | GLAMR_EXT_APPLY_WORLD_RES)) &&
                      !(ext->loss_mask >> GLAMR_EXT_NUM_LOSSES) && !(ext->monitor_mask >> GLAMR_EXT_NUM_LOSSES), "unknown bits in glamr_stage_ext");
    if (batch->frozen) return fail(GLAMR_E_UNSUPPORTED, "glamr_grecon_run_stage_ext: person-sharded batches (glamr_scene_batch.frozen) are not supported with the world-frame residuals");
    if (batch->g_traj_local) return fail(GLAMR_E_UNSUPPORTED, "glamr_grecon_run_stage_ext: g_traj_local is not supported with the world-frame residuals");
    if (ext->heading_vec) {      // heading_type = 'vec'
      GLAMR_REQUIRE(ext->heading_vec_workspace, "glamr_stage_ext.heading_vec needs heading_vec_workspace (glamr_grecon_heading_vec_workspace_bytes)");
      GLAMR_REQUIRE(!(ext->hv_loss_mask >> GLAMR_EXT_HV_NUM_LOSSES) && !(ext->hv_monitor_mask >> GLAMR_EXT_HV_NUM_LOSSES), "unknown bits in glamr_stage_ext.hv_loss_mask / hv_monitor_mask");
      GLAMR_REQUIRE(!ext->hv_loss_mask || ext->hv_losses, "glamr_stage_ext.hv_loss_mask needs hv_losses");
      if (stage->flags & GLAMR_FLAG_ABSOLUTE_HEADING)
        return fail(GLAMR_E_UNSUPPORTED, "glamr_grecon_run_stage_ext: GLAMR_FLAG_ABSOLUTE_HEADING is not supported with vector headings (glamr_stage_ext.heading_vec)");
      if ((stage->loss_mask >> GLAMR_LOSS_LOCAL_DHEADING_REG_NEW) & 1u)
        return fail(GLAMR_E_UNSUPPORTED, "glamr_grecon_run_stage_ext: GLAMR_LOSS_LOCAL_DHEADING_REG_NEW reads the scalar heading entries, which are dead with vector "
                                         "headings: take the bit off and set GLAMR_EXT_HV_LOSS_DHEADING_REG_NEW in glamr_stage_ext.hv_loss_mask");
    }
  }
  return run_stage_any(batch, stage, ext, grads_out, workspace, stream_);
}
#endif

#ifdef GLAMR_GRECON_WIDE
extern "C" int glamr_grecon_run_stage(const glamr_scene_batch* batch, const glamr_stage_desc* stage, float* grads_out,
                                      void* workspace, void* stream_ GLAMR_STAGE_EXT_PARAM) {
#else
namespace {
int run_stage_any(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const glamr_stage_ext* ext, float* grads_out, void* workspace, void* stream_) {
#endif
  GLAMR_REQUIRE(batch && stage && workspace, "null argument");
  GLAMR_REQUIRE(batch->n_scenes > 0 && batch->max_persons >= 1 && batch->max_persons <= WIDE_MAX_PERSONS && batch->max_len >= 2,
                "bad batch geometry: n_scenes=%d max_persons=%d (at most %d) max_len=%d", batch->n_scenes, batch->max_persons, WIDE_MAX_PERSONS, batch->max_len);
#ifndef GLAMR_GRECON_WIDE
  if (batch->max_persons > MAXP || (stage && (stage->flags & GLAMR_FLAG_ABSOLUTE_HEADING)) || ext) {
    const int rc = glamr_grecon_run_stage_wide_(batch, stage, grads_out, workspace, stream_, ext);
    if (rc == GLAMR_OK) record_launch(workspace, static_cast<hipStream_t>(stream_));
    return rc;
  }
#endif
  GLAMR_REQUIRE(batch->n_joints == NJ, "n_joints must be %d", NJ);
  GLAMR_REQUIRE(batch->max_len <= GLAMR_GRECON_MAX_FRAMES, "max_len=%d exceeds %d frames", batch->max_len, GLAMR_GRECON_MAX_FRAMES);
  GLAMR_REQUIRE(batch->n_persons && batch->seq_len && batch->fr_start && batch->fr_end && batch->vis && batch->j_local && batch->kp_2d &&
                    batch->kp_score && batch->cam_K && batch->traj_local_pred && batch->orient_cam && batch->base_orient &&
                    batch->base_trans && batch->person2cam && batch->cam_pose && batch->params && batch->losses && batch->orient_world &&
                    batch->trans_world && batch->kp_2d_pred && batch->orient_cam_in_world,
                "a required array of glamr_scene_batch is NULL");
  GLAMR_REQUIRE(batch->max_persons == 1 || batch->rel_transform_cam || !((stage->loss_mask >> GLAMR_LOSS_REL_TRANSFORM) & 1u),
                "rel_transform loss needs rel_transform_cam for multi-person scenes");
  GLAMR_REQUIRE(stage->niters >= 0, "niters must be >= 0");
  GLAMR_REQUIRE(!batch->g_traj_local || (grads_out && stage->niters >= 1 && !(stage->flags & GLAMR_FLAG_ABSOLUTE_HEADING) && !(batch->loss_history)),
                "g_traj_local needs grads_out and niters >= 1, and goes with neither absolute headings nor the loss history");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  KernelArgs ka;
  ka.b = *batch;
  ka.st = *stage;
  param_layout(batch->max_persons, batch->max_len, ka.lay);
  // workspace header: the launch's own clock stamps (read back with glamr_grecon_last_launch_ns)
  ka.stamps = static_cast<unsigned long long*>(workspace);
  GLAMR_HIP_CHECK(hipMemsetAsync(workspace, 0xFF, 8, stream));
  GLAMR_HIP_CHECK(hipMemsetAsync(static_cast<char*>(workspace) + 8, 0, 8, stream));
  ka.workspace = reinterpret_cast<float*>(static_cast<char*>(workspace) + GLAMR_GRECON_WS_HEADER);
  ka.adam_tab = nullptr;
  if (stage->niters > 0 && stage->niters <= ADAM_TAB_MAX && adam_table(stage->lr, (int)stage->niters, &ka.adam_tab) != GLAMR_OK) return GLAMR_E_HIP;
  ka.ws_floats_per_scene = align_up(scene_workspace_floats(batch->max_persons, layout_frames(batch->max_persons, batch->max_len)), 64);
  ka.grads_out = grads_out;
  // which instance, with how many threads and which arena: grecon_launch.hpp
  const int dev = current_device();
  const StagePlan plan = plan_stage({batch->n_scenes, batch->max_persons, batch->max_len, (int)stage->niters, camera_mode(*stage), grads_out != nullptr,
                                     batch->loss_history != nullptr, batch->g_traj_local != nullptr}, launch_env(device_cu_count(dev)));
  ka.use_lds = plan.use_lds; ka.fast_floats = plan.fast_floats; ka.layout_len = plan.layout_len;
  int rc = GLAMR_OK;
  const bool known = with_stage_instance(plan.inst, [&](auto tag) {
    constexpr StageInstance I = decltype(tag)::value;
#ifdef GLAMR_GRECON_WIDE
    if constexpr (!I.gt) {
      if (ext) { rc = launch_stage(grecon_stage_ext_kernel<I.fast>, plan, dev, stream, KernelArgsExt{ka, *ext}, ka.b.n_scenes); return; }
    }
#endif
    if constexpr (I.gt) rc = launch_stage(grecon_stage_traj_grad_kernel<I.fast>, plan, dev, stream, ka, ka.b.n_scenes);
    else rc = launch_stage(grecon_stage_kernel<I.fast, I.single, I.cam, I.tmc>, plan, dev, stream, ka, ka.b.n_scenes);
  });
  GLAMR_REQUIRE(known, "no stage kernel instance FAST=%d SINGLE=%d CAM=%d TMC=%d GT=%d", plan.inst.fast, plan.inst.single, plan.inst.cam, plan.inst.tmc, plan.inst.gt);
  if (rc) return rc;
  GLAMR_HIP_CHECK(hipGetLastError());
#ifndef GLAMR_GRECON_WIDE
  record_launch(workspace, stream);
#endif
  return GLAMR_OK;
}
#ifndef GLAMR_GRECON_WIDE
}  // namespace
#endif

#ifndef GLAMR_GRECON_WIDE
namespace {
void record_launch(const void* workspace, hipStream_t stream) {
  {
    // completion event of this launch, per workspace (not under stream capture: a captured launch has no completion of its own, and
    // glamr_grecon_last_launch_ns then falls back to a device-wide wait)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    std::lock_guard<std::mutex> lock(g_ws_mu);
    if (cap == hipStreamCaptureStatusNone) {
      if (g_ws_event.size() > 4096) forget_workspaces_locked();      // callers that never ask for the stamps
      auto it = g_ws_event.find(workspace);
      // an event somebody is waiting on keeps standing for the launch it was recorded after: this launch gets a new one
      if (it != g_ws_event.end() && it->second.use_count() > 1) { g_ws_event.erase(it); it = g_ws_event.end(); }
      if (it == g_ws_event.end()) {
        if (auto e = new_launch_event()) it = g_ws_event.emplace(workspace, std::move(e)).first;
      }
      if (it != g_ws_event.end() && hipEventRecord(it->second->ev, stream) != hipSuccess) { (void)hipGetLastError(); g_ws_event.erase(it); }
    } else {
      g_ws_event.erase(workspace);
    }
  }
}
}  // namespace

// torch.optim.Adam on a flat parameter vector, with the optimiser's own update function: the entry point the parity tests use to
// check the device arithmetic bit for bit against torch.optim.Adam (and a plain fused Adam for callers that keep their own loop)
__global__ void adam_step_kernel(int n, float* p, float* m, float* v, const float* g, glamr::grecon::AdamCoef c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) glamr::grecon::adam(p[i], m[i], v[i], g[i], c);
}
extern "C" int glamr_adam_step(int n, float* params, float* exp_avg, float* exp_avg_sq, const float* grad, double lr, int step, void* stream_) {
  GLAMR_REQUIRE(n >= 0 && (n == 0 || (params && exp_avg && exp_avg_sq && grad)), "null argument");
  GLAMR_REQUIRE(step >= 1 && lr > 0.0, "step must be >= 1 (1-based, as torch counts) and lr > 0");
  if (n == 0) return GLAMR_OK;
  float tab[2];
  adam_coef_host(lr, step, tab);
  AdamCoef c{tab[0], tab[1], 0.0f};
  c.inv_bc2_sqrt = 1.0f / tab[1];            // (host: IEEE division)
  hipLaunchKernelGGL(adam_step_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream_), n, params, exp_avg, exp_avg_sq, grad, c);
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}

// The same step with its number ON THE DEVICE: loops that are replayed as HIP graphs (the latent-optimisation mode's iteration) cannot carry
// a per-iteration scalar in a kernel argument.  `coef` holds two floats per step, made on the host (Python's arithmetic: libm pow in double).
__global__ void adam_step_indexed_kernel(int n, float* p, float* m, float* v, const float* g, const float* coef, const int32_t* step_index) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = *step_index;
  glamr::grecon::AdamCoef c{coef[2 * k], coef[2 * k + 1], 0.0f};
  c.finish();
  if (i < n) glamr::grecon::adam(p[i], m[i], v[i], g[i], c);
}
__global__ void counter_add_kernel(int32_t* c, int value) { *c += value; }

extern "C" int glamr_adam_coef_table(double lr, int n_steps, float* out_host) {
  GLAMR_REQUIRE(out_host && n_steps > 0 && lr > 0.0, "bad argument");
  for (int k = 0; k < n_steps; ++k) adam_coef_host(lr, k + 1, out_host + 2 * k);
  return GLAMR_OK;
}
extern "C" int glamr_adam_step_indexed(int n, float* params, float* exp_avg, float* exp_avg_sq, const float* grad, const float* coef_table,
                                       const int32_t* step_index, void* stream_) {
  GLAMR_REQUIRE(n >= 0 && (n == 0 || (params && exp_avg && exp_avg_sq && grad)) && coef_table && step_index, "null argument");
  if (n == 0) return GLAMR_OK;
  hipLaunchKernelGGL(adam_step_indexed_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream_), n, params, exp_avg, exp_avg_sq, grad,
                     coef_table, step_index);
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}
extern "C" int glamr_counter_add(int32_t* counter, int value, void* stream_) {
  GLAMR_REQUIRE(counter, "null argument");
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream_), counter, value);
  GLAMR_HIP_CHECK(hipGetLastError());
  return GLAMR_OK;
}

#ifdef GLAMR_PHASE_TIMING
// development builds only: per-phase time of workgroup 0 in the last stage launch, in 10 ns ticks
extern "C" int glamr_debug_phase_ticks(unsigned long long* out16) {
  GLAMR_HIP_CHECK(hipDeviceSynchronize());
  GLAMR_HIP_CHECK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(glamr::g_phase_ticks), 16 * sizeof(unsigned long long)));
  return GLAMR_OK;
}
#endif

extern "C" int glamr_grecon_last_launch_ns(const void* workspace, double* ns) {
  GLAMR_REQUIRE(workspace && ns, "null argument");
  unsigned long long st[2];
  // the stamps are read on the stream the launch ran on: this waits for the work of THAT stream, not for the device (a pipelined caller
  // keeps its other streams running).  A workspace this library has not seen a launch on falls back to a device-wide wait.
  // The launch's own completion event: waits for that launch, not for the device.  The table's mutex only covers the look-up; the wait holds a
  // reference to the event, so another thread's launch on the same workspace (record_launch) or the table's clean-up cannot destroy it under this
  // thread, and launches on any workspace proceed while it waits.
  bool waited = false;
  {
    std::shared_ptr<LaunchEvent> e;
    {
      std::lock_guard<std::mutex> lock(g_ws_mu);
      auto it = g_ws_event.find(workspace);
      if (it != g_ws_event.end()) e = it->second;
    }
    if (e) waited = hipEventSynchronize(e->ev) == hipSuccess;
  }
  if (!waited) {
    (void)hipGetLastError();
    GLAMR_HIP_CHECK(hipDeviceSynchronize());
  }
  // the 16 bytes come back on a stream of their own (non-blocking: a plain hipMemcpy goes through the null stream and would wait for every
  // blocking stream of the process)
  {
    static std::mutex cmu;
    static std::map<int, hipStream_t> copy_streams;
    std::lock_guard<std::mutex> lock(cmu);
    hipStream_t& cs = copy_streams[current_device()];
    if (!cs) GLAMR_HIP_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    GLAMR_HIP_CHECK(hipMemcpyAsync(st, workspace, sizeof(st), hipMemcpyDeviceToHost, cs));
    GLAMR_HIP_CHECK(hipStreamSynchronize(cs));
  }
  GLAMR_REQUIRE(st[0] != ~0ull, "no stage launch has completed on this workspace");
  *ns = st[1] > st[0] ? (double)(st[1] - st[0]) * 10.0 : 0.0;
  return GLAMR_OK;
}
#endif  // !GLAMR_GRECON_WIDE
