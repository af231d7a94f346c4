// TEST INFRASTRUCTURE: the stage launcher's plan and instance list (glamr_amd/csrc/grecon_launch.hpp) behind a C interface, for
// tests/test_stage_plan.py.  Included by grecon_host.cpp (the rules of the 8-person build) and grecon_wide_host.cpp (those of the 32-person build).
#pragma once
#include "../../glamr_amd/csrc/grecon_launch.hpp"

namespace stage_plan_shim {
using namespace glamr::GLAMR_GRECON_NS;
inline void put(const StageInstance& i, long long* out) { out[0] = i.fast; out[1] = i.single; out[2] = i.cam; out[3] = i.tmc; out[4] = i.gt; }
template <class... I> int list(InstanceList<I...>, long long* out, int cap) {
  const StageInstance all[] = {I::value...};
  for (int k = 0; k < (int)sizeof...(I) && k < cap; ++k) put(all[k], out + 5 * k);
  return (int)sizeof...(I);
}
}  // namespace stage_plan_shim

// out[10] = {FAST, SINGLE, CAM, TMC, GT, threads, dynamic LDS bytes, fast_floats, use_lds, layout_len}; -1 if `wide` is not this build
extern "C" int hostsim_grecon_stage_plan(int n_scenes, int max_persons, int max_len, int niters, int camera_mode, int grads_out, int loss_history,
                                         int g_traj_local, int n_cus, int has_lds_kb, int lds_kb, int no_const_layout, int no_mid_arena, int wide,
                                         long long* out) {
  using namespace stage_plan_shim;
  if ((wide != 0) != WIDE_BUILD) return -1;
  const StagePlan p = plan_stage(StageShape{n_scenes, max_persons, max_len, niters, camera_mode, grads_out != 0, loss_history != 0, g_traj_local != 0},
                                 LaunchEnv{n_cus, has_lds_kb != 0, lds_kb, no_const_layout != 0, no_mid_arena != 0});
  put(p.inst, out);
  out[5] = p.threads; out[6] = (long long)p.lds_bytes; out[7] = p.fast_floats; out[8] = p.use_lds; out[9] = p.layout_len;
  return 0;
}
// the instance list of this build, five numbers per entry (at most `cap` entries written); returns its length
extern "C" int hostsim_grecon_stage_instances(long long* out, int cap) { return stage_plan_shim::list(stage_plan_shim::StageInstances{}, out, cap); }
// the tags with_stage_instance hands its callback for this run-time instance; 0 if the list has no such entry (`out` untouched)
extern "C" int hostsim_grecon_stage_instance_tags(int fast, int single, int cam, int tmc, int gt, long long* out) {
  using namespace stage_plan_shim;
  return with_stage_instance(StageInstance{fast, single != 0, cam, tmc, gt != 0}, [&](auto tag) {
    put(decltype(tag)::value, out);
  });
}
