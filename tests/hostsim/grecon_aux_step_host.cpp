// TEST INFRASTRUCTURE: the algorithm of glamr_amd/csrc/grecon_aux_step.hpp (what glamr_grecon_aux_step launches) on the single-threaded host
// runtime, with host pointers and the argument checks of the entry point (aux_step_check, shared).  The scans of the pose VJP run in the
// DEVICE's order of additions (DeviceOrderRT of traj_global_bwd_host.cpp), as grecon_pose_bwd_host.cpp has them; everything else of that
// runtime is HostRT's, which grecon_aux_host.cpp and grecon_cam_bwd_host.cpp run on.  Never loaded by the product.
#include "traj_global_bwd_host.cpp"
#include "../../glamr_amd/csrc/grecon_aux_step.hpp"

extern "C" size_t hostsim_grecon_aux_step_workspace_floats(int n_scenes, int max_persons, int max_len) {
  return glamr::aux_step_workspace(n_scenes, max_persons, max_len).total;
}

// 0, or the entry point's codes: -1 invalid, -4 unsupported
extern "C" int hostsim_grecon_aux_step(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const glamr_aux_desc* aux, const float* root_trans_cam,
                                       float* values, int values_stride, int iteration, float* grads, float* exp_avg, float* exp_avg_sq, double lr, int step,
                                       float* workspace) {
  const char* msg = nullptr;
  const int rc = glamr::aux_step_check(batch, stage, aux, root_trans_cam, values, values_stride, iteration, grads, exp_avg, exp_avg_sq, lr, step, workspace, &msg);
  if (rc != 0 || batch->n_scenes == 0) return rc;
  glamr_param_layout l;
  param_layout(batch->max_persons, batch->max_len, l);
  const glamr::AuxStepBatch s = glamr::aux_step_batch(*batch, *stage, *aux, root_trans_cam, values, values_stride, iteration, grads, exp_avg, exp_avg_sq, lr, step, workspace);
  DeviceOrderRT rt;
  for (int si = 0; si < batch->n_scenes; ++si) {
    if (s.aux.cam_mode == glamr::GAUX_PER_FRAME) glamr::grecon_aux_step<glamr::GAUX_PER_FRAME>(rt, s, l, si);
    else if (s.aux.cam_mode == glamr::GAUX_FIXED) glamr::grecon_aux_step<glamr::GAUX_FIXED>(rt, s, l, si);
    else if (s.aux.cam_mode == glamr::GAUX_DERIVED) glamr::grecon_aux_step<glamr::GAUX_DERIVED>(rt, s, l, si);
    else glamr::grecon_aux_step<glamr::GAUX_CONSTANT>(rt, s, l, si);
  }
  return 0;
}
