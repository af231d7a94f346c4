// TEST INFRASTRUCTURE: the algorithm of glamr_amd/csrc/grecon_pose_bwd.hpp (what glamr_grecon_pose_backward launches) on the single-threaded
// host runtime, with host pointers and the argument checks of the entry point.  The scans run in the DEVICE's order of additions
// (DeviceOrderRT of traj_global_bwd_host.cpp).  Never loaded by the product.
#include "traj_global_bwd_host.cpp"
#include "../../glamr_amd/csrc/grecon_pose_bwd.hpp"

extern "C" size_t hostsim_grecon_pose_bwd_workspace_floats(int n_scenes, int max_persons, int max_len) {
  return (size_t)n_scenes * max_persons * max_len * glamr::GPB_WS_FLOATS_PER_FRAME;
}

// 0, or the entry point's codes: -1 invalid, -4 unsupported
extern "C" int hostsim_grecon_pose_bwd(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const float* g_orient_world, const float* g_trans_world, float* grads,
                                       int accumulate, float* workspace) {
  if (!batch || !stage || !grads || !workspace) return GLAMR_E_INVALID;
  if (batch->n_scenes < 0 || batch->max_persons < 1 || batch->max_persons > 32 || batch->max_len < 2) return GLAMR_E_INVALID;
  if (!g_orient_world && !g_trans_world) return GLAMR_E_INVALID;
  if (stage->flags & GLAMR_FLAG_ABSOLUTE_HEADING) return GLAMR_E_UNSUPPORTED;
  if (batch->n_scenes == 0) return 0;
  if (!batch->n_persons || !batch->seq_len || !batch->fr_start || !batch->fr_end || !batch->traj_local_pred || !batch->params) return GLAMR_E_INVALID;
  if ((stage->flags & GLAMR_FLAG_HAS_WORLD_DHEADING) && g_orient_world && !batch->base_orient) return GLAMR_E_INVALID;
  glamr_param_layout l;
  param_layout(batch->max_persons, batch->max_len, l);
  const glamr::PoseBwdBatch b = glamr::pose_bwd_batch(*batch, *stage, g_orient_world, g_trans_world, grads, accumulate, workspace);
  DeviceOrderRT rt;
  for (int slot = 0; slot < batch->n_scenes * batch->max_persons; ++slot) {
    if (!accumulate && slot % b.P == 0) glamr::grecon_pose_bwd_clear(rt, grads + (size_t)(slot / b.P) * l.scene_stride, l.person0);
    glamr::grecon_pose_bwd(rt, b, l, slot);
  }
  return 0;
}
