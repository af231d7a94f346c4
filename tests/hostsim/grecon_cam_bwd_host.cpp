// TEST INFRASTRUCTURE: the algorithm of glamr_amd/csrc/grecon_cam_bwd.hpp (what glamr_grecon_cam_backward launches) on the single-threaded
// host runtime of grecon_host.cpp, with host pointers and the argument checks of the entry point.  Never loaded by the product.
#include "grecon_host.cpp"
#include "../../glamr_amd/csrc/grecon_cam_bwd.hpp"

extern "C" size_t hostsim_grecon_cam_bwd_workspace_floats(int n_scenes, int max_persons, int max_len) {
  (void)max_persons;
  return (size_t)n_scenes * max_len * glamr::GCB_WS_FLOATS_PER_FRAME;
}

// 0, or the entry point's codes: -1 invalid, -4 unsupported
extern "C" int hostsim_grecon_cam_bwd(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const float* g_cam_pose, float* grads, int accumulate,
                                      float* g_orient_world, float* g_trans_world, float* workspace) {
  if (!batch || !stage || !g_cam_pose || !grads || !workspace) return GLAMR_E_INVALID;
  if (batch->n_scenes < 0 || batch->max_persons < 1 || batch->max_persons > 32 || batch->max_len < 1) return GLAMR_E_INVALID;
  const int mode = camera_mode(*stage);
  if (mode == glamr::GCB_CONSTANT) return GLAMR_E_UNSUPPORTED;
  if (mode == glamr::GCB_DERIVED && !(g_orient_world && g_trans_world)) return GLAMR_E_INVALID;
  if (batch->n_scenes == 0) return 0;
  if (!batch->seq_len || !batch->params) return GLAMR_E_INVALID;
  if (mode == glamr::GCB_DERIVED && !(batch->n_persons && batch->vis && batch->person2cam && batch->orient_world && batch->trans_world)) return GLAMR_E_INVALID;
  glamr_param_layout l;
  param_layout(batch->max_persons, batch->max_len, l);
  const glamr::CamBwdBatch b = glamr::cam_bwd_batch(*batch, g_cam_pose, grads, accumulate, g_orient_world, g_trans_world, workspace);
  HostRT rt;
  for (int si = 0; si < batch->n_scenes; ++si) {
    if (mode == glamr::GCB_PER_FRAME) glamr::grecon_cam_bwd<glamr::GCB_PER_FRAME>(rt, b, l, si);
    else if (mode == glamr::GCB_FIXED) glamr::grecon_cam_bwd<glamr::GCB_FIXED>(rt, b, l, si);
    else glamr::grecon_cam_bwd<glamr::GCB_DERIVED>(rt, b, l, si);
  }
  return 0;
}
