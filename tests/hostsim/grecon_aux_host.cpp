// TEST INFRASTRUCTURE: the algorithm of glamr_amd/csrc/grecon_aux.hpp (what glamr_grecon_aux_terms launches) on the single-threaded host
// runtime of grecon_host.cpp, with host pointers and the argument checks of the entry point (aux_check, shared).  Never loaded by the product.
#include "grecon_host.cpp"
#include "../../glamr_amd/csrc/grecon_aux.hpp"

extern "C" size_t hostsim_grecon_aux_workspace_ints(int n_scenes, int max_persons, int max_len) {
  (void)max_len;
  return (size_t)n_scenes * max_persons;
}

// 0, or the entry point's codes: -1 invalid, -4 unsupported
extern "C" int hostsim_grecon_aux_terms(const glamr_scene_batch* batch, const glamr_stage_desc* stage, const glamr_aux_desc* aux, const float* root_trans_cam,
                                        float* values, float* g_trans_world, float* g_cam_pose, float* grads, int accumulate, int32_t* workspace) {
  const char* msg = nullptr;
  const int rc = glamr::aux_check(batch, stage, aux, root_trans_cam, values, g_trans_world, g_cam_pose, grads, workspace, &msg);
  if (rc != 0 || batch->n_scenes == 0) return rc;
  glamr_param_layout l;
  param_layout(batch->max_persons, batch->max_len, l);
  const glamr::AuxBatch b = glamr::aux_batch(*batch, *stage, *aux, root_trans_cam, values, g_trans_world, g_cam_pose, grads, accumulate, workspace);
  HostRT rt;
  for (int si = 0; si < batch->n_scenes; ++si) glamr::grecon_aux_terms(rt, b, l, si);
  return 0;
}
