// TEST INFRASTRUCTURE: the stage algorithm's instance that also writes dL/d traj_local_pred (glamr_scene_batch.g_traj_local; run_scene's GT
// switch) on the single-threaded host runtime of grecon_host.cpp -- what csrc/grecon.hip launches for such a batch (several persons, any camera
// mode), with host pointers.  Never loaded by the product.
#include "grecon_host.cpp"

extern "C" int hostsim_grecon_run_stage_traj_grad(const glamr_scene_batch* b, const glamr_stage_desc* st, float* grads_out) {
  if (unsupported(st)) return 2;
  if (!b->g_traj_local || !grads_out || st->niters < 1) return -1;
  HostRT rt;
  return run_scenes(rt, b, st, grads_out, b->n_scenes, 0, 0, true);
}
