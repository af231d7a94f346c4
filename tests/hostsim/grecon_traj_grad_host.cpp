// TEST INFRASTRUCTURE: the stage algorithm's instance that also writes dL/d traj_local_pred (glamr_scene_batch.g_traj_local; run_scene's GT
// switch) on the single-threaded host runtime of grecon_host.cpp -- what csrc/grecon.hip launches for such a batch (several persons, any camera
// mode), with host pointers.  Never loaded by the product.
#include "grecon_host.cpp"

extern "C" int hostsim_grecon_run_stage_traj_grad(const glamr_scene_batch* b, const glamr_stage_desc* st, float* grads_out) {
  if (unsupported(st)) return 2;
  if (!b->g_traj_local || !grads_out || st->niters < 1) return -1;
  glamr_param_layout l;
  param_layout(b->max_persons, b->max_len, l);
  std::vector<float> ws(scene_workspace_floats(b->max_persons, b->max_len));
  std::vector<float> tab(2 * (size_t)st->niters);
  for (int i = 0; i < st->niters; ++i) adam_coef_host(st->lr, i + 1, &tab[2 * (size_t)i]);
  HostRT rt;
  for (int si = 0; si < b->n_scenes; ++si) {
    Scene sc;
    assemble_scene(*b, l, st, si, b->n_persons[si], b->seq_len[si], ws.data(), grads_out, sc);
    sc.adam_tab = st->niters <= ADAM_TAB_MAX ? tab.data() : nullptr;
    const TrajGradOut gt{b->g_traj_local + (size_t)si * b->max_persons * b->max_len * 11, b->max_persons, b->max_len};
    run_scene<0, false, 0, 0, true>(rt, sc, *st, l, gt);
  }
  return 0;
}
