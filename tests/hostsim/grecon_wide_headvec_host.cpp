// TEST INFRASTRUCTURE: grecon_wide_ext_host.cpp's twin of glamr_grecon_run_stage_ext with the vector headings of glamr_stage_ext
// (heading_vec, heading_type = 'vec'): the algorithm the way csrc/grecon_wide.hip compiles it on the single-threaded host runtime, every pointer
// a HOST pointer, the workspace instance <0, false, 0>, and the launcher's refusals.  Never loaded by the product.
#define GLAMR_GRECON_WIDE 1
#define GLAMR_MAX_PERSONS 32
#define GLAMR_GRECON_NS grecon_wide
#include "../../glamr_amd/csrc/grecon_launch.hpp"
#include <memory>
#include <vector>
using namespace glamr::grecon_wide;

namespace {
struct HostRT {      // (grecon_host.cpp's, for this namespace)
  static constexpr bool one_thread_per_frame = false;
  float* arena() const { return nullptr; }
  float* workspace() const { return nullptr; }
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
}  // namespace

extern "C" size_t hostsim_grecon_heading_vec_workspace_floats(int n_scenes, int max_persons, int max_len) {
  return (size_t)n_scenes * max_persons * max_len * GLAMR_EXT_HV_WS;
}

// ext == NULL: the plain stage.  -1: what glamr_grecon_run_stage_ext refuses outright (frozen slots, g_traj_local, a missing array);
// -2: its GLAMR_E_UNSUPPORTED with vector headings (absolute headings, the fused regulariser on the dead scalar entries).
extern "C" int hostsim_grecon_wide_run_stage_headvec(const glamr_scene_batch* b, const glamr_stage_desc* st, const glamr_stage_ext* ext, float* grads_out) {
  if (ext && (b->frozen || b->g_traj_local || !ext->residuals || !ext->losses || !ext->workspace)) return -1;
  if (ext && ext->heading_vec) {
    if (!ext->heading_vec_workspace || (ext->hv_loss_mask >> GLAMR_EXT_HV_NUM_LOSSES) || (ext->hv_monitor_mask >> GLAMR_EXT_HV_NUM_LOSSES) ||
        (ext->hv_loss_mask && !ext->hv_losses)) return -1;
    if ((st->flags & GLAMR_FLAG_ABSOLUTE_HEADING) || ((st->loss_mask >> GLAMR_LOSS_LOCAL_DHEADING_REG_NEW) & 1u)) return -2;
  }
  const glamr_param_layout l = make_layout(b->max_persons, b->max_len);
  std::vector<float> ws(scene_workspace_floats(b->max_persons, b->max_len));
  std::vector<float> tab(2 * (size_t)(st->niters > 0 ? st->niters : 1));
  for (size_t i = 0; 2 * i < tab.size(); ++i) adam_coef_host(st->lr, (int)i + 1, &tab[2 * i]);
  HostRT rt;
  auto sc = std::make_unique<Scene>();
  for (int si = 0; si < b->n_scenes; ++si) {
    assemble_scene(*b, l, st, si, b->n_persons[si], b->seq_len[si], ws.data(), grads_out, *sc);
    sc->adam_tab = st->niters <= ADAM_TAB_MAX ? tab.data() : nullptr;
    if (ext) {
      SceneExt x;
      bind_ext(x, *b, *ext, si, st->niters);
      run_scene<0, false, 0, 0, false, true>(rt, *sc, *st, l, TrajGradOut{nullptr, 0, 0}, &x);
    } else {
      run_scene<0, false, 0>(rt, *sc, *st, l);
    }
  }
  return 0;
}
