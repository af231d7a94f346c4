// TEST INFRASTRUCTURE: the per-scene optimiser algorithm the way csrc/grecon_wide.hip compiles it (32 persons, namespace grecon_wide, with the
// world-frame residuals of glamr_stage_ext) on the single-threaded host runtime: the CPU twin of glamr_grecon_run_stage_ext.  Same argument
// structs as the C ABI, every pointer a HOST pointer.  Runs the workspace instance <0, false, 0>, the one the wide launcher picks without an
// arena.  Never loaded by the product.
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

extern "C" size_t hostsim_grecon_wide_ext_workspace_floats(int n_scenes, int max_persons, int max_len) {
  return (size_t)n_scenes * max_persons * max_len * EXT_WS;
}

// ext == NULL: the plain stage.  -1: what glamr_grecon_run_stage_ext refuses (frozen slots, g_traj_local).
extern "C" int hostsim_grecon_wide_run_stage_ext(const glamr_scene_batch* b, const glamr_stage_desc* st, const glamr_stage_ext* ext, float* grads_out) {
  if (ext && (b->frozen || b->g_traj_local)) return -1;
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
