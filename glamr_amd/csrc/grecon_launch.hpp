// Launch plan of the optimiser stage kernel (csrc/grecon.hip): which instance a batch runs on, with how many threads, which on-chip arena and
// how much of it -- host-only arithmetic, no HIP header, so the CPU suite enumerates it (tests/test_stage_plan.py) -- and the ONE list of the
// instances that exist, which the device launcher and the host runtime of tests/hostsim both dispatch through.  Table of arena modes: DESIGN.md 3.
#pragma once
#include <algorithm>
#include <cstdlib>
#include "grecon_algo.hpp"

namespace glamr {
namespace GLAMR_GRECON_NS {
constexpr int MAX_THREADS = 512, WAVES_PER_EU = 2;
constexpr bool WIDE_BUILD = MAXP > 8;      // csrc/grecon_wide.hip: the description of 32 persons takes ~25 KB of static LDS
constexpr size_t LDS_MAX = (WIDE_BUILD ? 96 : 153) * 1024;      // the largest on-chip arena a stage launch asks for
constexpr size_t CU_LDS = 160 * 1024;
constexpr int STAGE_RED_FLOATS = 528;      // block_rt.hpp's RT_RED_FLOATS (a HIP header; grecon.hip asserts that the two agree)
// static LDS per workgroup: scene description (8 persons ~4 KB, 32 persons ~25 KB), scan scratch, stage descriptor, layout -- from the types
constexpr size_t STATIC_LDS = sizeof(Scene) + STAGE_RED_FLOATS * sizeof(float) + sizeof(glamr_stage_desc) + sizeof(glamr_param_layout) + 256;
static_assert(STATIC_LDS % sizeof(float) == 0 && CU_LDS % (8 * sizeof(float)) == 0, "every arena budget is a whole number of floats");

// ---- the instances that exist: grecon_stage_kernel<FAST, SINGLE, CAM, TMC>, and with GT grecon_stage_traj_grad_kernel<FAST> ------------------
// FAST: arena mode (0 none, 1 full, 2 lite, 3 full with the Adam state in the workspace, 4 mid); SINGLE: every scene holds one person; CAM: the
// camera_mode() it is specialised for (0 = any); TMC: frames of the constant layout (0 = the batch's); GT: also writes dL/d traj_local_pred
struct StageInstance {
  int fast; bool single; int cam, tmc; bool gt;
  constexpr bool operator==(const StageInstance& o) const { return fast == o.fast && single == o.single && cam == o.cam && tmc == o.tmc && gt == o.gt; }
};
template <int FAST, bool SINGLE, int CAM, int TMC = 0, bool GT = false>
struct Inst { static constexpr StageInstance value{FAST, SINGLE, CAM, TMC, GT}; };
template <class... I> struct InstanceList {};
constexpr int CL = GLAMR_CONST_LAYOUT_FRAMES;
// Per-camera-mode instances: 24.1 vs 26.1 us per iteration (1 person), 61.8 vs 66.2 (2 persons, main stage).  Several persons: modes 1 and 3 are
// the same layout (mode 3 runs FAST = 1), the constant camera (CAM = 3) has instances of its own, and only they have the mid arena.  The full
// and mid arenas of > 8 persons never fit: not instantiated.  (The compiler emits the kernels in the list's order, last entry first.)
using StageInstances = std::conditional_t<WIDE_BUILD,
    InstanceList<Inst<0, false, 0>, Inst<2, false, 0>, Inst<0, false, 0, 0, true>, Inst<2, false, 0, 0, true>>,
    InstanceList<Inst<0, false, 0>,
                 Inst<2, false, 0>, Inst<2, false, 3>, Inst<2, false, 2>, Inst<2, false, 1>, Inst<4, false, 0>, Inst<4, false, 3>, Inst<4, false, 2>, Inst<4, false, 1>,
                 Inst<2, true, 0>, Inst<2, true, 2>, Inst<2, true, 1>, Inst<1, false, 0>, Inst<1, false, 3>, Inst<1, false, 2>, Inst<1, false, 1>,
                 Inst<3, true, 0>, Inst<3, true, 2>, Inst<3, true, 1>, Inst<1, true, 0>, Inst<1, true, 2>, Inst<1, true, 1>,
                 Inst<1, true, 0, CL>, Inst<1, true, 2, CL>, Inst<1, true, 1, CL>, Inst<0, false, 0, 0, true>, Inst<2, false, 0, 0, true>>>;

// Run-time instance -> compile-time instance: calls f(Inst<...>{}) for the entry that equals `want`; false (and no call) if there is none --
// the caller fails, there is no fallback instance
template <class F, class... I>
inline bool with_instance(InstanceList<I...>, const StageInstance& want, F&& f) { return ((I::value == want ? (f(I{}), true) : false) || ...); }
template <class F>
inline bool with_stage_instance(const StageInstance& want, F&& f) { return with_instance(StageInstances{}, want, static_cast<F&&>(f)); }
// the camera mode an instance is specialised for: modes without an instance of their own run on CAM = 0
constexpr int instance_cam(bool single, int cam) { return (cam == 1 || cam == 2 || (cam == 3 && !single)) ? cam : 0; }

// ---- the plan --------------------------------------------------------------------------------------------------------------------------------
struct StageShape {
  int n_scenes, max_persons, max_len, niters, camera_mode;      // camera_mode(stage)
  bool grads_out, loss_history, g_traj_local;                   // whether the launch has them
};
struct LaunchEnv {      // the device's CUs and the development knobs (A-B tests, tools/overlap_probe.py)
  int n_cus;
  bool has_lds_kb; int lds_kb;               // GLAMR_GRECON_LDS_KB_RT
  bool no_const_layout, no_mid_arena;        // GLAMR_GRECON_NO_CONST_LAYOUT, GLAMR_GRECON_NO_MID_ARENA (several persons stay on the lite arena)
};
inline LaunchEnv launch_env(int n_cus) {      // read per launch: tests switch the knobs inside one process
  const char* kb = std::getenv("GLAMR_GRECON_LDS_KB_RT");
  return {n_cus, kb != nullptr, kb ? std::atoi(kb) : 0, std::getenv("GLAMR_GRECON_NO_CONST_LAYOUT") != nullptr, std::getenv("GLAMR_GRECON_NO_MID_ARENA") != nullptr};
}
struct StagePlan {
  StageInstance inst; int threads;
  size_t lds_bytes;          // dynamic LDS of the launch = the arena
  unsigned fast_floats;      // KernelArgs: the arena in floats,
  int use_lds, layout_len;   // its mode (several persons in mode 3 run the FAST = 1 instance) and the frames it is laid out for (0 = max_len)
};
inline StagePlan plan_stage(const StageShape& s, const LaunchEnv& env) {
  const int P = s.max_persons, T = s.max_len;
  const bool single = P == 1;      // SINGLE needs every scene of the batch to hold exactly one person: max_persons == 1 guarantees it
  const int threads = std::min((T + 63) / 64 * 64, MAX_THREADS);
  const bool per_frame = T <= threads;
  auto arena_bytes = [P](int frames, int mode) { return scene_fast_floats(P, frames, mode) * sizeof(float); };
  const size_t full_arena = arena_bytes(T, 3);      // the exchange arrays alone: 53 floats per frame; with parameters and Adam moments, mode 1: 113

  // 1. budget.  Occupancy: a workgroup's waves hold 256 registers each, so a CU (4 SIMDs x 512 registers) takes 8 / waves workgroups -- if their
  // arenas fit its 160 KB together.  When the batch has more scenes than the chip has CUs, the arena is capped at that share (the keypoint
  // table overflows into the workspace): 1024 scenes of 256 frames 40.1 -> 27.5 ms per 500 iterations.  A 300-frame scene has 5 waves: one
  // per CU.  The development knob replaces either, clamped to [16 KB, LDS_MAX].
  size_t budget = LDS_MAX;
  const int wgs_per_cu = 4 * WAVES_PER_EU / (threads / 64);
  const size_t share = CU_LDS / wgs_per_cu - STATIC_LDS;
  if (wgs_per_cu > 1 && s.n_scenes > env.n_cus && full_arena <= share && per_frame) budget = share;
  if (env.has_lds_kb) budget = std::min(std::max((size_t)env.lds_kb * 1024, (size_t)16384), LDS_MAX);

  // 2. constant layout (every array address of the loop a compile-time constant): one person, 257..304 frames, a thread per frame, the full
  // arena of the 304-frame layout fits, and the caller asks for neither the gradient record nor the loss history
  const bool loss_history = s.loss_history && s.niters > 0;
  const int lay_len = layout_frames(P, T);
  const bool const_layout = lay_len == CL && !s.grads_out && !env.no_const_layout && per_frame && !loss_history &&
                            scene_fast_floats(1, lay_len, 1) * sizeof(float) <= budget;
  const int arena_len = const_layout ? lay_len : T;

  // 3. arena mode (1 and 3 are single-pass instances, a thread per frame; 4: BASELINE configs[3]'s 4 x 300 frames take 143 of the 153 KB)
  const size_t full = arena_bytes(arena_len, 1), mid = arena_bytes(T, 4), lite = arena_bytes(T, 2);
  const int lite_or_none = lite <= budget ? 2 : 0;
  int mode;
  if (s.g_traj_local) mode = lite_or_none;      // the general instance (several persons, any camera mode): one pair per compile
  else if (loss_history) mode = 0;              // a diagnostic mode (the reporting evaluation every iteration): the arena instances' loops stay free of it
  else if (WIDE_BUILD) mode = lite_or_none;
  else if (full <= budget && per_frame) mode = 1;
  else if (full_arena <= budget && per_frame) mode = 3;
  else if (mid <= budget && !single && !env.no_mid_arena) mode = 4;
  else mode = lite_or_none;

  // 4. arena size: the mode's arrays first, then as much of the compact keypoint table as fits
  const size_t base = mode == 1 ? full : (mode == 3 ? full_arena : (mode == 4 ? mid : lite));
  const size_t want = base + (size_t)NJ * 6 * P * (s.g_traj_local ? T : arena_len) * sizeof(float);
  const size_t bytes = mode ? std::min(want, budget) : 0;

  // 5. instance
  StageInstance inst{mode, false, 0, 0, s.g_traj_local};
  if (!s.g_traj_local && !WIDE_BUILD && mode != 0)
    inst = {mode == 3 && !single ? 1 : mode, single, instance_cam(single, s.camera_mode), mode == 1 && single && const_layout ? CL : 0, false};
  return {inst, threads, bytes, (unsigned)(bytes / sizeof(float)), mode, (const_layout && !s.g_traj_local) ? lay_len : 0};
}
}  // namespace GLAMR_GRECON_NS
}  // namespace glamr
