"""The end-to-end cases of the six loss_cfg terms of packing.AUX_LOSS_IDS: scenes, schedules and weights shared by the fixture
generator (tools/aux_terms_golden.py: the UNMODIFIED reference with the names added to a shipped schedule) and tests/test_aux_terms_gpu.py.

Every case has a TWIN: the same scene, schedule and K with the six names deleted -- what the parent's path computes -- whose distance from its own
fixture is the yardstick of the K-step comparison.  Weights are chosen so that every term's first weighted gradient is at least 1 % of the norm
of its stage's whole gradient in the reference, except where that gradient is zero by construction (ZERO_AT_START); the generator asserts both
and prints the shares."""
import copy

import numpy as np

from glamr_amd.global_recon.configs import get_config
from glamr_amd.utils import synth

ON_CAMERA_VARIABLES = ('cam_rot_smoothness', 'cam_trans_smoothness')
EVERYWHERE = ('cam_depth_smoothness', 'traj_trans_smoothness', 'cam_traj_trans', 'local_traj_dheading_reg')
# case: config, frames, persons, seed, detection gap of person 0, (person, first, last) of synth.trim_person or None, iterations per stage,
# {stage: {name: loss_cfg entry}}
CASES = {
    'glamr_dynamic': dict(cfg_id='glamr_dynamic', T=40, P=1, seed=31, gap=(10, 18), trim=None, K=4, terms={
        'init_opt': {'cam_rot_smoothness': dict(weight=2.0e8), 'cam_trans_smoothness': dict(weight=5.0e7), 'cam_depth_smoothness': dict(weight=3.0e6),
                     'traj_trans_smoothness': dict(weight=1.0e2), 'cam_traj_trans': dict(weight=1.0e4, first_frame_weight=10.0),
                     'local_traj_dheading_reg': dict(weight=1.0e3)}}),
    'glamr_static_multi': dict(cfg_id='glamr_static_multi', T=36, P=2, seed=32, gap=(0, 0), trim=(1, 6, 30), K=3, terms={
        'init_opt': {'cam_depth_smoothness': dict(weight=1.0e3), 'traj_trans_smoothness': dict(weight=5.0e2), 'cam_traj_trans': dict(weight=1.0e4),
                     'local_traj_dheading_reg': dict(weight=1.0e3)},
        'main_opt': {'cam_rot_smoothness': dict(weight=2.0e3), 'cam_trans_smoothness': dict(weight=1.0e3), 'cam_depth_smoothness': dict(weight=1.0e3),
                     'traj_trans_smoothness': dict(weight=2.0e2), 'cam_traj_trans': dict(weight=1.0e4), 'local_traj_dheading_reg': dict(weight=1.0e3)}}),
    'glamr_3dpw': dict(cfg_id='glamr_3dpw', T=40, P=1, seed=33, gap=(12, 19), trim=None, K=4, terms={
        'init_opt': {'cam_depth_smoothness': dict(weight=1.0e1), 'traj_trans_smoothness': dict(weight=1.0e2), 'cam_traj_trans': dict(weight=1.0e4),
                     'local_traj_dheading_reg': dict(weight=1.0e3)},
        'main_opt': {'cam_depth_smoothness': dict(weight=1.0e1), 'traj_trans_smoothness': dict(weight=5.0e2), 'cam_traj_trans': dict(weight=3.0e5),
                     'local_traj_dheading_reg': dict(weight=1.0e5)}}),
}
# Terms whose FIRST gradient is zero (to rounding) by construction, so that no weight gives them a share of the stage's first gradient:
#   traj_trans_smoothness in a stage that moves the trajectory rigidly only (local_xy, local_heading: a shift and a turn about the first frame
#     leave every frame-to-frame step's length alone);
#   cam_traj_trans where the start satisfies it: init_data builds the world trajectory from root_trans_cam through the initial camera
#     (glamr_dynamic), or the camera is derived from the persons' own transforms (glamr_3dpw, first stage);
#   everything on a fixed camera's single row (cam_rot_smoothness, cam_trans_smoothness, cam_depth_smoothness of glamr_static_multi);
#   local_traj_dheading_reg: the increments start at zero, and with the default cam_fix_frames every increment is masked, so no stage moves them.
# The generator holds these to < 1e-4 of the stage's gradient and every other term to >= 1 %.
ZERO_AT_START = {
    'glamr_dynamic': {'init_opt': ('traj_trans_smoothness', 'cam_traj_trans', 'local_traj_dheading_reg')},
    'glamr_static_multi': {'init_opt': ('cam_depth_smoothness', 'local_traj_dheading_reg'),
                           'main_opt': ('cam_rot_smoothness', 'cam_trans_smoothness', 'cam_depth_smoothness', 'local_traj_dheading_reg')},
    'glamr_3dpw': {'init_opt': ('traj_trans_smoothness', 'cam_traj_trans', 'local_traj_dheading_reg'), 'main_opt': ('local_traj_dheading_reg',)},
}
# ... and of those, the terms whose VALUE is 0 over the whole run (the others' recorded value after the run is > 0)
STRUCTURALLY_ZERO = {'glamr_dynamic': ('local_traj_dheading_reg',),
                     'glamr_static_multi': ('cam_rot_smoothness', 'cam_trans_smoothness', 'cam_depth_smoothness', 'local_traj_dheading_reg'),
                     'glamr_3dpw': ('local_traj_dheading_reg',)}


def fixture_name(case, twin=False):
    return 'grecon_aux_%s%s' % (case, '_twin' if twin else '')


def in_dict_of(case):
    c = CASES[case]
    d = synth.make_in_dict(seed=c['seed'], num_frames=c['T'], num_persons=c['P'], smpl_model=synth.make_smpl_model(), gap=c['gap'])
    if c['trim']:
        synth.trim_person(d, *c['trim'])
    return d


def stage_specs_with_terms(opt_stage_specs, case, twin=False):
    """A copy of a schedule ({stage: spec}, the reference's or this package's) with the case's entries added to every stage's loss_cfg."""
    specs = copy.deepcopy(opt_stage_specs)
    if not twin:
        for stage, terms in CASES[case]['terms'].items():
            specs[stage]['loss_cfg'].update(copy.deepcopy(terms))
    return specs


def config_of(case, twin=False, edit=None):
    """This package's configuration of the case; edit(name, entry) may change an entry in place (monitor_only)."""
    cfg = get_config(CASES[case]['cfg_id'])
    cfg['opt_stage_specs'] = stage_specs_with_terms(cfg['opt_stage_specs'], case, twin)
    if edit is not None:
        for spec in cfg['opt_stage_specs'].values():
            for name, entry in spec['loss_cfg'].items():
                edit(name, entry)
    return cfg
