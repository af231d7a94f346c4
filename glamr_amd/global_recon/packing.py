"""Packs GLAMR's per-sequence `data` dictionaries (the structure GlobalReconOptimizer.init_data builds,
global_recon/models/global_recon_model.py:217-230) into the flat, padded arrays of `glamr_scene_batch` (include/glamr_hip.h)
and back.  Pure layout code: no reference arithmetic happens here."""
import ctypes
import math

import numpy as np
import torch

from .. import _lib

NJ = 26
LOSS_IDS = {'kp_2d': 0, 'kp_2d_dist': 1, 'rel_transform': 2, 'cam_traj_rot': 3, 'traj_rot_smoothness': 4, 'local_traj_dxy_reg': 5,
            'local_traj_dheading_reg_new': 6, 'local_traj_rot_reg': 7, 'local_traj_z_reg': 8, 'cam_inv_trans_residual_reg': 9,
            'cam_inv_rot_smoothness': 10, 'cam_origin_smoothness': 11, 'cam_up_reg': 12}
VAR_BITS = {'cam': 1, 'local_xy': 2, 'local_heading': 4, 'world_dheading': 8, 'local_dxy': 16, 'local_rot': 32, 'local_z': 64,
            'local_dheading': 128}
FLAG_FIXED_CAM, FLAG_CAM_FROM_PERSON, FLAG_HAS_WORLD_DHEADING = 1, 2, 4
FLAG_KEEP_CAM_PARAMS, FLAG_NO_CAMERA_TERMS = 8, 16          # launch-by-launch stages (glamr_amd/parallel.py PersonShardedSchedule)
FLAG_POSES_ONLY = 32                                       # a forward-only launch that stops after the world poses
FLAG_KEEP_TABLES = 256                                     # launch-by-launch schedules: same stage, same workspace as the previous launch -- the set-up's tables are kept
FLAG_NO_REPORT = 128                                       # launch-by-launch schedules: the launch's last evaluation writes no outputs / loss values
FLAG_ABSOLUTE_HEADING = 64                                 # specs absolute_heading: per-frame headings are absolute (csrc/grecon_wide.hip instances)

# The latent regularisers (loss_func.py:293-310), in the order of glamr_latent_reg's terms, with the flag that makes each one's
# latent an Adam parameter.  They are NOT terms of the fused stage kernel (stage_desc refuses them): latent_schedule.LatentSchedule takes them itself.
LATENT_REG_TERMS = {'motion_latent_reg': 'flag_opt_motion_latent', 'traj_latent_reg': 'flag_opt_traj_latent'}


def split_latent_regs(loss_cfg):
    """loss_cfg -> (loss_cfg without the latent regularisers, [(weight, GLAMR_LATENT_REG_* mode)] for motion_latent_reg, traj_latent_reg)."""
    rest = {n: c for n, c in loss_cfg.items() if n not in LATENT_REG_TERMS}
    regs = []
    for name in LATENT_REG_TERMS:
        c = loss_cfg.get(name)
        mode = _lib.LATENT_REG_ABSENT if c is None else _lib.LATENT_REG_MONITOR if c.get('monitor_only', False) else _lib.LATENT_REG_ACTIVE
        regs.append((0.0 if c is None else float(c['weight']), mode))
    return rest, regs


def check_latent_regs(opt_stage_specs, model_specs):
    """A latent regulariser reads `motion_latent` / `traj_latent` of pose_dict, which exist only when the latent is a parameter
    (global_recon_model.py:155-158): a KeyError in the reference, a ValueError here, before anything runs."""
    for stage, spec in opt_stage_specs.items():
        for name, flag in LATENT_REG_TERMS.items():
            if name in spec['loss_cfg'] and not model_specs.get(flag, False):
                raise ValueError('loss %r in stage %r needs %s in grecon_model_specs: the term regularises a latent that is not a parameter' % (name, stage, flag))


PENETRATION = 'penetration'      # loss_func.py:274-290; not a term of the fused stage kernel either: extra_loss_schedule runs it


def split_penetration(loss_cfg):
    """loss_cfg -> (loss_cfg without the penetration term -- what stage_desc is given --, None or dict(weight, monitor_only))."""
    c = loss_cfg.get(PENETRATION)
    if c is None:
        return loss_cfg, None
    rest = {n: v for n, v in loss_cfg.items() if n != PENETRATION}
    return rest, dict(weight=float(c['weight']), monitor_only=bool(c.get('monitor_only', False)))


def check_penetration(opt_stage_specs, model_specs):
    """The term reads `smpl_verts`, which the reference computes only with flag_use_pen_loss (global_recon_model.py:526-531): a KeyError
    there, a ValueError here, before anything runs."""
    for stage, spec in opt_stage_specs.items():
        if PENETRATION in spec['loss_cfg'] and not model_specs.get('flag_use_pen_loss', False):
            raise ValueError('loss %r in stage %r needs flag_use_pen_loss in grecon_model_specs: without it no vertices are computed' % (PENETRATION, stage))


# The remaining terms of the reference's loss_func_dict that need no variable the optimiser lacks (loss_func.py:60-73, 94-103, 135-144, 175-186,
# 216-217), in the order of glamr_grecon_aux_terms' values (GLAMR_AUX_*).  Not terms of the fused stage kernel either: extra_loss_schedule.AuxTerms
# runs them on a kernel of their own.
AUX_LOSS_IDS = {'cam_rot_smoothness': 0, 'cam_trans_smoothness': 1, 'cam_depth_smoothness': 2, 'traj_trans_smoothness': 3, 'cam_traj_trans': 4,
                'local_traj_dheading_reg': 5}
AUX_ON_CAM_VARIABLES = ('cam_rot_smoothness', 'cam_trans_smoothness')      # read data['cam_rot_6d'] / data['cam_trans']


def split_aux(loss_cfg):
    """loss_cfg -> (loss_cfg without the terms of AUX_LOSS_IDS, None or {name: dict(weight, monitor_only[, first_frame_weight])} in loss_cfg's order)."""
    aux = {}
    for name, c in loss_cfg.items():
        if name not in AUX_LOSS_IDS:
            continue
        if c.get('rot_type', '6d') != '6d' or c.get('first_frame_trans_only', False):
            raise NotImplementedError('loss option not supported: %s %s' % (name, c))
        aux[name] = dict(weight=float(c['weight']), monitor_only=bool(c.get('monitor_only', False)))
        if name == 'cam_traj_trans' and 'first_frame_weight' in c:
            aux[name]['first_frame_weight'] = float(c['first_frame_weight'])
    if not aux:
        return loss_cfg, None
    return {n: v for n, v in loss_cfg.items() if n not in AUX_LOSS_IDS}, aux


def check_aux(opt_stage_specs, model_specs):
    """cam_rot_smoothness / cam_trans_smoothness read data['cam_rot_6d'] / data['cam_trans'], which only a stage that optimises `cam` sets
    (global_recon_model.py:473-480): a KeyError in the reference -- or, silently, the stale tensor an earlier stage left behind.  A ValueError
    here, before anything runs."""
    for stage, spec in opt_stage_specs.items():
        for name in AUX_ON_CAM_VARIABLES:
            if name in spec['loss_cfg'] and 'cam' not in spec['opt_variables']:
                raise ValueError("loss %r in stage %r needs 'cam' in the stage's opt_variables: the term reads the camera variables themselves, which exist only "
                                 "in a stage that optimises them (a KeyError in the reference, or the stale tensor of an earlier stage)" % (name, stage))


def split_off_kernel(opt_stage_specs):
    """opt_stage_specs -> (the specs the stage kernel is given: every stage's loss_cfg without the penetration term and the terms of AUX_LOSS_IDS,
    {stage: split_penetration's second result}, {stage: split_aux's}) -- the stages that list none are left out.  Without such an entry anywhere
    the first result IS the argument; otherwise one new dictionary (the argument is not modified)."""
    rest_specs, pen_cfg, aux_cfg = {}, {}, {}
    for stage, spec in opt_stage_specs.items():
        rest, pen = split_penetration(spec['loss_cfg'])
        rest, aux = split_aux(rest)
        if pen is not None:
            pen_cfg[stage] = pen
        if aux is not None:
            aux_cfg[stage] = aux
        rest_specs[stage] = spec if rest is spec['loss_cfg'] else dict(spec, loss_cfg=rest)
    return (rest_specs if pen_cfg or aux_cfg else opt_stage_specs), pen_cfg, aux_cfg


# World-frame residuals: the variables `world_dxy` / `world_res` (global_recon_model.py:452-454, 467-468, 611-613, 628-631) and their
# regularisers (loss_func.py:189-209), in the order of glamr_stage_ext's bits.  Not part of glamr_stage_desc either (stage_desc refuses all
# four names): split_world takes them off a stage and world_ext makes the glamr_stage_ext that glamr_grecon_run_stage_ext runs beside it.
WORLD_VARS = {'world_dxy': 1, 'world_res': 2}                     # GLAMR_EXT_VAR_*
WORLD_TERMS = {'traj_rot_res': 0, 'traj_trans_res': 1}            # GLAMR_EXT_LOSS_*
EXT_HAS_WORLD_DXY, EXT_APPLY_WORLD_RES = 1, 2
EXT_FLOATS, EXT_WS_FLOATS = 8, 24                                 # per slot and frame: world_dxy 0-1, smpl_orient_world_res 2-4, root_trans_world_res 5-7
WORLD_KEYS = {'world_dxy': slice(0, 2), 'smpl_orient_world_res': slice(2, 5), 'root_trans_world_res': slice(5, 8)}      # pose_dict key -> columns


def split_world(spec):
    """A stage's spec -> (the spec stage_desc is given: without the names of WORLD_VARS and WORLD_TERMS -- the argument itself when it lists
    none --, None or dict(variables=[names of WORLD_VARS in the stage's order], terms={name: dict(weight, monitor_only)} in loss_cfg's order,
    loss_order=[every name of the stage's loss_cfg]))."""
    variables = [v for v in spec['opt_variables'] if v in WORLD_VARS]
    terms = {n: dict(weight=float(c['weight']), monitor_only=bool(c.get('monitor_only', False))) for n, c in spec['loss_cfg'].items() if n in WORLD_TERMS}
    if not variables and not terms:
        return spec, None
    rest = dict(spec, opt_variables=[v for v in spec['opt_variables'] if v not in WORLD_VARS],
                loss_cfg={n: c for n, c in spec['loss_cfg'].items() if n not in WORLD_TERMS})
    world = dict(variables=variables, terms=terms, loss_order=list(spec['loss_cfg']))
    rest['world_residuals'] = world      # (a schedule that is handed the stripped specs and cannot run the residuals sees that they were there: has_world)
    return rest, world


def has_world(opt_stage_specs):
    """Whether a schedule lists a world-frame residual's name, in its stages or taken off them by split_world."""
    return any(spec.get('world_residuals') or split_world(spec)[1] for spec in opt_stage_specs.values())


def split_world_specs(opt_stage_specs):
    """opt_stage_specs -> (the specs without the world-frame residuals' names -- the argument itself when no stage lists one --, {stage:
    split_world's second result} for the stages that do)."""
    rest, world = {}, {}
    for stage, spec in opt_stage_specs.items():
        rest[stage], w = split_world(spec)
        if w is not None:
            world[stage] = w
    return (rest if world else opt_stage_specs), world


# Vector headings: grecon_model_specs heading_type = 'vec' (global_recon_model.py:191-193, 403-405).  The variables
# traj_local_heading (2,) / traj_local_dheading (len - 1, 2) live in PackedScenes.t['heading_vec'] (S * P, T, 2), row 0 and rows e >= 1 of a slot;
# the entries local_heading / local_dheading of the params row are dead.  Both regularisers of the variable run in the extension, in the order of
# GLAMR_EXT_HV_LOSS_*: local_traj_dheading_reg (otherwise one of AUX_LOSS_IDS) and local_traj_dheading_reg_new (otherwise the fused term of LOSS_IDS).
HEADING_VEC_TERMS = {'local_traj_dheading_reg': 0, 'local_traj_dheading_reg_new': 1}
HEADING_VEC_WS_FLOATS = 4
HEADING_VEC_KEYS = ('traj_local_heading', 'traj_local_dheading')


def is_heading_vec(model_specs):
    ht = model_specs.get('heading_type', 'scalar')
    if ht not in ('scalar', 'vec'):
        raise NotImplementedError("heading_type %r in grecon_model_specs is not supported ('scalar' or 'vec')" % (ht,))
    return ht == 'vec'


def split_heading_vec(spec):
    """A stage's spec of a heading_type = 'vec' run -> (the spec without the names of HEADING_VEC_TERMS -- what split_off_kernel, split_world and
    stage_desc are given --, dict(terms={name: dict(weight, monitor_only)} in loss_cfg's order, loss_order=[every name of the stage's loss_cfg]))."""
    terms = {}
    for n, c in spec['loss_cfg'].items():
        if n in HEADING_VEC_TERMS:
            if c.get('rot_type', '6d') != '6d' or c.get('first_frame_trans_only', False):
                raise NotImplementedError('loss option not supported: %s %s' % (n, c))
            terms[n] = dict(weight=float(c['weight']), monitor_only=bool(c.get('monitor_only', False)))
    rest = dict(spec, loss_cfg={n: c for n, c in spec['loss_cfg'].items() if n not in HEADING_VEC_TERMS})
    heading = dict(terms=terms, loss_order=list(spec['loss_cfg']))
    rest['heading_vec'] = heading      # (a schedule that is handed the stripped specs and cannot run vector headings sees that: has_heading_vec)
    return rest, heading


def has_heading_vec(opt_stage_specs):
    """Whether a schedule's specs are those of a heading_type = 'vec' run (split_heading_vec marked them)."""
    return any(spec.get('heading_vec') is not None for spec in opt_stage_specs.values())


def split_heading_vec_specs(opt_stage_specs):
    """opt_stage_specs of a heading_type = 'vec' run -> (the specs without the two regularisers, {stage: split_heading_vec's second result})."""
    rest, heading = {}, {}
    for stage, spec in opt_stage_specs.items():
        rest[stage], heading[stage] = split_heading_vec(spec)
    return rest, heading


def world_ext(world, packed, niters=0, want_grads=False, want_hist=False, heading=None):
    """split_world's second result (or None: a stage that only carries an existing world_dxy along) -> glamr_stage_ext on `packed`'s residual
    arrays (packed.world_arrays makes them), and the tensors it points at beside the residuals: dict(losses, ws[, grads][, loss_history]).
    `heading`: split_heading_vec's second result (or {}: a forward pass) of a heading_type = 'vec' batch -- the descriptor then also carries
    packed.heading_vec_arrays() with hv_ws, hv_losses[, hv_grads][, hv_loss_history]; None: those fields stay zero, the call is what it was."""
    world = world or dict(variables=[], terms={})
    ex = _lib.StageExt()
    ex.var_mask = 0
    for v in world['variables']:
        ex.var_mask |= WORLD_VARS[v]
    ex.flags = (EXT_HAS_WORLD_DXY if packed.has_world_dxy else 0) | (EXT_APPLY_WORLD_RES if 'world_res' in world['variables'] else 0)
    ex.loss_mask = ex.monitor_mask = 0
    for i in range(len(WORLD_TERMS)):
        ex.loss_weight[i] = 0.0
    for name, c in world['terms'].items():
        i = WORLD_TERMS[name]
        ex.loss_mask |= 1 << i
        ex.loss_weight[i] = c['weight']
        if c['monitor_only']:
            ex.monitor_mask |= 1 << i
    res = packed.world_arrays()
    dev, S = res.device, packed.S
    ws_floats = _lib.lib().glamr_grecon_ext_workspace_bytes(S, packed.P, packed.T) // 4      # (the library sizes it: EXT_WS_FLOATS per slot and frame)
    assert ws_floats == res.shape[0] * res.shape[1] * EXT_WS_FLOATS, 'glamr_grecon_ext_workspace_bytes and packing.EXT_WS_FLOATS disagree'
    keep = dict(losses=torch.zeros((S, len(WORLD_TERMS)), dtype=torch.float32, device=dev),
                ws=torch.empty(ws_floats, dtype=torch.float32, device=dev).view(res.shape[:2] + (EXT_WS_FLOATS,)))
    if want_grads:
        keep['grads'] = torch.zeros_like(res)
    if want_hist and niters > 0:
        keep['loss_history'] = torch.zeros((S, int(niters), len(WORLD_TERMS)), dtype=torch.float32, device=dev)
    ex.residuals = ctypes.c_void_p(res.data_ptr())
    for name in ('losses', 'grads', 'loss_history'):
        setattr(ex, name, ctypes.c_void_p(keep[name].data_ptr()) if name in keep else None)
    ex.workspace = ctypes.c_void_p(keep['ws'].data_ptr())
    if heading is not None:
        if not packed.heading_vec:
            raise ValueError("vector headings on a batch that was not packed with heading_type = 'vec'")
        hv = packed.heading_vec_arrays()
        hv_floats = _lib.lib().glamr_grecon_heading_vec_workspace_bytes(S, packed.P, packed.T) // 4
        assert hv_floats == hv.shape[0] * hv.shape[1] * HEADING_VEC_WS_FLOATS, 'glamr_grecon_heading_vec_workspace_bytes and packing.HEADING_VEC_WS_FLOATS disagree'
        keep['hv_ws'] = torch.empty(hv_floats, dtype=torch.float32, device=dev).view(hv.shape[:2] + (HEADING_VEC_WS_FLOATS,))
        keep['hv_losses'] = torch.zeros((S, len(HEADING_VEC_TERMS)), dtype=torch.float32, device=dev)
        if want_grads:
            keep['hv_grads'] = torch.zeros_like(hv)
        if want_hist and niters > 0:
            keep['hv_loss_history'] = torch.zeros((S, int(niters), len(HEADING_VEC_TERMS)), dtype=torch.float32, device=dev)
        ex.hv_loss_mask = ex.hv_monitor_mask = 0
        for name, c in (heading.get('terms') or {}).items():
            i = HEADING_VEC_TERMS[name]
            ex.hv_loss_mask |= 1 << i
            ex.hv_loss_weight[i] = c['weight']
            if c['monitor_only']:
                ex.hv_monitor_mask |= 1 << i
        ex.heading_vec = ctypes.c_void_p(hv.data_ptr())
        ex.heading_vec_workspace = ctypes.c_void_p(keep['hv_ws'].data_ptr())
        ex.heading_vec_grads = ctypes.c_void_p(keep['hv_grads'].data_ptr()) if 'hv_grads' in keep else None
        ex.hv_losses = ctypes.c_void_p(keep['hv_losses'].data_ptr())
        ex.hv_loss_history = ctypes.c_void_p(keep['hv_loss_history'].data_ptr()) if 'hv_loss_history' in keep else None
    return ex, keep


def aux_desc(aux_cfg):
    """split_aux's second result -> glamr_aux_desc."""
    ad = _lib.AuxDesc()
    ad.loss_mask = ad.monitor_mask = 0
    ad.first_frame_weight = 1.0
    for i in range(_lib.AUX_NUM_TERMS):
        ad.weight[i] = 0.0
    for name, c in aux_cfg.items():
        i = AUX_LOSS_IDS[name]
        ad.loss_mask |= 1 << i
        ad.weight[i] = c['weight']
        if c['monitor_only']:
            ad.monitor_mask |= 1 << i
        if 'first_frame_weight' in c:
            ad.first_frame_weight = c['first_frame_weight']
    return ad


def param_layout_py(max_persons, max_len):
    """Mirror of glamr::grecon::param_layout (glamr_amd/csrc/grecon_algo.hpp); checked against the library in the tests."""
    T = max_len
    l = dict(cam_rot6d=0, cam_trans=6 * T, cam_inv_rot_res=9 * T, cam_inv_trans_res=15 * T, person0=18 * T,
             local_xy=0, local_heading=2, local_dxy=4)
    l['local_dheading'] = l['local_dxy'] + 2 * T
    l['local_z'] = l['local_dheading'] + T
    l['local_rot'] = l['local_z'] + T
    l['world_dheading'] = l['local_rot'] + 6 * T
    l['person_stride'] = l['world_dheading'] + T
    l['scene_stride'] = l['person0'] + max_persons * l['person_stride']
    return l


# The variables of a scene's params row under the reference's tensor names (global_recon_model.py:396-426,459-480): name -> (key of param_layout_py,
# shape of one frame's entry, rows).  `rows(n, Ts, empty)` picks the frames the reference tensor holds out of the max_len rows of the variable's
# block -- n: the person's existing frames, Ts: the scene's length, empty: the indices of the frames nobody is seen in --; None: the variable has
# no frame axis.  Everything that reads or writes a variable of a row goes through person_view / scene_view and var_rows.
_EXISTING, _STEPS, _SCENE, _FIRST = (lambda n, Ts, empty: slice(n)), (lambda n, Ts, empty: slice(1, n)), (lambda n, Ts, empty: slice(Ts)), (lambda n, Ts, empty: slice(1))
PERSON_VARS = {'traj_local_xy': ('local_xy', (2,), None), 'traj_local_heading': ('local_heading', (1,), None),
               'traj_local_dxy': ('local_dxy', (2,), _STEPS), 'traj_local_dheading': ('local_dheading', (), _STEPS),
               'traj_local_z': ('local_z', (), _EXISTING), 'traj_local_rot': ('local_rot', (6,), _EXISTING),
               'world_dheading': ('world_dheading', (1,), _SCENE)}
SCENE_VARS = {'cam_rot_6d': ('cam_rot6d', (6,), _SCENE), 'cam_trans': ('cam_trans', (3,), _SCENE),
              'cam_rot_6d_fix': ('cam_rot6d', (6,), _FIRST), 'cam_trans_fix': ('cam_trans', (3,), _FIRST),      # flag_fixed_cam: frame 0's entry is the variable
              'cam_inv_rot_residual': ('cam_inv_rot_res', (6,), lambda n, Ts, empty: empty), 'cam_inv_trans_residual': ('cam_inv_trans_res', (3,), _SCENE)}


def var_rows(name, n=None, Ts=None, empty=None):
    """The index into a variable's view (person_view / scene_view) that cuts the reference tensor `name`."""
    rows = (PERSON_VARS.get(name) or SCENE_VARS[name])[2]
    return slice(None) if rows is None else rows(n, Ts, empty)


def _var_view(block, layout, table, name):
    key, shape, rows = table[name]
    frames = () if rows is None else (layout['cam_trans'] // 6,)      # max_len: cam_rot6d holds 6 numbers per frame
    v = block[..., layout[key]:layout[key] + math.prod(frames + shape)]
    return v.reshape(tuple(v.shape[:-1]) + frames + shape)


def person_cols(layout, pi):
    """The columns of person slot `pi` in a params row."""
    return slice(layout['person0'] + pi * layout['person_stride'], layout['person0'] + (pi + 1) * layout['person_stride'])


def person_view(row, layout, pi, name=None):
    """A VIEW of person slot `pi`'s block of `row` -- a params row (scene_stride,) or any array (..., scene_stride) of them, numpy or torch: only
    the last axis is cut -- or, with `name`, of one variable of PERSON_VARS in it: (..., max_len) + the frame's shape, (...,) + shape without a frame axis."""
    block = row[..., person_cols(layout, pi)]
    return block if name is None else _var_view(block, layout, PERSON_VARS, name)


def scene_view(row, layout, name=None):
    """A VIEW of the camera block of `row` (as person_view), or of one variable of SCENE_VARS in it."""
    return row[..., :layout['person0']] if name is None else _var_view(row, layout, SCENE_VARS, name)


def pack_latents(latents, rows, n_windows, width, device):
    """Caller-given latents ([per sequence] {person id: {'motion': (windows, width), 'traj': (1, width)}}) -> (len(rows), n_windows, width) and
    (len(rows), width) on `device`, for rows [(sequence, person id), or None: an empty slot, zeros]; a person's unused windows stay zero."""
    meps = np.zeros((len(rows), n_windows, width), np.float32)
    teps = np.zeros((len(rows), width), np.float32)
    for k, row in enumerate(rows):
        if row is not None:
            lat = latents[row[0]][row[1]]
            m = np.asarray(lat['motion'], np.float32)
            meps[k, :m.shape[0]] = m
            teps[k] = np.asarray(lat['traj'], np.float32).reshape(-1)
    return torch.from_numpy(meps).to(device), torch.from_numpy(teps).to(device)


def stage_desc(stage_specs, model_specs, has_world_dheading=False, niters=None):
    """opt_stage_specs[stage] (+ grecon_model_specs flags) -> glamr_stage_desc.  Unknown loss names raise: nothing is dropped."""
    sd = _lib.StageDesc()
    sd.var_mask = 0
    for v in stage_specs['opt_variables']:
        if v not in VAR_BITS:
            raise NotImplementedError('optimisation variable %r is not supported by the fused optimiser' % v)
        sd.var_mask |= VAR_BITS[v]
    flags = 0
    if model_specs.get('flag_fixed_cam', False):
        flags |= FLAG_FIXED_CAM
    if model_specs.get('flag_opt_cam_from_person_pose', False):
        flags |= FLAG_CAM_FROM_PERSON
    if has_world_dheading:
        flags |= FLAG_HAS_WORLD_DHEADING
    if model_specs.get('absolute_heading', False):
        flags |= FLAG_ABSOLUTE_HEADING
    sd.flags = flags
    sd.niters = stage_specs['opt_niters'] if niters is None else niters
    sd.lr = stage_specs['opt_lr']
    sd.kp_min_conf = 0.05
    sd.rel_trans_weight = 1.0
    for i in range(16):
        sd.first_frame_weight[i] = 1.0
        sd.loss_weight[i] = 0.0
    sd.first_frame_weight[LOSS_IDS['rel_transform']] = 10.0
    sd.loss_mask = sd.monitor_mask = sd.first_frame_only_mask = 0
    for name, spec in stage_specs['loss_cfg'].items():
        if name not in LOSS_IDS:
            raise NotImplementedError('loss %r is not supported by the fused optimiser' % name)
        i = LOSS_IDS[name]
        sd.loss_mask |= 1 << i
        sd.loss_weight[i] = spec['weight']
        if spec.get('monitor_only', False):
            sd.monitor_mask |= 1 << i
        if spec.get('first_frame_only', False) and name != 'rel_transform':     # rel_transform_loss never reads it
            sd.first_frame_only_mask |= 1 << i
        if 'first_frame_weight' in spec:
            sd.first_frame_weight[i] = spec['first_frame_weight']
        if name in ('kp_2d', 'kp_2d_dist') and 'min_conf' in spec:
            sd.kp_min_conf = spec['min_conf']
        if name == 'rel_transform':
            sd.rel_trans_weight = spec.get('trans_weight', 1.0)
        if spec.get('rot_type', '6d') != '6d' or spec.get('first_frame_trans_only', False):
            raise NotImplementedError('loss option not supported: %s %s' % (name, spec))
    return sd


def carve_zeros(spec, device):
    """{name: zero tensor} for [(name, dtype, shape)] of 4-byte dtypes, all views of ONE zero-filled device allocation (64-float aligned)."""
    offs, total = [], 0
    for _, _, shape in spec:
        offs.append(total)
        total += (math.prod(shape) + 63) // 64 * 64
    slab = torch.zeros(total, dtype=torch.float32, device=device)
    out = {}
    for (name, dtype, shape), o in zip(spec, offs):
        v = slab[o:o + math.prod(shape)]
        out[name] = (v if dtype == torch.float32 else v.view(dtype)).view(shape)
    return out


class PackedScenes:
    """Flat tensors of a batch of scenes on `device` + the ctypes struct that points at them."""

    def _declare(self, device, S, P, T, seq_names=None):
        """The geometry, and what a batch carries beside its arrays -- set by whoever has it, None / [] until then: person_arrays (the per-person
        arrays of a device initialisation), exists, keepalive ((ResidentInputs, workspace, priors' outputs)), latents ((motion, trajectory) draws),
        stage_ws (the workspaces of the last schedule's stage launches, [] after a launch-by-launch one), last_ws (the last launch's workspace)."""
        self.device, self.S, self.P, self.T = device, S, P, T
        self.layout = param_layout_py(P, T)
        self.seq_names = list(seq_names) if seq_names else ['seq%d' % si for si in range(S)]      # (the per-iteration log names its sequence)
        self.person_arrays = self.exists = self.keepalive = self.latents = self.last_ws = None
        self.root_trans_cam = None      # (S * P, T, 3) the persons' pd['root_trans_cam'] of a batch packed from host dictionaries (cam_traj_trans reads it)
        self.stage_ws = []
        self.aux_values = None          # {stage: (S, iterations, 6)} on the device: aux_step_schedule.AuxStepSchedule's values of the last schedule (collect() publishes them)
        # world-frame residuals (split_world / world_ext): t['world_res'] (S * P, T, 8) exists once a stage needs it (world_arrays); `world_dxy` exists
        # from the first stage that lists it on, like has_world_dheading; the residual tensors are reported once a stage listed world_res or a term
        self.has_world_dxy = self.world_res_listed = False
        self.world_losses = None        # (S, 2) on the device: traj_rot_res, traj_trans_res of the last stage that ran with the extension
        # heading_type = 'vec': the batch's heading variables are t['heading_vec'] (heading_vec_arrays) and every launch carries the extension
        self.heading_vec = False
        self.heading_vec_losses = None  # (S, 2) on the device: local_traj_dheading_reg, local_traj_dheading_reg_new of the last stage

    def heading_vec_arrays(self):
        """t['heading_vec']: (S * P, T, 2) by EXISTING row -- row 0 traj_local_heading, row e >= 1 traj_local_dheading[e - 1]; zeros when first asked for."""
        if 'heading_vec' not in self.t:
            self.t['heading_vec'] = torch.zeros((self.S * self.P, self.T, 2), dtype=torch.float32, device=self.device)
        return self.t['heading_vec']

    def world_arrays(self):
        """t['world_res']: (S * P, T, 8) world_dxy | smpl_orient_world_res | root_trans_world_res by video frame, zeros when first asked for."""
        if 'world_res' not in self.t:
            self.t['world_res'] = torch.zeros((self.S * self.P, self.T, EXT_FLOATS), dtype=torch.float32, device=self.device)
        return self.t['world_res']

    @classmethod
    def empty(cls, n_scenes, max_persons, max_len, device, with_rel=None, seq_names=None):
        """All arrays allocated (zero) directly on `device`; the init kernels fill them (glamr_init_prepare / glamr_init_scenes)."""
        self = cls.__new__(cls)
        S, P, T = n_scenes, max_persons, max_len
        self._declare(device, S, P, T, seq_names)
        # ONE zero allocation carved into the arrays (22 allocations + 22 fill launches otherwise: host time on every batch, and on hosts
        # with slow driver calls the launches of a step are paced by it)
        spec = [('n_persons', torch.int32, (S,)), ('seq_len', torch.int32, (S,)), ('fr_start', torch.int32, (S * P,)), ('fr_end', torch.int32, (S * P,)),
                ('vis', torch.float32, (S * P, T)), ('kp_2d', torch.float32, (S * P, T, NJ, 2)), ('kp_score', torch.float32, (S * P, T, NJ)),
                ('cam_K', torch.float32, (S * P, T, 9)), ('traj_local_pred', torch.float32, (S * P, T, 11)), ('orient_cam', torch.float32, (S * P, T, 3)),
                ('base_orient', torch.float32, (S * P, T, 3)), ('base_trans', torch.float32, (S * P, T, 3)), ('person2cam', torch.float32, (S * P, T, 12)),
                ('cam_pose', torch.float32, (S, T, 12)), ('params', torch.float32, (S, self.layout['scene_stride'])), ('losses', torch.float32, (S, _lib.NUM_LOSSES)),
                ('orient_world', torch.float32, (S * P, T, 3)), ('trans_world', torch.float32, (S * P, T, 3)), ('kp_2d_pred', torch.float32, (S * P, T, NJ, 2)),
                ('orient_cam_in_world', torch.float32, (S * P, T, 3))]
        if P > 1 if with_rel is None else with_rel:
            spec.append(('rel_transform_cam', torch.float32, (S, P, P, T, 12)))
        self.t = carve_zeros(spec, device)
        self.t['j_local'] = None
        self.person_ids = None
        self.has_world_dheading = False
        return self

    def __init__(self, datas, j_locals, device, cam_fix_frames=((0, None),), heading_vec=False):
        """datas: list of `data` dicts (one per sequence); j_locals: list (per scene) of dict idx -> (T,26,3) joints computed
        with zero root orientation and zero root translation.  heading_vec: grecon_model_specs heading_type = 'vec' -- traj_local_heading is (2,)
        and traj_local_dheading (len - 1, 2); shapes that disagree with it raise ValueError."""
        S = len(datas)
        self.person_ids = [list(d['person_data'].keys()) for d in datas]
        P = max(len(ids) for ids in self.person_ids)
        T = max(int(d['seq_len']) for d in datas)
        if P > 32:
            raise NotImplementedError('at most 32 persons per scene (csrc/grecon_wide.hip)')
        self._declare(device, S, P, T, [str(d.get('seq_name', 'seq%d' % si)) for si, d in enumerate(datas)])
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)
        t = dict(n_persons=i32(S), seq_len=i32(S), fr_start=i32(S * P), fr_end=i32(S * P), vis=f32(S * P, T), j_local=f32(S * P, T, NJ, 3),
                 kp_2d=f32(S * P, T, NJ, 2), kp_score=f32(S * P, T, NJ), cam_K=f32(S * P, T, 9), traj_local_pred=f32(S * P, T, 11),
                 orient_cam=f32(S * P, T, 3), base_orient=f32(S * P, T, 3), base_trans=f32(S * P, T, 3), person2cam=f32(S * P, T, 12),
                 cam_pose=f32(S, T, 12), params=f32(S, self.layout['scene_stride']), losses=f32(S, _lib.NUM_LOSSES),
                 orient_world=f32(S * P, T, 3), trans_world=f32(S * P, T, 3), kp_2d_pred=f32(S * P, T, NJ, 2),
                 orient_cam_in_world=f32(S * P, T, 3))
        t['fr_end'] += 1
        need_mask = any(not (s == 0 and e is None) for (s, e) in cam_fix_frames)
        if need_mask:
            t['dheading_mask'] = f32(S * P, T)
        if P > 1:
            t['rel_transform_cam'] = f32(S, P, P, T, 12)
        cpu = lambda x: torch.as_tensor(x).detach().to('cpu')
        l = self.layout
        rtc = f32(S * P, T, 3) if all('root_trans_cam' in pd for d in datas for pd in d['person_data'].values()) else None
        # a continued optimisation resumes from the world-frame residuals an earlier run returned (world_dxy exists from then on)
        world = f32(S * P, T, EXT_FLOATS) if any(k in pd for d in datas for pd in d['person_data'].values() for k in WORLD_KEYS) else None
        hvec = f32(S * P, T, 2) if heading_vec else None
        for si, d in enumerate(datas):
            ids = self.person_ids[si]
            Ts = int(d['seq_len'])
            t['n_persons'][si], t['seq_len'][si] = len(ids), Ts
            t['cam_pose'][si, :Ts] = cpu(d['cam_pose'])[:, :3, :].reshape(Ts, 12).float()
            prm = t['params'][si]
            npers = cpu(d['fr_num_persons'])
            empty = torch.where(npers == 0)[0]
            if len(empty) and 'cam_inv_rot_residual' in d:
                scene_view(prm, l, 'cam_inv_rot_residual')[empty] = cpu(d['cam_inv_rot_residual']).float()
            res = cpu(d['cam_inv_trans_residual']).float()
            if res.shape[0] == Ts:
                scene_view(prm, l, 'cam_inv_trans_residual')[var_rows('cam_inv_trans_residual', Ts=Ts)] = res
            elif len(empty):
                raise NotImplementedError('flag_cam_inv_trans_res_all=False is not supported')
            for pi, idx in enumerate(ids):
                pd = d['person_data'][idx]
                slot = si * P + pi
                fs, fe = int(pd['fr_start']), int(pd['fr_end'])
                n = fe - fs
                t['fr_start'][slot], t['fr_end'][slot] = fs, fe
                t['vis'][slot, :Ts] = cpu(pd['vis_frames']).float()
                t['kp_2d'][slot, :Ts] = cpu(pd['kp_2d_aligned']).float()
                t['kp_score'][slot, :Ts] = cpu(pd['kp_2d_score']).float()
                t['cam_K'][slot, :Ts] = cpu(pd['cam_K']).reshape(Ts, 9).float()
                t['traj_local_pred'][slot, :n] = cpu(pd['traj_local_pred']).float()
                t['orient_cam'][slot, :Ts] = cpu(pd['smpl_orient_cam']).float()
                t['base_orient'][slot, :Ts] = cpu(pd['smpl_orient_world_base']).float()
                t['base_trans'][slot, :Ts] = cpu(pd['root_trans_world_base']).float()
                t['person2cam'][slot, :Ts] = cpu(pd['person2cam'])[:, :3, :].reshape(Ts, 12).float()
                if rtc is not None:
                    rtc[slot, :Ts] = cpu(pd['root_trans_cam']).float()
                for key, cols in WORLD_KEYS.items():
                    if key in pd:
                        world[slot, :Ts, cols] = cpu(pd[key]).float()
                if need_mask:
                    m = torch.ones(n - 1)
                    for (s, e) in cam_fix_frames:
                        m[s:e] = 0.0
                    t['dheading_mask'][slot, 1:n] = m
                h0, dh = cpu(pd['traj_local_heading']), cpu(pd['traj_local_dheading'])
                want = ((2,), (n - 1, 2)) if heading_vec else ((1,), (n - 1,))
                is_vec = tuple(h0.shape) == (2,) and tuple(dh.shape) == (n - 1, 2)
                if is_vec != bool(heading_vec):
                    raise ValueError("traj_local_heading %s / traj_local_dheading %s of person %r do not fit heading_type = %r (%s / %s): a result of one "
                                     "heading_type cannot be continued under the other"
                                     % (tuple(h0.shape), tuple(dh.shape), idx, 'vec' if heading_vec else 'scalar', want[0], want[1]))
                if heading_vec:
                    hvec[slot, 0], hvec[slot, 1:n] = h0.float(), dh.float()
                for name in PERSON_VARS:
                    if heading_vec and name in HEADING_VEC_KEYS:
                        continue      # (the scalar entries of the params row are dead)
                    if name != 'world_dheading' or name in pd:
                        person_view(prm, l, pi, name)[var_rows(name, n, Ts)] = cpu(pd[name])
            if P > 1 and d.get('rel_transform_cam'):
                for (i, j), M in d['rel_transform_cam'].items():
                    t['rel_transform_cam'][si, i, j, :Ts] = cpu(M)[:, :3, :].reshape(Ts, 12).float()
        if rtc is not None:
            self.root_trans_cam = rtc.to(device)
        jl_host = t.pop('j_local')
        self.t = {k: v.contiguous().to(device) for k, v in t.items()}
        first_jl = j_locals[0][self.person_ids[0][0]]
        on_device = torch.is_tensor(first_jl) and first_jl.device == torch.device(device) and first_jl.device.type != 'cpu'
        jl = torch.zeros(jl_host.shape, dtype=torch.float32, device=device) if on_device else jl_host      # (on the device: device-to-device copies only)
        for si, d in enumerate(datas):
            for pi, idx in enumerate(self.person_ids[si]):
                jl[si * P + pi, :int(d['seq_len'])] = j_locals[si][idx] if on_device else cpu(j_locals[si][idx]).float()
        self.t['j_local'] = jl if on_device else jl.contiguous().to(device)
        self.has_world_dheading = any('world_dheading' in pd for d in datas for pd in d['person_data'].values())
        if hvec is not None:
            self.heading_vec = True
            self.t['heading_vec'] = hvec.to(device)
        if world is not None:
            self.t['world_res'] = world.to(device)
            self.has_world_dxy = any('world_dxy' in pd for d in datas for pd in d['person_data'].values())
            self.world_res_listed = any('smpl_orient_world_res' in pd for d in datas for pd in d['person_data'].values())

    def struct(self):
        sb = _lib.SceneBatch()
        sb.n_scenes, sb.max_persons, sb.max_len, sb.n_joints = self.S, self.P, self.T, NJ
        for name, _ in _lib.SceneBatch._fields_[4:]:
            ten = self.t.get(name)
            setattr(sb, name, ctypes.c_void_p(ten.data_ptr()) if ten is not None else None)
        return sb

    def person_params(self, si, pi):
        return person_view(self.t['params'][si], self.layout, pi)

    def set_cam_pose(self, cam_poses):
        """cam_poses: list (per scene) of (T,4,4) world->camera arrays."""
        host = torch.zeros((self.S, self.T, 12), dtype=torch.float32)
        for si, c in enumerate(cam_poses):
            c = torch.as_tensor(c).float()
            host[si, :c.shape[0]] = c[:, :3, :].reshape(-1, 12)
        self.t['cam_pose'] = host.to(self.device)

    def fetch(self, names=('params', 'cam_pose', 'orient_world', 'trans_world', 'kp_2d_pred', 'orient_cam_in_world', 'losses')):
        """One device->host copy per tensor."""
        return {k: self.t[k].detach().cpu().numpy() for k in names}

    def unpack_into(self, datas, stage_specs, model_specs, as_torch=True):
        """Writes optimised variables and the outputs of the last forward pass back into the `data` dictionaries, with the
        tensor names the reference uses (global_recon_model.py:396-426,459-480,512-528,598-606)."""
        l, P = self.layout, self.P
        h = self.fetch()
        world = self.t['world_res'].detach().cpu().numpy() if 'world_res' in self.t else None
        world_keys = [k for k in WORLD_KEYS if world is not None and (self.has_world_dxy if k == 'world_dxy' else self.world_res_listed)]
        hvec = self.heading_vec_arrays().detach().cpu().numpy() if self.heading_vec else None
        conv = (lambda a: torch.from_numpy(np.ascontiguousarray(a))) if as_torch else (lambda a: np.ascontiguousarray(a))
        var = set(stage_specs['opt_variables']) if stage_specs is not None else set()
        for si, d in enumerate(datas):
            Ts = int(d['seq_len'])
            cam = np.zeros((Ts, 4, 4), np.float32)
            cam[:, :3, :] = h['cam_pose'][si, :Ts].reshape(Ts, 3, 4)
            cam[:, 3, 3] = 1.0
            inv = np.zeros_like(cam)
            inv[:, :3, :3] = cam[:, :3, :3].transpose(0, 2, 1)
            inv[:, :3, 3] = -np.einsum('tji,tj->ti', cam[:, :3, :3], cam[:, :3, 3])
            inv[:, 3, 3] = 1.0
            d['cam_pose'], d['cam_pose_inv'] = conv(cam), conv(inv)
            prm = h['params'][si]
            # the residual tensors live in `data` from init_data on (:171-177) whatever the stages optimise: always written back, so a
            # later optimize(continue_opt=True) restarts from them (the device path's _materialise does the same)
            empty = np.where(np.asarray(d['fr_num_persons']) == 0)[0]
            cam_vars = () if 'cam' not in var else ('cam_rot_6d_fix', 'cam_trans_fix') if model_specs.get('flag_fixed_cam', False) else ('cam_rot_6d', 'cam_trans')
            for name in cam_vars + ('cam_inv_rot_residual', 'cam_inv_trans_residual'):
                d[name] = conv(scene_view(prm, l, name)[var_rows(name, Ts=Ts, empty=empty)])
            for pi, idx in enumerate(self.person_ids[si]):
                pd = d['person_data'][idx]
                slot = si * P + pi
                n = int(pd['fr_end']) - int(pd['fr_start'])
                for name in PERSON_VARS:
                    if name != 'world_dheading' or name in var or name in pd:
                        pd[name] = conv(person_view(prm, l, pi, name)[var_rows(name, n, Ts)])
                if hvec is not None:      # heading_type = 'vec': (2,) and (len - 1, 2), from the array of their own
                    pd['traj_local_heading'], pd['traj_local_dheading'] = conv(hvec[slot, 0]), conv(hvec[slot, 1:n])
                for key in world_keys:
                    pd[key] = conv(world[slot, :Ts, WORLD_KEYS[key]])
                pd['smpl_orient_world'] = conv(h['orient_world'][slot, :Ts])
                pd['root_trans_world'] = conv(h['trans_world'][slot, :Ts])
                pd['kp_2d_pred'] = conv(h['kp_2d_pred'][slot, :Ts])
                pd['smpl_orient_cam_in_world'] = conv(h['orient_cam_in_world'][slot, :Ts])
