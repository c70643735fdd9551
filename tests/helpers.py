"""Shared test helpers: model marshalling, oracle construction, the host SIMT emulator binding and the
debug-record layout of the kernel.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from gym_quadruped_amd.cabi import GQ_CON_STRIDE, GQ_DYN, ALL_OBS, IMU_OBS, OBS_DIMS, OBS_NAMES, GqImuCfg, GqModelDesc, MarshalledModel, obs_ids_from_names  # noqa: E402
from gym_quadruped_amd.mjcf import load_compiled  # noqa: E402
from gym_quadruped_amd.robot_cfgs import get_robot_config  # noqa: E402

# debug record layout (csrc/gq_model_dev.h GQ_DBG_*)
DBG = {}
_o = 0
for _name, _n in [('M', 324), ('qfrc_bias', 18), ('qfrc_smooth', 18), ('qacc_smooth', 18), ('qfrc_constraint', 18),
                  ('xpos', 39), ('xmat', 117), ('nefc', 1), ('ncon', 1), ('niter', 1), ('efc_J', 64 * 18),
                  ('efc_aref', 64), ('efc_R', 64), ('efc_b', 64), ('efc_force', 64), ('efc_type', 64),
                  ('contact_dist', 12), ('contact_geom', 12), ('foot_pos', 12), ('qacc', 18), ('timer', 32), ('xq', 16)]:
    DBG[_name] = (_o, _n)
    _o += _n
DBG_SIZE = _o


def marshalled(robot='mini_cheetah', solver=0, iterations=100, tolerance=1e-8, timestep=0.002,
               terrain_limits=(1e4, -1e4, 1e4, -1e4), noise_floor=0.0, boxes=None, hfield=None, self_collision=None, mesh_graph=True):
    cfg = get_robot_config(robot)
    md = load_compiled(Path(cfg.mjcf_filename).stem)
    qpos0 = md.qpos0.copy()
    if cfg.qpos0_js is not None:
        qpos0[7:] = np.asarray(cfg.qpos0_js, dtype=np.float64)
    return MarshalledModel(md, qpos0=qpos0, feet_geom_names=cfg.feet_geom_names, terrain_limits=terrain_limits,
                           timestep=timestep, solver=solver, iterations=iterations, tolerance=tolerance,
                           noise_floor=noise_floor, boxes=boxes, hfield=hfield, self_collision=self_collision, mesh_graph=mesh_graph)


def random_states(md, n, rng, z_range=(0.18, 0.45), contact_bias=True):
    """Reference-reset-like random states (quadruped_env.py:343-373) without the lift loop: keyframe + joint noise,
    random roll/pitch/yaw, heights spanning flight and ground contact."""
    from scipy.spatial.transform import Rotation
    qpos = np.tile(md.key_qpos[0], (n, 1))
    qpos[:, 7:] += rng.uniform(-0.35, 0.35, (n, 12))
    qpos[:, 0:2] = rng.uniform(-5, 5, (n, 2))
    qpos[:, 2] = rng.uniform(*z_range, n)
    eul = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-np.pi, np.pi, n)], 1)
    qpos[:, 3:7] = Rotation.from_euler('xyz', eul).as_quat(scalar_first=True)
    qvel = rng.normal(0, 1.0, (n, 18))
    qvel[:, 0:3] *= 0.5
    return qpos, qvel


_EMU = None


def emu_lib():
    global _EMU
    if _EMU is None:
        d = ROOT / 'tests' / 'simt_emu'
        subprocess.run(['make', '-s', '-C', str(d)], check=True, capture_output=True)
        _EMU = C.CDLL(str(d / 'libgq_emu.so'))
    return _EMU


_PROBE = None


def probe_lib():
    """tests/device_probe: the product's device routines behind one C entry point each, built with the product's device flags"""
    global _PROBE
    if _PROBE is None:
        d = ROOT / 'tests' / 'device_probe'
        subprocess.run(['make', '-s', '-C', str(d)], check=True, capture_output=True)
        _PROBE = C.CDLL(str(d / 'libgq_probe.so'))
    return _PROBE


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _emu_launch_args(mm, ctrl, ctrl_shape, qpos, qvel, warm=None, applied=None, time=None, friction=None, cmd=None, obs_names=ALL_OBS,
                     legs_order=(0, 1, 2, 3), mask=None, debug_envs=0, auto_reset=None, episode=None, first_pass=0, imu=None,
                     imu_bias=None, step_num=None, pending=None, lift_pending=None, friction_next=None, lift_failed=None, obs=None, rows=False):
    """The host tensors of an emulated step launch and the two runs of arguments both step entries of the emulator take
    (tests/simt_emu/emu_step.cpp): (st, model ... step_num, auto_reset ... lift_pending); st['dyn'] / st['contacts'] go last in both.  ctrl None: zeros of ctrl_shape, or no tensor
    at all where ctrl_shape is None.  obs: the observation rows an earlier launch left (the inline PD policy reads them)."""
    n = qpos.shape[0]
    ids = np.asarray(obs_ids_from_names(obs_names), dtype=np.int32)
    od = int(sum(OBS_DIMS[i] for i in ids))
    f32 = lambda a, shape: np.zeros(shape, np.float32) if a is None else np.ascontiguousarray(a, dtype=np.float32)
    st = dict(
        ctrl=None if ctrl is None and ctrl_shape is None else f32(ctrl, ctrl_shape),
        qpos=np.ascontiguousarray(qpos, dtype=np.float64), qvel=f32(qvel, (n, 18)),
        qacc=np.zeros((n, 18), np.float32), warm=f32(warm, (n, 18)), applied=f32(applied, (n, 18)),
        time=f32(time, (n,)), friction=np.full(n, -1, np.float32) if friction is None else f32(friction, (n,)),
        cmd=f32(cmd, (n, 4)), obs=f32(obs, (n, od)), reward=np.zeros(n, np.float32),
        terminated=np.zeros(n, np.uint8), truncated=np.zeros(n, np.uint8), invalid=np.zeros(n, np.uint8),
        step_num=np.zeros(n, np.int32) if step_num is None else np.ascontiguousarray(step_num, dtype=np.int32), debug=np.zeros((max(debug_envs, 1), DBG_SIZE), np.float32),
        episode=np.zeros(n, np.int32) if episode is None else np.ascontiguousarray(episode, dtype=np.int32),
        lift_failed=np.zeros(n, np.uint8) if lift_failed is None else lift_failed,
        friction_next=np.zeros(n, np.float32) if friction_next is None else np.ascontiguousarray(friction_next, dtype=np.float32),
        lift_pending=np.zeros(n, np.uint8) if lift_pending is None else np.ascontiguousarray(lift_pending, dtype=np.uint8),
        pending=np.zeros(n, np.uint8) if pending is None else np.ascontiguousarray(pending, dtype=np.uint8),
        imu_bias=np.zeros((n, 6), np.float32) if imu_bias is None else np.ascontiguousarray(imu_bias, dtype=np.float32),
        # rows=True: the rows of gq_batch_set_outputs (accessors=True) - the kernel's own dynamics and contact rows, NaN where it wrote nothing;
        # otherwise none, as in a launch of the benchmark
        dyn=np.full((n, GQ_DYN['STRIDE']), np.nan, np.float32) if rows else None, contacts=np.full((n, GQ_CON_STRIDE), np.nan, np.float32) if rows else None)
    st['obs_names'] = list(obs_names)
    # (the arrays the calls only read are kept alive by the dict)
    st['_ids'], st['_legs'], st['_mask'] = ids, np.asarray(legs_order, dtype=np.int32), None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    head = [C.byref(mm.desc), n, _p(ids), len(ids), _p(st['_legs']), _p(st['ctrl']), _p(st['_mask']), _p(st['qpos']), _p(st['qvel']),
            _p(st['qacc']), _p(st['warm']), _p(st['applied']), _p(st['time']), _p(st['friction']), _p(st['cmd']),
            _p(st['obs']), _p(st['reward']), _p(st['terminated']), _p(st['truncated']), _p(st['invalid']), _p(st['step_num'])]
    tail = [None if auto_reset is None else C.byref(auto_reset), _p(st['episode']), _p(st['lift_failed']), _p(st['friction_next']), int(first_pass),
            None if imu is None else C.byref(imu), _p(st['imu_bias']), _p(st['pending']), _p(st['lift_pending'])]
    return st, head, tail


def emu_step(mm, ctrl, qpos, qvel, debug_envs=0, **kw):
    """Run the instrumented step kernel (mode 1) under the emulator. Arrays are updated in place like the device tensors would be."""
    st, head, tail = _emu_launch_args(mm, ctrl, (qpos.shape[0], 12), qpos, qvel, debug_envs=debug_envs, **kw)
    err = C.create_string_buffer(512)
    rc = emu_lib().emu_step(*head, _p(st['debug']), debug_envs, *tail, err, 512, _p(st['dyn']), _p(st['contacts']))
    if rc < 0:
        raise RuntimeError(err.value.decode())
    return st


class PolicyPdDev(C.Structure):   # csrc/gq_step_kernel.h
    _fields_ = [('kp', C.c_float * 12), ('kd', C.c_float * 12), ('qdes', C.c_float * 12), ('col_q', C.c_int32 * 12), ('col_qd', C.c_int32 * 12),
                ('sigma', C.c_float), ('seed_lo', C.c_uint32), ('seed_hi', C.c_uint32), ('step0', C.c_int32), ('env_id_offset', C.c_int32)]


class JointCmdDev(C.Structure):   # csrc/gq_joint_cmd.h
    _fields_ = [('q_des', C.c_void_p), ('qd_des', C.c_void_p), ('tau_ff', C.c_void_p), ('kp', C.c_void_p), ('kd', C.c_void_p),
                ('tau_out', C.c_void_p), ('term_any', C.c_void_p), ('gain_stride', C.c_int32), ('pad_', C.c_int32)]


class FootCmdDev(C.Structure):   # csrc/gq_foot_cmd.h
    _fields_ = [('p_des', C.c_void_p), ('v_des', C.c_void_p), ('f_ff', C.c_void_p), ('tau_ff', C.c_void_p), ('kp', C.c_void_p), ('kd', C.c_void_p),
                ('tau_out', C.c_void_p), ('term_any', C.c_void_p), ('gain_stride', C.c_int32), ('frame', C.c_int32)]


_POLICY_KINDS = (PolicyPdDev, JointCmdDev, FootCmdDev)   # emu_step_window's policy_kind


def emu_window(mm, ctrl_seq, qpos, qvel, n_steps=1, policy=None, obs_seq=False, act_seq=False, **kw):
    """Run the production step kernels (mode 0) under the emulator, as the library launches them: the single-step kernel, or - with
    n_steps > 1 or a policy - the persistent window of n_steps steps per env in one launch.  ctrl_seq [n_steps][N][12] or None (an inline
    policy, or zero control); policy: a PolicyPdDev, JointCmdDev or FootCmdDev whose pointers name arrays the caller keeps alive; obs_seq /
    act_seq: record every step's observation rows / actions into st['obs_seq'] [n_steps][N][obs_dim] / st['act_seq'] [n_steps][N][12].
    Arrays are updated in place like emu_step's."""
    L = emu_lib()
    sizes = (C.c_int * 3)()
    L.emu_policy_sizes(sizes)
    assert list(sizes) == [C.sizeof(t) for t in _POLICY_KINDS], 'the policy blocks of helpers.py do not mirror the library\'s'
    n = qpos.shape[0]
    st, head, tail = _emu_launch_args(mm, ctrl_seq, None if ctrl_seq is None else (n_steps, n, 12), qpos, qvel, **kw)
    st['obs_seq'] = np.zeros((n_steps, n, st['obs'].shape[1]), np.float32) if obs_seq else None
    st['act_seq'] = np.zeros((n_steps, n, 12), np.float32) if act_seq else None
    kind = 0 if policy is None else _POLICY_KINDS.index(type(policy))
    err = C.create_string_buffer(512)
    rc = L.emu_step_window(*head, *tail, n * 12, int(n_steps), _p(st['obs_seq']), _p(st['act_seq']), kind, None if policy is None else C.byref(policy), err, 512,
                           _p(st['dyn']), _p(st['contacts']))
    if rc < 0:
        raise RuntimeError(err.value.decode())
    return st


def emu_camera(mm, qpos, body, pos, quat, fovy, width, height, znear=0.01, zfar=10.0, flags=3):
    """gq_camera (depth and segmentation) under the emulator: csrc/gq_camera.h's pose and pixel passes over mm's model and the qpos rows.
    flags: 1 the robot, 2 the static scene, 4 GQ_CAM_TRACK.  Returns dict(depth [N][H][W], seg, xpos [N][3], xmat [N][9])."""
    from gym_quadruped_amd.cabi import hull_planes
    L = emu_lib()
    q = np.ascontiguousarray(qpos, dtype=np.float64)
    n = q.shape[0]
    P, adr = hull_planes(mm.md)
    P32, adr = np.ascontiguousarray(P, dtype=np.float32), np.ascontiguousarray(adr, dtype=np.int32)
    # the images sit in front of a guard block that is checked after the call: a lane of a partial tile that is not masked stores up to
    # 7 rows and 7 columns past the image.  Past the last env that lands in the guard; past any other env it lands in the next env's image,
    # which the emulator has rendered before (it takes the envs last to first), so the comparison with the reference sees it
    npx, guard = n * height * width, 8 * (width + 8)
    dbuf, sbuf = np.full(npx + guard, -7.0, np.float32), np.full(npx + guard, -7, np.int32)
    out = dict(depth=dbuf[:npx].reshape(n, height, width), seg=sbuf[:npx].reshape(n, height, width), xpos=np.zeros((n, 3)), xmat=np.zeros((n, 9), np.float32))
    p3, q4 = np.ascontiguousarray(pos, dtype=np.float64), np.ascontiguousarray(quat, dtype=np.float64)
    err = C.create_string_buffer(512)
    rc = L.emu_camera(C.byref(mm.desc), n, _p(q), q.shape[1], int(body), _p(p3), _p(q4), C.c_float(fovy), int(width), int(height), C.c_float(znear),
                      C.c_float(zfar), int(flags), _p(P32) if len(P32) else None, _p(adr) if len(P32) else None, _p(out['depth']), _p(out['seg']),
                      _p(out['xpos']), _p(out['xmat']), err, 512)
    if rc < 0:
        raise RuntimeError(err.value.decode())
    assert (dbuf[npx:] == -7.0).all() and (sbuf[npx:] == -7).all(), 'the pixel pass stored past the images'
    assert (out['seg'] != -7).all() and (out['depth'] != -7.0).all(), 'the pixel pass left pixels unwritten'
    return out


def dbg(rec, name):
    o, n = DBG[name]
    return rec[o:o + n]


def split_obs(row, obs_names):
    out, k = {}, 0
    for nme in obs_names:
        d = OBS_DIMS[OBS_NAMES.index(nme)]
        out[nme] = row[k:k + d]
        k += d
    return out


def emu_reset(mm, n, cfg, qpos_new=None, qvel_new=None, mask=None, episode=None):
    """Run the reset kernel body under the emulator; returns dict of host arrays."""
    L = emu_lib()
    st = dict(qpos=np.zeros((n, 19)), qvel=np.zeros((n, 18), np.float32), qacc=np.ones((n, 18), np.float32),
              warm=np.ones((n, 18), np.float32), applied=np.ones((n, 18), np.float32), time=np.ones(n, np.float32),
              cmd=np.zeros((n, 4), np.float32), friction_next=np.zeros(n, np.float32), step_num=np.full(n, 7, np.int32),
              episode=np.zeros(n, np.int32) if episode is None else np.ascontiguousarray(episode, dtype=np.int32),
              lift_failed=np.zeros(n, np.uint8), lift_pending=np.zeros(n, np.uint8))
    err = C.create_string_buffer(512)
    m8 = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    qn = None if qpos_new is None else np.ascontiguousarray(qpos_new, dtype=np.float64)
    vn = None if qvel_new is None else np.ascontiguousarray(qvel_new, dtype=np.float32)
    rc = L.emu_reset(C.byref(mm.desc), n, _p(m8), _p(qn), _p(vn), C.byref(cfg), _p(st['qpos']), _p(st['qvel']), _p(st['qacc']),
                     _p(st['warm']), _p(st['applied']), _p(st['time']), _p(st['cmd']), _p(st['friction_next']),
                     _p(st['step_num']), _p(st['episode']), _p(st['lift_failed']), _p(st['lift_pending']), err, 512)
    if rc < 0:
        raise RuntimeError(err.value.decode())
    return st


def default_reset_cfg(seed=0, random=1, hip_height=0.225, lin=(0.5, 0.5), ang=(0.0, 0.0), fric=(1.0, 1.0), cmd='forward'):
    from gym_quadruped_amd.cabi import GqResetCfg
    return GqResetCfg(seed=seed, random=random, q_pos_amp=20 * np.pi / 180, q_vel_amp=0.5, roll_sweep=10 * np.pi / 180,
                      pitch_sweep=10 * np.pi / 180, hip_height=hip_height, lin_vel_range=(C.c_float * 2)(*lin),
                      ang_vel_range=(C.c_float * 2)(*ang), friction_range=(C.c_float * 2)(*fric),
                      cmd_forward=int('forward' in cmd), cmd_random=int('forward' not in cmd and 'random' in cmd),
                      cmd_rotate=int('rotate' in cmd), cmd_human=int('human' in cmd))


GQ_MAXCON, GQ_MAXEFC = 12, 63   # csrc/gq_model_dev.h


def oracle_fits_row_budget(o, cone):
    """Does the oracle's (uncapped) constraint set fit the kernel's per-wave row budget?  The kernel keeps whole contacts in
    MuJoCo's order while contacts <= 12, rows <= 63 and - elliptic cones - rows + the (dim - 1) virtual Hessian rows reserved
    per cone contact <= 64 (csrc/gq_step_body.h S6, gq_boxes.h); a prefix rule, so everything fits iff the totals do."""
    if o.ncon == 0:
        return True
    dims = o.get('contact_dim').astype(int)
    reserve = int(sum(d - 1 for d in dims if d > 1)) if cone else 0
    return o.ncon <= GQ_MAXCON and o.nefc <= GQ_MAXEFC and o.nefc + reserve <= (64 if cone else GQ_MAXEFC)


def tally_note(msg):
    """Print a measured tally line and keep it: GPU sessions append to gpurun_out/parity_tallies.txt (merged back by gpurun,
    copied to profiles/rNN_parity_tallies.txt), so the numbers the test bounds were set from are on record."""
    print(msg)
    try:
        import os
        if 'GQ_TALLY_FILE' not in os.environ and not os.path.exists('/dev/kfd'):
            return   # GPU-less container: the emulator tests' tallies are printed only
        f = os.environ.get('GQ_TALLY_FILE', str(ROOT / 'gpurun_out' / 'parity_tallies.txt'))
        os.makedirs(os.path.dirname(f), exist_ok=True)
        with open(f, 'a') as fh:
            fh.write(msg + '\n')
    except OSError:
        pass


def oracle_reset_lift(o, q0, v0, hip_height):
    """The reference's lift loop (quadruped_env.py:376-388) on the oracle: mj_step1, then z += 1.1 max|dist| over the contacts
    of the calf bodies until none is left (<= 100 iterations).  Returns (lifted z, iterations)."""
    z, it = float(hip_height), 0
    while True:
        o.set_state(np.r_[q0[:2], z, q0[3:]], v0, np.zeros(18), np.zeros(18), 0.0, -1.0)
        o.forward(np.zeros(12), stage=1)
        bodies = o.get('contact_body').astype(int) if o.ncon else np.zeros(0, int)
        dist = o.get('contact_dist') if o.ncon else np.zeros(0)
        calf = np.array([(b - 2) % 3 == 2 for b in bodies], bool)
        if not calf.any() or it >= 100:
            return z, it
        z += 1.1 * np.abs(dist[calf]).max()
        it += 1


GQ_SELF_ROWS = 64


def oracle_fits_self_budget(o, cone):
    """oracle_fits_row_budget, plus the tighter cap (GQ_SELF_ROWS rows + virtual rows) the kernel applies to robot-robot
    contacts so that the dense Newton Hessian fits above the rows."""
    if not oracle_fits_row_budget(o, cone):
        return False
    if o.ncon == 0 or not (o.get('contact_body1') > 0).any():
        return True
    dims = o.get('contact_dim').astype(int)
    reserve = int(sum(d - 1 for d in dims if d > 1)) if cone else 0
    return o.nefc + reserve <= GQ_SELF_ROWS   # = the general budget since the dense step works out of registers


def within_budget_share(qpos, qvel, o, cone):
    """Per drawn state: does the oracle's constraint set at the position / velocity stage fit the kernel's row budget?  (The kernel keeps a
    prefix of MuJoCo's constraint list for an over-budget env - step_parity.ParityTally.check_budget_prefix - but its solution cannot be
    compared, so a test that draws mostly such states verifies little.)"""
    fits = []
    for e in range(len(qpos)):
        o.set_state(qpos[e], np.asarray(qvel[e], np.float64), np.zeros(18), np.zeros(18), 0.0, 0.8)
        o.forward(np.zeros(12), stage=1)
        fits.append(oracle_fits_self_budget(o, cone))
    return np.asarray(fits, bool)


def budgeted_states(n, draw, o, cone, max_over=0.08):
    """n states from draw(k) -> (qpos, qvel) with at most max_over * n of them over the kernel's row budget (by the oracle's
    own constraint count at the position / velocity stage)."""
    allow = int(max_over * n)
    Q, V, over = [], [], 0
    for _ in range(40):
        q, v = draw(2 * n)
        fits = within_budget_share(q, v, o, cone)
        for e in range(len(q)):
            if len(Q) == n:
                break
            if fits[e] or over < allow:
                Q.append(q[e]); V.append(v[e]); over += 0 if fits[e] else 1
        if len(Q) == n:
            break
    assert len(Q) == n, f'only {len(Q)} of {n} states found'
    return np.stack(Q), np.stack(V)


def self_contact_states(md, n, rng, o, z=(0.5, 0.9), want_cross=None, cone=None, max_over=None):
    """Random poses with wide joint excursions (legs folded across each other), kept when the oracle finds a robot-robot
    contact (want_cross: also require / forbid a contact between two different legs)."""
    out_q, out_v = [], []
    leg = lambda b: (b - 2) // 3 if b >= 2 else -1
    tries = over = 0
    allow = n if max_over is None else int(max_over * n)   # over-budget states kept (see budgeted_states)
    while len(out_q) < n and tries < 60000:
        tries += 1
        q, v = random_states(md, 1, rng, z_range=z)
        q, v = q[0], v[0]
        q[7:] = md.key_qpos[0][7:] + rng.uniform(-1.6, 1.6, 12)
        o.set_state(q, v, np.zeros(18), np.zeros(18), 0.0, -1.0); o.forward(np.zeros(12), stage=1)
        if not o.ncon:
            continue
        b1, b2 = o.get('contact_body1').astype(int), o.get('contact_body').astype(int)
        if not (b1 > 0).any():
            continue
        cross = any(x > 0 and leg(x) >= 0 and leg(x) != leg(y) for x, y in zip(b1, b2))
        if want_cross is not None and cross != want_cross:
            continue
        if max_over is not None and not oracle_fits_self_budget(o, cone):
            if over >= allow:
                continue
            over += 1
        out_q.append(q); out_v.append(v)
    assert len(out_q) == n, f'only {len(out_q)} self-contact states found'
    return np.stack(out_q), np.stack(out_v)


def emu_cam_prim(kind, o, d, par=(), planes=None):
    """csrc/gq_camera.h's robot-geom primitives on n rays (geom frame): kind 'sphere' (par r), 'cylinder' (r, h), 'capsule' (r, h), 'cone'
    (rb, zb, zt), 'hull' (planes [P][4]).  Returns (t [n] as returned, part [n])."""
    L = emu_lib()
    o, d = np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)
    n = len(o)
    t, part = np.zeros(n, np.float32), np.zeros(n, np.int32)
    pr = np.ascontiguousarray(list(par) + [0.0], dtype=np.float32)
    P = None if planes is None else np.ascontiguousarray(planes, dtype=np.float32)
    L.emu_cam_prim(['sphere', 'cylinder', 'capsule', 'cone', 'hull'].index(kind), n, _p(o), _p(d), _p(pr), _p(P), 0 if P is None else len(P), _p(t), _p(part))
    return t, part


def emu_ray_slab(ol, dl, s, tin=-1e30, tout=1e30):
    """ray_slab<float>: returns (hit, tin, tout, axis), axis -1 where no slab raised tin"""
    L = emu_lib()
    ol, dl, s = (np.ascontiguousarray(x, dtype=np.float32) for x in (ol, dl, s))
    n = len(ol)
    ti, to, ax, hit = np.full(n, tin, np.float32), np.full(n, tout, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    L.emu_ray_slab(n, _p(ol), _p(dl), _p(s), _p(ti), _p(to), _p(ax), _p(hit))
    return hit.astype(bool), ti, to, ax


def emu_ray_triangle(o, d, a, b, c, dtype):
    """ray_triangle<float> / <double>: returns (hit, t)"""
    L = emu_lib()
    o, d, a, b, c = (np.ascontiguousarray(x, dtype=dtype) for x in (o, d, a, b, c))
    n = len(o)
    t, hit = np.zeros(n, dtype), np.zeros(n, np.int32)
    (L.emu_ray_triangle_f if dtype == np.float32 else L.emu_ray_triangle_d)(n, _p(o), _p(d), _p(a), _p(b), _p(c), _p(t), _p(hit))
    return hit.astype(bool), t


def emu_ray_hfield(H, sx, sy, ol, d, tmin):
    """ray_hfield<double> over the grid H [nrow][ncol] (float32 elevations) spanning [-sx, sx] x [-sy, sy]: returns (t, tri)"""
    L = emu_lib()
    H = np.ascontiguousarray(H, dtype=np.float32)
    nr, nc = H.shape
    ol, d, tmin = (np.ascontiguousarray(x, dtype=np.float64) for x in (ol, d, tmin))
    n = len(ol)
    t, tri = np.zeros(n), np.zeros(n, np.int32)
    f = C.c_float
    L.emu_ray_hfield(_p(H), nr, nc, f(sx), f(sy), f(2 * sx / (nc - 1)), f(2 * sy / (nr - 1)), f(float(H.max())), n, _p(ol), _p(d), _p(tmin), _p(t), _p(tri))
    return t, tri
