"""The step's epilogue and observation stage (csrc/gq_step_body.h S10 - S11) under the host emulator, on the start states of tests/obs_lane_cases.py
that the GPU digests of tests/test_gpu_obs_lanes.py use: one step per case, held to the fp64 oracle by the one-step parity helper - the
state under the named set of the case, every observable of the layout under OBS (below).  No emulator digest is recorded: libm differs
between hosts.

OBS: the bounds the suite already holds these observables to.  Contact forces, foot velocities and the contact state: the ones of
step_parity.TERRAIN_NEWTON_STEP.  base_lin_acc (this step's qacc) and the two energy terms (products of qacc / qfrc with qvel): below(5e-3),
step_parity.SELF_STEP_GPU's bound on base_lin_acc.  Everything else is kinematics of the new qpos / qvel, held to 2e-4 max(1, max|ref|) as
in test_kernel_emulated.test_step_stagewise_and_obs."""
import ctypes as C

import numpy as np

import obs_lane_cases as oc
import step_parity as sp
from contact_list import Shapes
from helpers import ALL_OBS, IMU_OBS, GqImuCfg, emu_step, marshalled, split_obs
from step_parity import ParityTally, below, emu_record
from oracle.oracle import Oracle

N = 8
_FORCES = sp.TERRAIN_NEWTON_STEP['obs']
OBS = {k: _FORCES.get(k, below(5e-3) if k in ('base_lin_acc', 'base_lin_acc:base', 'kinetic_energy', 'work') else below(2e-4)) for k in ALL_OBS}
STATE = {'qacc': below(2e-4), 'qvel': sp.Tol(5e-4), 'qpos': sp.Tol(2e-6)}


def _models(robot, solver=1):
    """(kernel model, oracle): Newton at 1e-10 against the oracle's at 1e-12, or the same PGS sweeps on both sides"""
    if solver == 0:
        mm = marshalled(robot, solver=0, iterations=50, tolerance=0.0)
        return mm, Oracle(mm)
    return marshalled(robot, solver=1, iterations=100, tolerance=1e-10, noise_floor=0.0), Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-12))


def _hold(mm, o, q, v, ctrl, state_tols, obs_names=ALL_OBS, legs_order=(0, 1, 2, 3), what='', obs_tols=OBS, **kw):
    """One emulated step from (q, v), every env held to the oracle: state_tols + OBS over the layout's observables.  -> (state, records, tally, classes)"""
    OBS = obs_tols
    n = len(q)
    cmd = np.tile(np.asarray(oc.CMD, np.float32), (n, 1))
    fr = np.full(n, 0.8, np.float32)
    st = emu_step(mm, ctrl, q.copy(), v.copy(), cmd=cmd, friction=fr, obs_names=obs_names, legs_order=legs_order, debug_envs=n, rows=True, **kw)
    tols = {**state_tols, 'obs': {k: OBS[k] for k in obs_names if k in OBS}, **sp.FLAGS}
    tally = ParityTally(mm.md.cone == 1, 3e-7, shapes=Shapes(mm))
    recs, classes = [], []
    for e in range(n):
        recs.append(emu_record(st, e, contacts=True))
        classes.append(tally.step_env(e, o, (q[e], v[e], np.zeros(18), np.zeros(18), 0.0, 0.8), ctrl[e], recs[e], tols,
                                      cmd=oc.CMD, legs_order=legs_order, mass=mm.md.total_mass))
    tally.report(f'emulated observation stage, {what}')
    assert not tally.mismatch
    return st, recs, tally, classes


def test_gimbal_pole():
    mm, o = _models('mini_cheetah')
    q, v = oc.gimbal_states(N)
    # the pitch at the pole is asin of a sine within a few fp32 roundings of 1: sy = 2 (xz - wy) of fp32 quaternion entries is off by up to
    # ~4 * 2^-24, and asin(1 - d) = pi/2 - sqrt(2 d), so the angle by up to sqrt(8 * 2^-24) = 6.9e-4 rad (one rounding: 3.5e-4) - held to 1e-3
    pole = {**OBS, 'base_ori_euler_xyz': below(1e-3)}
    st, recs, tally, classes = _hold(mm, o, q, v, np.zeros((N, 12), np.float32), STATE, what='gimbal pole', obs_tols=pole)
    assert all(c == 'ok' for c in classes), classes
    e = np.stack([r['obs']['base_ori_euler_xyz'] for r in recs])
    assert (e[:, 0] == 0.0).all() and np.allclose(e[:, 1], np.where(np.arange(N) % 2 == 0, 1, -1) * np.pi / 2, atol=1e-3), e   # the pole's branch: roll exactly 0


def test_folded_robots_sum_contacts_per_foot():
    for solver in (1, 0):
        mm, o = _models('mini_cheetah', solver)
        q, v = oc.folded_states(N)
        state = sp.SELF_STEP if solver == 1 else sp.pick(sp.TERRAIN_PGS_STEP, 'efc_J', 'efc_aref', 'qacc', 'qvel')
        st, recs, tally, classes = _hold(mm, o, q, v, oc.controls(N, 1, sigma=5.0)[0], state, what=f'folded robots, solver {solver}')
        calves = [4 + 3 * leg for leg in range(4)]
        multi = 0
        for e in range(N):   # (the oracle's list after its step from the same state)
            o.set_state(q[e], v[e], np.zeros(18), np.zeros(18), 0.0, 0.8)
            o.forward(np.zeros(12), stage=1)
            multi += int(classes[e] in sp.COMPARED and max(oc.calf_contacts(o, calves).values()) >= 2)
        assert multi >= N // 2, (solver, classes, multi)   # compared by value AND with a foot body that sums several contacts


def test_elliptic_cone_with_a_long_contact_list():
    mm, o = _models('go2')
    assert mm.md.cone == 1
    q, v, ncon = oc.crouch_states('go2', N)
    assert max(ncon) >= 8
    st, recs, tally, classes = _hold(mm, o, q, v, oc.controls(N, 1)[0], sp.ELLIPTIC_STEP, what='elliptic crouch')
    got = [int(r['ncon'][0]) for r in recs]
    assert max(n for n, c in zip(got, classes) if c in sp.COMPARED) >= 8, (got, classes)


def test_layouts_that_skip_blocks():
    # the default layout (73 scalars) in another leg order: no base block, no energy, no contact forces
    names, legs = ('qpos', 'qvel', 'tau_ctrl_setpoint', 'feet_pos:base', 'feet_vel:base'), (3, 0, 2, 1)
    mm, o = _models('mini_cheetah')
    q, v = oc.floor_states('mini_cheetah', N, z=(0.95, 1.5))
    st, recs, tally, classes = _hold(mm, o, q, v, oc.controls(N, 1)[0], STATE, obs_names=names, legs_order=legs, what='default layout')
    assert st['obs'].shape[1] == 73 and sum(c in sp.COMPARED for c in classes) >= N // 2, classes
    # every observable and the IMU's six on a robot that carries the sensor
    mm, o = _models('aliengo')
    pos, quat = (0.05, -0.02, 0.03), np.array([0.9, 0.1, -0.3, 0.2])
    quat = quat / np.linalg.norm(quat)
    imu = GqImuCfg(site_pos=(C.c_double * 3)(*pos), site_quat=(C.c_double * 4)(*quat), accel_noise=0.01, gyro_noise=0.02, accel_bias_rate=0.03, gyro_bias_rate=0.04, seed=777)
    q, v = oc.floor_states('aliengo', N, z=(0.95, 1.5))
    names = tuple(ALL_OBS) + tuple(IMU_OBS)
    st, recs, tally, classes = _hold(mm, o, q, v, oc.controls(N, 1)[0], STATE, obs_names=names, what='every observable + IMU', imu=imu)
    assert st['obs'].shape[1] == 245 and sum(c in sp.COMPARED for c in classes) >= N // 2, classes
    assert np.isfinite(st['obs']).all() and np.abs(split_obs(st['obs'][0], names)['imu_acc']).max() > 0
