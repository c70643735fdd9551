"""GPU parity: the HIP path (through the C-ABI / QuadrupedEnv) against the CPU fp64 oracle on identical
qpos / qvel / ctrl.  Tolerances are fp32-vs-fp64 with the same PGS iteration count:
  stage internals (M, bias, J, aref, R) rel 1e-4; constraint forces 2e-3 of the largest force;
  qacc 1e-3 * max|qacc| ; one-step qvel 1e-4 + 1e-5*|.| ; qpos 1e-6 ; observations 2e-3 * max(1, |obs|).
"""
import os

import numpy as np
import pytest
import torch

from helpers import ROOT, budgeted_states, oracle_fits_row_budget, ALL_OBS, marshalled, random_states, self_contact_states, split_obs, tally_note
import newton_first_step as nfs
import step_parity as sp
from contact_list import Shapes
from step_parity import ParityTally, gpu_records

pytestmark = pytest.mark.gpu

N = 256


def _make_env(n, obs=ALL_OBS, iters=50, tol=0.0, solver='pgs', robot='mini_cheetah', **kw):
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    return QuadrupedEnv(robot, state_obs_names=tuple(obs), num_envs=n, device='cuda:0',
                        solver=solver, solver_iterations=iters, solver_tolerance=tol, seed=0, **kw)


def _oracle(env):
    from oracle.oracle import Oracle
    return Oracle(env._mm)


def _one_more_step_against_oracle(env, o, g, what, count):
    """One more step from a rollout's state, checked against the oracle: every env that does not spend the step on its reset is held to
    ROLLOUT_STATE_STEP - an env over the row budget to the prefix rule: its rows are the oracle's first rows, the flags the oracle's, and the
    caller is told what was cut.  Returns the sum of count() over the compared envs that have contacts."""
    n = env.num_envs
    q0, v0, w0, fr = env.qpos.cpu().numpy().copy(), env.qvel.cpu().numpy().copy(), env._warm.cpu().numpy().copy(), env._friction.cpu().numpy().copy()
    pend = env._terminated_b.cpu().numpy().copy()
    act = torch.randn(n, 12, generator=g, device='cuda:0') * 15
    env.enable_debug(n)
    env.step(act)
    kern = gpu_records(env, n, ['qacc', 'nefc', 'ncon', 'efc_J', 'efc_R', 'efc_aref'])
    a = act.cpu().numpy()
    total = 0
    tally = ParityTally(env.mjModel.cone == 1, 3e-6)
    for e in np.where(~pend)[0].tolist():
        if tally.step_env(e, o, (q0[e], v0[e], w0[e], np.zeros(18), 0.0, float(fr[e])), a[e], kern[e], sp.ROLLOUT_STATE_STEP, prefix=True) == 'ok' and o.ncon:
            total += count()
    tally.finish(what, min_checked=0.7, max_tie=0.15, max_budget=0.1)
    return total


def test_loaded_native_lib():
    from gym_quadruped_amd import _lib
    assert _lib.LIB_PATH.exists()
    _lib.lib()


def test_step_matches_oracle_stagewise():
    env = _make_env(N)
    rng = np.random.default_rng(0)
    qpos, qvel = random_states(env.mjModel, N, rng)
    warm = rng.normal(0, 5, (N, 18)).astype(np.float32)
    ctrl = (rng.normal(0, 1, (N, 12)) * 30).astype(np.float32)
    cmd = np.tile(np.array([0.5, 0.1, 0.0, 0.3], np.float32), (N, 1))
    env.reset(qpos=qpos, qvel=qvel.astype(np.float32))   # explicit-state reset performs one step; overwrite after
    env._qpos.copy_(torch.as_tensor(qpos)); env._qvel.copy_(torch.as_tensor(qvel.astype(np.float32)))
    env._warm.copy_(torch.as_tensor(warm)); env._cmd.copy_(torch.as_tensor(cmd)); env._time.zero_()
    env._friction.fill_(-1.0)
    ndbg = 32
    env.enable_debug(ndbg)
    obs, rew, term, trunc, info = env.step(torch.as_tensor(ctrl))
    torch.cuda.synchronize()
    names = ['M', 'qfrc_bias', 'qfrc_smooth', 'qacc_smooth', 'nefc', 'ncon', 'efc_J', 'efc_aref', 'efc_R', 'efc_force', 'qacc']
    dbg = env.debug_internals(ndbg, names)
    o = _oracle(env)
    qpos_g, qvel_g = env.qpos.cpu().numpy(), env.qvel.cpu().numpy()
    obs_g = env._obs_buf.cpu().numpy()
    term_g, inv_g = term.cpu().numpy(), info['invalid_contacts'].cpu().numpy()
    n_contact, n_tie = 0, 0
    for e in range(N):
        o.set_state(qpos[e], qvel[e].astype(np.float32), warm[e], np.zeros(18), 0.0, -1.0)
        o.step(ctrl[e].astype(np.float64))
        # a link geom resting on two hull vertices of (numerically) equal depth has no unique "deepest vertex":
        # fp32 and fp64 may legitimately pick different ones.  Such envs are only checked for sanity.
        if sp.has_tie(o, 3e-7):
            n_tie += 1
            assert np.all(np.isfinite(qvel_g[e])) and np.abs(qvel_g[e] - o.qvel).max() < 5.0   # (a tie moves the mesh's whole manifold: up to three contacts)
            continue
        if not oracle_fits_row_budget(o, False):   # a robot pressed into the floor: its mesh manifolds exceed the kernel's 12 contacts / 63 rows (the budget tests hold those to the prefix rule)
            if e < ndbg:
                assert int(dbg[e]['nefc'][0]) < o.nefc
            continue
        if e < ndbg:
            d = dbg[e]
            assert int(d['nefc'][0]) == o.nefc and int(d['ncon'][0]) == o.ncon
            ne = o.nefc
            np.testing.assert_allclose(d['M'].reshape(18, 18), o.M, rtol=1e-4, atol=2e-5)
            np.testing.assert_allclose(d['qfrc_bias'], o.qfrc_bias, rtol=1e-4, atol=2e-3)
            sp.compare(o, d, sp.GPU_STAGE_ROWS, e)
            fmax = max(1.0, np.abs(o.efc_force).max())
            assert np.abs(d['efc_force'][:ne] - o.efc_force).max() < 2e-4 * fmax
            amax = max(1.0, np.abs(o.qacc).max())
            assert np.abs(d['qacc'] - o.qacc).max() < 5e-5 * amax   # measured p99 1.4e-6, max 4.6e-6
        n_contact += o.ncon > 0
        assert np.abs(qpos_g[e] - o.qpos).max() < 1e-6 + 2e-6 * np.abs(o.qpos).max()
        assert np.abs(qvel_g[e] - o.qvel).max() < 1e-4 + 1e-5 * np.abs(o.qvel).max()
        ref, t, inv = o.get_obs(ALL_OBS, cmd[e])
        got = split_obs(obs_g[e], ALL_OBS)
        for k in ALL_OBS:
            tol = 2e-3 * max(1.0, np.abs(ref[k]).max())
            assert np.abs(got[k] - ref[k]).max() < tol, (e, k, got[k], ref[k])
        assert bool(term_g[e]) == t and bool(inv_g[e]) == inv
    assert n_contact > N // 4, 'test states must exercise contacts'
    assert n_tie < N // 10


def test_rollout_tracks_oracle():
    """20 steps from reset states: trajectories stay within solver/fp32 tolerance of the oracle."""
    n = 32
    env = _make_env(n, obs=('qpos', 'qvel'), iters=50)
    env.reset(random=True)
    torch.cuda.synchronize()
    from oracle.oracle import Oracle
    orc = [Oracle(env._mm) for _ in range(n)]
    for e, o in enumerate(orc):
        o.set_state(env.qpos[e].cpu().numpy(), env.qvel[e].cpu().numpy().astype(np.float64),
                    env._warm[e].cpu().numpy().astype(np.float64), np.zeros(18), float(env._time[e]), float(env._friction[e]))
    g = torch.Generator(device='cuda:0').manual_seed(3)
    for s in range(20):
        act = torch.randn(n, 12, generator=g, device='cuda:0') * 10
        env.step(act)
        qp, qv = env.qpos.cpu().numpy(), env.qvel.cpu().numpy()
        for e, o in enumerate(orc):
            o.step(act[e].cpu().numpy().astype(np.float64))
            assert np.abs(qp[e] - o.qpos).max() < 2e-5, (s, e)    # 20 steps: measured drift 5e-7 at 10 steps, 8e-7 at 30
            assert np.abs(qv[e] - o.qvel).max() < 5e-4, (s, e)


@pytest.mark.parametrize('robot_name', ['b2', 'go1', 'go2', 'hyqreal1', 'hyqreal2', 'mini_cheetah', 'aliengo'])
def test_reset_contract_and_shapes(robot_name):
    """The reference's own test (tests/env_test.py:13-53) re-expressed for the batch, same robot list, scene 'flat'
    (its second scene, 'perlin': test_perlin_scene_contract_and_parity): three resets, shapes, 10 steps."""
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    n = 64
    env = QuadrupedEnv(robot=robot_name, scene='flat', ref_base_lin_vel=(0.5, 1.0), ground_friction_coeff=(0.2, 1.5),
                       base_vel_command_type='forward+rotate', state_obs_names=tuple(QuadrupedEnv.ALL_OBS), num_envs=n)
    state = env.reset()
    qpos, qvel = state['qpos'].clone(), state['qvel'].clone()
    state = env.reset(random=True)
    state = env.reset(qpos=env.qpos.clone(), qvel=env.qvel.clone())
    for name in QuadrupedEnv.ALL_OBS:
        assert tuple(state[name].shape) == (n,) + tuple(env.observation_space[name].shape)
    assert not bool(env.lift_failed.any())
    fr = env._friction.cpu().numpy()
    assert np.all(fr >= 0.2) and np.all(fr <= 1.5)
    cmd = env._cmd.cpu().numpy()
    assert np.all(cmd[:, 0] >= 0.5) and np.all(cmd[:, 0] <= 1.0) and np.all(cmd[:, 1] == 0)
    for _ in range(10):
        action = torch.as_tensor(np.stack([env.action_space.sample() for _ in range(n)])) * 50
        state, reward, term, trunc, info = env.step(action)
    torch.cuda.synchronize()
    assert torch.isfinite(state['qpos']).all() and torch.isfinite(state['qvel']).all()
    assert int(info['step_num'][0]) == 9 and abs(float(info['time'][0]) - 11 * 0.002) < 1e-6


def test_full_size_invariants():
    """4096 envs (BASELINE config 2): finite state, unit quaternions, no feet below the floor by more than the
    soft-contact depth, energy bounded; auto-reset keeps every env alive over a 200-step random rollout."""
    n = 4096
    env = _make_env(n, obs=('qpos', 'qvel', 'feet_pos', 'kinetic_energy'), iters=50, tol=1e-8, auto_reset=True)   # PGS, same-step
    env.reset(random=True)
    g = torch.Generator(device='cuda:0').manual_seed(0)
    nterm = 0
    for _ in range(200):
        obs, rew, term, trunc, info = env.step(torch.randn(n, 12, generator=g, device='cuda:0') * 50)
        nterm += int(term.sum())
    torch.cuda.synchronize()
    q = env.qpos
    assert torch.isfinite(q).all() and torch.isfinite(env.qvel).all()
    assert (q[:, 3:7].norm(dim=1) - 1).abs().max() < 1e-5
    assert obs["feet_pos"].reshape(n, 4, 3)[:, :, 2].min() > -0.15  # violent impacts do sink into the soft floor
    assert obs['kinetic_energy'].max() < 1e4
    assert nterm > 0, 'random +-50 Nm actions must terminate some envs'


def test_next_step_auto_reset_equals_manual_reset_loop():
    """gymnasium NEXT_STEP auto-reset: the terminating step returns the terminal observation with terminated=True; the
    env's next step call ignores the action and performs reset() (state write, lift loop, the reset's own mj_step) -
    exactly what the reference user loop `if terminated: env.reset()` does, so an explicit masked reset of a twin env
    (same seed, same episode counters) lands on the same state."""
    n = 512
    kw = dict(obs=('qpos', 'qvel'), iters=50, tol=1e-8, solver='newton')
    auto = _make_env(n, auto_reset='next_step', **kw)
    twin = _make_env(n, auto_reset=False, **kw)
    auto.reset(random=True); twin.reset(random=True)
    assert torch.equal(auto.qpos, twin.qpos)
    g = torch.Generator(device='cuda:0').manual_seed(3)
    pending = torch.zeros(n, dtype=torch.bool, device='cuda:0')
    nreset = 0
    for _ in range(150):
        act = torch.randn(n, 12, generator=g, device='cuda:0') * 50
        o1, _, t1, _, _ = auto.step(act)
        # twin: every env steps; the envs that terminated LAST step are then reset (reset() rewrites their whole state and
        # clears their flags, so the dropped step leaves no trace) - the reference user's `if terminated: env.reset()`
        o2, _, t2, _, _ = twin.step(act)
        if bool(pending.any()):
            o2 = twin.reset(random=True, env_ids=pending)
            nreset += int(pending.sum())
        assert torch.equal(t1, twin._terminated_b)
        assert torch.equal(auto.qpos, twin.qpos) and torch.equal(auto.qvel, twin.qvel)
        assert torch.equal(o1['qpos'], o2['qpos']) and torch.equal(o1['qvel'], o2['qvel'])
        assert not bool((t1 & pending).any())   # a reset step never reports termination
        pending = t1.clone()
    assert nreset > 0


def test_go2_rollout_elliptic_condim6_invariants():
    """BASELINE config 4 (go2, flat, elliptic cones, feet condim 6) at one shard: 4096 envs, 150 random-action steps with
    next-step auto-reset: state stays finite, quaternions unit, feet above the soft-contact depth, envs get re-spawned."""
    n = 4096
    env = _make_env(n, obs=('qpos', 'qvel', 'feet_pos', 'contact_forces'), iters=100, tol=1e-8, solver='newton', robot='go2',
                    auto_reset='next_step')
    env.reset(random=True)
    g = torch.Generator(device='cuda:0').manual_seed(1)
    nterm = 0
    for _ in range(150):
        obs, rew, term, trunc, info = env.step(torch.randn(n, 12, generator=g, device='cuda:0') * 20)
        nterm += int(term.sum())
    torch.cuda.synchronize()
    q = env.qpos
    assert torch.isfinite(q).all() and torch.isfinite(env.qvel).all() and torch.isfinite(obs['contact_forces']).all()
    assert (q[:, 3:7].norm(dim=1) - 1).abs().max() < 1e-5
    assert obs['feet_pos'].reshape(n, 4, 3)[:, :, 2].min() > -0.15
    fz = obs['contact_forces'].reshape(n, 4, 3)[:, :, 2]
    assert fz.min() > -1e-3 and fz.max() < 5e4    # unilateral, bounded
    assert nterm > 0


@pytest.mark.parametrize('robot', ['mini_cheetah', 'aliengo', 'hyqreal2', 'b2', 'go1', 'go2', 'hyqreal1', 'spot'])
def test_newton_step_matches_converged_oracle(robot):
    """solver='newton' (MuJoCo's default) on every robot of the registry - pyramidal cones (mini_cheetah, aliengo,
    hyqreal2, b2) and elliptic cones with impratio 100 (hyqreal1 condim 3; go1 / go2 / spot feet condim 6): one step from random
    contact-rich states against the oracle's Newton solution converged to 1e-12.  Tolerances: qacc 2e-4 * max|qacc|
    (solver tolerance 1e-8 + fp32), qvel 5e-4, qpos 2e-6, observations 2e-3 * max(1,|obs|)."""
    from oracle.oracle import Oracle
    n = 192
    env = _make_env(n, iters=100, tol=1e-8, solver='newton', robot=robot)
    mmN = marshalled(robot, solver=1, iterations=100, tolerance=1e-12)
    hip = env.robot_cfg.hip_height
    rng = np.random.default_rng(21)
    o = Oracle(mmN)
    # states that press trunk and thighs into the floor exceed the kernel's row budget (4 points per lying box geom): at most 8 % of
    # the drawn states may (they are held to the prefix rule), the rest is compared value by value
    qpos, qvel = budgeted_states(n, lambda k: random_states(env.mjModel, k, rng, z_range=(0.6 * hip, 1.6 * hip)), o, env.mjModel.cone == 1, max_over=0.08)
    qvel = qvel.astype(np.float32)
    warm = rng.normal(0, 5, (n, 18)).astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 40).astype(np.float32)
    cmd = np.tile(np.array([0.4, -0.2, 0.0, 0.1], np.float32), (n, 1))
    env._qpos.copy_(torch.as_tensor(qpos)); env._qvel.copy_(torch.as_tensor(qvel)); env._warm.copy_(torch.as_tensor(warm))
    env._cmd.copy_(torch.as_tensor(cmd)); env._friction.fill_(0.8)
    env.enable_debug(n)
    obs, rew, term, trunc, info = env.step(torch.as_tensor(ctrl))
    kern = gpu_records(env, n, ['qacc', 'niter', 'nefc', 'ncon', 'efc_J', 'efc_R', 'efc_aref'])
    ncon = 0
    tally = ParityTally(env.mjModel.cone == 1, 3e-7)
    cone = env.mjModel.cone == 1
    mg = 9.81 * float(env.mjModel.total_mass)
    ea, ev, ep, eo, ef = [], [], [], [], []
    for e in range(n):
        k = kern[e]
        # over the row budget: held to the prefix rule, and info['contacts_dropped'] says so to the caller; ties and those are counted and bounded
        # below; a row-count mismatch fails the test
        if tally.step_env(e, o, (qpos[e], qvel[e], warm[e], np.zeros(18), 0.0, 0.8), ctrl[e], k, sp.FLAGS, prefix=True) != 'ok':
            continue
        ncon += o.ncon
        ea.append(np.abs(k['qacc'] - o.qacc).max() / max(1.0, np.abs(o.qacc).max()))
        ev.append(np.abs(k['qvel'] - o.qvel).max()); ep.append(np.abs(k['qpos'] - o.qpos).max())
        ref, _, _ = o.get_obs(ALL_OBS, cmd[e])
        got = k['obs']
        eo.append(max(np.abs(got[k_] - ref[k_]).max() / max(1.0, np.abs(ref[k_]).max()) for k_ in ALL_OBS if not k_.startswith('contact_forces')))
        ef.append(max(np.abs(got[k_] - ref[k_]).max() for k_ in ('contact_forces', 'contact_forces:base')) / max(np.abs(ref['contact_forces']).max(), 0.1 * mg))
        assert k['niter'][0] <= (20 if not cone else 100)   # condim-6 cones converge slowly (the fp64 oracle too)
    # Asserted bounds = ~10 x the p99 and ~5 x the maximum measured over 512 states per robot on MI355X
    # (profiles/r02_newton_parity_report.txt: tests/reports/newton_parity_report.py).  Elliptic condim-6 contacts (go1, go2,
    # spot): torsional / rolling rows are almost unregularised directions, the forces of a light contact move by ~1e-3 of the
    # weight between MuJoCo's "improvement < 1e-8" and the oracle's 1e-12 while qacc agrees to 1e-5.
    p99 = lambda x: float(np.percentile(x, 99))
    lim = dict(qacc=(1e-4, 1e-3), qvel=(7e-4, 2e-3), qpos=(2.5e-6, 3.5e-6), obs=(3e-4, 5e-3), force=(1.5e-2, 5e-2)) if cone else \
          dict(qacc=(2e-5, 1e-3), qvel=(5e-5, 2e-3), qpos=(2.5e-6, 3.5e-6), obs=(3e-4, 5e-3), force=(5e-5, 1e-3))
    for name, err in (('qacc', ea), ('qvel', ev), ('qpos', ep), ('obs', eo), ('force', ef)):
        assert p99(err) < lim[name][0] and max(err) < lim[name][1], (robot, name, p99(err), max(err))
    # These random states press trunk and thighs into the floor; with MuJoCo's multi-point plane routines a lying box-geom
    # robot carries 4 contacts per box (measured over-budget share on MI355X, profiles/r03_parity_tallies.txt: mini_cheetah 0,
    # aliengo 0.16, hyqreal2 0.18, b2 0.24, go1 / go2 <= 0.4).  The benchmark's own states (test_step_parity_on_benchmark_
    # rollout_states) stay inside the budget; here the over-budget envs are held to the prefix rule instead of being skipped.
    tally.finish(f'newton one-step parity {robot}', min_checked=0.8, max_tie=0.12, max_budget=0.1)
    assert tally.checked >= 150 and ncon > 0.8 * n


def test_sensors_imu_and_heightmap_on_gpu():
    """aliengo + IMU plug-in + HeightMap (examples/aliengo_with_imu.py, aliengo_with_heightmap.py re-expressed)."""
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    from gym_quadruped_amd.sensors import IMU, HeightMap
    from oracle.oracle import Oracle
    from philox_ref import imu_normals
    n = 32
    names = ('qpos', 'qvel', 'base_ori_euler_xyz') + IMU.ALL_OBS
    kw = dict(accel_name='imu_acc', gyro_name='imu_gyro', imu_site_name='imu', accel_noise=0.01, gyro_noise=0.02,
              accel_bias_rate=0.03, gyro_bias_rate=0.04, seed=5)
    env = QuadrupedEnv('aliengo', state_obs_names=names, num_envs=n, sensors=(IMU,), sensors_kwargs=(kw,), solver='newton')
    env.reset(random=True)
    torch.cuda.synchronize()
    o = Oracle(marshalled('aliengo', solver=1, iterations=100, tolerance=1e-12))
    o.set_imu((0, 0, 0), (1, 0, 0, 0))
    q0, v0, w0 = env.qpos.cpu().numpy().copy(), env.qvel.cpu().numpy().copy(), env._warm.cpu().numpy().copy()
    fr, b0 = env._friction.cpu().numpy().copy(), env.sensors[0].bias_state.cpu().numpy().copy()
    ep = env._episode.cpu().numpy().copy()
    act = torch.randn(n, 12, device='cuda') * 20
    obs, *_ = env.step(act)
    torch.cuda.synchronize()
    for e in range(n):
        o.set_state(q0[e], v0[e].astype(np.float64), w0[e].astype(np.float64), np.zeros(18), 0.002, float(fr[e]))
        o.step(act[e].cpu().numpy().astype(np.float64))
        z = imu_normals(5, e, 0, int(ep[e]))
        ab, gb = b0[e, :3] + z[3:6] * 0.03, b0[e, 3:] + z[9:12] * 0.04
        assert np.abs(obs['imu_acc'][e].cpu().numpy() - (o.imu_acc + ab + z[0:3] * 0.01)).max() < 2e-3 * max(1, np.abs(o.imu_acc).max())
        assert np.abs(obs['imu_gyro'][e].cpu().numpy() - (o.imu_gyro + gb + z[6:9] * 0.02)).max() < 1e-4
        assert np.abs(env.sensors[0].get_observation('imu_gyro_bias')[e].cpu().numpy() - gb).max() < 1e-6
    hm = HeightMap(num_rows=5, num_cols=4, dist_x=0.1, dist_y=0.2, mj_model=env.mjModel, mj_data=env)
    data = hm.update_height_map(env.qpos[:, 0:3], yaw=obs['base_ori_euler_xyz'][:, 2])
    torch.cuda.synchronize()
    assert tuple(data.shape) == (n, 5, 4, 1, 3)
    d = data.cpu().numpy()[:, :, :, 0, :]
    c, yaw = env.qpos.cpu().numpy()[:, :3], obs['base_ori_euler_xyz'][:, 2].cpu().numpy()
    assert np.all(d[..., 2] == 0.0)                                           # rays end on the floor
    for e in range(0, n, 7):                                                  # grid layout of heightmap.py:106-146
        R = np.array([[np.cos(yaw[e]), np.sin(yaw[e])], [-np.sin(yaw[e]), np.cos(yaw[e])]])
        for i in range(5):
            for j in range(4):
                off = R.T @ np.array([0.1 * (2 - i), 0.2 * (2 - j) - 0.1])
                assert np.abs(d[e, i, j, :2] - (c[e, :2] + off)).max() < 1e-4 + 1e-7 * np.abs(c[e, :2]).max()


def test_mpc_accessors_match_oracle():
    """The reference's on-demand getters (quadruped_env.py:488-1016) as batched views: observation-backed ones
    (accessors=True) and the ones that read MuJoCo internals of the last forward pass (mj_fullM, qfrc_bias, mj_jac,
    body xpos, subtree_com) from the kernel's inspection record on the device - against the fp64 oracle."""
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    from oracle.oracle import Oracle
    n = 24
    env = QuadrupedEnv('aliengo', state_obs_names=('qpos', 'qvel'), num_envs=n, solver='newton', accessors=True, seed=3)
    env.reset(random=True)
    with pytest.raises(Exception):
        QuadrupedEnv('aliengo', state_obs_names=('qpos',), num_envs=2).base_lin_vel('base')   # not assembled, no accessors
    # accessors=True: the production kernel writes the dynamics / contact rows itself - no inspection record, no instrumented variant
    rec_env = QuadrupedEnv('aliengo', state_obs_names=tuple(QuadrupedEnv.ALL_OBS), num_envs=n, solver='newton', seed=3)   # fallback path
    rec_env.reset(random=True)
    _ = None
    try:
        rec_env.legs_mass_matrix      # first use without accessors=True: switches the instrumented kernel on, record still empty
    except Exception as e:
        _ = e
    assert _ is not None
    g = torch.Generator(device='cuda:0').manual_seed(0)
    for _ in range(30):
        act = torch.randn(n, 12, generator=g, device='cuda:0') * 15
        q0, v0, w0 = env.qpos.cpu().numpy().copy(), env.qvel.cpu().numpy().copy(), env._warm.cpu().numpy().copy()
        fr = env._friction.cpu().numpy().copy()
        obs, *_rest = env.step(act)
        rec_env.step(act)
    torch.cuda.synchronize()
    assert getattr(env, '_rec_tensor', None) is None and env._dyn is not None
    # the two paths agree: same kernel arithmetic, production vs instrumented variant (up to the compiler's contraction choices)
    for leg in ('FL', 'FR', 'RL', 'RR'):
        torch.testing.assert_close(env.legs_mass_matrix[leg], rec_env.legs_mass_matrix[leg], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(env.legs_qfrc_bias[leg], rec_env.legs_qfrc_bias[leg], rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(env.feet_jacobians('world')[leg], rec_env.feet_jacobians('world')[leg], rtol=1e-5, atol=1e-6)
    md = env.mjModel
    o = Oracle(marshalled('aliengo', solver=1, iterations=100, tolerance=1e-12))
    con = env.contacts()
    f_first = env.mj_contactForce(0)
    M_legs, bias, Jp = env.legs_mass_matrix, env.legs_qfrc_bias, env.feet_jacobians('world')
    Jb, Jrb = env.feet_jacobians('base', return_rot_jac=True)
    hips, com, Ib = env.hip_positions('world'), env.com, env.get_base_inertia()
    fp_w, fv_b = env.feet_pos('world'), env.feet_vel('base', relative=True)
    cs, _, grf = env.feet_contact_state('world', ground_reaction_forces=True)
    X = env.base_configuration
    a = act.cpu().numpy()
    for e in range(n):
        o.set_state(q0[e], v0[e], w0[e], np.zeros(18), 0.0, float(fr[e])); o.step(a[e].astype(np.float64))
        M = o.M
        ref, _t, _i = o.get_obs(ALL_OBS, env._cmd[e].cpu().numpy())
        for k, leg in enumerate(('FL', 'FR', 'RL', 'RR')):
            idx = env.legs_qvel_idx[leg]
            np.testing.assert_allclose(M_legs[leg][e].cpu().numpy(), M[np.ix_(idx, idx)], rtol=1e-4, atol=1e-6)
            np.testing.assert_allclose(bias[leg][e].cpu().numpy(), o.qfrc_bias[idx], rtol=1e-3, atol=2e-3)
            g_id = md.geom_names.index(env.robot_cfg.feet_geom_names[leg])
            jp, jr = o.jac(o.geom_xpos[g_id], int(md.geom_bodyid[g_id]))
            np.testing.assert_allclose(Jp[leg][e].cpu().numpy(), jp, atol=2e-5)
            Rb = o.xmat[1]
            np.testing.assert_allclose(Jb[leg][e].cpu().numpy(), Rb.T @ jp, atol=2e-5)
            np.testing.assert_allclose(Jrb[leg][e].cpu().numpy(), Rb.T @ jr, atol=2e-5)
            hip_b = md.body_names.index(f'{leg}_hip')
            np.testing.assert_allclose(hips[leg][e].cpu().numpy(), o.xpos[hip_b], atol=5e-6 * max(1.0, np.abs(o.xpos[hip_b]).max()))
            sl = slice(3 * k, 3 * k + 3)
            np.testing.assert_allclose(fp_w[leg][e].cpu().numpy(), ref['feet_pos'][sl], atol=5e-6 * max(1.0, np.abs(ref['feet_pos']).max()))
            np.testing.assert_allclose(fv_b[leg][e].cpu().numpy(), ref['feet_vel_rel:base'][sl], atol=2e-3 * max(1.0, np.abs(ref['feet_vel_rel:base']).max()))
            np.testing.assert_allclose(grf[leg][e].cpu().numpy(), ref['contact_forces'][sl], atol=2e-3 * max(1.0, np.abs(ref['contact_forces']).max()))
            assert bool(cs[leg][e]) == bool(ref['contact_state'][k])
        np.testing.assert_allclose(Ib[e].cpu().numpy(), M[3:6, 3:6], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(env._record('M')[e].cpu().numpy().reshape(18, 18), M, rtol=1e-4, atol=1e-5)    # mj_fullM, dense
        # mjData.contact + mj_contactForce (reference :836-870): list order, geoms, distances, frames, forces
        nc = int(con['ncon'][e])
        if o.ncon <= 12 and o.nefc <= 63:
            assert nc == o.ncon
            if nc:
                np.testing.assert_array_equal(con['geom2'][e, :nc].cpu().numpy(), o.get('contact_geom').astype(int))
                np.testing.assert_array_equal(con['geom1'][e, :nc].cpu().numpy(), o.get('contact_geom1').astype(int))
                np.testing.assert_allclose(con['dist'][e, :nc].cpu().numpy(), o.get('contact_dist'), atol=2e-6)
                np.testing.assert_allclose(con['frame'][e, :nc].cpu().numpy(), o.contact_frame, atol=2e-5)
                pos = con['pos'][e, :nc].cpu().numpy().astype(np.float64); pos[:, :2] += q0[e, :2]
                np.testing.assert_allclose(pos, o.contact_pos, atol=5e-6 * max(1.0, np.abs(o.contact_pos).max()))
                fo = o.contact_force
                np.testing.assert_allclose(con['force'][e, :nc].cpu().numpy(), fo, atol=2e-3 * max(1.0, np.abs(fo).max()))
                np.testing.assert_allclose(f_first[e].cpu().numpy(), fo[0], atol=2e-3 * max(1.0, np.abs(fo).max()))
            else:
                assert not f_first[e].any()
            assert not con['force'][e, nc:].any()
        sc = o.get('subtree_com').reshape(-1, 3)
        com_ref = (np.asarray(md.body_mass)[:, None] * sc).sum(0) / np.asarray(md.body_mass).sum()
        np.testing.assert_allclose(com[e].cpu().numpy(), com_ref, atol=5e-6 * max(1.0, np.abs(com_ref).max()))
        np.testing.assert_allclose(X[e, :3, :3].cpu().numpy().ravel(), ref['base_ori_SO3'], atol=1e-5)
        np.testing.assert_allclose(env.base_lin_vel('base')[e].cpu().numpy(), ref['base_lin_vel:base'], atol=1e-4)
    # feet_jacobians_dot (mj_jacDot) against a finite difference of the oracle's mj_jac along the velocity: the record holds the
    # poses of the last forward pass (q0) and the getters use the CURRENT velocity (env.qvel), like the reference's would
    Jd = env.feet_jacobians_dot('world')
    vnow = env.qvel.cpu().numpy().astype(np.float64)
    eps = 1e-6
    for e in range(0, n, 5):
        def jac_at(q):
            o.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18)); o.forward(np.zeros(12), stage=1)
            return {leg: o.jac(o.geom_xpos[md.geom_names.index(env.robot_cfg.feet_geom_names[leg])],
                               int(md.geom_bodyid[md.geom_names.index(env.robot_cfg.feet_geom_names[leg])]))[0] for leg in ('FL', 'FR', 'RL', 'RR')}
        q1 = q0[e].copy()
        q1[0:3] += eps * vnow[e, 0:3]; q1[7:] += eps * vnow[e, 6:]
        wq = vnow[e, 3:6] * eps   # body-frame angular increment: q <- q * exp(w dt)
        ang = np.linalg.norm(wq)
        dq = np.r_[np.cos(ang / 2), np.sin(ang / 2) * wq / max(ang, 1e-30)]
        a0 = q0[e, 3:7]
        q1[3:7] = [a0[0] * dq[0] - a0[1:] @ dq[1:], *(a0[0] * dq[1:] + dq[0] * a0[1:] + np.cross(a0[1:], dq[1:]))]
        Ja, Jb = jac_at(q0[e]), jac_at(q1)
        for leg in ('FL', 'FR', 'RL', 'RR'):
            fd = (Jb[leg] - Ja[leg]) / eps
            np.testing.assert_allclose(Jd[leg][e].cpu().numpy(), fd, atol=2e-3 * max(1.0, np.abs(fd).max()))


def test_step_is_hip_graph_capturable():
    """gq_step is a single stream-ordered launch with its pointers in a device-resident block: it can be captured into a
    HIP graph (torch.cuda.CUDAGraph) and replayed; the replayed rollout is bit-identical to the eager one."""
    n = 128
    def mk():
        e = _make_env(n, obs=('qpos', 'qvel'), iters=100, tol=1e-8, solver='newton', auto_reset='next_step')
        e.reset(random=True)
        return e
    eager, graphed = mk(), mk()
    fresh = graphed.state_dict()
    g = torch.Generator(device='cuda:0').manual_seed(0)
    seq = [torch.randn(n, 12, generator=g, device='cuda:0') * 30 for _ in range(25)]
    for x in seq:
        eager.step(x)
    act = torch.zeros(n, 12, device='cuda:0')
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        graphed.step(act)            # warm-up on the capture stream: uploads the argument block outside the capture
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        graphed.step(act)
    graphed.load_state_dict(fresh)
    for x in seq:
        act.copy_(x)
        gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager.qpos, graphed.qpos) and torch.equal(eager.qvel, graphed.qvel)


@pytest.mark.parametrize('robot,scene', [('aliengo', 'random_boxes'), ('hyqreal1', 'random_boxes'), ('mini_cheetah', 'stairs'),
                                         ('go2', 'random_pyramids'), ('aliengo', 'ramp'), ('b2', 'slippery'), ('go1', 'random_boxes')])  # go1: 12 cylinder geoms (rim clouds on boxes)
def test_box_scenes_rollout_and_step_parity(robot, scene):
    """Scenes with static world boxes (terrain.py: random_boxes / random_pyramids procedural, ramp / slippery / stairs static;
    BASELINE config 5 is hyqreal1 on random_boxes): reset inside the scene's limits, a random rollout with next-step
    auto-reset stays finite, and one step from the rollout state matches the fp64 oracle (same box narrow phase)."""
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    from oracle.oracle import Oracle
    n = 256
    env = QuadrupedEnv(robot, scene=scene, state_obs_names=tuple(QuadrupedEnv.ALL_OBS), num_envs=n, solver='newton',
                       auto_reset='next_step', seed=11)
    assert len(env.scene_desc['boxes']) > 0
    env.reset(random=True)
    lim = env.terrain_limits
    q = env.qpos
    assert bool(((q[:, 0] <= lim[0]) & (q[:, 0] >= lim[1]) & (q[:, 1] <= lim[2]) & (q[:, 1] >= lim[3])).all())
    g = torch.Generator(device='cuda:0').manual_seed(2)
    for _ in range(120):
        obs, rew, term, trunc, info = env.step(torch.randn(n, 12, generator=g, device='cuda:0') * 15)
    torch.cuda.synchronize()
    assert torch.isfinite(env.qpos).all() and torch.isfinite(env.qvel).all() and torch.isfinite(env._obs_buf).all()
    o = Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-12, boxes=env.scene_desc['boxes'], terrain_limits=lim))
    nbox = _one_more_step_against_oracle(env, o, g, f'box scene one-step parity {robot} {scene}',
                                         lambda: int((np.abs(o.contact_frame[:, 0, 2] - 1.0) > 1e-9).sum() + (np.abs(o.contact_pos[:, 2]) > 5e-3).sum()))
    assert nbox > 0


def test_heightmap_rays_hit_world_boxes():
    """HeightMap on a box scene: every ray's hit height equals the highest box top (or the floor) under it (numpy ray-box)."""
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    from gym_quadruped_amd.sensors import HeightMap
    from scipy.spatial.transform import Rotation
    n = 64
    env = QuadrupedEnv('aliengo', scene='random_boxes', state_obs_names=('qpos',), num_envs=n, solver='newton', seed=5)
    env.reset(random=True)
    hm = HeightMap(num_rows=5, num_cols=5, dist_x=0.1, dist_y=0.1, mj_model=env.mjModel, mj_data=env)
    data = hm.update_height_map(env.qpos[:, 0:3], yaw=0.3).reshape(n, -1, 3).cpu().numpy()
    boxes = env.scene_desc['boxes']
    R = [Rotation.from_quat(np.asarray(b['quat']), scalar_first=True).as_matrix() for b in boxes]
    nhit = 0
    for e in range(0, n, 7):
        for p in data[e]:
            top = 0.0
            for b, Rb in zip(boxes, R):
                o_l = Rb.T @ (np.array([p[0], p[1], 10.0]) - np.asarray(b['pos'])); d_l = Rb.T @ np.array([0.0, 0.0, -1.0])
                tin, tout, ok = -1e30, 1e30, True
                for k in range(3):
                    if abs(d_l[k]) < 1e-12:
                        ok &= abs(o_l[k]) <= b['size'][k]
                        continue
                    t0, t1 = (-b['size'][k] - o_l[k]) / d_l[k], (b['size'][k] - o_l[k]) / d_l[k]
                    tin, tout = max(tin, min(t0, t1)), min(tout, max(t0, t1))
                if ok and tin <= tout and tout >= 0:
                    top = max(top, 10.0 - tin)
            assert abs(p[2] - top) < 1e-4, (e, p, top)
            nhit += top > 1e-6
    assert nhit > 0


def _env_on_grid(monkeypatch, robot, name, n, **kw):
    """QuadrupedEnv takes scene names only: the grid of tests/hfield_cases.py goes in through generate_terrain"""
    import gym_quadruped_amd.quadruped_env as qe
    import hfield_cases as hc
    monkeypatch.setattr(qe, 'generate_terrain', lambda scene, hip, seed=10: hc.scene(name))
    env = qe.QuadrupedEnv(robot, scene='perlin', num_envs=n, solver='newton', **kw)
    assert env.scene_desc['hfield'] is hc.grid(name)
    return env


@pytest.mark.parametrize('rows,cols', [(9, 9), (6, 4)])   # 81 cells: the strided cell loop and its cells - 1 mirror lanes; both dimensions even
def test_heightmap_and_rays_on_a_non_square_height_field(monkeypatch, rows, cols):
    """HeightMap and gq_ray (mj_ray) on the mild_coarse grid of tests/hfield_cases.py - cells of 0.11 x 0.07 m, 41 x 57 samples, 40 m from the
    origin - against the numpy surface (triangle interpolation with the same diagonal): hit heights to 1e-4, the grid layout to the tolerance
    of test_sensors_imu_and_heightmap_on_gpu; map centres and rays over the grid, beside and beyond its border (there: the floor)."""
    import hfield_cases as hc
    from gym_quadruped_amd.sensors import HeightMap
    n = 32
    env = _env_on_grid(monkeypatch, 'aliengo', 'mild_coarse', n, state_obs_names=('qpos',), seed=5)
    hf = hc.grid('mild_coarse')
    pos, sx, sy = np.asarray(hf['pos']), hf['size'][0], hf['size'][1]
    rng = np.random.default_rng(8)

    def top(x, y):
        h, _, inside, _ = hc.surface(hf, x - pos[0], y - pos[1])
        near = np.minimum(np.abs(np.abs(x - pos[0]) - sx), np.abs(np.abs(y - pos[1]) - sy)) < 1e-5   # on the border line: either answer
        return np.where(inside, np.maximum(pos[2] + h, 0.0), 0.0), near
    dx_, dy_ = 0.045, 0.06
    c = np.stack([pos[0] + rng.uniform(-sx - 0.3, sx + 0.3, n), pos[1] + rng.uniform(-sy - 0.3, sy + 0.3, n), rng.uniform(0.5, 0.9, n)], 1)
    c[:8, 0] = pos[0] + np.where(np.arange(8) % 2 == 0, -sx, sx) + rng.uniform(-0.1, 0.1, 8)   # maps that straddle the border
    yaw = rng.uniform(-np.pi, np.pi, n).astype(np.float32)
    hm = HeightMap(num_rows=rows, num_cols=cols, dist_x=dx_, dist_y=dy_, mj_model=env.mjModel, mj_data=env)
    d = hm.update_height_map(torch.as_tensor(c, device='cuda:0'), yaw=torch.as_tensor(yaw, device='cuda:0')).cpu().numpy()[:, :, :, 0, :]
    assert d.shape == (n, rows, cols, 3)
    ii, jj = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
    gx, gy = dx_ * ((rows - 1) / 2 - ii), dy_ * ((cols - 1) / 2 - jj)
    non, noff = 0, 0
    for e in range(n):
        cy, sn = np.cos(yaw[e]), np.sin(yaw[e])
        px, py = c[e, 0] + cy * gx - sn * gy, c[e, 1] + sn * gx + cy * gy
        assert np.abs(d[e, :, :, 0] - px).max() < 1e-4 + 1e-7 * np.abs(c[e, :2]).max() and np.abs(d[e, :, :, 1] - py).max() < 1e-4 + 1e-7 * np.abs(c[e, :2]).max()
        ref, near = top(d[e, :, :, 0].astype(np.float64), d[e, :, :, 1].astype(np.float64))
        assert (np.abs(d[e, :, :, 2] - ref)[~near] < 1e-4).all(), (e, np.abs(d[e, :, :, 2] - ref).max())
        non += int((ref > 0).sum()); noff += int((ref == 0).sum())
    assert non > 10 * rows and noff > 10 * rows, (non, noff)
    # gq_ray: vertical rays from above, over the grid and around it
    R = 64
    o = np.stack([pos[0] + rng.uniform(-sx - 0.2, sx + 0.2, (n, R)), pos[1] + rng.uniform(-sy - 0.2, sy + 0.2, (n, R)), np.full((n, R), 2.0)], -1)
    o[:, :8, 1] = pos[1] + np.where(np.arange(8) % 2 == 0, -sy, sy) + rng.uniform(-0.01, 0.01, (n, 8))
    vec = np.tile(np.array([0.0, 0.0, -1.0], np.float32), (n, R, 1))
    dist = env.mj_ray(o, vec).cpu().numpy()
    ref, near = top(o[..., 0], o[..., 1])
    assert (np.abs((2.0 - dist) - ref)[~near] < 1e-4).all(), np.abs((2.0 - dist) - ref)[~near].max()
    assert (ref > 0).sum() > 100 and (ref == 0).sum() > 100


@pytest.mark.parametrize('name', ['mild_coarse', 'rough_coarse', 'mild_fine', 'rough_fine'])
@pytest.mark.parametrize('robot', ['aliengo', 'hyqreal1'])   # primitive geoms, pyramidal cones / hulls, elliptic cones
def test_height_field_step_on_rough_fine_grids_matches_oracle(monkeypatch, robot, name):
    """The emulated test of the same name on the device, 64 envs per grid: hfield_item_scan under the STRICT row rule on rough and mild, coarse
    and fine, non-square grids away from the origin, a quarter of the robots at the border.
    The states keep every foot at least 0.01 m from the ridge it touches (hfield_cases.min_lever: closer, an fp32 normal cannot hold efc_J)."""
    import hfield_cases as hc
    from oracle.oracle import Oracle
    n = 64
    env = _env_on_grid(monkeypatch, robot, name, n, state_obs_names=tuple(ALL_OBS), seed=3)
    hf = hc.grid(name)
    mmN = marshalled(robot, solver=1, iterations=100, tolerance=1e-13, hfield=hf, terrain_limits=env.terrain_limits)
    hc.assert_foot_form(mmN, hf, name, robot)
    rng = np.random.default_rng(32)
    o = Oracle(mmN)
    qpos, qvel = hc.step_states(mmN, robot, name, n, rng, o)
    warm = rng.normal(0, 3, (n, 18)).astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    env._qpos.copy_(torch.as_tensor(qpos)); env._qvel.copy_(torch.as_tensor(qvel)); env._warm.copy_(torch.as_tensor(warm))
    env._cmd.zero_(); env._friction.fill_(0.8)
    env.enable_debug(n)
    env.step(torch.as_tensor(ctrl))
    kern = gpu_records(env, n, ['qacc', 'nefc', 'ncon', 'efc_J', 'efc_R', 'efc_aref'])
    tally = ParityTally(env.mjModel.cone == 1, 3e-6)
    tot = np.zeros(3, int)
    for e in range(n):
        if tally.step_env(e, o, (qpos[e], qvel[e], warm[e], np.zeros(18), 0.0, 0.8), ctrl[e], kern[e], sp.TERRAIN_NEWTON_STEP, mass=float(env.mjModel.total_mass)) == 'ok':
            tot += hc.count_contacts(o, mmN, hf)
    sp.tally_note(f'gpu {name} {robot}: height-field contacts {tot[0]} over {tally.checked} compared envs, {tot[1]} foot contacts on an edge or corner, {tot[2]} link-geom contacts')
    tally.finish_count(f'gpu {name} {robot}', n // 2)
    assert tot[0] >= 4 * tally.checked and tot[2] >= 1 and (tot[1] >= 1 or 'rough' not in name), tot


@pytest.mark.parametrize('robot,scene', [('hyqreal1', 'random_boxes'), ('aliengo', 'perlin'), ('aliengo', 'random_boxes')])
def test_heightmap_following_the_base_equals_the_ray_kernel(robot, scene):
    """HeightMap(follow_base=True): the step kernel casts the rays of the map centred on the new base position with the new heading
    (gq_batch_set_heightmap).  Every step it must hold what the separate ray kernel returns for update_height_map(qpos[0:3],
    yaw=base_ori_euler_xyz[2]) - the call the reference's examples make after env.step - re-spawning envs included; after a reset the
    argument-less update launches the ray kernel itself; a flat scene refuses the fused form."""
    from gym_quadruped_amd import _lib
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    from gym_quadruped_amd.sensors import HeightMap
    n = 384
    env = QuadrupedEnv(robot, scene=scene, state_obs_names=('qpos', 'base_ori_euler_xyz'), num_envs=n, solver='newton', auto_reset='next_step', seed=4)
    obs = env.reset(random=True)
    fused = HeightMap(num_rows=5, num_cols=7, dist_x=0.1, dist_y=0.08, mj_model=env.mjModel, mj_data=env, follow_base=True)
    plain = HeightMap(num_rows=5, num_cols=7, dist_x=0.1, dist_y=0.08, mj_model=env.mjModel, mj_data=env)
    a0 = fused.update_height_map().clone()                      # after a reset: the ray kernel, centre / heading taken from qpos
    b0 = plain.update_height_map(env.qpos[:, 0:3], yaw=obs['base_ori_euler_xyz'][:, 2]).clone()
    assert torch.allclose(a0, b0, atol=2e-5), float((a0 - b0).abs().max())
    g = torch.Generator(device='cuda:0').manual_seed(1)
    on_geom = 0
    for k in range(80):
        obs, _, term, _, _ = env.step(torch.randn(n, 12, generator=g, device='cuda:0') * 60)
        a = fused.update_height_map()                           # no launch: written by the step
        b = plain.update_height_map(env.qpos[:, 0:3], yaw=obs['base_ori_euler_xyz'][:, 2])
        if k % 8 == 7:
            assert torch.allclose(a, b, atol=2e-5), (k, float((a - b).abs().max()))
            on_geom += int((b[..., 2] > 1e-3).sum())
    assert on_geom > 0 and int(env._episode.max()) > 1          # rays land on the scene's geoms; envs re-spawned on the way
    obs = env.reset(random=True)
    assert not env._hm_fresh
    a1 = fused.update_height_map().clone()
    b1 = plain.update_height_map(env.qpos[:, 0:3], yaw=obs['base_ori_euler_xyz'][:, 2])
    assert torch.allclose(a1, b1, atol=2e-5)
    # one base-following map per env: a second one is refused (the kernel has one output slot per batch) ...
    with pytest.raises(ValueError):
        HeightMap(num_rows=5, num_cols=7, dist_x=0.1, dist_y=0.08, mj_model=env.mjModel, mj_data=env, follow_base=True)
    # ... a custom centre on the base-following map goes to a tensor of its own and leaves the kernel's alone ...
    env.step(torch.zeros(n, 12, device='cuda:0'))
    keep = fused.update_height_map().clone()
    far = fused.update_height_map(env.qpos[:, 0:3] + torch.tensor([0.3, 0.0, 0.0], device='cuda:0', dtype=torch.float64), yaw=0.5)
    assert far.data_ptr() != fused.sensor_data_matrix.data_ptr()
    assert torch.equal(fused.update_height_map(), keep)
    # ... and an in-place write to the state makes the kernel's map stale: the next argument-less update casts the rays again
    env.qpos[:, 0] += 0.25
    moved = fused.update_height_map().clone()
    ref = plain.update_height_map(env.qpos[:, 0:3], yaw=env._obs_views['base_ori_euler_xyz'][:, 2])
    assert torch.allclose(moved, ref, atol=2e-5) and not torch.allclose(moved, keep, atol=1e-3)
    fused.close()
    env.step(torch.zeros(n, 12, device='cuda:0'))               # detached: the step no longer writes the map
    torch.cuda.synchronize()
    flat = QuadrupedEnv(robot, scene='flat', state_obs_names=('qpos',), num_envs=8)
    with pytest.raises(_lib.GqError):
        HeightMap(num_rows=5, num_cols=5, dist_x=0.1, dist_y=0.1, mj_model=flat.mjModel, mj_data=flat, follow_base=True)


def test_baseline_config5_hyqreal1_boxes_imu_heightmap():
    """BASELINE.json configs[4]: hyqreal1 on random_boxes with the IMU plug-in and a 5x5 HeightMap, the full observation
    pipeline (ALL_OBS + 6 IMU observables): reset, a short auto-resetting rollout, everything finite and shaped."""
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    from gym_quadruped_amd.sensors import IMU, HeightMap
    n = 512
    names = tuple(QuadrupedEnv.ALL_OBS) + IMU.ALL_OBS
    kw = dict(accel_name='Body_Acc', gyro_name='Body_Gyro', imu_site_name='imu', accel_noise=0.01, gyro_noise=0.01,
              accel_bias_rate=0.01, gyro_bias_rate=0.01, seed=1)
    env = QuadrupedEnv('hyqreal1', scene='random_boxes', state_obs_names=names, num_envs=n, sensors=(IMU,), sensors_kwargs=(kw,),
                       solver='newton', auto_reset='next_step', seed=2)
    obs = env.reset(random=True)
    hm = HeightMap(num_rows=5, num_cols=5, dist_x=0.1, dist_y=0.1, mj_model=env.mjModel, mj_data=env)
    g = torch.Generator(device='cuda:0').manual_seed(0)
    nterm = 0
    for _ in range(60):
        obs, rew, term, trunc, info = env.step(torch.randn(n, 12, generator=g, device='cuda:0') * 60)
        nterm += int(term.sum())
        heights = hm.update_height_map(env.qpos[:, 0:3], yaw=obs['base_ori_euler_xyz'][:, 2])
    torch.cuda.synchronize()
    assert tuple(heights.shape) == (n, 5, 5, 1, 3) and torch.isfinite(heights).all()
    assert float(heights[..., 2].max()) > 0.02 and float(heights[..., 2].min()) >= 0.0    # some rays land on boxes, none below the floor
    for k in names:
        assert torch.isfinite(obs[k]).all(), k
    assert tuple(obs['imu_acc'].shape) == (n, 3) and float(obs['imu_acc'].abs().max()) > 1.0


def test_api_edge_cases_single_env_action_forms_and_errors():
    """Drop-in edge cases: one env (the reference's shape), [nu] and numpy actions, masked reset leaving other envs alone,
    and the reference's error behaviour (unknown observable / robot / scene names raise ValueError; 'hyqreal' alone is not a
    registry key; PGS with elliptic cones is refused with a reason)."""
    from gym_quadruped_amd import _lib
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    env = QuadrupedEnv('mini_cheetah', num_envs=1)
    obs = env.reset()
    assert tuple(obs['qpos'].shape) == (1, 19)
    a = env.action_space.sample() * 10                      # numpy [nu]
    o1, r, term, trunc, info = env.step(a)
    assert tuple(o1['qvel'].shape) == (1, 18) and r.shape == (1,) and term.dtype == torch.bool
    o2, *_ = env.step(torch.as_tensor(a, dtype=torch.float64))   # wrong dtype / device: converted, same semantics
    with pytest.raises(ValueError):
        env.step(np.zeros((1, 7)))
    env4 = QuadrupedEnv('mini_cheetah', num_envs=4, seed=1)
    env4.reset(random=True)
    before = env4.qpos.clone()
    env4.reset(random=True, env_ids=[1, 3])
    after = env4.qpos
    assert torch.equal(after[0], before[0]) and torch.equal(after[2], before[2])
    assert not torch.equal(after[1], before[1]) and not torch.equal(after[3], before[3])
    with pytest.raises(ValueError):
        QuadrupedEnv('mini_cheetah', state_obs_names=('qpos', 'not_an_observable'), num_envs=1)
    with pytest.raises(ValueError):
        QuadrupedEnv('hyqreal', num_envs=1)
    with pytest.raises(ValueError):
        QuadrupedEnv('mini_cheetah', scene='moon', num_envs=1)
    with pytest.raises(_lib.GqError, match='Newton'):
        QuadrupedEnv('go2', solver='pgs', num_envs=1)                      # elliptic cones: no per-contact QCQP in the PGS path
    with pytest.raises(_lib.GqError, match='Newton'):
        QuadrupedEnv('hyqreal1', scene='random_boxes', solver='pgs', num_envs=1)
    QuadrupedEnv('aliengo', scene='stairs', solver='pgs', num_envs=1).close()   # pyramidal cones: PGS serves every scene (round 4)


@pytest.mark.parametrize('scene', ['perlin', 'random_boxes'])
def test_pgs_on_world_geoms_and_self_collision_matches_oracle_pgs(scene):
    """BASELINE config 3's scene (aliengo, perlin) and a box field under the solver the north-star names: PGS with height field /
    world boxes / robot self-collision rows.  Same rows as the Newton variant (the oracle builds one constraint list), force and
    acceleration of the oracle's PGS after the same 40 sweeps, contact forces read back through the parked contact normals; and a
    200-step rollout at 1024 envs stays finite, re-spawns and reports its capacity cuts."""
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    from oracle.oracle import Oracle
    n = 48
    env = QuadrupedEnv('aliengo', scene=scene, state_obs_names=ALL_OBS, num_envs=n, device='cuda:0', solver='pgs', solver_iterations=40,
                       solver_tolerance=0.0, self_collision=True, auto_reset=False, seed=5)
    env.reset(random=True)
    g = torch.Generator(device='cuda:0').manual_seed(1)
    for _ in range(60):   # fall onto the terrain
        env.step(torch.randn(n, 12, generator=g, device='cuda:0') * 20)
    env.enable_debug(n)
    q0, v0, w0 = env.qpos.cpu().numpy().copy(), env.qvel.cpu().numpy().copy(), env._warm.cpu().numpy().copy()
    fr = env._friction.cpu().numpy().copy()
    act = torch.randn(n, 12, generator=g, device='cuda:0') * 20
    obs, _, term, _, info = env.step(act)
    kern = gpu_records(env, n, ['nefc', 'ncon', 'qacc', 'efc_J', 'efc_aref'])
    o = Oracle(env._mm)
    a = act.cpu().numpy()
    world = 0
    tally = ParityTally(False, 3e-6, lenient_rows=True)
    for e in range(n):
        if tally.step_env(e, o, (q0[e], v0[e], w0[e], np.zeros(18), 0.0, float(fr[e])), a[e], kern[e], sp.TERRAIN_PGS_STEP_GPU, mass=env.mjModel.total_mass) != 'ok':
            assert int(kern[e]['nefc'][0]) <= o.nefc
            continue
        world += int((np.abs(o.contact_frame[:, 0, 2] - 1.0) > 1e-6).sum()) if o.ncon else 0
    tally.finish_count(f'PGS on world geoms {scene}', n // 2)
    assert world >= 8, world
    env.close()
    big = QuadrupedEnv('aliengo', scene=scene, state_obs_names=ALL_OBS, num_envs=1024, device='cuda:0', solver='pgs', self_collision=True,
                       auto_reset='next_step', seed=2)
    big.reset(random=True)
    for _ in range(200):
        _, _, _, _, info = big.step(torch.randn(1024, 12, generator=g, device='cuda:0') * 50)
    torch.cuda.synchronize()
    assert torch.isfinite(big.qpos).all() and torch.isfinite(big.qvel).all()
    assert int(big._episode.max()) > 1 and int(info['contacts_dropped'].max()) <= 40
    big.close()


def _hfield_height(hf, x, y):
    """Elevation of the height field's triangulated surface at world (x, y) (numpy, the triangulation of gq_boxes.h)."""
    data = np.asarray(hf['data'], np.float64); sx, sy, sz, _ = hf['size']; px, py, pz = hf.get('pos', (0.0, 0.0, 0.0))
    nr, nc = data.shape
    fx, fy = (x - px + sx) / (2 * sx) * (nc - 1), (y - py + sy) / (2 * sy) * (nr - 1)
    c, r = min(int(fx), nc - 2), min(int(fy), nr - 2)
    u, v = fx - c, fy - r
    h00, h10, h01, h11 = sz * data[r, c], sz * data[r, c + 1], sz * data[r + 1, c], sz * data[r + 1, c + 1]
    return pz + (h00 + u * (h10 - h00) + v * (h01 - h00) if u + v <= 1 else h11 + (1 - u) * (h01 - h11) + (1 - v) * (h10 - h11))


@pytest.mark.parametrize('robot', ['aliengo', 'hyqreal1', 'mini_cheetah'])
def test_perlin_scene_contract_and_parity(robot):
    """BASELINE.json configs[2] (aliengo on 'perlin', the second scene of the reference's own test tests/env_test.py:13-53):
    reset lifts every robot clear of the hills, a random rollout with next-step auto-reset stays finite and on the terrain,
    one step from the rollout state matches the fp64 oracle (same height-field narrow phase), HeightMap rays land on the
    triangulated surface."""
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    from gym_quadruped_amd.sensors import HeightMap
    from oracle.oracle import Oracle
    n = 256
    env = QuadrupedEnv(robot, scene='perlin', state_obs_names=tuple(QuadrupedEnv.ALL_OBS), num_envs=n, solver='newton',
                       auto_reset='next_step', seed=11)
    hf = env.scene_desc['hfield']
    state = env.reset(random=True)
    torch.cuda.synchronize()
    assert not bool(env.lift_failed.any())
    for name in QuadrupedEnv.ALL_OBS:
        assert tuple(state[name].shape) == (n,) + tuple(env.observation_space[name].shape)
    lim = env.terrain_limits
    q = env.qpos.cpu().numpy()
    assert np.all((q[:, 0] <= lim[0]) & (q[:, 0] >= lim[1]) & (q[:, 1] <= lim[2]) & (q[:, 1] >= lim[3]))
    ground = np.array([_hfield_height(hf, q[e, 0], q[e, 1]) for e in range(n)])
    assert np.all(q[:, 2] > ground) and ground.max() > 0.3 * hf['size'][2]       # bases above the local surface, hills present
    g = torch.Generator(device='cuda:0').manual_seed(2)
    nterm = 0
    for _ in range(150):
        obs, rew, term, trunc, info = env.step(torch.randn(n, 12, generator=g, device='cuda:0') * 15)
        nterm += int(term.sum())
    torch.cuda.synchronize()
    assert torch.isfinite(env.qpos).all() and torch.isfinite(env.qvel).all() and torch.isfinite(env._obs_buf).all()
    q = env.qpos.cpu().numpy()
    ground = np.array([_hfield_height(hf, q[e, 0], q[e, 1]) for e in range(n)])
    assert np.all(q[:, 2] > ground - 0.05), 'a robot fell through the terrain'
    assert float(obs['contact_state'].float().mean()) > 0.03                     # feet on the hills (most robots are mid-fall after a respawn)
    o = Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-12, hfield=hf, terrain_limits=lim))
    nhf = _one_more_step_against_oracle(env, o, g, f'perlin one-step parity {robot}', lambda: int((np.abs(o.contact_frame[:, 0, 2] - 1.0) > 1e-9).sum()))
    assert nhf > n // 4, nhf
    # HeightMap: vertical rays against the same surface
    hm = HeightMap(num_rows=5, num_cols=5, dist_x=0.1, dist_y=0.1, mj_model=env.mjModel, mj_data=env)
    data = hm.update_height_map(env.qpos[:, 0:3], yaw=0.3).reshape(n, -1, 3).cpu().numpy()
    for e in range(0, n, 9):
        for p in data[e]:
            assert abs(p[2] - max(0.0, _hfield_height(hf, p[0], p[1]))) < 2e-4, (e, p)


def test_rollout_recorder_exports_reference_layout(tmp_path):
    """utils/data.py: device-side recording of a batched rollout, exported in the reference H5Writer's layout
    (recordings/<obs> (trajectory, time, dim) float64 + env_hparams) - here through the dependency-free npz path."""
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    from gym_quadruped_amd.utils.data import RolloutRecorder, load_npz
    n, T = 32, 20
    env = QuadrupedEnv('mini_cheetah', state_obs_names=('qpos', 'qvel', 'feet_pos:base', 'contact_state'), num_envs=n, seed=3)
    obs = env.reset(random=True)
    rec = RolloutRecorder(env, horizon=T)
    g = torch.Generator(device='cuda:0').manual_seed(0)
    acts, qposes = [], []
    for t in range(T):
        a = torch.randn(n, 12, generator=g, device='cuda:0') * 10
        obs, rew, term, trunc, info = env.step(a)
        rec.append(obs, a)
        acts.append(a.cpu().numpy()); qposes.append(obs['qpos'].cpu().numpy())
    with pytest.raises(IndexError):
        rec.append(obs, a)
    path = rec.to_npz(tmp_path / 'roll.npz')
    data, hp = load_npz(path)
    assert hp['robot'] == 'mini_cheetah' and hp['num_envs'] == n
    assert data['qpos'].shape == (n, T, 19) and data['qpos'].dtype == np.float64 and data['time'].shape == (n, T, 1)
    assert data['action'].shape == (n, T, 12) and data['feet_pos:base'].shape == (n, T, 12)
    np.testing.assert_allclose(data['action'], np.stack(acts, 1), atol=0)
    np.testing.assert_allclose(data['qpos'], np.stack(qposes, 1), atol=0)
    np.testing.assert_allclose(data['time'][:, :, 0], np.tile(0.002 * np.arange(1, T + 1), (n, 1)) + data['time'][:, :1, 0] - 0.002, atol=1e-6)


def test_subset_of_observables_equals_the_full_set():
    """Observation groups nobody requested are skipped by the kernel (GqDevBatch::obs_need); what IS requested must be
    bit-identical to the same columns of an ALL_OBS env, for the reference's default set and for single-group requests."""
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    n = 128
    subsets = [QuadrupedEnv._DEFAULT_OBS, ('qpos', 'kinetic_energy', 'work'), ('contact_forces:base', 'contact_state'),
               ('base_ori_euler_xyz', 'gravity_vector:base'), ('qvel',)]
    full = QuadrupedEnv('aliengo', state_obs_names=tuple(QuadrupedEnv.ALL_OBS), num_envs=n, seed=5, auto_reset='next_step')
    envs = [QuadrupedEnv('aliengo', state_obs_names=tuple(s), num_envs=n, seed=5, auto_reset='next_step') for s in subsets]
    ref = full.reset(random=True)
    obs = [e.reset(random=True) for e in envs]
    g = torch.Generator(device='cuda:0').manual_seed(4)
    for t in range(40):
        a = torch.randn(n, 12, generator=g, device='cuda:0') * 40
        ref, _, term, _, _ = full.step(a)
        for i, e in enumerate(envs):
            o, _, term_i, _, _ = e.step(a)
            assert torch.equal(term, term_i)
            for k in subsets[i]:
                assert torch.equal(o[k], ref[k]), (t, k)


@pytest.mark.parametrize('robot', ['mini_cheetah', 'aliengo', 'go2', 'go1', 'hyqreal1', 'b2', 'spot'])
def test_robot_self_collision_step_parity(robot):
    """Robot-robot contacts (MuJoCo's default contype = conaffinity = 1: legs hit each other and the trunk; capsule proxies,
    gym_quadruped_amd/selfcol.py) on the GPU against the fp64 oracle: every test state has at least one such contact, about
    half of them between two different legs (dense Newton step), mixed with floor contacts."""
    from oracle.oracle import Oracle
    n = 160
    env = _make_env(n, iters=100, tol=1e-8, solver='newton', robot=robot, accessors=True)   # (accessors=True: the contact row, read through env.contacts())
    o = Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-12))
    hip = env.robot_cfg.hip_height
    rng = np.random.default_rng(5)
    cone = env.mjModel.cone == 1
    qa, va = self_contact_states(env.mjModel, n // 2, rng, o, z=(0.7 * hip, 1.3 * hip), want_cross=True, cone=cone, max_over=0.08)
    qb, vb = self_contact_states(env.mjModel, n - n // 2, rng, o, z=(0.7 * hip, 2.5 * hip), want_cross=None, cone=cone, max_over=0.08)
    qpos, qvel = np.concatenate([qa, qb]), np.concatenate([va, vb]).astype(np.float32)
    warm = np.zeros((n, 18), np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 30).astype(np.float32)
    cmd = np.tile(np.array([0.4, -0.2, 0.0, 0.1], np.float32), (n, 1))
    env._qpos.copy_(torch.as_tensor(qpos)); env._qvel.copy_(torch.as_tensor(qvel)); env._warm.copy_(torch.as_tensor(warm))
    env._cmd.copy_(torch.as_tensor(cmd)); env._friction.fill_(0.8)
    env.enable_debug(n)   # (the instrumented variant writes the contact row too: one env, one launch, both records)
    obs, rew, term, trunc, info = env.step(torch.as_tensor(ctrl))
    kern = gpu_records(env, n, ['qacc', 'niter', 'nefc', 'ncon', 'efc_J', 'efc_R', 'efc_aref'])
    assert all('contacts' in k for k in kern)
    tally = ParityTally(cone, 3e-7, shapes=Shapes(env._mm))
    nself = ncross = 0
    leg = lambda b: (b - 2) // 3 if b >= 2 else -1
    ea, ev = [], []
    for e in range(n):
        # (over the budget: held to the prefix rule like everywhere else, and reported to the caller; the observables of SELF_STEP_GPU: robot-robot
        # contacts set no foot contact state and no termination.  An env whose contact POINTS alone are undecided - two flat faces of CAD hulls, a
        # cylinder rim on a box: up to 60 % on b2 / hyqreal1 - has its list held contact by contact and is compared like an 'ok' env against the
        # oracle that took the kernel's points: ParityTally.step_env_with_list)
        k = kern[e]
        if tally.step_env(e, o, (qpos[e], qvel[e], warm[e], np.zeros(18), 0.0, 0.8), ctrl[e], k, sp.SELF_STEP_GPU, prefix=True, cmd=cmd[e]) not in sp.COMPARED:
            continue
        b1, b2 = o.get('contact_body1').astype(int), o.get('contact_body').astype(int)
        nself += int((b1 > 0).any()); ncross += int(any(x > 0 and leg(x) >= 0 and leg(x) != leg(y) for x, y in zip(b1, b2)))
        ea.append(np.abs(k['qacc'] - o.qacc).max() / max(1.0, np.abs(o.qacc).max()))
        ev.append(np.abs(k['qvel'] - o.qvel).max() / max(1.0, 0.002 * np.abs(o.qacc).max()))   # relative to the step's velocity change once that exceeds 1
        # deeply interpenetrating random states reach |qacc| of 1e5 rad/s^2: the position error is dt^2 times the (relative) qacc error
        assert np.abs(k['qpos'] - o.qpos).max() < 3.5e-6 + 4e-6 * (2e-4 if cone else 2e-5) * max(1.0, np.abs(o.qacc).max())
    p99 = lambda x: float(np.percentile(x, 99))
    assert p99(ea) < (1e-4 if cone else 2e-5) * 5 and max(ea) < 2e-3, (p99(ea), max(ea))
    assert p99(ev) < (7e-4 if cone else 5e-5) * 5 and max(ev) < 5e-3, (p99(ev), max(ev))
    # at least 0.9 n envs compared by value ('ok' ones and the ones held by substitution; the oracle alone classes 0.93 - 0.98 of these draws so), at
    # most 0.03 n left out for a capped convex pair or a vertex tie that changed a manifold (the oracle alone: at most 2 of 160), no mismatch
    tally.finish_held(f'self-collision one-step parity {robot}', min_checked=0.75, max_uncompared=0.03, max_budget=0.1, min_compared=0.9,
                      max_normal_tie=sp.GO1_NORMAL_TIES if robot == 'go1' else 0.0)
    compared = tally.checked + tally.point_held + tally.tie_held
    assert nself >= 0.9 * compared and ncross >= 0.25 * compared, (nself, ncross, compared)


@pytest.mark.parametrize('robot', ['go1', 'spot', 'b2'])
def test_newton_ends_on_captured_hard_states(robot):
    """The captured go1 states of tests/golden/newton_stagnation_go1.npz (see the emulated twin of this test): the solve
    ends far below the iteration cap, at the oracle's solution."""
    z = sp.hard_states(robot)
    n = len(z['qpos'])
    env = _make_env(n, solver='newton', iters=100, tol=1e-8, robot=robot)
    env.reset(qpos=z['qpos'], qvel=z['qvel'])
    env._qpos.copy_(torch.as_tensor(z['qpos'])); env._qvel.copy_(torch.as_tensor(z['qvel']))
    env._warm.copy_(torch.as_tensor(z['warm'])); env._applied.copy_(torch.as_tensor(z['applied'])); env._time.zero_()
    env._friction.copy_(torch.as_tensor(z['friction']))
    env.enable_debug(n)
    env.step(torch.as_tensor(z['ctrl']))
    torch.cuda.synchronize()
    sp.hold_hard_states(z, _oracle(env), env.debug_internals(n, ['niter', 'qacc']))


@pytest.mark.parametrize('robot,scene', [('mini_cheetah', 'flat'), ('go2', 'flat'), ('aliengo', 'flat'), ('hyqreal1', 'flat'), ('b2', 'flat'),
                                         ('go1', 'flat'), ('aliengo', 'perlin'), ('hyqreal1', 'random_boxes')])   # BASELINE configs 2-5 (+ b2, go1)
def test_step_parity_on_benchmark_rollout_states(robot, scene):
    """One-step parity on the states the BENCHMARK visits (random torques 50 N(0,1), auto-reset, 120 steps in: robots falling,
    lying, tangled - the distribution the random-state tests do not draw): a sample of envs is stepped by the kernel and by
    the fp64 oracle from the same (qpos, qvel, friction, ctrl); contact sets must agree (0 mismatches), qacc within the
    one-step tolerances of the report."""
    n, nsample = 1024, 160
    env = _make_env(n, solver='newton', iters=100, tol=1e-8, robot=robot, scene=scene, auto_reset='next_step', accessors=True)   # (the contact row: extra outputs,
    env.reset(random=True)                                                                                                         #  every contact still played - 'dropped' below)
    g = torch.Generator(device='cuda').manual_seed(3)
    for _ in range(120):
        env.step(torch.randn(n, 12, generator=g, device='cuda') * 50)
    pend = env._terminated.cpu().numpy().astype(bool)          # these envs spend the next launch on their auto-reset
    idx = np.where(~pend)[0][:nsample]
    qpos, qvel = env._qpos.cpu().numpy().copy(), env._qvel.cpu().numpy().copy()
    warm, app, fr = env._warm.cpu().numpy().copy(), env._applied.cpu().numpy().copy(), env._friction.cpu().numpy().copy()
    a = torch.randn(n, 12, generator=g, device='cuda') * 50
    env.enable_debug(n)
    env.step(a)
    ctrl = a.cpu().numpy()
    d = gpu_records(env, int(idx.max()) + 1, ['qacc', 'nefc', 'ncon', 'niter', 'efc_J', 'efc_R', 'efc_aref'])
    o = _oracle(env)
    cone = env.mjModel.cone == 1
    assert all('contacts' in d[e] for e in idx)
    tally = ParityTally(cone, 3e-7 if scene == 'flat' else 3e-6, shapes=Shapes(env._mm))
    ea, ev, nit = [], [], []
    for e in idx:
        cls = tally.step_env(e, o, (qpos[e], qvel[e], warm[e], app[e], 0.0, float(fr[e])), ctrl[e], d[e], sp.CONTACT_COUNT)
        if cls == 'budget':
            tally.check_budget_prefix(e, o, d[e])
        if cls not in sp.COMPARED:
            continue
        assert d[e]['dropped'] == 0   # the benchmark's states are played with every contact
        ea.append(np.abs(d[e]['qacc'] - o.qacc).max() / max(1.0, np.abs(o.qacc).max()))
        ev.append(np.abs(d[e]['qvel'] - o.qvel).max() / max(1.0, 0.002 * np.abs(o.qacc).max()))
        nit.append((int(d[e]['niter'][0]), o.solver_niter))
    p99 = lambda x: float(np.percentile(x, 99))
    tally_note(f'benchmark-state errors {robot} {scene}: qacc rel p50 {np.median(ea):.2e} p99 {p99(ea):.2e} max {max(ea):.2e}; qvel p99 {p99(ev):.2e} max {max(ev):.2e}; '
          f'niter kernel mean {np.mean([x[0] for x in nit]):.2f} oracle {np.mean([x[1] for x in nit]):.2f}')
    assert p99(ea) < (1e-4 if cone else 2e-5) and max(ea) < 2e-3, (p99(ea), max(ea))
    assert p99(ev) < (7e-4 if cone else 5e-5) and max(ev) < 5e-3, (p99(ev), max(ev))
    # measured on MI355X (profiles/r03_parity_tallies.txt): 0 of 160 over the row budget for every robot on flat; ties only on
    # hull robots.  A regression that drops contacts shows up as budget / mismatch counts far above these bounds.
    tally.finish_held(f'benchmark-state one-step parity {robot} {scene}', min_checked=0.85, max_uncompared=0.12, max_budget=0.03, min_compared=0.85)


@pytest.mark.parametrize('mode', ['step', 'rollout', 'spot_boxes', 'sharded'])
def test_pair_exchange_is_bit_identical(mode):
    """The convex pair exchange (csrc/gq_exchange.h): wavefronts of one launch compute each other's hull pairs.  4096 mini_cheetah envs under
    random torques without auto-reset - robots fall, fold up and stay that way: the state distribution with the most entangled envs -
    stepped with the exchange on and off end in bit-identical states, through the step loop and through the persistent rollout (one launch:
    slots are reserved, freed and reused step after step).  The heavy launches also have to END: nothing in the protocol may wait for ever.
    'spot_boxes': the world-box kernel variant (the convex block is compiled as an unlikely region there) with a mesh robot on random_boxes and
    the in-kernel auto-reset; 'sharded': the pipelined rollout - two shards' launches overlap on two streams and share the batch's table."""
    n, steps = (4096, 300) if mode in ('step', 'rollout') else (2048, 150)
    kw = dict(robot='spot', scene='random_boxes', auto_reset='next_step') if mode == 'spot_boxes' else dict(auto_reset=False)
    g = torch.Generator(device='cuda:0').manual_seed(5)
    acts = torch.randn(steps, n, 12, generator=g, device='cuda:0') * 40
    out = []
    for on in (True, False):
        env = _make_env(n, obs=('qpos', 'qvel'), iters=100, tol=1e-8, solver='newton', pair_exchange=on, **kw)
        assert env._mm.self_collision == 'convex'
        env.reset(random=True)
        if mode in ('step', 'spot_boxes'):
            for k in range(steps):
                env.step(acts[k])
        else:
            env.rollout(acts, shards=0 if mode == 'rollout' else 2)
        torch.cuda.synchronize()
        out.append((env.qpos.clone(), env.qvel.clone(), env._contacts_dropped.clone()))
        env.close()
    assert torch.isfinite(out[0][0]).all()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])


@pytest.fixture(scope='module')
def first_step_notes():
    """the measured lines of the first-step test, merged into the device probe's report when the module is done (one line per configuration)"""
    notes = []
    yield notes
    if notes:
        try:
            nfs.merge_report(os.environ.get('GQ_PROBE_REPORT', str(ROOT / 'profiles' / 'device_probe_report.txt')), notes)
        except OSError:   # a read-only checkout: the lines are printed and in the tally file
            pass


@pytest.mark.parametrize('robot,kind', nfs.CONFIGS)
def test_first_newton_step_solves_the_exact_hessian(robot, kind, first_step_notes):
    """One Newton iteration on the GPU (solver_iterations=1; tests/newton_first_step.py): qacc - qacc_smooth solves H d = -alpha g for the float64
    Hessian of the kernel's own rows - what the converged minimiser of the parity tests above does not depend on."""
    o = nfs.oracle_for(robot)
    qpos, qvel, ctrl = nfs.draw_states(robot, kind, o)
    n = len(qpos)
    env = _make_env(n, iters=1, tol=1e-8, solver='newton', robot=robot)
    env._qpos.copy_(torch.as_tensor(qpos)); env._qvel.copy_(torch.as_tensor(qvel)); env._warm.zero_(); env._friction.fill_(nfs.FRICTION)
    env.enable_debug(n)
    env.step(torch.as_tensor(ctrl))
    kern = gpu_records(env, n, nfs.NAMES)
    env.close()
    nfs.hold_first_step(robot, kind, o, qpos, qvel, ctrl, kern, 'GPU', notes=first_step_notes)
