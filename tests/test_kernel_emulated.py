"""The UNMODIFIED HIP kernel bodies (csrc/gq_step_body.h) executed by the host SIMT emulator (tests/simt_emu) against
the CPU oracle: same parity contract as tests/test_gpu_parity.py, runnable without a GPU."""
from pathlib import Path
import ctypes as C
import numpy as np
import pytest

from helpers import ALL_OBS, dbg, oracle_fits_row_budget, default_reset_cfg, emu_reset, emu_step, marshalled, oracle_fits_self_budget, oracle_reset_lift, random_states, self_contact_states, split_obs
import newton_first_step as nfs
import step_parity as sp
from contact_list import Shapes
from step_parity import ParityTally, emu_record
from oracle.oracle import Oracle
from philox_ref import draws


def test_step_stagewise_and_obs():
    n = 24
    mm = marshalled('mini_cheetah', solver=0, iterations=30, tolerance=0.0)
    rng = np.random.default_rng(11)
    qpos, qvel = random_states(mm.md, n, rng)
    qvel = qvel.astype(np.float32)
    warm = rng.normal(0, 5, (n, 18)).astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 40).astype(np.float32)   # beyond ctrlrange: exercises the clamp
    cmd = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    fric = np.where(np.arange(n) % 2 == 0, -1.0, 0.55).astype(np.float32)
    lo = (2, 0, 3, 1)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), warm=warm.copy(), cmd=cmd, friction=fric, legs_order=lo, debug_envs=n)
    o = Oracle(mm)
    ncon_total = 0
    for e in range(n):
        o.set_state(qpos[e], qvel[e], warm[e], np.zeros(18), 0.0, float(fric[e]))
        o.step(ctrl[e].astype(np.float64))
        if sp.has_tie(o, 3e-7):
            continue
        rec = st['debug'][e]
        ne = o.nefc
        if not oracle_fits_row_budget(o, False):   # (a robot pressed into the floor: its mesh manifolds exceed the kernel's 12 contacts / 63 rows; the budget tests hold those to the prefix rule)
            assert int(dbg(rec, 'nefc')[0]) < ne
            continue
        ncon_total += o.ncon
        assert int(dbg(rec, 'nefc')[0]) == ne and int(dbg(rec, 'ncon')[0]) == o.ncon
        np.testing.assert_allclose(dbg(rec, 'M').reshape(18, 18), o.M, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(dbg(rec, 'qfrc_bias'), o.qfrc_bias, rtol=1e-5, atol=5e-4)
        sp.compare(o, emu_record(st, e), sp.EMU_STAGE_ROWS, e)
        fmax = max(1.0, np.abs(o.efc_force).max())
        assert np.abs(dbg(rec, 'efc_force')[:ne] - o.efc_force).max() < 1e-4 * fmax
        assert np.abs(dbg(rec, 'qacc') - o.qacc).max() < 2e-5 * max(1.0, np.abs(o.qacc).max())
        assert np.abs(st['qvel'][e] - o.qvel).max() < 5e-5
        assert np.abs(st['qpos'][e] - o.qpos).max() < 1e-6
        ref, term, inv = o.get_obs(ALL_OBS, cmd[e], lo)
        got = split_obs(st['obs'][e], ALL_OBS)
        for k in ALL_OBS:
            assert np.abs(got[k] - ref[k]).max() < 2e-4 * max(1.0, np.abs(ref[k]).max()), (e, k)
        assert bool(st['terminated'][e]) == term and bool(st['invalid'][e]) == inv
        assert st['step_num'][e] == 1 and abs(st['time'][e] - 0.002) < 1e-9 and st['reward'][e] == 0
    assert ncon_total > 30


def test_mask_leaves_other_envs_untouched():
    mm = marshalled('mini_cheetah', iterations=5)
    rng = np.random.default_rng(2)
    qpos, qvel = random_states(mm.md, 4, rng)
    q0, v0 = qpos.copy(), qvel.astype(np.float32).copy()
    st = emu_step(mm, np.zeros((4, 12)), qpos, qvel, mask=[1, 0, 0, 1])
    assert np.array_equal(st['qpos'][1], q0[1]) and np.array_equal(st['qvel'][2], v0[2])
    assert not np.array_equal(st['qpos'][0], q0[0]) and st['step_num'].tolist() == [1, 0, 0, 1]


def test_out_of_bounds_terminates_far_from_origin_in_f64():
    """Base x/y are carried in f64: 1 mm steps at |x| = 9999.9995 m are resolved and the terrain limit trips."""
    mm = marshalled('mini_cheetah', iterations=5)
    q = np.tile(mm.md.key_qpos[0], (2, 1)); q[:, 2] = 1.0
    q[0, 0] = 9999.9995; q[1, 0] = 9999.0
    v = np.zeros((2, 18), np.float32); v[:, 0] = 0.5
    st = emu_step(mm, np.zeros((2, 12)), q, v)
    assert abs(st['qpos'][0, 0] - (9999.9995 + 0.002 * 0.5)) < 1e-9
    assert st['terminated'].tolist() == [1, 0]


def test_reset_kernel_stream_lift_and_bookkeeping():
    mm = marshalled('mini_cheetah', terrain_limits=(5, -5, 5, -5))
    seed = 987654321987
    cfg = default_reset_cfg(seed=seed, lin=(0.5, 1.0), ang=(-0.3, 0.3), fric=(0.2, 1.5), cmd='random+rotate')
    n = 6
    st = emu_reset(mm, n, cfg, episode=np.arange(n))
    o = Oracle(mm)
    key = mm.md.key_qpos[0]
    for e in range(n):
        u = draws(seed, e, e)
        np.testing.assert_allclose(st['qpos'][e, 7:], key[7:] + (2 * u[0:12] - 1) * np.float32(20 * np.pi / 180), atol=1e-6)
        np.testing.assert_allclose(st['qvel'][e, 6:], (2 * u[12:24] - 1) * 0.5, atol=1e-6)
        assert abs(st['qpos'][e, 0] - (5 - 10 * float(u[24]))) < 1e-9 and abs(st['qpos'][e, 1] - (5 - 10 * float(u[25]))) < 1e-9
        norm, head = 0.5 + 0.5 * u[28], (2 * u[29] - 1) * np.pi
        np.testing.assert_allclose(st['cmd'][e], [norm * np.cos(head), norm * np.sin(head), 0, -0.3 + 0.6 * u[30]], atol=1e-5)
        assert abs(st['friction_next'][e] - (0.2 + 1.3 * u[31])) < 1e-6
        assert st['episode'][e] == e + 1 and st['step_num'][e] == -1 and st['time'][e] == 0
        assert not st['qacc'][e].any() and not st['warm'][e].any() and not st['applied'][e].any()
        # flat scene: the reset kernel writes the spawn pose at hip height and leaves word that the lift loop is due; it
        # runs inside the reset's own mj_step (below)
        assert st['lift_pending'][e] == 1 and abs(st['qpos'][e, 2] - 0.225) < 1e-7
    spawn_q, spawn_v = st['qpos'].copy(), st['qvel'].copy()
    st1 = emu_step(mm, np.zeros((n, 12)), st['qpos'], st['qvel'], warm=st['warm'], applied=st['applied'], time=st['time'],
                   cmd=st['cmd'], step_num=st['step_num'], episode=st['episode'], first_pass=1, lift_pending=st['lift_pending'],
                   friction_next=st['friction_next'], obs_names=['qpos', 'feet_pos'])
    nlift = 0
    for e in range(n):
        # lift loop on the oracle (the reference's rule), then the reset's mj_step from the lifted pose
        z, it = oracle_reset_lift(o, spawn_q[e], spawn_v[e].astype(np.float64), 0.225)
        nlift += it > 0
        q0 = spawn_q[e].copy(); q0[2] = z
        o.set_state(q0, spawn_v[e].astype(np.float64), np.zeros(18), np.zeros(18), 0.0, -1.0); o.step(np.zeros(12))
        assert not st1['lift_failed'][e] and st1['step_num'][e] == 0
        assert np.abs(st1['qpos'][e] - o.qpos).max() < 1e-6 and np.abs(st1['qvel'][e] - o.qvel).max() < 5e-5, (e, it)
        ref, _, _ = o.get_obs(['feet_pos'])
        assert np.abs(split_obs(st1['obs'][e], ['qpos', 'feet_pos'])['feet_pos'] - ref['feet_pos']).max() < 2e-5   # old kinematics AT THE LIFTED POSE
        assert abs(st1['friction'][e] - st['friction_next'][e]) < 1e-9      # committed after the reset's step (:403-404)
    assert nlift > 0
    # explicit state: copied verbatim, no lift
    qn = np.tile(key, (2, 1)); qn[:, 2] = 0.05
    st2 = emu_reset(mm, 2, cfg, qpos_new=qn, qvel_new=np.ones((2, 18), np.float32))
    assert np.array_equal(st2['qpos'], qn) and np.all(st2['qvel'] == 1)


def test_imu_truth_noise_and_bias_walk():
    """IMU observables out of the step kernel: ground truth == oracle's mj_sensorAcc/Vel restatement, noise and bias
    random walk == the documented Philox normal stream (tests/philox_ref.py), draw order of sensors/imu.py:110-139."""
    import ctypes as C
    from helpers import IMU_OBS, GqImuCfg
    from philox_ref import imu_normals
    mm = marshalled('aliengo', solver=1, iterations=100, tolerance=1e-8)
    o = Oracle(marshalled('aliengo', solver=1, iterations=100, tolerance=1e-12))
    pos, quat = (0.05, -0.02, 0.03), np.array([0.9, 0.1, -0.3, 0.2])
    quat = quat / np.linalg.norm(quat)
    o.set_imu(pos, quat)
    imu = GqImuCfg(site_pos=(C.c_double * 3)(*pos), site_quat=(C.c_double * 4)(*quat), accel_noise=0.01, gyro_noise=0.02,
                   accel_bias_rate=0.03, gyro_bias_rate=0.04, seed=777)
    rng = np.random.default_rng(5)
    n = 8
    qpos, qvel = random_states(mm.md, n, rng, z_range=(0.3, 0.5))
    qvel = qvel.astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    b0 = rng.normal(0, 0.1, (n, 6)).astype(np.float32)
    names = ['qpos'] + list(IMU_OBS)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), obs_names=names, imu=imu, imu_bias=b0.copy(), step_num=np.arange(n) + 10,
                  episode=np.arange(n))
    compared = 0
    for e in range(n):
        o.set_state(qpos[e], qvel[e], np.zeros(18), np.zeros(18), 0, -1)
        o.step(ctrl[e].astype(np.float64))
        if not oracle_fits_self_budget(o, mm.md.cone):
            continue   # more contacts than one wavefront's rows: the accelerations differ by construction
        compared += 1
        got = split_obs(st['obs'][e], names)
        z = imu_normals(777, e, 10 + e, e)
        an, ab, gn, gb = z[0:3] * 0.01, b0[e, :3] + z[3:6] * 0.03, z[6:9] * 0.02, b0[e, 3:] + z[9:12] * 0.04
        tol = 2e-5 * max(1.0, np.abs(o.imu_acc).max())
        assert np.abs(got['imu_acc'] - (o.imu_acc + ab + an)).max() < tol
        assert np.abs(got['imu_gyro'] - (o.imu_gyro + gb + gn)).max() < 1e-5
        np.testing.assert_allclose(got['imu_acc_noise'], an, atol=1e-7); np.testing.assert_allclose(got['imu_gyro_noise'], gn, atol=1e-7)
        np.testing.assert_allclose(got['imu_acc_bias'], ab, atol=1e-6); np.testing.assert_allclose(got['imu_gyro_bias'], gb, atol=1e-6)
        np.testing.assert_allclose(st['imu_bias'][e], np.r_[ab, gb], atol=1e-6)
    assert compared >= n // 2
    # free fall: the accelerometer reads zero (and +g once something holds the base still: a = 0 -> reading = -gravity)
    mm2 = marshalled('aliengo', solver=1)
    o2 = Oracle(mm2)
    q = mm2.md.key_qpos[0].copy(); q[2] = 2.0
    o2.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18))
    o2.forward(np.zeros(12))
    assert np.abs(o2.imu_acc).max() < 1e-9 and np.abs(o2.imu_gyro).max() == 0
    hold = np.zeros(18); hold[2] = mm2.md.total_mass * 9.81          # external force cancelling the weight
    o2.set_state(q, np.zeros(18), np.zeros(18), hold)
    o2.forward(np.zeros(12))
    assert np.abs(o2.imu_acc - [0, 0, 9.81]).max() < 0.5               # legs still sag, the base barely moves


def test_auto_reset_same_step_and_next_step_agree():
    """A terminated env (base out of bounds) is re-spawned either inside the same launch (second pass) or by its next
    launch (gymnasium NEXT_STEP): both run reset_wave + the reset's own mj_step on the same RNG counters, so the state
    after 'step' (same-step) equals the state after 'step, step' (next-step); the untouched env just steps."""
    mm = marshalled('mini_cheetah', iterations=20, terrain_limits=(5, -5, 5, -5))
    q = np.tile(mm.md.key_qpos[0], (2, 1)); q[:, 2] = 0.6
    q[0, 0] = 5.5    # env 0 is outside the terrain -> terminates
    v = np.zeros((2, 18), np.float32)
    ctrl = np.ones((2, 12), np.float32)
    epi = np.array([3, 4], np.int32)
    cfg_same = default_reset_cfg(seed=77, fric=(0.3, 0.9))
    cfg_next = default_reset_cfg(seed=77, fric=(0.3, 0.9)); cfg_next.autoreset_next_step = 1
    a = emu_step(mm, ctrl, q.copy(), v.copy(), auto_reset=cfg_same, episode=epi.copy())
    assert a['terminated'].tolist() == [1, 0] and a['episode'].tolist() == [4, 4] and a['pending'].tolist() == [0, 0]
    assert a['step_num'].tolist() == [0, 1] and abs(a['qpos'][0, 0]) <= 5.0
    b1 = emu_step(mm, ctrl, q.copy(), v.copy(), auto_reset=cfg_next, episode=epi.copy())
    assert b1['terminated'].tolist() == [1, 0] and b1['pending'].tolist() == [1, 0] and b1['episode'].tolist() == [3, 4]
    assert abs(b1['qpos'][0, 0] - 5.5) < 1e-4 and b1['step_num'].tolist() == [1, 1]      # terminal state / observation kept
    np.testing.assert_array_equal(b1['qpos'][1], a['qpos'][1])
    q1_prev = b1['qpos'][1].copy()   # emu_step updates the arrays in place
    b2 = emu_step(mm, ctrl, b1['qpos'], b1['qvel'], warm=b1['warm'], time=b1['time'], friction=b1['friction'], cmd=b1['cmd'],
                  auto_reset=cfg_next, episode=b1['episode'], pending=b1['pending'], step_num=b1['step_num'])
    assert b2['terminated'].tolist() == [0, 0] and b2['pending'].tolist() == [0, 0] and b2['episode'].tolist() == [4, 4]
    assert b2['step_num'].tolist() == [0, 2]
    for k in ('qpos', 'qvel', 'warm', 'time', 'friction', 'cmd'):
        np.testing.assert_array_equal(b2[k][0], a[k][0], err_msg=k)   # same draws, same reset step: bit-identical
    np.testing.assert_array_equal(b2['obs'][0], a['obs'][0])
    assert not np.array_equal(b2['qpos'][1], q1_prev)          # env 1 kept stepping with the user's control


@pytest.mark.parametrize('robot', ['hyqreal1', 'go2'])
def test_elliptic_cone_step_matches_converged_oracle(robot):
    """Elliptic friction cones (cone="elliptic", impratio 100; go2 feet are condim 6: torsional + rolling rows): rows,
    regularisation and the Newton solution of the kernel against the fp64 oracle converged to 1e-12."""
    n = 24
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-8, noise_floor=1e-5)
    mmN = marshalled(robot, solver=1, iterations=200, tolerance=1e-13)
    rng = np.random.default_rng(5)
    hip = float(mm.desc.key_qpos[2])
    qpos, qvel = random_states(mm.md, n, rng, z_range=(0.9 * hip, 1.2 * hip))   # feet and a few links down; a robot lying
    qvel = qvel.astype(np.float32)                                               # flat exceeds the 64-row budget (and is terminated)
    warm = rng.normal(0, 3, (n, 18)).astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    fric = np.where(np.arange(n) % 2 == 0, -1.0, 0.6).astype(np.float32)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), warm=warm.copy(), friction=fric.copy(), debug_envs=n)
    o = Oracle(mmN)
    ncon = 0
    tally = ParityTally(cone=True, tie_threshold=3e-7)
    for e in range(n):
        if tally.step_env(e, o, (qpos[e], qvel[e], warm[e], np.zeros(18), 0.0, float(fric[e])), ctrl[e], emu_record(st, e), sp.ELLIPTIC_STEP) == 'ok':
            ncon += o.ncon
    # go2: 12 friction-loss rows + four condim-6 feet (6 rows + 5 reserved virtual rows each) leave 8 of the 64 slots
    tally.finish(f'elliptic {robot}', min_checked=0.4, max_tie=0.1, max_budget=0.6)
    assert ncon >= tally.checked


def test_divergence_guard_freezes_and_flags_the_env():
    """mj_checkAcc analogue: a state whose acceleration is not finite must not propagate NaN - the env keeps a finite state,
    and is flagged terminated + truncated (so that an auto-resetting batch re-spawns it); healthy envs are untouched."""
    mm = marshalled('mini_cheetah', solver=1, iterations=20)
    q = np.tile(mm.md.key_qpos[0], (2, 1)); q[:, 2] = 0.6
    v = np.zeros((2, 18), np.float32); v[0, 8] = np.float32(3e19)      # absurd joint velocity -> Coriolis terms overflow
    st = emu_step(mm, np.zeros((2, 12)), q, v)
    assert st['terminated'].tolist() == [1, 0] and st['truncated'].tolist() == [1, 0]
    assert np.isfinite(st['qpos']).all() and np.isfinite(st['qacc']).all()
    assert np.isfinite(st['qvel'][1]).all() and np.isfinite(st['obs'][1]).all()


def _random_boxes_scene(hip):
    from gym_quadruped_amd.terrain import generate_terrain
    return generate_terrain('random_boxes', hip, seed=10)


@pytest.mark.parametrize('robot', ['aliengo', 'hyqreal1'])   # pyramidal / elliptic cones (go2's condim-6 feet + 27 link geoms
def test_world_boxes_step_matches_oracle(robot):                # exhaust the 64-row budget when it sinks into a box field)
    """BOXES kernel variant on the reference's random_boxes scene (100 tilted boxes, seed 10): rows, frames and the Newton
    solution against the fp64 oracle, robots dropped over the box field; plus the raised-floor identity (a wide slab
    under the robot == the floor plane that much lower, bit-for-bit the same rows)."""
    from gym_quadruped_amd.robot_cfgs import get_robot_config
    hip = get_robot_config(robot).hip_height
    scene, lim = _random_boxes_scene(hip)
    kw = dict(solver=1, iterations=100)
    mm = marshalled(robot, tolerance=1e-8, noise_floor=1e-5, boxes=scene['boxes'], **kw)
    mmN = marshalled(robot, tolerance=1e-13, boxes=scene['boxes'], **kw)
    rng = np.random.default_rng(12)
    n = 16
    qpos, qvel = random_states(mm.md, n, rng, z_range=(0.75 * hip, 1.05 * hip))
    # over the box field (boxes start at x ~ 0.5 + 2 hip, y ~ -3 .. +3 hip-scaled): sample xy inside the spawn limits
    qpos[:, 0] = rng.uniform(0.5 + 2 * hip, 0.5 + 10 * hip, n); qpos[:, 1] = rng.uniform(-3 + 2 * hip, -3 + 12 * hip, n)
    qpos[:, 2] += 0.25 * hip    # the boxes are slabs of height ~hip/2 centred 2 cm above the floor: tops at ~hip/4
    qvel = qvel.astype(np.float32)
    warm = rng.normal(0, 3, (n, 18)).astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), warm=warm.copy(), debug_envs=n)
    o = Oracle(mmN)
    nbox_con = 0
    tally = ParityTally(mm.md.cone == 1, 3e-6, lenient_rows=True)
    for e in range(n):
        if tally.step_env(e, o, (qpos[e], qvel[e], warm[e], np.zeros(18)), ctrl[e], emu_record(st, e), sp.TERRAIN_NEWTON_STEP, mass=mm.md.total_mass) == 'ok':
            nbox_con += int((np.abs(o.contact_frame[:, 0, 2] - 1.0) > 1e-6).sum()) if o.ncon else 0
    tally.finish_count(f'emulated world boxes {robot}', n // 2)
    assert nbox_con >= 4, nbox_con


@pytest.mark.parametrize('robot', ['aliengo', 'hyqreal1'])   # primitives / hulls (the general convex routine) against tilted world boxes
def test_world_box_contact_lists_match_oracle(robot):
    """The contact row on the random_boxes scene, contact by contact under the strict rule (contact_list.hold_contact_list): world boxes as the first
    geom (geom1 = -1 with a normal that is not vertical), floor, box and robot-robot contacts in one list, frames made from computed normals, the
    point of every contact - a face of a hull lying on a box is held to the contact feature and compared after substitution - and mj_contactForce."""
    from gym_quadruped_amd.robot_cfgs import get_robot_config
    hip = get_robot_config(robot).hip_height
    scene, lim = _random_boxes_scene(hip)
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-8, noise_floor=1e-5, boxes=scene['boxes'])
    o = Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-13, boxes=scene['boxes']))
    rng = np.random.default_rng(12)
    n = 12
    qpos, qvel = random_states(mm.md, n, rng, z_range=(0.75 * hip, 1.05 * hip))
    qpos[:, 0] = rng.uniform(0.5 + 2 * hip, 0.5 + 10 * hip, n); qpos[:, 1] = rng.uniform(-3 + 2 * hip, -3 + 12 * hip, n)
    qpos[:, 2] += 0.25 * hip
    qvel = qvel.astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n, rows=True)
    tally = ParityTally(mm.md.cone == 1, 3e-6, shapes=Shapes(mm))
    tilted = 0
    for e in range(n):
        if tally.step_env(e, o, (qpos[e], qvel[e], np.zeros(18), np.zeros(18)), ctrl[e], emu_record(st, e, contacts=True), sp.TERRAIN_NEWTON_STEP, mass=mm.md.total_mass) in sp.COMPARED:
            tilted += int(((o.get('contact_geom1') < 0) & (np.abs(o.contact_frame[:, 0, 2] - 1.0) > 1e-6)).sum()) if o.ncon else 0
    msg = tally.report(f'emulated world-box contact lists {robot}')
    assert not tally.mismatch and tally.checked + tally.point_held + tally.tie_held >= n // 2 and tilted >= 4, (msg, tilted)


def test_pyramidal_cone_with_condim_6_is_refused():
    """The step's pyramid rows and the contact row's pyramid decode cover condim 1 and 3.  No robot model pairs a pyramidal cone with condim 4 or
    6 (torsional / rolling friction); a model that does is refused by the model builder instead of reporting a wrong contact force."""
    for robot in ('mini_cheetah', 'aliengo', 'go2', 'go1', 'hyqreal1', 'hyqreal2', 'b2', 'spot'):
        md = marshalled(robot, solver=1).md
        assert md.cone == 1 or max(int(c) for g, c in enumerate(md.geom_condim) if md.geom_cloudid[g] >= 0 and md.geom_bodyid[g] != 0) <= 3, robot
    mm = marshalled('aliengo', solver=1)
    q, v = random_states(mm.md, 1, np.random.default_rng(0))
    emu_step(mm, None, q.copy(), v.copy())
    g = next(g for g in range(mm.md.ngeom) if mm.md.geom_cloudid[g] >= 0 and mm.md.geom_bodyid[g] != 0)
    mm.desc.geom_condim[g] = 6
    with pytest.raises(RuntimeError, match='condim 6'):
        emu_step(mm, None, q.copy(), v.copy())


@pytest.mark.parametrize('robot', ['mini_cheetah', 'go1'])
def test_dynamics_row_matches_oracle(robot):
    """The dynamics row of gq_batch_set_outputs as the production kernel writes it (accessors=True): mj_fullM through the index map of
    AccessorsMixin._dense_mass, qfrc_bias, body xpos / xmat and the foot points against the oracle, at the tolerances of the aliengo check on
    the GPU (tests/test_gpu_parity.py::test_mpc_accessors_match_oracle)."""
    from gym_quadruped_amd.accessors import AccessorsMixin
    from gym_quadruped_amd.cabi import GQ_DYN
    from helpers import emu_window
    n = 4
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-8)
    o = Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-12))
    rng = np.random.default_rng(4)
    qpos, qvel = random_states(mm.md, n, rng)
    qvel = qvel.astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 10).astype(np.float32)
    st = emu_window(mm, ctrl[None], qpos.copy(), qvel.copy(), rows=True)
    assert not np.isnan(st['dyn'][:, :GQ_DYN['FOOT'] + 12]).any()

    class _Rows(AccessorsMixin):   # _dense_mass over the emulated rows: the map itself is the product's, not a copy
        def __init__(self, dyn):
            import torch
            self._dyn, self.num_envs, self.device = torch.as_tensor(dyn), len(dyn), 'cpu'
    M = _Rows(st['dyn'])._dense_mass().numpy().reshape(n, 18, 18)
    for e in range(n):
        o.set_state(qpos[e], qvel[e], np.zeros(18), np.zeros(18)); o.step(ctrl[e].astype(np.float64))
        row = st['dyn'][e].astype(np.float64)
        np.testing.assert_allclose(M[e], o.M, rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(row[GQ_DYN['BIAS']:GQ_DYN['BIAS'] + 18], o.qfrc_bias, rtol=1e-3, atol=2e-3)
        xpos = row[GQ_DYN['XPOS']:GQ_DYN['XPOS'] + 39].reshape(13, 3).copy()
        xpos[:, :2] += qpos[e, :2]   # (x / y of the row are relative to the pre-step base)
        np.testing.assert_allclose(xpos, o.xpos[1:14], atol=5e-6 * max(1.0, np.abs(o.xpos).max()))
        np.testing.assert_allclose(row[GQ_DYN['XMAT']:GQ_DYN['XMAT'] + 117].reshape(13, 3, 3), o.xmat[1:14], atol=1e-5)
        foot = row[GQ_DYN['FOOT']:GQ_DYN['FOOT'] + 12].reshape(4, 3).copy()
        foot[:, :2] += qpos[e, :2]
        ref, _t, _i = o.get_obs(['feet_pos'])
        np.testing.assert_allclose(foot.ravel(), ref['feet_pos'], atol=5e-6 * max(1.0, np.abs(ref['feet_pos']).max()))


@pytest.mark.parametrize('robot', ['hyqreal1', 'go2'])   # hulls, elliptic cones / primitives, condim 6
def test_production_and_instrumented_variants_write_the_same_rows(robot):
    """The production kernel (mode 0, what accessors=True runs) and the instrumented one (mode 1, what the parity tests read their records from)
    step from the same states: identical contact rows - list, frames, points, forces - and dynamics rows, bit for bit under the emulator, and
    the same next state."""
    from helpers import emu_window
    n = 8
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-8)
    o = Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-12))
    rng = np.random.default_rng(9)
    qpos, qvel = self_contact_states(mm.md, n, rng, o)
    qvel = qvel.astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    kw = dict(friction=np.full(n, 0.7, np.float32), rows=True)
    a = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n, **kw)
    b = emu_window(mm, ctrl[None], qpos.copy(), qvel.copy(), **kw)
    assert a['contacts'][:, 0].sum() >= n and not np.isnan(a['contacts'][:, :3]).any()
    for name in ('contacts', 'dyn', 'qpos', 'qvel', 'qacc'):
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)


@pytest.mark.parametrize('scene_name', ['random_boxes', 'flat'])
def test_pgs_with_world_boxes_and_self_collision_matches_oracle_pgs(scene_name):
    """PGS (the solver the north-star names) beyond the flat floor: world boxes + robot self-collision rows (pyramidal cones; aliengo's
    box / capsule link geoms take the exact pair routines).  The collision stages use the L'DL factors' LDS as scratch, so this variant
    factors after the rows are built and carries the contact normals across the solve in a register (gq_step_body.h S8): same rows as
    the Newton variant, and the force / acceleration of the oracle's PGS after the same number of sweeps."""
    from gym_quadruped_amd.robot_cfgs import get_robot_config
    robot = 'aliengo'
    hip = get_robot_config(robot).hip_height
    boxes = _random_boxes_scene(hip)[0]['boxes'] if scene_name == 'random_boxes' else None
    mm = marshalled(robot, solver=0, iterations=40, tolerance=0.0, boxes=boxes, self_collision=True)
    rng = np.random.default_rng(21)
    n = 24 if boxes is not None else 16
    qpos, qvel = random_states(mm.md, n, rng, z_range=(0.85 * hip, 1.15 * hip) if boxes is not None else (0.6 * hip, 1.0 * hip))
    if boxes is not None:   # (feet and a link or two on the boxes: a robot lying in the box field exceeds the 12-contact capacity, a case of its own)
        qpos[:, 0] = rng.uniform(0.5 + 2 * hip, 0.5 + 10 * hip, n); qpos[:, 1] = rng.uniform(-3 + 2 * hip, -3 + 12 * hip, n)
        qpos[:, 2] += 0.25 * hip
    if boxes is None:   # legs folded across each other: states in which the oracle finds robot-robot contacts, inside the row capacity
        qpos, qvel = self_contact_states(mm.md, n, rng, Oracle(marshalled(robot, solver=1, self_collision=True)), z=(0.9 * hip, 1.6 * hip), cone=0, max_over=0.0)
    qvel = qvel.astype(np.float32)
    warm = rng.normal(0, 3, (n, 18)).astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), warm=warm.copy(), debug_envs=n)
    o = Oracle(mm)
    nself = nworld = 0
    tally = ParityTally(False, 3e-6, lenient_rows=True)
    for e in range(n):   # (the contact force observables: S11 reads the contact normals that were parked in a register)
        if tally.step_env(e, o, (qpos[e], qvel[e], warm[e], np.zeros(18)), ctrl[e], emu_record(st, e), sp.TERRAIN_PGS_STEP, mass=mm.md.total_mass) == 'ok' and o.ncon:
            nworld += int((np.abs(o.contact_frame[:, 0, 2] - 1.0) > 1e-6).sum())
            nself += int((o.get('contact_body1')[:o.ncon] > 0).sum())
    tally.finish_count(f'emulated PGS {scene_name}', n // 2)
    if boxes is not None:
        assert nworld >= 4, nworld
    else:
        assert nself >= 1, nself


def test_world_box_slab_equals_raised_floor_in_the_kernel():
    from gym_quadruped_amd.terrain import _box
    H = 1.37
    slab = _box([0.0, 0.0, H - 1.0], [0.0, 0.0, 0.0], [12.0, 12.0, 2.0])
    # a hull robot without its hull graphs (see test_flat_height_field_equals_raised_floor_in_the_kernel): one point per geom on the floor - the
    # support vertex - and on a box - the convex routine's single contact, which is that vertex against the slab's top face
    mmF = marshalled('mini_cheetah', solver=1, iterations=100, tolerance=1e-8, mesh_graph=False)
    mmB = marshalled('mini_cheetah', solver=1, iterations=100, tolerance=1e-8, boxes=[slab], mesh_graph=False)
    rng = np.random.default_rng(3)
    n = 8
    qpos, qvel = random_states(mmF.md, n, rng, z_range=(0.18, 0.3))
    qvel = qvel.astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 10).astype(np.float32)
    a = emu_step(mmF, ctrl, qpos.copy(), qvel.copy(), debug_envs=n)
    qb = qpos.copy(); qb[:, 2] += H
    b = emu_step(mmB, ctrl, qb, qvel.copy(), debug_envs=n)
    seen = 0
    for e in range(n):
        na, nb = int(dbg(a['debug'][e], 'nefc')[0]), int(dbg(b['debug'][e], 'nefc')[0])
        assert na == nb
        seen += na > 12
        np.testing.assert_allclose(dbg(b['debug'][e], 'qacc'), dbg(a['debug'][e], 'qacc'), rtol=2e-4, atol=2e-4 * max(1.0, np.abs(dbg(a['debug'][e], 'qacc')).max()))
        np.testing.assert_allclose(b['qvel'][e], a['qvel'][e], atol=1e-4)
    assert seen >= 4


def test_reset_lifts_clear_of_world_boxes():
    """Reset on the random_boxes scene: spawn inside the scene's limits, then the reference's lift loop (:376-388) - here
    re-evaluating floor AND nearby boxes per iteration - must end with no foot-body geom touching anything."""
    from gym_quadruped_amd.robot_cfgs import get_robot_config
    hip = get_robot_config('aliengo').hip_height
    scene, lim = _random_boxes_scene(hip)
    mm = marshalled('aliengo', solver=1, terrain_limits=lim, boxes=scene['boxes'])
    cfg = default_reset_cfg(seed=4242, hip_height=hip)
    n = 12
    st = emu_reset(mm, n, cfg, episode=np.arange(n))
    o = Oracle(mm)
    lifted = nfailed = 0
    for e in range(n):
        assert lim[1] <= st['qpos'][e, 0] <= lim[0] and lim[3] <= st['qpos'][e, 1] <= lim[2]
        o.set_state(st['qpos'][e], st['qvel'][e].astype(np.float64), np.zeros(18), np.zeros(18)); o.forward(np.zeros(12), stage=1)
        bodies = o.get('contact_body') if o.ncon else []
        calf_touch = [c for c, bd in enumerate(bodies) if (int(bd) - 2) % 3 == 2]
        if st['lift_failed'][e]:
            # a foot leaving a box through a steep side face gains only 1.1 |dist| n_z per iteration: after the reference's
            # 100 iterations a hair of penetration is left and the reference raises RuntimeError (:387-388); here: the flag
            nfailed += 1
            assert calf_touch and np.abs(o.get('contact_dist')[calf_touch]).max() < 1e-3
        else:
            assert not calf_touch, 'a calf body still touches the floor or a box'
        lifted += st['qpos'][e, 2] > hip + 1e-4
    assert lifted >= 3 and nfailed <= 2   # some spawn poses did sit in a box


@pytest.mark.parametrize('robot', ['aliengo', 'hyqreal1'])   # pyramidal / elliptic cones
def test_perlin_height_field_step_matches_oracle(robot):
    """BOXES kernel variant on the reference's perlin scene (128 x 128 height field, terrain.py:345-356): contact rows,
    frames and the Newton solution against the fp64 oracle for robots dropped onto the hills."""
    from gym_quadruped_amd.robot_cfgs import get_robot_config
    from gym_quadruped_amd.terrain import generate_terrain
    hip = get_robot_config(robot).hip_height
    scene, lim = generate_terrain('perlin', hip)
    kw = dict(solver=1, iterations=100, hfield=scene['hfield'], terrain_limits=lim)
    mm = marshalled(robot, tolerance=1e-8, noise_floor=1e-5, **kw)
    mmN = marshalled(robot, tolerance=1e-13, **kw)
    rng = np.random.default_rng(21)
    n = 16
    qpos, qvel = random_states(mm.md, n, rng, z_range=(0.75 * hip, 1.05 * hip))
    qpos[:, 0:2] = rng.uniform(-0.7 * lim[0], 0.7 * lim[0], (n, 2))
    # terrain elevation under the base: put the robots at their drawn height above the local surface
    hf = scene['hfield']; data = np.asarray(hf['data'], float); sx, sy, sz, _ = hf['size']
    ci = np.clip(((qpos[:, 0] + sx) / (2 * sx) * (data.shape[1] - 1)).round().astype(int), 0, data.shape[1] - 1)
    ri = np.clip(((qpos[:, 1] + sy) / (2 * sy) * (data.shape[0] - 1)).round().astype(int), 0, data.shape[0] - 1)
    qpos[:, 2] += sz * data[ri, ci]
    qvel = qvel.astype(np.float32)
    warm = rng.normal(0, 3, (n, 18)).astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), warm=warm.copy(), debug_envs=n)
    o = Oracle(mmN)
    nhf_con = 0
    tally = ParityTally(mm.md.cone == 1, 3e-6, lenient_rows=True)
    for e in range(n):
        if tally.step_env(e, o, (qpos[e], qvel[e], warm[e], np.zeros(18)), ctrl[e], emu_record(st, e), sp.TERRAIN_NEWTON_STEP, mass=mm.md.total_mass) == 'ok':
            nhf_con += int((np.abs(o.contact_frame[:, 0, 2] - 1.0) > 1e-9).sum()) if o.ncon else 0
    tally.finish_count(f'emulated perlin {robot}', n // 2)
    assert nhf_con >= 8, nhf_con


@pytest.mark.parametrize('name', ['mild_coarse', 'rough_coarse', 'mild_fine', 'rough_fine'])
@pytest.mark.parametrize('robot', ['aliengo', 'hyqreal1'])   # primitive geoms, pyramidal cones / hulls, elliptic cones
def test_height_field_step_on_rough_fine_grids_matches_oracle(robot, name):
    """hfield_item_scan - the phase-A cull with hf_maxslope of non-square cells, the flattened and serial cloud passes, the 2 x 2 parallel foot
    form (coarse grids) and the serial one (fine grids), the grid's border, a grid far from the origin - on the grids of tests/hfield_cases.py
    under the STRICT row rule: an env whose row count differs from the oracle's without a tie or the budget explaining it fails the test."""
    import hfield_cases as hc
    hf = hc.grid(name)
    kw = dict(solver=1, iterations=100, hfield=hf, terrain_limits=hc.limits(hf, 0.0))
    mm = marshalled(robot, tolerance=1e-8, noise_floor=1e-5, **kw)
    mmN = marshalled(robot, tolerance=1e-13, **kw)
    hc.assert_foot_form(mm, hf, name, robot)
    rng = np.random.default_rng(31)
    n = 12
    o = Oracle(mmN)
    qpos, qvel = hc.step_states(mm, robot, name, n, rng, o)
    warm = rng.normal(0, 3, (n, 18)).astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), warm=warm.copy(), debug_envs=n)
    tally = ParityTally(mm.md.cone == 1, 3e-6)
    tot = np.zeros(3, int)
    for e in range(n):
        if tally.step_env(e, o, (qpos[e], qvel[e], warm[e], np.zeros(18)), ctrl[e], emu_record(st, e), sp.TERRAIN_NEWTON_STEP, mass=mm.md.total_mass) == 'ok':
            tot += hc.count_contacts(o, mm, hf)
    sp.tally_note(f'emulated {name} {robot}: height-field contacts {tot[0]} over {tally.checked} compared envs, {tot[1]} foot contacts on an edge or corner, {tot[2]} link-geom contacts')
    tally.finish_count(f'emulated {name} {robot}', n // 2)
    assert tot[0] >= 4 * tally.checked and tot[2] >= 1 and (tot[1] >= 1 or 'rough' not in name), tot


def test_flat_height_field_equals_raised_floor_in_the_kernel():
    H = 1.37
    flat = dict(data=np.zeros((17, 17), np.float32), size=(8.0, 8.0, 1.0, 0.01), pos=(0.0, 0.0, H))
    # a hull robot: its geoms meet the plane and the height field alike in ONE point (the primitive geoms of aliengo take the
    # multi-point plane routines on the floor and the single-point cloud rule on a height field)
    # (mesh_graph off: with its hull graph a mesh brings up to three points to the floor, mjc_PlaneConvex's neighbour walk, and still one to the height field)
    mmF = marshalled('mini_cheetah', solver=1, iterations=100, tolerance=1e-8, mesh_graph=False)
    mmH = marshalled('mini_cheetah', solver=1, iterations=100, tolerance=1e-8, hfield=flat, mesh_graph=False)
    rng = np.random.default_rng(3)
    n = 8
    qpos, qvel = random_states(mmF.md, n, rng, z_range=(0.18, 0.3))
    qvel = qvel.astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 10).astype(np.float32)
    a = emu_step(mmF, ctrl, qpos.copy(), qvel.copy(), debug_envs=n)
    qb = qpos.copy(); qb[:, 2] += H
    b = emu_step(mmH, ctrl, qb, qvel.copy(), debug_envs=n)
    seen = 0
    for e in range(n):
        na, nb = int(dbg(a['debug'][e], 'nefc')[0]), int(dbg(b['debug'][e], 'nefc')[0])
        assert na == nb
        seen += na > 12
        np.testing.assert_allclose(dbg(b['debug'][e], 'qacc'), dbg(a['debug'][e], 'qacc'), rtol=2e-4, atol=2e-4 * max(1.0, np.abs(dbg(a['debug'][e], 'qacc')).max()))
        np.testing.assert_allclose(b['qvel'][e], a['qvel'][e], atol=1e-4)
    assert seen >= 4


def test_reset_lifts_clear_of_the_height_field():
    """Reset on the perlin scene: the keyframe pose spawns inside the hills (elevation up to 2 x hip height); the lift loop
    (:376-388), re-evaluating floor and height field per iteration, must end with no calf-body geom touching anything."""
    from gym_quadruped_amd.robot_cfgs import get_robot_config
    from gym_quadruped_amd.terrain import generate_terrain
    hip = get_robot_config('aliengo').hip_height
    scene, lim = generate_terrain('perlin', hip)
    mm = marshalled('aliengo', solver=1, terrain_limits=lim, hfield=scene['hfield'])
    cfg = default_reset_cfg(seed=77, hip_height=hip)
    n = 12
    st = emu_reset(mm, n, cfg, episode=np.arange(n))
    o = Oracle(mm)
    lifted = 0
    for e in range(n):
        assert lim[1] <= st['qpos'][e, 0] <= lim[0] and lim[3] <= st['qpos'][e, 1] <= lim[2]
        assert not st['lift_failed'][e]
        o.set_state(st['qpos'][e], st['qvel'][e].astype(np.float64), np.zeros(18), np.zeros(18)); o.forward(np.zeros(12), stage=1)
        bodies = o.get('contact_body') if o.ncon else []
        assert not [c for c, bd in enumerate(bodies) if (int(bd) - 2) % 3 == 2], 'a calf body still touches the terrain'
        lifted += st['qpos'][e, 2] > hip + 1e-3
    assert lifted >= n // 2


def test_general_impedance_power_matches_oracle():
    """solimp power other than MuJoCo's default 2 (and than 1): the kernel's exp2/log2 form of x^p / mid^(p-1) against the
    oracle's pow()."""
    import copy
    mm0 = marshalled('aliengo', solver=1, iterations=100, tolerance=1e-8)
    md = copy.copy(mm0.md)
    md.geom_solimp = np.array(md.geom_solimp, dtype=np.float64).reshape(-1, 5).copy()
    md.geom_solimp[:, 4] = 3.5; md.geom_solimp[:, 3] = 0.3
    floor = dict(solimp=(0.9, 0.95, 0.001, 0.3, 3.5))
    from gym_quadruped_amd.cabi import MarshalledModel
    kw = dict(qpos0=np.array(mm0.md.qpos0), feet_geom_names=None, solver=1, iterations=100, floor=floor)
    from gym_quadruped_amd.robot_cfgs import get_robot_config
    kw['feet_geom_names'] = get_robot_config('aliengo').feet_geom_names
    mm = MarshalledModel(md, tolerance=1e-8, **kw)
    mmN = MarshalledModel(md, tolerance=1e-13, **kw)
    rng = np.random.default_rng(5)
    n = 8
    qpos, qvel = random_states(md, n, rng, z_range=(0.3, 0.42))
    qvel = qvel.astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 10).astype(np.float32)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n)
    o = Oracle(mmN)
    rows = 0
    for e in range(n):
        o.set_state(qpos[e], qvel[e].astype(np.float64), np.zeros(18), np.zeros(18)); o.step(ctrl[e].astype(np.float64))
        nefc = int(dbg(st['debug'][e], 'nefc')[0])
        assert nefc == o.nefc
        rows += nefc - 12
        sp.compare(o, emu_record(st, e), sp.IMPEDANCE_STEP, e)
    assert rows > 40


@pytest.mark.parametrize('robot,want_cross', [('mini_cheetah', True), ('aliengo', False), ('aliengo', True), ('go2', True), ('go1', None), ('b2', True)])
def test_robot_self_collision_matches_oracle(robot, want_cross):
    """Robot-robot contacts (MuJoCo's default contype = conaffinity = 1; capsule proxies, selfcol.py): pair filter, broad
    and narrow phase, two-body Jacobian rows, and the Newton step - tree-sparse when the contact stays inside one leg or
    touches the trunk, dense when it couples two legs - against the oracle: contact list, J, R, aref, forces, qacc."""
    n = 10
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-10, noise_floor=0.0)
    o = Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-12))
    rng = np.random.default_rng(7)
    qpos, qvel = self_contact_states(mm.md, n, rng, o, want_cross=want_cross)
    qvel = qvel.astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n, friction=np.full(n, 0.7, np.float32), rows=True)
    nself = 0
    tally = ParityTally(mm.md.cone == 1, 3e-7, shapes=Shapes(mm))   # (a skipped env: over the row budget or a capped convex pair; one whose contact POINTS
    tols = sp.SELF_STEP if mm.md.cone == 0 else sp.SELF_STEP_ELLIPTIC   #  are not determined - gq_oracle.c cvx_point_tie - is compared after substitution)
    for e in range(n):
        if tally.step_env(e, o, (qpos[e], qvel[e], np.zeros(18), np.zeros(18), 0.0, 0.7), ctrl[e], emu_record(st, e, contacts=True), tols) not in sp.COMPARED:
            continue
        nself += int((o.get('contact_body1') > 0).sum())
        # internal forces: no net force on the base dofs from a robot-robot contact row (Newton's third law)
        J = o.efc_J
        b1 = o.get('contact_body1').astype(int); adr = o.get('contact_efc_address').astype(int); dims = o.get('contact_dim').astype(int)
        for c in range(o.ncon):
            if b1[c] > 0:
                nr = dims[c] if mm.md.cone == 1 else (1 if dims[c] == 1 else 2 * (dims[c] - 1))
                assert np.abs(J[adr[c]:adr[c] + nr, :6]).max() < 1e-12
    tally.finish_count(f'emulated self-collision {robot} cross={want_cross}', n // 2)
    assert nself > 0


@pytest.mark.parametrize('robot,need', [('b2', 8), ('hyqreal1', 8), ('go1', 8), ('mini_cheetah', 1)])   # (mini_cheetah's draws hold few face-on-face contacts)
def test_undetermined_contact_points_are_held_by_substitution(robot, need):
    """The envs the self-collision test could not compare by value: a convex contact between two faces, a face and an edge or parallel edges
    has a determined depth and normal but every point of the overlap is a valid witness.  Such an env has its contact list held to the
    oracle's - the undetermined point to the midplane and the contact feature - and, once the oracle has taken the kernel's points for
    exactly those contacts, its rows, forces, qacc, qvel and qpos like any other (ParityTally.step_env_with_list).  `need` of the n states
    are of that class by the oracle's own tiegap; the rest are whatever the draw gives."""
    n = 24
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-10, noise_floor=0.0)
    o = Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-12))
    cone = mm.md.cone == 1
    rng = np.random.default_rng(11)
    point, other = [], []
    for _ in range(40):   # the oracle alone: draw until `need` states of the point class are there
        for q, v in zip(*self_contact_states(mm.md, n, rng, o, cone=cone, max_over=0.0)):
            o.set_state(q, v, np.zeros(18), np.zeros(18), 0.0, 0.7); o.forward(np.zeros(12), stage=1)
            gaps = o.get('contact_tiegap')
            (point if (gaps.min() == -1.0 and (gaps[gaps < 3e-7] == -1.0).all()) else other).append((q, v))
        if len(point) >= need and len(point) + len(other) >= n:
            break
    assert len(point) >= need, (len(point), need)
    keep = point[:max(need, n - len(other))]
    keep += other[:n - len(keep)]
    qpos, qvel = np.stack([q for q, _ in keep]), np.stack([v for _, v in keep]).astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n, friction=np.full(n, 0.7, np.float32), rows=True)
    tally = ParityTally(cone, 3e-7, shapes=Shapes(mm))
    tols = sp.SELF_STEP if not cone else sp.SELF_STEP_ELLIPTIC
    for e in range(n):
        tally.step_env(e, o, (qpos[e], qvel[e], np.zeros(18), np.zeros(18), 0.0, 0.7), ctrl[e], emu_record(st, e, contacts=True), tols)
    msg = tally.report(f'emulated undetermined points {robot}')
    assert not tally.mismatch and tally.point_held >= need and tally.list_stats.n['undetermined'] >= need, msg
    assert tally.checked + tally.point_held + tally.tie_held >= 0.9 * n, msg
    # a second minimum translation of equal depth: go1's cylinder prisms only (GO1_NORMAL_TIES: by the oracle alone, 0.29 of such envs have one)
    assert tally.list_stats.n['normal_tie'] <= (sp.GO1_NORMAL_TIES * n if robot == 'go1' else 0), msg


def test_contact_list_comparison_rejects_broken_rows():
    """The comparison itself: a correct contact row of b2 states with face-on-face contacts passes hold_contact_list, and the same row fails it
    with the two geoms swapped, with a normal flipped, with a distance off by 5e-6 - and with the point of an undetermined contact moved 1 mm
    off the overlap of the two faces, in its midplane: the one break only the contact-feature condition can see."""
    import copy
    from contact_cases import CVX_TOL
    from contact_list import contact_env, decode_contact_rows, hold_contact_list
    n = 6
    mm = marshalled('b2', solver=1, iterations=100, tolerance=1e-10)
    o = Oracle(marshalled('b2', solver=1, iterations=100, tolerance=1e-12))
    rng = np.random.default_rng(11)
    Q = []
    while len(Q) < n:
        for q, v in zip(*self_contact_states(mm.md, n, rng, o, cone=False, max_over=0.0)):
            o.set_state(q, v, np.zeros(18), np.zeros(18), 0.0, 0.7); o.forward(np.zeros(12), stage=1)
            gaps = o.get('contact_tiegap')
            if gaps.min() == -1.0 and (gaps[gaps < 3e-7] == -1.0).all():
                Q.append((q, v))
    qpos, qvel = np.stack([q for q, _ in Q[:n]]), np.stack([v for _, v in Q[:n]]).astype(np.float32)
    st = emu_step(mm, None, qpos.copy(), qvel.copy(), friction=np.full(n, 0.7, np.float32), rows=True)
    rows, sh = decode_contact_rows(st['contacts']), Shapes(mm)
    moved = 0
    for e in range(n):
        o.set_state(qpos[e], qvel[e], np.zeros(18), np.zeros(18), 0.0, 0.7); o.step(np.zeros(12))
        good = contact_env(rows, e)
        hold = lambda con: hold_contact_list(o, con, qpos[e, :2], sh, False, 3e-7, e)
        hold(good)

        def broken(what, **kw):
            con = copy.deepcopy(good)
            for k, f in kw.items():
                con[k] = f(con[k])
            with pytest.raises(AssertionError, match=what):
                hold(con)
        c = int(np.argmin(o.get('contact_tiegap')))   # an undetermined contact
        broken('geoms', geom1=lambda a: good['geom2'].copy(), geom2=lambda a: good['geom1'].copy())
        def flip(fr):
            fr = fr.copy(); fr[c, 0] *= -1; fr[c, 2] *= -1; return fr   # (still a right-handed orthonormal frame)
        broken('normal', frame=flip)
        def deeper(d):
            d = d.copy(); d[c] += 5e-6; return d
        broken('dist', dist=deeper)
        # the point: along a tangent to the edge of the overlap (the condition holds on an interval), then 1 mm further
        pk = good['pos'][c].astype(np.float64) + np.r_[qpos[e, :2], 0.0]
        t, dist = o.contact_frame[c][1], o.get('contact_dist')[c]
        lo, hi = 0.0, 0.5
        assert sh.on_feature(o, c, pk, dist)[0] and not sh.on_feature(o, c, pk + hi * t, dist)[0]
        while hi - lo > 1e-5:
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if sh.on_feature(o, c, pk + mid * t, dist)[0] else (lo, mid)
        def off(pos):
            pos = pos.copy(); pos[c] = (pk + (hi + 1e-3) * t - np.r_[qpos[e, :2], 0.0]).astype(np.float32); return pos
        assert abs(o.contact_frame[c][0] @ ((hi + 1e-3) * t)) < CVX_TOL['pos']   # (the moved point stays in the midplane: only the feature condition sees it)
        broken('off the contact feature', pos=off)
        moved += 1
    assert moved == n


@pytest.mark.parametrize('robot', ['go1', 'spot', 'b2'])
def test_newton_ends_on_captured_hard_states(robot):
    """States captured from benchmark rollouts on the GPU (tools/capture_stuck.py -> tests/golden/newton_stagnation_*.npz)
    on which the fp32 Newton solver ran into the iteration cap (100 iterations = 1.1 ms for the whole launch):
    go1 - cycling between neighbouring fp32 iterates at a gradient of 1e-7 of its starting value (stagnation exit);
    spot - a line search whose Newton trials overshot each other across a kink of phi' and whose unverified last candidate
    raised the cost (bracketed secant, lower bracket end on exhaustion) - qacc was WRONG there;
    b2 - two contacts between different legs in a model without friction-loss rows: first coupling row 0 was read as "no
    coupling" and the tree-sparse solve was used on a Hessian that is not tree-sparse.
    All must end within the order of the fp64 oracle's iteration count, at the oracle's solution."""
    z = sp.hard_states(robot)
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-8)
    n = len(z['qpos'])
    st = emu_step(mm, z['ctrl'].copy(), z['qpos'].copy(), z['qvel'].copy(), warm=z['warm'].copy(), applied=z['applied'].copy(),
                  friction=z['friction'].copy(), debug_envs=n)
    sp.hold_hard_states(z, Oracle(mm), [dict(niter=dbg(st['debug'][e], 'niter'), qacc=st['qacc'][e]) for e in range(n)])


def test_newton_with_22_virtual_rows_go1_on_boxes():
    """go1 on random_boxes, states captured on the GPU (tools/capture_stuck.py) where the solver needed 31-100 iterations against
    the oracle's 4-12: four condim-6 feet contacts and one condim-3 contact, all in the middle zone of their elliptic cones,
    make 4 x 5 + 2 = 22 virtual Hessian rows = 396 outputs, and the lane-parallel construction held 6 x 64 = 384 - the last row
    kept stale entries, the Hessian was wrong and Newton fell back to the linear rate of a line-searched gradient method.
    Now 8 per lane.  Each state must end within a few iterations, at the oracle's solution when the contact sets agree."""
    from gym_quadruped_amd.terrain import generate_terrain
    from gym_quadruped_amd.robot_cfgs import get_robot_config
    z = np.load(Path(__file__).parent / 'golden' / 'newton_stagnation_go1_random_boxes.npz')
    scene, lim = generate_terrain('random_boxes', get_robot_config('go1').hip_height)
    mm = marshalled('go1', solver=1, iterations=100, tolerance=1e-8, noise_floor=1e-5, boxes=scene['boxes'], terrain_limits=lim)
    o = Oracle(marshalled('go1', solver=1, iterations=100, tolerance=1e-10, boxes=scene['boxes'], terrain_limits=lim))
    n = len(z['qpos'])
    st = emu_step(mm, z['ctrl'].copy(), z['qpos'].copy(), z['qvel'].copy(), warm=z['warm'].copy(), applied=z['applied'].copy(),
                  friction=z['friction'].copy(), debug_envs=n)
    same = 0
    for e in range(n):
        nit = int(dbg(st['debug'][e], 'niter')[0])
        assert nit <= 12, (e, nit, int(z['niter_before_fix'][e]))
        o.set_state(z['qpos'][e], z['qvel'][e].astype(np.float64), z['warm'][e].astype(np.float64), z['applied'][e].astype(np.float64), 0.0, float(z['friction'][e]))
        o.step(z['ctrl'][e].astype(np.float64))
        if int(o.nefc) == int(dbg(st['debug'][e], 'nefc')[0]):   # (the others exceed the kernel's row budget: prefix rule, other tests)
            qa = np.array(o.qacc)
            assert np.abs(st['qacc'][e] - qa).max() <= 5e-5 * max(1.0, np.abs(qa).max()), (e, nit)
            same += 1
    assert same >= 1


@pytest.mark.parametrize('robot', ['aliengo', 'go1', 'b2', 'hyqreal2', 'go2'])
def test_plane_multipoint_contacts_match_oracle(robot):
    """MuJoCo's multi-point plane routines in the kernel (csrc/gq_step_body.h floor_candidates: box corners, both capsule end
    spheres with the axis-aligned frame, the cylinder's four rim points) against the oracle's restatement on poses that put
    trunk, hip and thigh geoms on the floor: contact list (order, distances), rows, frames (through J) and the Newton solution.
    States whose oracle row count exceeds one wavefront's budget are held to the PREFIX rule: the kernel's rows equal the
    oracle's first rows."""
    from test_oracle_invariants import _lying_states
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-8, noise_floor=1e-5, self_collision=False)
    mmN = marshalled(robot, solver=1, iterations=200, tolerance=1e-13, self_collision=False)
    md, o = mm.md, Oracle(mmN)
    rng = np.random.default_rng(23)
    hip = float(mm.desc.key_qpos[2])
    cone = bool(md.cone)
    # keep poses with a multi-point contact of a primitive geom, up to n of them
    n, Q = 20, []
    for q in _lying_states(md, 4000, rng, (0.25 * hip, 0.9 * hip)):
        o.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18)); o.forward(np.zeros(12), stage=1)
        if not o.ncon or o.ncon > 10:
            continue
        g = o.get('contact_geom').astype(int)
        if max(np.bincount(g)) >= 2:
            Q.append(q)
        if len(Q) == n:
            break
    assert len(Q) == n
    qpos = np.stack(Q)
    qvel = rng.normal(0, 0.5, (n, 18)).astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 10).astype(np.float32)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n, rows=True)
    tally = ParityTally(cone=cone, tie_threshold=3e-7, shapes=Shapes(mm))
    types = set()
    for e in range(n):
        kern = emu_record(st, e, contacts=True)   # (with the contact row: primitives on the floor, geom1 = -1, the capsule's axis as the tangent hint)
        cls = tally.step_env(e, o, (qpos[e], qvel[e], np.zeros(18), np.zeros(18)), ctrl[e], kern, sp.PLANE_STEP, mass=md.total_mass)
        if cls not in sp.COMPARED + ('budget',):
            continue
        # contact list: all of it ('ok') or the kernel's prefix of the oracle's list ('budget'), whose rows and flags (a body-level test, taken
        # before any capping) are held to the oracle's first rows; an 'ok' env has been held to everything in PLANE_STEP
        ncon = int(kern['ncon'][0])
        np.testing.assert_allclose(kern['contact_dist'][:ncon], o.get('contact_dist')[:ncon], atol=2e-6)
        if cls == 'budget':
            sp.compare(o, kern, sp.PLANE_PREFIX, e)
            continue
        og = o.get('contact_geom').astype(int)
        types |= {int(md.geom_type[g]) for g in og if np.count_nonzero(og == g) > 1}
    tally.finish_held(f'plane multi-point {robot}', min_checked=0.4, max_uncompared=0.1, max_budget=0.6, min_compared=0.4)
    have = {int(t) for g, t in enumerate(md.geom_type) if md.geom_bodyid[g] != 0 and md.geom_cloudid[g] >= 0 and t in (3, 5, 6)}
    assert types == have, (types, have)   # every primitive type of the robot produced a multi-point contact that was compared


def test_pair_routines_kernel_equals_oracle():
    """csrc/gq_pairs.h (capsule_box, box_box: fp32, called directly under the emulator) against the oracle's restatement
    (oracle/gq_oracle.c, fp64) on random and on resting configurations: same number of points, same order, distances /
    positions / normals to fp32 accuracy.  The oracle versions are pinned against brute-force geometry in
    tests/test_oracle_invariants.py.  Cases and asserts: tests/contact_cases.py, shared with the GPU probe."""
    import contact_cases as cc
    cases = cc.pair_cases()
    cc.check_pairs(cases, cc.emu_pairs(cases))


def test_height_field_routines_kernel_equals_oracle():
    """csrc/gq_boxes.h's closest_on_triangle, hf_triangle_under and sphere_hfield (fp32, called directly under the emulator with a GqDevModel
    filled as csrc/gq_host_model.cpp fills it) against the oracle's restatement on the four grids of tests/hfield_cases.py - rough and mild,
    coarse and fine, non-square cells, away from the origin, queries beside and beyond the border: presence, distance and normal to
    contact_cases.PAIR_TOL, ties settled among the truth's candidates.  The oracle's routines are pinned against brute force in
    tests/test_oracle_invariants.py.  Cases and asserts: tests/hfield_cases.py, shared with the GPU probe."""
    import device_cases as dc
    import hfield_cases as hc
    from helpers import emu_lib
    hc.run_backend(dc.Backend(emu_lib(), 'emu_'), 'emulator')


@pytest.mark.parametrize('robot', [None, 'mini_cheetah', 'hyqreal1', 'go1'])
def test_convex_routine_kernel_equals_oracle(robot):
    """csrc/gq_convex.h (GJK + EPA on one wavefront: lane = vertex support scans, lane = face polytope; fp32 points, fp64 simplex and
    face-plane arithmetic) called directly under the emulator against the oracle's restatement (oracle/gq_convex.h, fp64, pinned
    against the exact Minkowski-difference hull in tests/test_oracle_invariants.py): random polytopes and the robots' own mesh /
    cylinder clouds, against an analytic box and against each other, from 12 mm apart to 30 mm deep, with and without an inflation
    radius.  Same contacts; distance to 1e-6 m, normal to 0.1 degree, point to 2e-5 m wherever the oracle says the point is determined
    (not face on face / edge in face) and the polytope did not run into the iteration cap both sides share.  Cases and asserts:
    tests/contact_cases.py, shared with the GPU probe."""
    import contact_cases as cc
    cases = cc.convex_cases(robot)
    cc.check_convex(cases, cc.emu_convex(cases))


def test_capsule_proxy_mode_matches_oracle():
    """QuadrupedEnv(self_collision='capsule') / GqModelDesc.self_convex = 0: robot-robot pairs that involve a mesh go through the capsule proxies
    of geom_capsule instead of the convex routine, in kernel and oracle alike (the approximate, fast mode: DESIGN.md section 3)."""
    n = 10
    mm = marshalled('mini_cheetah', solver=1, iterations=100, tolerance=1e-10, noise_floor=0.0, self_collision='capsule')
    o = Oracle(marshalled('mini_cheetah', solver=1, iterations=100, tolerance=1e-12, self_collision='capsule'))
    assert mm.desc.self_convex == 0 and mm.self_collision == 'capsule'
    rng = np.random.default_rng(7)
    qpos, qvel = self_contact_states(mm.md, n, rng, o, want_cross=True)
    qvel = qvel.astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n, friction=np.full(n, 0.7, np.float32))
    tally = ParityTally(False, 3e-7)
    for e in range(n):
        tally.step_env(e, o, (qpos[e], qvel[e], np.zeros(18), np.zeros(18), 0.0, 0.7), ctrl[e], emu_record(st, e), sp.CAPSULE_PROXY_STEP)
    tally.finish_count('emulated capsule proxies', n // 2)


@pytest.mark.parametrize('robot', ['mini_cheetah', 'hyqreal1'])
def test_pair_exchange_changes_nothing(robot):
    """The convex pair exchange (csrc/gq_exchange.h): an env with several hull pairs in reach probes them, publishes all but the first
    undecided one to the batch's queue, claims items back and collects the results - the step it produces is bit-identical to the one
    without the exchange, and items do pass through the queue.  (Under emulation the wavefronts run one after the other: the owner claims
    its own items - every queue operation, no concurrency; the device test in test_gpu_parity.py covers that.)"""
    from helpers import emu_lib
    n = 12
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-10, noise_floor=0.0)
    o = Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-12))
    rng = np.random.default_rng(11)
    qpos, qvel = self_contact_states(mm.md, n, rng, o, want_cross=True)
    # two envs in the key posture in front (one per window of the emulator's 256-slot table): envs without convex work of their own, whose
    # passing by is what makes the entangled ones publish (gq_exchange.h: owners publish only while potential helpers are around)
    q0, v0 = random_states(mm.md, 2, rng, z_range=(0.6, 0.7))
    q0[:, 7:] = mm.md.key_qpos[0][7:]; q0[:, 3:7] = [1, 0, 0, 0]
    qpos, qvel = np.concatenate([q0, qpos]), np.concatenate([0 * v0, qvel])
    n += 2
    qvel = qvel.astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    L = emu_lib()
    L.emu_set_exchange(0)
    a = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n)
    stats0 = (C.c_int * 4)(); L.emu_exchange_stats(stats0)
    L.emu_set_exchange(1)
    try:
        b = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n)
        c = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n)   # a second launch: the last leaver rewound the queue, new epoch
    finally:
        L.emu_set_exchange(0)
    stats = (C.c_int * 4)(); L.emu_exchange_stats(stats)
    assert stats[0] - stats0[0] > 0, 'no env published a pair: the test does not reach the exchange'
    for k in ('qpos', 'qvel', 'warm', 'obs'):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    for e in range(n):
        for f in ('ncon', 'nefc', 'efc_J', 'efc_aref', 'contact_dist', 'contact_geom', 'qacc'):
            assert np.array_equal(dbg(a['debug'][e], f), dbg(b['debug'][e], f)), (e, f)


@pytest.mark.parametrize('robot,kind', nfs.CONFIGS)
def test_first_newton_step_solves_the_exact_hessian(robot, kind):
    """One Newton iteration of the kernel (tests/newton_first_step.py): qacc - qacc_smooth solves H d = -alpha g for the float64 Hessian of the
    kernel's own rows - the assembly, the middle-zone virtual rows and the tree-sparse, Sherman-Morrison or dense solve, which the minimiser
    that the parity tests compare does not depend on."""
    o = nfs.oracle_for(robot)
    qpos, qvel, ctrl = nfs.draw_states(robot, kind, o)
    n = len(qpos)
    mm = marshalled(robot, solver=1, iterations=1, tolerance=1e-8, noise_floor=0.0)
    st = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n, friction=np.full(n, nfs.FRICTION, np.float32))
    nfs.hold_first_step(robot, kind, o, qpos, qvel, ctrl, [emu_record(st, e) for e in range(n)], 'emulated')
