"""The production step kernels (mode 0) under the host SIMT emulator, through the kernels' own driver (csrc/gq_step_driver.h
step_kernel_body): the persistent window of gq_rollout, the inline policies of gq_rollout_closed (mode='inline'), gq_step_joint_cmd
and gq_step_foot_cmd - with act_seq / obs_seq / tau_out / term_any - and next-step auto-reset inside a window.  Each window is held,
bit for bit, to a loop of single steps through helpers.emu_step - the instrumented kernel, the path tests/test_kernel_emulated.py
holds to the oracle - fed the torques the window's law is documented to produce.

Three envs: one airborne, one standing in contact, one that leaves the terrain - and terminates - after its second substep.  go2 runs
the SCENE_FLAT_SELF_PRIM kernels (CVX = false) and has elliptic cones, mini_cheetah the SCENE_FLAT_SELF_HULL ones with pyramidal cones
(tests/test_scene_split_emulated.py asserts both scene choices)."""
import ctypes as C

import numpy as np
import pytest

from foot_cmd_ref import C_BOUND
from helpers import FootCmdDev, JointCmdDev, PolicyPdDev, dbg, default_reset_cfg, emu_step, emu_window, marshalled
from test_foot_cmd_host import REC, _build as build_foot_law, _ref as foot_ref, _reference as foot_reference

ROBOTS = ('go2', 'mini_cheetah')
N, D = 3, 3
STATE = ('qpos', 'qvel', 'warm', 'time', 'step_num', 'obs', 'reward', 'terminated', 'truncated', 'pending')
CARRY = ('warm', 'applied', 'time', 'friction', 'cmd', 'step_num', 'episode', 'pending', 'lift_pending', 'friction_next')   # with qpos / qvel: what a launch hands the next

_MODELS = {}


def model(robot):
    if robot not in _MODELS:
        _MODELS[robot] = marshalled(robot, solver=1, iterations=100, tolerance=1e-8, terrain_limits=(5, -5, 5, -5))
    return _MODELS[robot]


def start(mm, seed=3):
    """(qpos [3][19], qvel [3][18]): env 0 airborne, env 1 standing on its feet, env 2 airborne 1.5 mm inside the terrain's x limit and
    moving out at 1 mm per step: in bounds after its first step, out - terminated - after its second"""
    rng = np.random.default_rng(seed)
    q = np.tile(mm.md.key_qpos[0], (N, 1))
    q[:, 7:] += rng.uniform(-0.1, 0.1, (N, 12))
    q[0, 2] += 0.5; q[2, 2] += 0.5
    q[2, 0] = 4.9985
    v = np.zeros((N, 18), np.float32)
    v[:, 6:] = rng.normal(0, 0.5, (N, 12))
    v[2, 0] = 0.5
    return q, v


def words(x):
    return np.ascontiguousarray(x).view(np.uint8)


def assert_same_state(a, b):
    for k in STATE:
        assert np.array_equal(words(a[k]), words(b[k])), k


def carried(st):
    return {k: st[k].copy() for k in CARRY}


def single_steps(mm, q, v, steps, torque, first=None, **kw):
    """The reference: `steps` launches of the single step, env state handed from one to the next; torque(k, st) -> [N][12] float32 from
    the state in front of step k (st: qpos, qvel, and - after a step - obs).  first: the carried tensors of the launch before.
    Returns (the last launch's tensors, torques [steps][N][12], observation rows [steps][N][od], terminated [steps][N])."""
    st = dict(qpos=q.copy(), qvel=v.copy(), **(first or {}))
    acts, rows, terms = [], [], []
    for k in range(steps):
        u = np.ascontiguousarray(torque(k, st), dtype=np.float32)
        st = emu_step(mm, u, st['qpos'], st['qvel'], **{c: st[c] for c in CARRY if c in st}, **kw)
        acts.append(u); rows.append(st['obs'].copy()); terms.append(st['terminated'].copy())
    return st, np.stack(acts), np.stack(rows), np.stack(terms)


def joint_state(st):
    """the joint angles and rates the kernel stages in LDS: float32 of qpos[7:], qvel[6:]"""
    return st['qpos'][:, 7:].astype(np.float32), st['qvel'][:, 6:].astype(np.float32)


@pytest.mark.parametrize('robot', ROBOTS)
def test_single_step_of_the_production_kernel_equals_the_instrumented_one(robot):
    mm = model(robot)
    q, v = start(mm)
    ctrl = (np.random.default_rng(1).normal(0, 8, (N, 12))).astype(np.float32)
    a = emu_step(mm, ctrl, q.copy(), v.copy(), debug_envs=N)
    b = emu_window(mm, ctrl[None], q.copy(), v.copy())
    assert_same_state(a, b)
    assert np.array_equal(words(a['qacc']), words(b['qacc']))
    # the three envs are what the module says they are: no contact, a robot on its four feet, no contact - and nobody out of bounds yet
    ncon = [int(dbg(a['debug'][e], 'ncon')[0]) for e in range(N)]
    assert ncon[0] == 0 and ncon[1] >= 4 and ncon[2] == 0
    assert a['terminated'].tolist() == [0, 0, 0] and a['step_num'].tolist() == [1, 1, 1]


@pytest.mark.parametrize('robot', ROBOTS)
def test_open_loop_window_equals_single_steps(robot):
    mm = model(robot)
    q, v = start(mm)
    ctrl_seq = (np.random.default_rng(2).normal(0, 8, (D, N, 12))).astype(np.float32)
    ref, _, rows, terms = single_steps(mm, q, v, D, lambda k, st: ctrl_seq[k])
    win = emu_window(mm, ctrl_seq, q.copy(), v.copy(), n_steps=D, obs_seq=True)
    assert_same_state(ref, win)
    assert np.array_equal(words(win['obs_seq']), words(rows))
    assert terms[:, 2].tolist() == [0, 1, 1] and not terms[:, :2].any()   # the third env left the terrain inside the window
    assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])


def joint_command(rng, gain_stride, with_rates):
    """(the arrays, the JointCmdDev that names them, law(st) -> the float32 elementwise expression of joint_cmd_law - the restatement
    tests/test_joint_cmd_host.py pins to the header's bits)"""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    A = dict(q_des=f(rng.uniform(-0.3, 0.3, (N, 12))), kp=f(rng.uniform(20, 60, (N, 12) if gain_stride else (12,))), kd=f(rng.uniform(0.5, 2, (N, 12) if gain_stride else (12,))),
             qd_des=f(rng.uniform(-1, 1, (N, 12))) if with_rates else None, tau_ff=f(rng.uniform(-5, 5, (N, 12))) if with_rates else None,
             tau_out=np.full((N, 12), np.nan, np.float32), term_any=np.full(N, 7, np.uint8))
    p = lambda a: None if a is None else a.ctypes.data
    J = JointCmdDev(q_des=p(A['q_des']), qd_des=p(A['qd_des']), tau_ff=p(A['tau_ff']), kp=p(A['kp']), kd=p(A['kd']), tau_out=p(A['tau_out']),
                    term_any=p(A['term_any']), gain_stride=gain_stride)
    zero = np.zeros((N, 12), np.float32)

    def law(st):
        qj, qd = joint_state(st)
        u = A['kp'] * (A['q_des'] - qj) + A['kd'] * ((zero if A['qd_des'] is None else A['qd_des']) - qd) + (zero if A['tau_ff'] is None else A['tau_ff'])
        assert u.dtype == np.float32
        return u
    return A, J, law


@pytest.mark.parametrize('with_rates', [False, True], ids=['q_des', 'q_des+qd_des+tau_ff'])
@pytest.mark.parametrize('gain_stride', [0, 12])
@pytest.mark.parametrize('robot', ROBOTS)
def test_joint_command_window_equals_single_steps_with_the_law(robot, gain_stride, with_rates):
    mm = model(robot)
    q, v = start(mm)
    A, J, law = joint_command(np.random.default_rng(4), gain_stride, with_rates)
    A['q_des'] += q[:, 7:].astype(np.float32)   # (in place: the block names the array) a posture near the one the robot has
    ref, acts, rows, terms = single_steps(mm, q, v, D, lambda k, st: law(st))
    win = emu_window(mm, None, q.copy(), v.copy(), n_steps=D, policy=J, obs_seq=True, act_seq=True)
    assert_same_state(ref, win)
    assert np.array_equal(words(win['act_seq']), words(acts)) and np.array_equal(words(win['obs_seq']), words(rows))
    assert np.array_equal(words(A['tau_out']), words(acts[-1]))
    assert np.array_equal(A['term_any'], terms.any(axis=0).astype(np.uint8)) and A['term_any'].tolist() == [0, 0, 1]
    assert np.abs(acts).max() > 1.0 and not np.array_equal(acts[0], acts[1])


@pytest.mark.parametrize('robot', ROBOTS)
def test_joint_command_window_with_next_step_auto_reset(robot):
    mm = model(robot)
    q, v = start(mm)
    A, J, law = joint_command(np.random.default_rng(5), 12, True)
    A['q_des'] += q[:, 7:].astype(np.float32)
    cfg = default_reset_cfg(seed=77, fric=(0.3, 0.9)); cfg.autoreset_next_step = 1
    epi = np.array([3, 4, 5], np.int32)
    ref, acts, rows, terms = single_steps(mm, q, v, D, lambda k, st: law(st), first=dict(episode=epi.copy()), auto_reset=cfg)
    # the third env terminates at the second substep of three and spends the third on its re-spawn
    assert terms[:, 2].tolist() == [0, 1, 0] and not terms[:, :2].any()
    assert ref['episode'].tolist() == [3, 4, 6] and ref['step_num'].tolist() == [3, 3, 0] and ref['pending'].tolist() == [0, 0, 0]
    win = emu_window(mm, None, q.copy(), v.copy(), n_steps=D, policy=J, obs_seq=True, act_seq=True, episode=epi.copy(), auto_reset=cfg)
    assert_same_state(ref, win)
    for k in ('episode', 'friction', 'cmd'):
        assert np.array_equal(words(ref[k]), words(win[k])), k
    assert np.array_equal(words(win['obs_seq']), words(rows))
    # the re-spawn substep's torque - the law on the terminal state - is recorded although the reset's own step runs without control
    assert np.array_equal(words(win['act_seq']), words(acts)) and np.abs(acts[2, 2]).max() > 1.0
    assert np.array_equal(words(A['tau_out']), words(acts[-1]))
    assert A['term_any'].tolist() == [0, 0, 1] and win['terminated'].tolist() == [0, 0, 0]
    assert abs(win['qpos'][2, 0]) <= 5.0   # back inside the terrain


@pytest.fixture(scope='module')
def foot_law(tmp_path_factory):
    return build_foot_law(tmp_path_factory.mktemp('foot_cmd_window'))


@pytest.mark.parametrize('frame', ['base', 'world'])
@pytest.mark.parametrize('robot', ROBOTS)
def test_foot_command_window_equals_single_steps_with_its_recorded_torques(foot_law, robot, frame):
    mm = model(robot)
    q, v = start(mm)
    rng = np.random.default_rng(6)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    # feet under the hips, a spring towards them, a damper, a push and a joint feed-forward (gains per env and axis)
    A = dict(p_des=f(rng.uniform(-0.3, 0.3, (N, 12))), v_des=f(rng.uniform(-0.5, 0.5, (N, 12))), f_ff=f(rng.uniform(-20, 20, (N, 12))),
             tau_ff=f(rng.uniform(-2, 2, (N, 12))), kp=f(rng.uniform(100, 400, (N, 12))), kd=f(rng.uniform(1, 10, (N, 12))),
             tau_out=np.full((N, 12), np.nan, np.float32), term_any=np.full(N, 7, np.uint8))
    F = FootCmdDev(**{k: a.ctypes.data for k, a in A.items()}, gain_stride=12, frame=int(frame == 'world'))
    win = emu_window(mm, None, q.copy(), v.copy(), n_steps=D, policy=F, obs_seq=True, act_seq=True)
    acts = win['act_seq']
    ref, _, rows, terms = single_steps(mm, q, v, D, lambda k, st: acts[k])
    assert_same_state(ref, win)
    assert np.array_equal(words(win['obs_seq']), words(rows))
    assert np.array_equal(words(A['tau_out']), words(acts[-1]))
    assert np.array_equal(A['term_any'], terms.any(axis=0).astype(np.uint8)) and A['term_any'].tolist() == [0, 0, 1]
    # the first substep's torques against the host build of csrc/gq_foot_cmd.h (foot_cmd_law over plain arguments), within the bound
    # tests/test_foot_cmd_host.py holds that build to: C_BOUND 2^-24 scale, scale from the fp64 reference
    qj, qd = joint_state(dict(qpos=q, qvel=v))
    rec = np.concatenate([qj, qd, q[:, 3:7].astype(np.float32), A['p_des'], A['v_des'], A['f_ff'], A['kp'], A['kd'], A['tau_ff']], axis=1)
    assert rec.shape == (N, REC)
    fr = foot_ref(robot)
    host = foot_law(fr.mm, rec, frame)
    _, scale = foot_reference(fr, rec, frame)
    assert (np.abs(acts[0].astype(np.float64) - host.astype(np.float64)) <= C_BOUND * 2.0 ** -24 * scale).all()
    assert np.abs(acts[0]).max() > 1.0 and not np.array_equal(acts[0], acts[1])


@pytest.mark.parametrize('robot', ROBOTS)
def test_inline_pd_rollout_equals_single_steps_with_the_pd_law(robot):
    K = 4
    mm = model(robot)
    q, v = start(mm)
    names = ['qpos', 'qvel']   # joint angles at columns 7 .., joint rates at 19 + 6 ..
    rng = np.random.default_rng(8)
    kp, kd = rng.uniform(20, 60, 12).astype(np.float32), rng.uniform(0.5, 2, 12).astype(np.float32)
    qdes = (mm.md.key_qpos[0][7:] + rng.uniform(-0.2, 0.2, 12)).astype(np.float32)
    col_q, col_qd = np.arange(12) + 7, np.arange(12) + 19 + 6
    P = PolicyPdDev(kp=(C.c_float * 12)(*kp), kd=(C.c_float * 12)(*kd), qdes=(C.c_float * 12)(*qdes), col_q=(C.c_int32 * 12)(*col_q),
                    col_qd=(C.c_int32 * 12)(*col_qd), sigma=0.0, seed_lo=1, seed_hi=2, step0=0, env_id_offset=0)
    s0 = emu_step(mm, np.zeros((N, 12), np.float32), q.copy(), v.copy(), obs_names=names)   # the observation row exists
    q1, v1, row1 = s0['qpos'].copy(), s0['qvel'].copy(), s0['obs'].copy()

    def pd(k, st):   # on the previous step's row
        row = st.get('obs', row1)
        u = kp * (qdes - row[:, col_q]) - kd * row[:, col_qd]
        assert u.dtype == np.float32
        return u
    ref, acts, rows, _ = single_steps(mm, q1, v1, K, pd, first=carried(s0), obs_names=names)
    # (the inline policy reads the batch's observation tensor: the window is given the rows the step above left)
    win = emu_window(mm, None, q1.copy(), v1.copy(), n_steps=K, policy=P, obs_seq=True, act_seq=True, obs_names=names, obs=row1.copy(), **carried(s0))
    assert_same_state(ref, win)
    assert np.array_equal(words(win['act_seq']), words(acts)) and np.array_equal(words(win['obs_seq']), words(rows))
    assert np.abs(acts).max() > 1.0 and not np.array_equal(acts[0], acts[1])
