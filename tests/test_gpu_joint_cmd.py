"""GPU tests of joint-impedance actions held over a decimation window (include/gq.h gq_step_joint_cmd, QuadrupedEnv.step_pd): one
launch plays `decimation` physics steps of every env under tau = kp (q_des - q) + kd (qd_des - qd) + tau_ff, the law evaluated at
every substep from the env's fresh joint state with the env's own command.

* state, flags, observation rows and recorded torques equal those of the loop it replaces - `decimation` x (torch expression,
  env.step) - bit for bit, re-spawns inside the window included;
* `terminated` is the OR over the window, the flag buffer keeps the last substep's;
* with one command for every env and no velocity target / feed-forward it is the inline closed-loop rollout, bit for bit;
* the law reads the state rows: an observation row without joint columns works;
* what the persistent kernel cannot do is refused before a launch, and the env stays usable.

Every third env starts on its back with the trunk in the floor: it terminates at once and re-spawns inside a window - each case
asserts that this happened (a case in which nothing re-spawned proves nothing)."""
import numpy as np
import pytest
import torch

from test_gpu_closed_loop import STATE

pytestmark = pytest.mark.gpu

WINDOWS = 6
FLIP_Z = 0.03   # base origin of the envs put on their back, m above the floor: less than half a trunk's height of every robot here


def _env(robot, scene, n, **kw):
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    kw.setdefault('state_obs_names', ('qpos_js', 'qvel_js', 'base_lin_vel', 'contact_forces'))
    kw.setdefault('auto_reset', 'next_step')
    kw.setdefault('solver', 'newton')
    return QuadrupedEnv(robot, scene=scene, num_envs=n, device='cuda:0', seed=11, **kw)


def _twin(robot, scene, n, **kw):
    """two envs in the same state; every third env on its back, a few centimetres above the floor"""
    a, b = _env(robot, scene, n, **kw), _env(robot, scene, n, **kw)
    for e in (a, b):
        e.reset(random=True)
        ids = torch.arange(0, n, 3, device='cuda:0')
        qpos = e.qpos.clone()
        qpos[ids, 2] = FLIP_Z
        qpos[ids, 3:7] = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64, device='cuda:0')   # half a turn about x
        e.reset(qpos=qpos, qvel=torch.zeros(n, 18, device='cuda:0'), env_ids=ids)
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    return a, b


def _commands(env, g, uniform=False):
    """one window's command: keyframe +- 0.6 rad, qd_des +- 1 rad/s, tau_ff +- 5 N m, per env and joint"""
    n = env.num_envs
    key = env._key_qpos[7:19].float()
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, 12, generator=g, device='cuda:0')
    return key + u(-0.6, 0.6), u(-1.0, 1.0), u(-5.0, 5.0)


def _gains(n, g):
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, 12, generator=g, device='cuda:0')
    return u(20.0, 60.0), u(0.5, 2.0)


def _loop(a, D, q_des, kp, kd, qd_des=None, tau_ff=None):
    """the loop step_pd replaces, on env a: returns the torques, the observation rows and the OR of the termination flags"""
    taus, rows, any_term = [], [], torch.zeros(a.num_envs, dtype=torch.bool, device='cuda:0')
    for _ in range(D):
        q, qd = a.qpos[:, 7:].float(), a.qvel[:, 6:]
        if qd_des is None:
            tau = kp * (q_des - q) - kd * qd
        else:
            tau = kp * (q_des - q) + kd * (qd_des - qd) + tau_ff
        _, _, term, _, _ = a.step(tau)
        taus.append(tau); rows.append(a._obs_buf.clone()); any_term |= term
    return torch.stack(taus), torch.stack(rows), any_term


def _assert_respawns(D, advanced, hidden, any_terminated):
    assert advanced, 'no env re-spawned inside a window: the case proves nothing'
    if D > 1:
        assert hidden, 'no env had terminated (window OR) true with the last substep\'s flag false: the case proves nothing'
    else:
        assert any_terminated   # (a window of one substep: its OR is that substep's flag)


@pytest.mark.parametrize('decimation', [1, 4])
@pytest.mark.parametrize('robot,scene,n', [('mini_cheetah', 'flat', 65), ('go2', 'flat', 63), ('aliengo', 'random_boxes', 64), ('mini_cheetah', 'flat', 1)])
def test_step_pd_equals_the_step_loop_with_the_torch_law(robot, scene, n, decimation):
    D = decimation
    a, b = _twin(robot, scene, n)
    g = torch.Generator(device='cuda:0').manual_seed(4)
    kp, kd = _gains(n, g)
    advanced = hidden = any_terminated = False
    for w in range(WINDOWS):
        q_des, qd_des, tau_ff = _commands(b, g)
        ep0 = b._episode.clone()
        obs, reward, term, trunc, info = b.step_pd(q_des, kp, kd, qd_des=qd_des, tau_ff=tau_ff, decimation=D, record_obs=True, record_actions=True)
        taus, rows, any_term = _loop(a, D, q_des, kp, kd, qd_des, tau_ff)
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(getattr(a, k), getattr(b, k)), (w, k)
        assert torch.equal(info['actions'], taus), w
        assert torch.equal(info['obs_seq'], rows), w
        assert term.dtype == torch.bool and torch.equal(term, any_term), w
        assert torch.equal(trunc, a._truncated_b) and torch.equal(reward, a._reward)
        assert torch.equal(b.torque_ctrl_setpoint, taus[-1]), w
        assert obs is b._obs_views and torch.equal(info['step_num'], a._info['step_num'])
        advanced |= bool((b._episode > ep0).any())
        hidden |= bool((term & ~b._terminated_b).any())
        any_terminated |= bool(term.any())
    assert torch.isfinite(b.qpos).all()
    _assert_respawns(D, advanced, hidden, any_terminated)
    # and the batch is an ordinary batch afterwards
    act = torch.randn(n, 12, generator=g, device='cuda:0') * 10
    a.step(act); b.step(act)
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_step_pd_with_one_command_for_all_is_the_inline_closed_loop_rollout():
    n, D = 65, 4
    a, b = _twin('mini_cheetah', 'flat', n)
    key = b._key_qpos[7:19].float()
    q_des = key.expand(n, 12).contiguous()
    advanced = hidden = False
    for w in range(WINDOWS):
        ep0 = b._episode.clone()
        _, _, term, _, info = b.step_pd(q_des, 25.0, 0.8, decimation=D, record_actions=True)
        r = a.rollout_closed_loop(D, 25.0, 0.8, key.cpu().numpy(), mode='inline', record_actions=True)
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(getattr(a, k), getattr(b, k)), (w, k)
        # (the rollout's first action reads the observation row of the previous step, whose joint columns are that state)
        assert torch.equal(info['actions'], r['actions']), w
        advanced |= bool((b._episode > ep0).any())
        hidden |= bool((term & ~b._terminated_b).any())
    _assert_respawns(D, advanced, hidden, True)


def test_step_pd_needs_no_joint_columns_in_the_observation_row():
    n, D = 63, 4
    a, b = _twin('mini_cheetah', 'flat', n, state_obs_names=('base_lin_vel',))
    g = torch.Generator(device='cuda:0').manual_seed(6)
    kp = torch.linspace(20.0, 60.0, 12, device='cuda:0')   # 12 values on the device: one shared row, copied there
    advanced = hidden = False
    for w in range(WINDOWS):
        q_des, qd_des, tau_ff = _commands(b, g)
        ep0 = b._episode.clone()
        _, _, term, _, info = b.step_pd(q_des, kp, 1.0, qd_des=qd_des, tau_ff=tau_ff, decimation=D, record_actions=True)
        taus, _, any_term = _loop(a, D, q_des, kp, torch.full((12,), 1.0, device='cuda:0'), qd_des, tau_ff)
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(getattr(a, k), getattr(b, k)), (w, k)
        assert torch.equal(info['actions'], taus) and torch.equal(term, any_term)
        advanced |= bool((b._episode > ep0).any())
        hidden |= bool((term & ~b._terminated_b).any())
    _assert_respawns(D, advanced, hidden, True)


def test_step_pd_refuses_what_it_cannot_do_and_leaves_the_env_usable():
    n = 8
    g = torch.Generator(device='cuda:0').manual_seed(7)

    def usable(env):
        launches = env._launches
        obs, _, term, _, _ = env.step(torch.zeros(n, 12, device='cuda:0'))
        torch.cuda.synchronize()
        assert env._launches == launches + 1 and torch.isfinite(env._obs_buf).all() and term.shape == (n,)

    env = _env('mini_cheetah', 'flat', n)
    env.reset(random=True)
    q_des, _, _ = _commands(env, g)
    launches = env._launches
    with pytest.raises(ValueError):
        env.step_pd(q_des[:, :11], 25.0, 0.8)                       # bad shape
    with pytest.raises(ValueError):
        env.step_pd(q_des[:-1], 25.0, 0.8)
    with pytest.raises(ValueError):
        env.step_pd(q_des.double(), 25.0, 0.8)                      # bad dtype
    with pytest.raises(ValueError):
        env.step_pd(q_des, torch.ones(n, 11, device='cuda:0'), 0.8)  # bad gain shape
    with pytest.raises(ValueError):
        env.step_pd(q_des, 25.0, [0.8] * 5)
    with pytest.raises(ValueError):
        env.step_pd(q_des, 25.0, 0.8, decimation=0)
    assert env._launches == launches                                # nothing was launched
    usable(env)
    env.step_pd(q_des, 25.0, 0.8, decimation=3)                     # ... and the method itself still works
    assert env._launches == launches + 4
    for kw in (dict(solver='pgs'), dict(auto_reset='same_step')):
        e2 = _env('mini_cheetah', 'flat', n, **kw)
        e2.reset(random=True)
        launches = e2._launches
        with pytest.raises(ValueError):
            e2.step_pd(q_des, 25.0, 0.8)
        assert e2._launches == launches
        usable(e2)
    # the library's own refusals, behind the Python checks (a binding that skips them must not get a launch either)
    import ctypes as C
    from gym_quadruped_amd import _lib
    from gym_quadruped_amd.cabi import GqJointCmd
    gains = torch.ones(2, 12, device='cuda:0')
    cmd = GqJointCmd(struct_size=C.sizeof(GqJointCmd), gain_stride=0, q_des=q_des.data_ptr(), kp=gains[0].data_ptr(), kd=gains[1].data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    for e, dec, what in ((env, 0, 'decimation'), (e2, 4, 'next-step auto-reset')):
        rc = e._L.gq_step_joint_cmd(e._hbatch, C.byref(cmd), dec, e._st, e._out, e._auto_cfg, e._episode.data_ptr(), e._lift_failed.data_ptr(), None, None, stream)
        assert rc < 0 and what in _lib.lib().gq_last_error().decode()
