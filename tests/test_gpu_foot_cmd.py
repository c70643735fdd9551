"""GPU tests of foot-space actions held over a decimation window (include/gq.h gq_step_foot_cmd, QuadrupedEnv.step_feet): one launch
plays `decimation` physics steps of every env under tau_leg = J^T (f_ff + kp (p_des - p) + kd (v_des - v)) + tau_ff, evaluated at every
substep from the env's fresh state.

* plumbing, bit for bit: the window leaves the state, flags and observation rows of `decimation` x env.step(recorded torques), re-spawns
  inside the window included; `terminated` is the OR over the window;
* law values: every recorded torque of every env and substep against the fp64 reference (tests/foot_cmd_ref.py) evaluated at the state
  the twin had before that substep, within the bound the host run fixed (foot_cmd_ref.C_BOUND; tests/test_foot_cmd_host.py);
* with zero gains and no force it is step_pd with zero gains, bit for bit;
* an observation row without joint columns works; what cannot be done is refused before a launch.

The twin-env construction (every third env on its back: it terminates at once and re-spawns inside a window) is
tests/test_gpu_joint_cmd.py's."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from foot_cmd_ref import C_BOUND, FootCmdRef  # noqa: E402
from test_gpu_closed_loop import STATE  # noqa: E402
from test_gpu_joint_cmd import WINDOWS, _assert_respawns, _env, _twin  # noqa: E402

pytestmark = pytest.mark.gpu

LEG_NAMES = ['FL', 'FR', 'RL', 'RR']
DEV = 'cuda:0'


def _to_user(x, legs_order):
    """canonical foot rows [N, 12] (FL FR RL RR) -> the rows in the env's legs_order"""
    idx = [LEG_NAMES.index(leg) for leg in legs_order]
    return x.view(-1, 4, 3)[:, idx].reshape(-1, 12).contiguous()


def _commands(env, ref, g):
    """one window's command, canonical foot order: the keyframe footholds (base frame) +- 0.1 m, v_des +- 1 m/s, f_ff +- m g / 2 per axis,
    tau_ff +- 5 N m - per env"""
    n = env.num_envs
    key = env._key_qpos.cpu().numpy()
    p_key = np.concatenate([(kin[5].T @ kin[0]) for kin in ref.kinematics(key)])
    u = lambda a: (2 * torch.rand(n, 12, generator=g, device=DEV) - 1) * a
    return (torch.tensor(p_key, dtype=torch.float32, device=DEV) + u(0.1), u(1.0), u(0.5 * ref.mass * 9.81), u(5.0))


def _gains(n, g):
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, 12, generator=g, device=DEV)
    return u(100.0, 800.0), u(2.0, 20.0)


def _law_state(qpos, qvel):
    """the state the law reads: float32 joint angles, base quaternion and joint rates (load_rows stages them so); the base at the origin"""
    q = qpos.clone()
    q[:, :3] = 0.0
    q[:, 3:] = q[:, 3:].float().double()
    return q.cpu().numpy(), qvel.double().cpu().numpy()


CASES = [('mini_cheetah', 'flat', 65, 'base', None), ('go2', 'flat', 63, 'world', ('FR', 'RL', 'FL', 'RR')), ('go1', 'flat', 64, 'base', None),
         ('hyqreal1', 'random_boxes', 64, 'world', None), ('aliengo', 'random_boxes', 64, 'base', None), ('mini_cheetah', 'flat', 1, 'world', None)]


@pytest.mark.parametrize('decimation', [1, 4])
@pytest.mark.parametrize('robot,scene,n,frame,legs_order', CASES)
def test_step_feet_equals_the_step_loop_and_the_reference_law(robot, scene, n, frame, legs_order, decimation):
    D = decimation
    kw = {} if legs_order is None else dict(legs_order=legs_order)
    order = legs_order or tuple(LEG_NAMES)
    a, b = _twin(robot, scene, n, **kw)
    ref = FootCmdRef(b._mm)
    g = torch.Generator(device=DEV).manual_seed(4)
    kp, kd = _gains(n, g)
    advanced = hidden = any_terminated = False
    worst = 0.0
    for w in range(WINDOWS):
        p_des, v_des, f_ff, tau_ff = _commands(b, ref, g)
        ep0 = b._episode.clone()
        obs, reward, term, trunc, info = b.step_feet(_to_user(p_des, order), _to_user(kp, order), _to_user(kd, order), v_des=_to_user(v_des, order),
                                                     f_ff=_to_user(f_ff, order), tau_ff=tau_ff, frame=frame, decimation=D, record_obs=True, record_actions=True)
        rows, states, any_term = [], [], torch.zeros(n, dtype=torch.bool, device=DEV)
        for k in range(D):
            states.append(_law_state(a.qpos, a.qvel))
            _, _, t, _, _ = a.step(info['actions'][k])
            rows.append(a._obs_buf.clone()); any_term |= t
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(getattr(a, k), getattr(b, k)), (w, k)
        assert torch.equal(info['obs_seq'], torch.stack(rows)), w
        assert term.dtype == torch.bool and torch.equal(term, any_term), w
        assert torch.equal(trunc, a._truncated_b) and torch.equal(reward, a._reward)
        assert torch.equal(b.torque_ctrl_setpoint, info['actions'][-1]), w
        assert obs is b._obs_views and torch.equal(info['step_num'], a._info['step_num'])
        advanced |= bool((b._episode > ep0).any())
        hidden |= bool((term & ~b._terminated_b).any())
        any_terminated |= bool(term.any())
        # the law's values: every env (the re-spawning ones too: their recorded torque is computed from the terminal state) and substep
        acts = info['actions'].double().cpu().numpy()
        cmd = [x.double().cpu().numpy() for x in (p_des, kp, kd, v_des, f_ff, tau_ff)]
        assert np.isfinite(acts).all()
        for k in range(D):
            qpos, qvel = states[k]
            for e in range(n):
                want, scale = ref.torques(qpos[e], qvel[e], cmd[0][e], cmd[1][e], cmd[2][e], v_des=cmd[3][e], f_ff=cmd[4][e], tau_ff=cmd[5][e], frame=frame)
                ratio = float((np.abs(acts[k, e] - want) / (2.0 ** -24 * scale)).max())
                worst = max(worst, ratio)
                assert ratio <= C_BOUND, (w, k, e, ratio, acts[k, e], want)
    print(f'{robot} {scene} n={n} D={D} {frame}: largest |tau - tau_ref| / (2^-24 scale) = {worst:.2f} (bound {C_BOUND})')
    assert torch.isfinite(b.qpos).all()
    _assert_respawns(D, advanced, hidden, any_terminated)
    # and the batch is an ordinary batch afterwards
    act = torch.randn(n, 12, generator=g, device=DEV) * 10
    a.step(act); b.step(act)
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_step_feet_without_gains_and_force_is_step_pd_without_gains():
    n, D = 65, 4
    a, b = _twin('mini_cheetah', 'flat', n)
    g = torch.Generator(device=DEV).manual_seed(5)
    z = torch.zeros(n, 12, device=DEV)
    advanced = False
    for w in range(WINDOWS):
        x = (2 * torch.rand(n, 12, generator=g, device=DEV) - 1) * 5 + 1e-3
        ep0 = b._episode.clone()
        _, _, tb, _, ib = b.step_feet(torch.rand(n, 12, generator=g, device=DEV), 0.0, 0.0, tau_ff=x, frame=('base', 'world')[w % 2], decimation=D,
                                      record_obs=True, record_actions=True)
        _, _, ta, _, ia = a.step_pd(z, 0.0, 0.0, tau_ff=x, decimation=D, record_obs=True, record_actions=True)
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(getattr(a, k), getattr(b, k)), (w, k)
        assert torch.equal(ib['actions'], ia['actions']) and torch.equal(ib['actions'][0], x), w
        assert torch.equal(ib['obs_seq'], ia['obs_seq']) and torch.equal(ta, tb), w
        advanced |= bool((b._episode > ep0).any())
    assert advanced, 'no env re-spawned inside a window'


def test_step_feet_needs_no_joint_columns_and_takes_shared_gains_and_legs_attr():
    """env b: a permuted legs_order (not its own inverse), targets as a LegsAttr, shared gains of 3 (per axis) and 12 values (per foot and
    axis, in ITS legs_order, host list and device tensor); env a: the default order, everything as [N, 12] rows in canonical order"""
    from gym_quadruped_amd.utils.quadruped_utils import LegsAttr
    n, D = 63, 4
    order = ('RR', 'FL', 'FR', 'RL')
    a = _twin('mini_cheetah', 'flat', n, state_obs_names=('base_lin_vel',))[0]
    b = _twin('mini_cheetah', 'flat', n, state_obs_names=('base_lin_vel',), legs_order=order)[0]
    for k in STATE:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    ref = FootCmdRef(b._mm)
    g = torch.Generator(device=DEV).manual_seed(6)
    advanced = False
    for w in range(WINDOWS):
        p_des, v_des, f_ff, tau_ff = _commands(b, ref, g)
        ep0 = b._episode.clone()
        legs = LegsAttr(**{leg: p_des[:, 3 * i:3 * i + 3].contiguous() for i, leg in enumerate(LEG_NAMES)})
        kp12 = torch.linspace(200.0, 750.0, 12, device=DEV)          # canonical: foot k, axis i -> 200 + 50 (3 k + i)
        kd12 = torch.linspace(4.0, 15.0, 12, device=DEV)
        kp_user, kd_user = _to_user(kp12[None], order)[0], _to_user(kd12[None], order)[0]
        if w % 3 == 0:      # 3 values per axis (host list) / a scalar
            gb, ga = ([300.0, 300.0, 500.0], 8.0), (torch.tensor([300.0, 300.0, 500.0] * 4, device=DEV).expand(n, 12).contiguous(), torch.full((n, 12), 8.0, device=DEV))
        elif w % 3 == 1:    # 12 values on the host, in b's legs_order
            gb, ga = (kp_user.tolist(), kd_user.tolist()), (kp12.expand(n, 12).contiguous(), kd12.expand(n, 12).contiguous())
        else:               # 12 values on the device, in b's legs_order; 3 values on the device
            gb, ga = (kp_user, torch.tensor([6.0, 7.0, 9.0], device=DEV)), (kp12.expand(n, 12).contiguous(), torch.tensor([6.0, 7.0, 9.0] * 4, device=DEV).expand(n, 12).contiguous())
        _, _, tb, _, ib = b.step_feet(legs, gb[0], gb[1], f_ff=_to_user(f_ff, order), decimation=D, record_actions=True)
        _, _, ta, _, ia = a.step_feet(p_des, ga[0], ga[1], f_ff=f_ff, decimation=D, record_actions=True)
        torch.cuda.synchronize()
        for k in STATE:
            assert torch.equal(getattr(a, k), getattr(b, k)), (w, k)
        assert torch.equal(ib['actions'], ia['actions']) and torch.equal(ta, tb), w
        advanced |= bool((b._episode > ep0).any())
    assert advanced, 'no env re-spawned inside a window'


def test_step_feet_refuses_what_it_cannot_do_and_leaves_the_env_usable():
    n = 8
    g = torch.Generator(device=DEV).manual_seed(7)

    def usable(env):
        launches = env._launches
        obs, _, term, _, _ = env.step(torch.zeros(n, 12, device=DEV))
        torch.cuda.synchronize()
        assert env._launches == launches + 1 and torch.isfinite(env._obs_buf).all() and term.shape == (n,)

    env = _env('mini_cheetah', 'flat', n)
    env.reset(random=True)
    p = torch.rand(n, 12, generator=g, device=DEV) - 0.5
    launches = env._launches
    for bad in (lambda: env.step_feet(p[:, :11], 100.0, 5.0),                                  # bad shape
                lambda: env.step_feet(p[:-1], 100.0, 5.0),
                lambda: env.step_feet(p.double(), 100.0, 5.0),                                 # bad dtype
                lambda: env.step_feet(p.cpu(), 100.0, 5.0),                                    # bad device
                lambda: env.step_feet(p, 100.0, 5.0, v_des=p[:, :3]),
                lambda: env.step_feet(p, 100.0, 5.0, tau_ff=p.double()),
                lambda: env.step_feet(p, 100.0, 5.0, frame='feet'),                            # bad frame
                lambda: env.step_feet(p, torch.ones(n, 11, device=DEV), 5.0),                  # bad gain shape
                lambda: env.step_feet(p, 100.0, [5.0] * 5),
                lambda: env.step_feet(p, 100.0, 5.0, decimation=0)):
        with pytest.raises(ValueError):
            bad()
    assert env._launches == launches                                # nothing was launched
    usable(env)
    launches = env._launches
    env.step_feet(p, 100.0, 5.0, decimation=3)                      # ... and the method itself still works
    assert env._launches == launches + 3
    others = {}
    for kw in (dict(solver='pgs'), dict(auto_reset='same_step')):
        e2 = others[next(iter(kw))] = _env('mini_cheetah', 'flat', n, **kw)
        e2.reset(random=True)
        launches = e2._launches
        with pytest.raises(ValueError):
            e2.step_feet(p, 100.0, 5.0)
        assert e2._launches == launches
        usable(e2)
    # the library's own refusals, behind the Python checks (a binding that skips them must not get a launch either)
    import ctypes as C
    from gym_quadruped_amd import _lib
    from gym_quadruped_amd.cabi import GqFootCmd
    gains = torch.ones(2, 12, device=DEV)
    ok = dict(struct_size=C.sizeof(GqFootCmd), gain_stride=0, frame=0, p_des=p.data_ptr(), kp=gains[0].data_ptr(), kd=gains[1].data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    for e, dec, over, what in ((env, 0, {}, 'decimation'), (others['auto_reset'], 4, {}, 'next-step auto-reset'), (others['solver'], 4, {}, 'Newton solver'), (env, 4, dict(frame=2), 'frame'),
                               (env, 4, dict(gain_stride=3), 'gain_stride'), (env, 4, dict(p_des=None), 'p_des'),
                               (env, 4, dict(struct_size=8), 'stale binding')):
        cmd = GqFootCmd(**{**ok, **over})
        rc = e._L.gq_step_foot_cmd(e._hbatch, C.byref(cmd), dec, e._st, e._out, e._auto_cfg, e._episode.data_ptr(), e._lift_failed.data_ptr(), None, None, stream)
        assert rc < 0 and what in _lib.lib().gq_last_error().decode(), what
    usable(env)
