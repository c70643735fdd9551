"""GPU tests of the learning half of the MLP rollout (include/gq.h gq_rollout_policy_learn / gq_reward_eval,
QuadrupedEnv.rollout_policy(reward=, record_transitions=) / reward_eval, csrc/gq_reward.h):

* the reward law on the device has the bits of the host program and lies within the CPU test's bounds of the float64 reference;
* the transition records are the row the network saw and what it said before the noise;
* rewards and dones are the reference loop over the replayed steps, bit for bit - re-spawn steps, dead windows, the last step (the closing
  visit), every window flushing (decimation 1);
* observing changes nothing; what cannot be done is refused with a message and leaves the batch usable.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_mlp_ref as PR
import reward_ref as R
from learn_windows import _replay_flags, _same, reference_windows
from test_gpu_closed_loop import STATE, _env, _twin

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KP, KD, SCALE = 25.0, 0.8, 0.25
OBS = R.OBS_NAMES
ROW_COUNTS = (1, 63, 64, 65, 131)


@pytest.fixture(scope='module')
def handle():
    env = _env(n=16, seed=1, state_obs_names=OBS)
    env.reset(random=True)
    return env


def test_the_law_on_the_device(handle):
    assert handle._obs_dim == R.OBS_DIM
    dt = handle._sim_dt
    steps = R.random_steps(max(ROW_COUNTS), seed=5)
    edge = R.edge_steps()
    steps = tuple(np.concatenate([e, s])[:max(ROW_COUNTS)] for e, s in zip(edge, steps))   # the edge rows first: every count from 63 on holds all of them
    dev = [torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in steps]
    plain, full = R.spec_no_exp(), R.specs()['all']
    host_plain, host_full = R.host_reward(plain, *steps, dt=dt), R.host_reward(full, *steps, dt=dt)
    ref, bound = R.issue_bound(full, steps, dt=dt)
    tight = R.first_order_bound(full, steps, dt=dt)
    fin = np.isfinite(ref) & np.isfinite(bound)
    for n in ROW_COUNTS:
        cut = [v[:n] for v in dev]
        got = handle.reward_eval(plain, *cut)
        assert got.shape == (n,) and np.array_equal(got.cpu().numpy().view(np.uint32), host_plain[:n].view(np.uint32)), n
        got = handle.reward_eval(full, *cut).cpu().numpy()
        print(f'n={n}: the full spec has the host\'s bits: {np.array_equal(got.view(np.uint32), host_full[:n].view(np.uint32))}')
        err = np.abs(got.astype(np.float64) - ref[:n])
        f = fin[:n]
        assert (err[f] <= bound[:n][f]).all() and (err[f] <= tight[:n][f]).all(), n
    # what is off is not read: no torques, no actions, no flags for a spec that needs none
    alive = handle.reward_eval(R.specs()['alive'], dev[0][:5])
    assert (alive == np.float32(dt) * np.float32(0.25)).all()


def test_the_records_are_what_the_network_saw_and_said():
    n, K, D, sigma = 200, 12, 4, 0.3
    env = _env(n=n, seed=7, state_obs_names=OBS)
    env.reset(random=True)
    p = PR.make_policy('odd', 'elu')
    before, step0, seed = env._obs_buf.clone(), int(env._launches) & 0x7fffffff, int(env._seed)
    r = env.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, noise_sigma=sigma, record_obs=True, record_transitions=True)
    code, _, played = env.closed_loop_status()
    assert code == 0 and played == n * K
    assert set(r) == {'obs', 'obs_seq', 'actions', 'policy_actions', 'policy_obs', 'policy_means'} and r['actions'] is None
    pobs, means, pol, obs = r['policy_obs'], r['policy_means'], r['policy_actions'], r['obs_seq']
    assert pobs.shape == (K // D, n, p.in_dim) and means.shape == (K // D, n, 12) and pol.shape == (K // D, n, 12)
    for s in range(K // D):
        row = before if s == 0 else obs[D * s - 1]
        prev = torch.zeros(n, 12, device=DEV) if s == 0 else pol[s - 1]
        assert _same(pobs[s], torch.cat([row[:, :p.in_obs], prev], dim=1)), s
        assert _same(means[s], env.policy_eval(p, pobs[s])), s
        z = torch.from_numpy(PR.policy_noise(seed, step0 + D * s, n)).to(DEV)
        assert _same(pol[s], means[s] + torch.tensor(sigma, dtype=torch.float32, device=DEV) * z), s
    assert float((pol - means).abs().max()) > 0.05


def _windows(env, spec, rows, term, torques, pol, pending, D):
    """learn_windows.reference_windows with reward_eval as the step's reward"""
    step = lambda k, s, air: env.reward_eval(spec, rows[k], torques[k], pol[s], pol[s - 1] if s > 0 else pol[0], term[k])
    return reference_windows(step, term, pending, D)[:2]


@pytest.mark.parametrize('robot,n,K', [('mini_cheetah', 131, 24), ('go2', 1000, 20)])
def test_the_reward_is_the_reference_loop(robot, n, K):
    D = 4
    a, b = _twin(robot, n, state_obs_names=OBS)
    p = PR.make_policy('odd', 'elu')
    spec = R.specs()['all']
    for call in range(2):   # the second call starts with the envs that fell in the first one's last step waiting for their re-spawn
        pending = b._terminated.clone().bool()
        r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, noise_sigma=0.1, record_obs=True, record_actions=True, reward=spec)
        code, _, played = b.closed_loop_status()
        assert code == 0 and played == n * K
        assert r['rewards'].shape == (K // D, n) and r['rewards'].dtype == torch.float32 and r['dones'].shape == (K // D, n) and r['dones'].dtype == torch.bool
        rows, term = _replay_flags(a, b, r, K, STATE)
        want_r, want_d = _windows(b, spec, rows, term, r['actions'], r['policy_actions'], pending, D)
        assert torch.equal(r['dones'], want_d)
        assert _same(r['rewards'], want_r), float((r['rewards'] - want_r).abs().max())   # every env, every window
        assert torch.isfinite(r['rewards']).all() and float(r['rewards'].abs().max()) > 0
        early = bool(term.view(K // D, D, n)[:, :D - 1].any())
        print(f'{robot} n={n} call {call}: windows with done {int(r["dones"].sum())}, pending before the call {int(pending.sum())}, terminations inside a window {early}')
        if n == 1000 and call == 0:
            assert bool(r['dones'].any()), 'the workload must contain a window with a termination'
            assert early, 'the workload must contain a termination that is not the last substep of its window'


@pytest.mark.parametrize('D', [1, 4])
@pytest.mark.parametrize('n,step_waves', [(1, 0), (7, 0), (120, 0), (128, 0), (136, 0), (9, 2048)])
def test_edge_sizes_the_last_step_and_the_first_window(n, step_waves, D):
    from gym_quadruped_amd.reward import RewardSpec
    a, b = _env(n=n, seed=3, state_obs_names=OBS), _env(n=n, seed=3, state_obs_names=OBS)
    a.reset(random=True); b.reset(random=True)
    p = PR.make_policy('odd', 'relu')
    full, rate = R.specs()['all'], RewardSpec(action_rate=-1.0)
    for K in (D, 2 * D):
        for spec in (full, rate):
            pending = b._terminated.clone().bool()
            r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, record_obs=True, record_actions=True, step_waves=step_waves, reward=spec,
                                 record_transitions=True)
            code, _, played = b.closed_loop_status()
            assert code == 0 and played == n * K
            rows, term = _replay_flags(a, b, r, K, STATE)
            want_r, want_d = _windows(b, spec, rows, term, r['actions'], r['policy_actions'], pending, D)
            assert _same(r['rewards'], want_r) and torch.equal(r['dones'], want_d), (K, float((r['rewards'] - want_r).abs().max()))
            if spec is rate:
                assert (r['rewards'][0] == 0).all(), 'action_rate is 0 in the first window of a call'
                if K == 2 * D:
                    assert (r['rewards'][1] < 0).any(), '... and not in the second'
            else:
                assert (r['rewards'][-1] != 0).any(), 'the last window holds the last step\'s reward'


def test_observing_changes_nothing():
    n, K, D = 300, 16, 4
    a, b = _twin('mini_cheetah', n, state_obs_names=OBS)
    p = PR.make_policy('odd', 'tanh')
    kw = dict(action_scale=SCALE, decimation=D, noise_sigma=0.2, record_actions=True)
    ra = a.rollout_policy(K, p, KP, KD, **kw)
    rb = b.rollout_policy(K, p, KP, KD, reward=R.specs()['all'], record_transitions=True, **kw)
    assert a.closed_loop_status()[2] == n * K and b.closed_loop_status()[2] == n * K
    assert set(ra) == {'obs', 'obs_seq', 'actions', 'policy_actions'}
    for f in STATE:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert _same(ra['actions'], rb['actions']) and _same(ra['policy_actions'], rb['policy_actions'])
    # the mailbox machinery is as it was: a plain closed-loop rollout on the observed batch still equals the step loop
    r = b.rollout_closed_loop(10, KP, KD, mode='mailbox', record_obs=True, record_actions=True)
    assert b.closed_loop_status()[2] == n * 10
    _replay_flags(a, b, r, 10, STATE)


def _raw(env, m, g, K=4):
    from gym_quadruped_amd import _lib
    stream = torch.cuda.current_stream(env.device).cuda_stream
    _lib.check(env._L.gq_rollout_policy_learn(env._hbatch, K, C.byref(m), 0, 0, 5.0, env._st, env._out, env._auto_cfg, env._episode.data_ptr(), env._lift_failed.data_ptr(),
                                              None, None, C.byref(g), stream), 'gq_rollout_policy_learn')


def test_refusals_leave_the_batch_usable():
    from gym_quadruped_amd import _lib
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    from gym_quadruped_amd.reward import RewardSpec
    n = 64
    names = tuple(o for o in OBS if o != 'gravity_vector:base')
    a, env = _env(n=n, seed=5, state_obs_names=names), _env(n=n, seed=5, state_obs_names=names)
    a.reset(random=True); env.reset(random=True)
    p = PR.make_policy('odd', 'relu')
    w = R.weights_full()
    full = R.spec_of(w)
    ok = R.spec_of({k: v for k, v in w.items() if k != 'orientation'})
    with pytest.raises(_lib.GqError, match='gravity_vector:base'):   # a weighted term whose observable is not in the row
        env.rollout_policy(4, p, KP, KD, reward=full)
    with pytest.raises(_lib.GqError, match='gravity_vector:base'):
        env.reward_eval(full, env._obs_buf, torch.zeros(n, 12, device=DEV), torch.zeros(n, 12, device=DEV), torch.zeros(n, 12, device=DEV))
    with pytest.raises(ValueError, match='RewardSpec'):
        env.rollout_policy(4, p, KP, KD, reward=dict(alive=1.0))

    def blocks(**kw):
        m = env._policy_struct(p)
        m.decimation = 4
        g = ok._struct()
        for k, v in kw.items():
            setattr(g, k, v)
        return m, g
    for kw, msg in ((dict(struct_size=8), 'stale'), (dict(sigma_lin=0.0), 'sigma_lin'), (dict(sigma_ang=-1.0), 'sigma_ang'), (dict(w_alive=float('nan')), 'not finite'),
                    (dict(w_torques=float('inf')), 'not finite')):
        with pytest.raises(_lib.GqError, match=msg):
            _raw(env, *blocks(**kw))
    m, g = blocks()
    m.decimation = 3                                                  # ... and everything gq_rollout_policy refuses
    with pytest.raises(_lib.GqError, match='multiple'):
        _raw(env, m, g)
    with pytest.raises(_lib.GqError, match='Newton'):                 # PGS
        e3 = QuadrupedEnv('mini_cheetah', num_envs=8, device=DEV, solver='pgs', auto_reset='next_step', state_obs_names=names)
        e3.reset(random=True)
        e3.rollout_policy(4, p, KP, KD, reward=ok)
    with pytest.raises(_lib.GqError, match='next-step'):              # same-step auto-reset
        e4 = QuadrupedEnv('mini_cheetah', num_envs=8, device=DEV, solver='newton', auto_reset='same_step', state_obs_names=names)
        e4.reset(random=True)
        e4.rollout_policy(4, p, KP, KD, reward=ok)
    # the batch steps normally afterwards, and a learn rollout works on it
    act = torch.randn(n, 12, device=DEV) * 20
    a.step(act); env.step(act)
    pending = env._terminated.clone().bool()
    r = env.rollout_policy(8, p, KP, KD, record_obs=True, record_actions=True, reward=ok, record_transitions=True)
    assert env.closed_loop_status()[2] == n * 8
    rows, term = _replay_flags(a, env, r, 8, STATE)
    want_r, want_d = _windows(env, ok, rows, term, r['actions'], r['policy_actions'], pending, 4)
    assert _same(r['rewards'], want_r) and torch.equal(r['dones'], want_d)
