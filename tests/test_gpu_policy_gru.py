"""GPU tests of the recurrent policy inside the closed-loop rollout (include/gq.h gq_rollout_policy_gru / gq_policy_gru_eval,
QuadrupedEnv.rollout_policy(GruPolicy) / policy_eval(hidden=) / policy_hidden, csrc/gq_policy_gru.h):

* the matrix-core form (gru_tile_forward) and the plain loops that define the law (gru_row_forward) give the same bits on the device, actions
  and next hidden state, also chained over steps, and lie within the derived bound of float64; a row's result does not depend on its tile;
* the loop is closed: the state fed at every policy step is the one the episode rule leaves, every action and next state is the law on the
  recorded row, previous action and that state, every torque the joint law on the held action, bit for bit;
* the recorded torques replayed through the step loop leave the same state; rewards and dones are the reference windows'; the hidden state
  fed at step s + 1 is zero exactly where dones[s] - in the plain mode and in the learn + feet mode, across two calls;
* edge sizes; an MLP rollout and the mailbox rollout on the same batch are what they were; reset; refusals.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_gru_ref as G
import policy_mlp_ref as PR
from learn_windows import _replay_flags, _same, reference_windows  # noqa: F401  (reference_windows: through test_gpu_foot_reward._windows)
from test_gpu_closed_loop import STATE, _env, _twin
from test_gpu_foot_reward import CMD, OBS, SIGMA, _spec, _windows

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KP, KD, SCALE = 25.0, 0.8, 0.25
ROW_COUNTS = (1, 15, 16, 17, 131)


@pytest.fixture(scope='module')
def handle():
    env = _env(n=16, seed=1)
    env.reset(random=True)
    return env


def _dev(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


@pytest.mark.parametrize('shape', ['odd', 'wide', 'minimal'])
def test_tile_and_scalar_forms_have_the_same_bits(handle, shape):
    p = G.make_policy(shape, 'elu', 'tanh' if shape == 'odd' else None)
    rows, h = G.rows_for(p, max(ROW_COUNTS))
    (ra, rh), (ea, eh) = G.step_bound(p, rows, h)
    drows, dh = _dev(rows), _dev(h)
    for n in ROW_COUNTS:
        ta, th = handle.policy_eval(p, drows[:n], hidden=dh[:n], impl='tile')
        sa, sh = handle.policy_eval(p, drows[:n], hidden=dh[:n], impl='scalar')
        assert ta.shape == (n, 12) and th.shape == (n, p.hidden)
        assert _same(ta, sa) and _same(th, sh), (n, float((ta - sa).abs().max()), float((th - sh).abs().max()))
        err_a, err_h = np.abs(ta.cpu().numpy().astype(np.float64) - ra[:n]), np.abs(th.cpu().numpy().astype(np.float64) - rh[:n])
        print(f'{shape} n={n}: worst error / bound: actions {float((err_a / ea[:n]).max()):.2e}, hidden {float((err_h / eh[:n]).max()):.2e}')
        assert (err_a <= ea[:n]).all() and (err_h <= eh[:n]).all()
    assert torch.equal(dh, _dev(h)), 'the state handed in is not written'
    # the same 17 rows alone and embedded in a 131-row call: other tiles, other slots, the ragged end
    mr, mh = G.rows_for(p, 17, seed=2)
    mr, mh = _dev(mr), _dev(mh)
    alone_a, alone_h = handle.policy_eval(p, mr, hidden=mh)
    for at in (0, 5, 19, 114):
        r2, h2 = G.rows_for(p, 131, seed=3 + at)
        r2, h2 = _dev(r2) * 5, _dev(h2)
        r2[at:at + 17], h2[at:at + 17] = mr, mh
        a2, hn2 = handle.policy_eval(p, r2, hidden=h2)
        assert _same(a2[at:at + 17], alone_a) and _same(hn2[at:at + 17], alone_h), at
    # eight chained steps, each form carrying its own state
    ht, hs = dh.clone(), dh.clone()
    for step in range(8):
        x = _dev(G.rows_for(p, max(ROW_COUNTS), seed=20 + step)[0])
        at_, ht = handle.policy_eval(p, x, hidden=ht, impl='tile')
        as_, hs = handle.policy_eval(p, x, hidden=hs, impl='scalar')
        assert _same(at_, as_) and _same(ht, hs), step
    assert torch.isfinite(ht).all() and float(ht.abs().max()) <= 1.0 + 1e-6


def _torque(env, a_held, row):
    q0 = env._key_qpos[7:19].float()
    q, qd = row[:, 0:12], row[:, 12:24]
    return KP * ((q0 + SCALE * a_held) - q) + KD * (0 - qd) + 0


def test_the_loop_is_closed():
    from gym_quadruped_amd.reward import RewardSpec
    n, K, D = 200, 12, 4
    env = _env(n=n, seed=7)
    env.reset(random=True)
    p = G.make_policy('odd', 'elu')
    H = p.hidden
    assert env.policy_hidden is None
    env.policy_hidden = torch.rand(n, H, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV) * 2 - 1
    before, h0, pending = env._obs_buf.clone(), env.policy_hidden.clone(), env._terminated.clone().bool()
    r = env.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, record_obs=True, record_actions=True, record_transitions=True,
                           reward=RewardSpec(alive=1.0, termination=-1.0))
    code, _, played = env.closed_loop_status()
    assert code == 0 and played == n * K
    obs, acts, pol, hid = r['obs_seq'], r['actions'], r['policy_actions'], r['policy_hidden']
    assert hid.shape == (K // D, n, H) and pol.shape == (K // D, n, 12) and r['policy_obs'].shape == (K // D, n, p.in_dim)
    zero = torch.zeros(n, H, device=DEV)
    fed = torch.where(pending[:, None], zero, h0)
    for s in range(K // D):
        assert _same(hid[s], fed), s                                   # the state the rule leaves
        row = before if s == 0 else obs[D * s - 1]
        prev = torch.zeros(n, 12, device=DEV) if s == 0 else pol[s - 1]
        x = torch.cat([row[:, :p.in_obs], prev], dim=1)
        assert _same(r['policy_obs'][s], x), s
        want_a, want_h = env.policy_eval(p, x, hidden=hid[s])
        assert _same(pol[s], want_a) and _same(r['policy_means'][s], want_a), s
        fed = torch.where(r['dones'][s][:, None], zero, want_h)       # (the learning modes' closing visit included)
    assert _same(env.policy_hidden, fed), 'the state after the call: the last next-state with the rule of the closing visit'
    for k in range(K):
        assert _same(acts[k], _torque(env, pol[k // D], before if k == 0 else obs[k - 1])), k
    assert torch.isfinite(pol).all() and float(pol.abs().max()) > 0.01 and float(env.policy_hidden.abs().max()) > 0.01


@pytest.mark.parametrize('mode', ['plain', 'feet'])
@pytest.mark.parametrize('robot,n,K', [('mini_cheetah', 131, 24), ('go2', 1000, 20)])
def test_replay_rewards_and_the_hidden_rule_across_two_calls(robot, n, K, mode):
    D, feet = 4, mode == 'feet'
    # warm = 60: the robots of _twin are dropped at reset and the first of them fall about 50 steps later - after the default warm-up of 30 steps
    # the first call (steps 30 .. 50) ends before any env has fallen, whatever the batch size (go2: no re-spawn among 4096 envs in the plain
    # mode, none pending before the second call among 4096 in the learn + feet mode); from step 60 on falls and re-spawns come steadily
    a, b = _twin(robot, n, warm=60, **(dict(state_obs_names=OBS, **CMD) if feet else {}))
    p = G.make_policy('odd', 'elu')
    H, S = p.hidden, K // D
    spec = _spec()
    zero = torch.zeros(n, H, device=DEV)
    b.policy_hidden = torch.rand(n, H, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV) * 2 - 1
    seen = dict(done=0, early=False, pending=[])
    for call in range(2):   # the second call starts with the envs that fell in the first one's last step waiting for their re-spawn
        pending = b._terminated.clone().bool()
        h0, before, air = b.policy_hidden.clone(), b._obs_buf.clone(), b.feet_air_time.clone()
        if feet:
            r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, noise_sigma=SIGMA, record_obs=True, record_actions=True, reward=spec,
                                 record_transitions=True)
        else:
            r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, record_obs=True, record_actions=True)
            assert set(r) == {'obs', 'obs_seq', 'actions', 'policy_actions'}
        code, _, played = b.closed_loop_status()
        assert code == 0 and played == n * K
        rows, term = _replay_flags(a, b, r, K, STATE)                  # the recorded torques through `step`: the same STATE, bit for bit
        win = term.view(S, D, n).any(dim=1)                            # window s contained a termination
        if feet:
            want_r, want_d, want_air, _ = _windows(b, spec, rows, term, r['actions'], r['policy_actions'], pending, D, air)
            assert torch.equal(r['dones'], want_d) and _same(r['rewards'], want_r) and _same(b.feet_air_time, want_air)
            assert torch.equal(r['dones'], win), 'dones[s] <=> window s contained a termination'
            hid = r['policy_hidden']
            # all zero exactly where dones[s], non-zero elsewhere - across the call boundary too: the first state of the second call is zero where
            # the first call's last window had a termination (the envs pending before the call among them)
            first = pending if call == 0 else prev_last
            assert not bool((pending & ~first).any())
            assert torch.equal((hid[0] == 0).all(dim=1), first) and torch.equal((hid[1:] == 0).all(dim=2), r['dones'][:-1])
            assert torch.equal((hid[0] != 0).any(dim=1), ~first) and torch.equal((hid[1:] != 0).any(dim=2), ~r['dones'][:-1])
            prev_last = r['dones'][-1]
        # the hidden sequence rebuilt from the state before the call, the flags and the rule; every action is the law on it
        fed = torch.where(pending[:, None], zero, h0)
        for s in range(S):
            row = before if s == 0 else rows[D * s - 1]
            prev = torch.zeros(n, 12, device=DEV) if s == 0 else r['policy_actions'][s - 1]
            if feet:
                assert _same(r['policy_hidden'][s], fed), (call, s)
            act, hn = b.policy_eval(p, torch.cat([row[:, :p.in_obs], prev], dim=1), hidden=fed)
            assert _same(r['policy_means' if feet else 'policy_actions'][s], act), (call, s)
            fed = torch.where(win[s][:, None], zero, hn)
        # after the call: the learning modes' closing visit sees a fall in step K - 1, the plain mode leaves it to the next call's k == 0
        last = win[S - 1] if feet else term[D * (S - 1):K - 1].any(dim=0)
        assert _same(b.policy_hidden, torch.where(last[:, None], zero, hn)), call
        seen['done'] += int(win.sum())
        seen['early'] = seen['early'] or bool(term.view(S, D, n)[:, :D - 1].any())
        seen['pending'].append(int(pending.sum()))
        print(f'{robot} n={n} {mode} call {call}: windows with a termination {int(win.sum())}, pending before the call {int(pending.sum())}')
    if robot == 'go2':   # the workload is not empty
        assert seen['done'] > 0, 'the workload must contain a window with a termination'
        assert seen['early'], 'the workload must contain a termination that is not the last substep of its window'
        assert seen['pending'][1] > 0, 'the workload must contain an env pending before the second call'


@pytest.mark.parametrize('D', [1, 4])
@pytest.mark.parametrize('n,step_waves', [(1, 0), (7, 0), (120, 0), (128, 0), (136, 0), (9, 2048)])
def test_edge_sizes_and_single_policy_steps(n, step_waves, D):
    a, b = _env(n=n, seed=3), _env(n=n, seed=3)
    a.reset(random=True); b.reset(random=True)
    p = G.make_policy('odd', 'relu')
    for K in (D, 2 * D):
        before, pending = b._obs_buf.clone(), b._terminated.clone().bool()
        h0 = torch.zeros(n, p.hidden, device=DEV) if b.policy_hidden is None else b.policy_hidden.clone()
        r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, record_obs=True, record_actions=True, step_waves=step_waves)
        code, _, played = b.closed_loop_status()
        assert code == 0 and played == n * K
        fed = torch.where(pending[:, None], torch.zeros_like(h0), h0)
        want_a, want_h = b.policy_eval(p, torch.cat([before[:, :p.in_obs], torch.zeros(n, 12, device=DEV)], dim=1), hidden=fed)
        assert _same(r['policy_actions'][0], want_a)
        assert _same(r['actions'][0], _torque(b, want_a, before))
        rows, term = _replay_flags(a, b, r, K, STATE)
        if K == D:   # one policy step: the state after the call is its next state, zeroed by the falls the call's visits saw
            assert _same(b.policy_hidden, torch.where(term[:K - 1].any(dim=0)[:, None], torch.zeros_like(h0), want_h))


def test_nothing_else_moved_and_reset_zeroes_the_masked_rows():
    n = 64
    a, b = _env(n=n, seed=5), _env(n=n, seed=5)
    a.reset(random=True); b.reset(random=True)
    p = G.make_policy('odd', 'elu')
    r = b.rollout_policy(8, p, KP, KD, action_scale=SCALE, record_obs=True, record_actions=True)
    assert b.closed_loop_status()[2] == n * 8
    _replay_flags(a, b, r, 8, STATE)
    hidden = b.policy_hidden.clone()
    # an MlpPolicy rollout and the mailbox rollout on the same batch still equal the step loop, and leave the hidden state alone
    r = b.rollout_policy(8, PR.make_policy('odd', 'elu'), KP, KD, action_scale=SCALE, record_obs=True, record_actions=True)
    assert b.closed_loop_status()[2] == n * 8 and 'policy_hidden' not in r
    _replay_flags(a, b, r, 8, STATE)
    r = b.rollout_closed_loop(10, KP, KD, mode='mailbox', record_obs=True, record_actions=True)
    assert b.closed_loop_status()[2] == n * 10
    _replay_flags(a, b, r, 10, STATE)
    assert _same(b.policy_hidden, hidden)
    # reset of a mask zeroes exactly those rows; the checkpoint carries the state; another H is refused until the tensor is reassigned
    b.policy_hidden = torch.arange(1, n * p.hidden + 1, device=DEV).reshape(n, p.hidden).float()
    keep, ptr = b.policy_hidden.clone(), b.policy_hidden.data_ptr()
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[[0, 5, 63]] = True
    b.reset(env_ids=mask)
    assert (b.policy_hidden[mask] == 0).all() and torch.equal(b.policy_hidden[~mask], keep[~mask]) and b.policy_hidden.data_ptr() == ptr
    sd = b.state_dict()
    assert torch.equal(sd['_policy_hidden'], b.policy_hidden)
    b.reset(random=True)
    assert (b.policy_hidden == 0).all()
    b.load_state_dict(sd)
    assert torch.equal(b.policy_hidden, sd['_policy_hidden'])
    with pytest.raises(ValueError, match='hidden units'):
        b.rollout_policy(4, G.make_policy('odd', 'elu', hidden=24), KP, KD)
    b.policy_hidden = torch.zeros(n, 24, device=DEV)
    b.rollout_policy(4, G.make_policy('odd', 'elu', hidden=24), KP, KD)
    assert b.closed_loop_status()[2] == n * 4 and b.policy_hidden.shape == (n, 24) and float(b.policy_hidden.abs().max()) > 0


def _raw(env, m, g, K=4):
    from gym_quadruped_amd import _lib
    stream = torch.cuda.current_stream(env.device).cuda_stream
    _lib.check(env._L.gq_rollout_policy_gru(env._hbatch, K, C.byref(m), C.byref(g), 0, 0, 5.0, env._st, env._out, env._auto_cfg, env._episode.data_ptr(),
                                            env._lift_failed.data_ptr(), None, None, None, None, stream), 'gq_rollout_policy_gru')


def test_what_cannot_be_done_is_refused_and_the_batch_stays_usable():
    from gym_quadruped_amd import _lib
    from gym_quadruped_amd.policy import GruPolicy
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    n = 64
    a, env = _env(n=n, seed=5), _env(n=n, seed=5)
    a.reset(random=True); env.reset(random=True)
    p = G.make_policy('odd', 'relu')
    z = lambda *s: np.zeros(s, np.float32)
    cell = lambda k, H: (z(k, 3 * H), z(H, 3 * H), z(3 * H), z(3 * H))
    with pytest.raises(ValueError, match='hidden units'):     # hidden outside 1 .. 128
        GruPolicy(*cell(24, 129), [z(129, 12)], [z(12)])
    with pytest.raises(ValueError, match='linear layers'):    # a head with more than 3 layers
        GruPolicy(*cell(24, 8), [z(8, 8)] * 3 + [z(8, 12)], [z(8)] * 3 + [z(12)])
    with pytest.raises(ValueError, match='12'):               # a head whose output is not 12
        GruPolicy(*cell(24, 8), [z(8, 11)], [z(11)])
    with pytest.raises(ValueError, match='256'):              # the cell's input row beyond 256 columns
        GruPolicy(*cell(257, 8), [z(8, 12)], [z(12)])
    with pytest.raises(ValueError, match='hidden'):           # a GruPolicy needs its state in policy_eval
        env.policy_eval(p, torch.zeros(3, p.in_dim, device=DEV))
    hidden = torch.zeros(n, p.hidden, device=DEV)

    def blocks(mk=None, gk=None):   # the same refusals from the library, for a binding that does not go through GruPolicy
        m, g = env._policy_struct(p)
        m.decimation, g.hidden_state = 4, hidden.data_ptr()
        for k, v in (mk or {}).items():
            setattr(m, k, v)
        for k, v in (gk or {}).items():
            setattr(g, k, v)
        return m, g
    for mk, gk, msg in ((None, dict(struct_size=8), 'GqPolicyGru.struct_size'), (dict(struct_size=8), None, 'GqPolicyMlp.struct_size'), (None, dict(hidden=0), 'hidden'),
                        (None, dict(hidden=129), 'hidden'), (dict(n_layers=4), None, 'head has 4 linear layers'), (dict(width=(C.c_int32 * 4)(33, 11, 0, 0)), None, '12'),
                        (None, dict(hidden_state=None), 'hidden_state'), (None, dict(blob_floats=7), 'blob_floats'), (None, dict(blob=None), 'blob is null'),
                        (dict(in_obs=env._obs_dim + 1), None, 'in_obs'), (dict(decimation=3), None, 'multiple'), (dict(width=(C.c_int32 * 4)(300, 12, 0, 0)), None, 'outputs')):
        with pytest.raises(_lib.GqError, match=msg):
            _raw(env, *blocks(mk, gk))
    with pytest.raises(ValueError, match='observation columns'):   # in_obs beyond the user's row (39 columns)
        env.rollout_policy(4, G.make_policy('wide'), KP, KD)
    with pytest.raises(_lib.GqError, match='Newton'):        # PGS
        e3 = QuadrupedEnv('mini_cheetah', num_envs=8, device=DEV, solver='pgs', auto_reset='next_step', state_obs_names=env.state_obs_names)
        e3.reset(random=True)
        e3.rollout_policy(4, p, KP, KD)
    with pytest.raises(_lib.GqError, match='next-step'):     # same-step auto-reset
        e4 = QuadrupedEnv('mini_cheetah', num_envs=8, device=DEV, solver='newton', auto_reset='same_step', state_obs_names=env.state_obs_names)
        e4.reset(random=True)
        e4.rollout_policy(4, p, KP, KD)
    # the batch steps normally afterwards, and the recurrent rollout works on it
    act = torch.randn(n, 12, device=DEV) * 20
    a.step(act); env.step(act)
    r = env.rollout_policy(8, p, KP, KD, record_obs=True, record_actions=True)
    assert env.closed_loop_status()[2] == n * 8
    _replay_flags(a, env, r, 8, STATE)
