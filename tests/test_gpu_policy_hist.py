"""GPU tests of the observation history of the in-loop MLP policy (include/gq.h gq_rollout_policy_hist, QuadrupedEnv.rollout_policy with
MlpPolicy(history=ObsHistory(...)) / policy_history, csrc/gq_policy_hist.h), bit for bit:

* the loop is closed: every row the network was fed is the one rebuilt from the state before the call, the recorded rows and actions, the
  preset history, `pending` and `dones` by the ten-line reference; every mean is the network on that row, every torque the joint law on the
  held action, and the store after the call is the rebuilt one;
* the recorded torques replayed through the step loop leave the same state; rewards and dones are the reference windows'; the history fed at
  step s + 1 is zero exactly where dones[s] - in the plain mode and in the learn + feet mode, across two calls;
* with a height scan the row is obs | scan | action | frames; edge sizes; the other rollouts on the same batch are what they were; reset,
  checkpoint, refusals.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import height_scan_ref as HS
import policy_gru_ref as G
import policy_hist_ref as R
import policy_mlp_ref as PR
from learn_windows import _replay_flags, _same
from test_gpu_closed_loop import STATE, _env, _twin
from test_gpu_foot_reward import CMD, OBS, SIGMA, _spec, _windows

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KP, KD, SCALE = 25.0, 0.8, 0.25
IN_OBS = 24
SHAPES = [(3, 24), (3, 13), (1, 24)]   # (L, cols): in_dim 144, 111 (odd offsets, K padding), 72


def _policy(L, cols, scan=None, widths=(33, 12), seed=0):
    """an MlpPolicy on 24 observation columns with feed_last_action, shift / scale, and an ObsHistory(L, cols)"""
    from gym_quadruped_amd.policy import MlpPolicy, ObsHistory
    rng = np.random.default_rng(seed + 31 * L + cols)
    in_dim = IN_OBS + (scan.cells if scan is not None else 0) + 12 + L * (cols + 12)
    ws, bs, k = [], [], in_dim
    for w in widths:
        ws.append((rng.standard_normal((k, w)) / np.sqrt(k)).astype(np.float32))
        bs.append((0.1 * rng.standard_normal(w)).astype(np.float32))
        k = w
    p = MlpPolicy(ws, bs, activation='elu', feed_last_action=True, height_scan=scan, history=ObsHistory(L, cols),
                  obs_shift=(0.3 * rng.standard_normal(IN_OBS)).astype(np.float32), obs_scale=(0.5 + rng.random(IN_OBS)).astype(np.float32))
    assert (p.in_dim, p.in_obs, p.hist_cols, p.hist_words) == (in_dim, IN_OBS, cols, cols + 12)
    return p


def _np(t):
    return t.detach().cpu().numpy()


def _t(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


def _rebuild(p, before, rows, pol, hist0, pending, term, D, closing, scans=None):
    """the rows fed at every policy step and the store after the call, from the replayed loop and the reference (policy_hist_ref.fed_history):
    rows [K, n, od] after every step, pol [S, n, 12] the policy's actions, term [S * D', n] with D' = D (per step) or 1 (per window)"""
    S, n, c = pol.shape[0], pol.shape[1], p.hist_cols
    cur_rows = [before if s == 0 else rows[(len(rows) // S) * s - 1] for s in range(S)]
    prev = [torch.zeros(n, 12, device=DEV) if s == 0 else pol[s - 1] for s in range(S)]
    cur = np.stack([_np(torch.cat([cur_rows[s][:, :c], prev[s]], dim=1)) for s in range(S)])
    fed, after = R.fed_history(cur, _np(hist0), _np(pending), _np(term), D, closing)
    xs = []
    for s in range(S):
        parts = [cur_rows[s][:, :p.in_obs]] + ([scans[s]] if scans is not None else []) + [prev[s], _t(fed[s].reshape(n, -1))]
        xs.append(torch.cat(parts, dim=1))
        assert xs[-1].shape[1] == p.in_dim
    return xs, fed, _t(after)


def _torque(env, a_held, row):
    q0 = env._key_qpos[7:19].float()
    q, qd = row[:, 0:12], row[:, 12:24]
    return KP * ((q0 + SCALE * a_held) - q) + KD * (0 - qd) + 0


@pytest.mark.parametrize('L,cols', SHAPES)
def test_the_loop_is_closed(L, cols):
    from gym_quadruped_amd.reward import RewardSpec
    n, K, D = 200, 24, 4
    env = _env(n=n, seed=7)
    env.reset(random=True)
    p = _policy(L, cols)
    F = p.hist_words
    assert env.policy_history is None
    env.policy_history = torch.rand(n, L, F, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV) * 2 - 1
    before, h0, pending = env._obs_buf.clone(), env.policy_history.clone(), env._terminated.clone().bool()
    r = env.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, record_obs=True, record_actions=True, record_transitions=True,
                           reward=RewardSpec(alive=1.0, termination=-1.0))
    code, _, played = env.closed_loop_status()
    assert code == 0 and played == n * K
    obs, acts, pol = r['obs_seq'], r['actions'], r['policy_actions']
    assert pol.shape == (K // D, n, 12) and r['policy_obs'].shape == (K // D, n, p.in_dim)
    xs, fed, after = _rebuild(p, before, obs, pol, h0, pending, r['dones'], 1, True)   # (the learning modes' closing visit included)
    for s, x in enumerate(xs):
        assert _same(r['policy_obs'][s], x), (s, int((r['policy_obs'][s] != x).sum()))
        want = env.policy_eval(p, r['policy_obs'][s])
        assert _same(r['policy_means'][s], want) and _same(pol[s], want), s
        assert _same(want, env.policy_eval(p, x, impl='scalar')), s
    assert _same(env.policy_history, after), 'the store after the call is the rebuilt one'
    for k in range(K):
        assert _same(acts[k], _torque(env, pol[k // D], before if k == 0 else obs[k - 1])), k
    assert torch.isfinite(pol).all() and float(pol.abs().max()) > 0.01 and float(env.policy_history.abs().max()) > 0.01
    # shift / scale reach the frames by their original column: the float64 network on the recorded row agrees with the means
    ref = p.reference(_np(r['policy_obs'][K // D - 1]))
    assert np.abs(ref - _np(r['policy_means'][K // D - 1])).max() < 1e-3


@pytest.mark.parametrize('mode', ['plain', 'feet'])
@pytest.mark.parametrize('robot,n,K', [('mini_cheetah', 131, 24), ('go2', 1000, 20)])
def test_replay_rewards_and_the_history_rule_across_two_calls(robot, n, K, mode):
    D, feet = 4, mode == 'feet'
    # warm = 60: as in test_gpu_policy_gru.py - from step 60 on the robots of _twin fall and re-spawn steadily
    a, b = _twin(robot, n, warm=60, **(dict(state_obs_names=OBS, **CMD) if feet else {}))
    p = _policy(3, 13)
    L, F, S, col0 = 3, p.hist_words, K // D, IN_OBS + 12
    spec = _spec()
    b.policy_history = torch.rand(n, L, F, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV) + 0.5
    seen = dict(done=0, early=False, pending=[])
    for call in range(2):   # the second call starts with the envs that fell in the first one's last step waiting for their re-spawn
        pending = b._terminated.clone().bool()
        h0, before, air = b.policy_history.clone(), b._obs_buf.clone(), b.feet_air_time.clone()
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
        xs, fed, after = _rebuild(p, before, rows, r['policy_actions'], h0, pending, term, D, feet)
        if feet:
            want_r, want_d, want_air, _ = _windows(b, spec, rows, term, r['actions'], r['policy_actions'], pending, D, air)
            assert torch.equal(r['dones'], want_d) and _same(r['rewards'], want_r) and _same(b.feet_air_time, want_air)
            assert torch.equal(r['dones'], win), 'dones[s] <=> window s contained a termination'
            hist = r['policy_obs'][:, :, col0:]
            # all zero exactly where dones[s], a non-zero word elsewhere - across the call boundary too: the first history of the second call is
            # zero where the first call's last window had a termination (the envs pending before the call among them)
            first = pending if call == 0 else prev_last
            assert not bool((pending & ~first).any())
            assert torch.equal((hist[0] == 0).all(dim=1), first) and torch.equal((hist[1:] == 0).all(dim=2), r['dones'][:-1])
            assert torch.equal((hist[0] != 0).any(dim=1), ~first) and torch.equal((hist[1:] != 0).any(dim=2), ~r['dones'][:-1])
            prev_last = r['dones'][-1]
        for s, x in enumerate(xs):   # every action is the network on the rebuilt row
            if feet:
                assert _same(r['policy_obs'][s], x), (call, s)
            assert _same(r['policy_means' if feet else 'policy_actions'][s], b.policy_eval(p, x)), (call, s)
        # after the call: the learning modes' closing visit sees a fall in step K - 1, the plain mode leaves it to the next call's k == 0
        assert _same(b.policy_history, after), call
        last = win[S - 1] if feet else term[D * (S - 1):K - 1].any(dim=0)
        assert torch.equal((b.policy_history == 0).all(dim=2).all(dim=1), last)
        seen['done'] += int(win.sum())
        seen['early'] = seen['early'] or bool(term.view(S, D, n)[:, :D - 1].any())
        seen['pending'].append(int(pending.sum()))
        print(f'{robot} n={n} {mode} call {call}: windows with a termination {int(win.sum())}, pending before the call {int(pending.sum())}')
    if robot == 'go2':   # the workload is not empty
        assert seen['done'] > 0, 'the workload must contain a window with a termination'
        assert seen['early'], 'the workload must contain a termination that is not the last substep of its window'
        assert seen['pending'][1] > 0, 'the workload must contain an env pending before the second call'


def test_with_a_scan_the_row_is_obs_scan_action_frames():
    from gym_quadruped_amd.policy import HeightScan
    from gym_quadruped_amd.reward import RewardSpec
    from test_gpu_policy_scan import ZCOL, _replay, _scan_twin
    n, K, D, L = 64, 8, 4, 2
    a, b, hm_a, hm_b = _scan_twin(n, 'perlin', 3, 5)
    spec = HeightScan(3, 5, offset=0.3, clip=0.1, scale=5.0)
    p = _policy(L, IN_OBS, scan=spec)
    assert p.in_dim == 24 + 15 + 12 + 2 * 36
    b.policy_history = torch.rand(n, L, 36, generator=torch.Generator(device=DEV).manual_seed(9), device=DEV) - 0.5
    before, pending, h0 = b._obs_buf.clone(), b._terminated.clone().bool(), b.policy_history.clone()
    hits0 = hm_a.update_height_map().clone()     # the twin is in the same state: its rays, cast apart from the rollout
    r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, noise_sigma=2.0, record_obs=True, record_actions=True, record_transitions=True,
                         reward=RewardSpec(alive=1.0, termination=-1.0))
    code, _, played = b.closed_loop_status()
    assert code == 0 and played == n * K
    rows, term, maps = _replay(a, hm_a, b, r, K)
    scans = []
    for s in range(K // D):
        row, hits = (before, hits0) if s == 0 else (rows[D * s - 1], maps[D * s - 1])
        scans.append(_t(HS.scan_of(spec, _np(hits), _np(row[:, ZCOL]))))
    xs, fed, after = _rebuild(p, before, rows, r['policy_actions'], h0, pending, r['dones'], 1, True, scans=scans)
    for s, x in enumerate(xs):
        got = r['policy_obs'][s]
        for name, lo, hi in (('obs', 0, 24), ('scan', 24, 39), ('action', 39, 51), ('frame 1', 51, 87), ('frame 2', 87, 123)):
            assert _same(got[:, lo:hi], x[:, lo:hi]), (s, name)
        assert _same(r['policy_means'][s], b.policy_eval(p, x)), s
    assert _same(b.policy_history, after) and float(r['policy_obs'][:, :, 24:39].abs().max()) > 0


@pytest.mark.parametrize('mode', ['plain', 'feet'])
def test_with_a_scan_the_plain_and_the_foot_term_kernels_equal_the_replayed_loop(mode):
    """policy_mlp_kernel<24> (scan and history, no learning half) and <26> (scan, history, foot terms), which no test above launches: one full
    tile of 16 rows and a tile of one row, two policy steps"""
    from gym_quadruped_amd.policy import HeightScan
    from test_gpu_policy_scan import ZCOL, _replay, _scan_twin
    n, D, L, feet = 17, 2, 2, mode == 'feet'
    K, S = 2 * D, 2
    a, b, hm_a, hm_b = _scan_twin(n, 'perlin', 3, 5, **(CMD if feet else {}))
    spec = HeightScan(3, 5, offset=0.3, clip=0.1, scale=5.0)
    p = _policy(L, 13, scan=spec, widths=(20, 12, 12))
    b.policy_history = torch.rand(n, L, p.hist_words, generator=torch.Generator(device=DEV).manual_seed(9), device=DEV) - 0.5
    if feet:
        b.feet_air_time = torch.rand(n, 4, device=DEV) * 0.05
    before, pending, h0, air = b._obs_buf.clone(), b._terminated.clone().bool(), b.policy_history.clone(), b.feet_air_time.clone()
    hits0 = hm_a.update_height_map().clone()     # the twin is in the same state: its rays, cast apart from the rollout
    if feet:
        reward = _spec()
        r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, noise_sigma=SIGMA, record_obs=True, record_actions=True, record_transitions=True, reward=reward)
    else:
        r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, record_obs=True, record_actions=True)
        assert set(r) == {'obs', 'obs_seq', 'actions', 'policy_actions'}
    code, _, played = b.closed_loop_status()
    assert code == 0 and played == n * K
    rows, term, maps = _replay(a, hm_a, b, r, K)
    scans = []
    for s in range(S):
        row, hits = (before, hits0) if s == 0 else (rows[D * s - 1], maps[D * s - 1])
        scans.append(_t(HS.scan_of(spec, _np(hits), _np(row[:, ZCOL]))))
    xs, fed, after = _rebuild(p, before, rows, r['policy_actions'], h0, pending, term, D, feet, scans=scans)
    for s, x in enumerate(xs):
        if feet:
            assert _same(r['policy_obs'][s], x), s
        assert _same(r['policy_means' if feet else 'policy_actions'][s], b.policy_eval(p, x)), s
    assert _same(b.policy_history, after)
    if feet:
        want_r, want_d, want_air, _ = _windows(b, reward, rows, term, r['actions'], r['policy_actions'], pending, D, air)
        assert torch.equal(r['dones'], want_d) and _same(r['rewards'], want_r) and _same(b.feet_air_time, want_air)


@pytest.mark.parametrize('D', [1, 4])
@pytest.mark.parametrize('n,step_waves', [(1, 0), (7, 0), (120, 0), (128, 0), (136, 0), (9, 2048)])
def test_edge_sizes_and_single_policy_steps(n, step_waves, D):
    L = 2
    a, b = _env(n=n, seed=3), _env(n=n, seed=3)
    a.reset(random=True); b.reset(random=True)
    p = _policy(L, 13)
    for K in (D, 2 * D, (L + 2) * D):
        before, pending = b._obs_buf.clone(), b._terminated.clone().bool()
        h0 = torch.zeros(n, L, p.hist_words, device=DEV) if b.policy_history is None else b.policy_history.clone()
        r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, record_obs=True, record_actions=True, step_waves=step_waves)
        code, _, played = b.closed_loop_status()
        assert code == 0 and played == n * K
        fed = torch.where(pending[:, None, None], torch.zeros_like(h0), h0)
        x0 = torch.cat([before[:, :IN_OBS], torch.zeros(n, 12, device=DEV), fed.reshape(n, -1)], dim=1)   # the hand-built first row
        want_a = b.policy_eval(p, x0)
        assert _same(r['policy_actions'][0], want_a)
        assert _same(r['actions'][0], _torque(b, want_a, before))
        rows, term = _replay_flags(a, b, r, K, STATE)
        xs, _, after = _rebuild(p, before, rows, r['policy_actions'], h0, pending, term, D, False)
        assert _same(xs[0], x0)
        for s, x in enumerate(xs):
            assert _same(r['policy_actions'][s], b.policy_eval(p, x)), (K, s)
        assert _same(b.policy_history, after), K


def _raw(env, m, hs, sc=None, K=4):
    from gym_quadruped_amd import _lib
    stream = torch.cuda.current_stream(env.device).cuda_stream
    _lib.check(env._L.gq_rollout_policy_hist(env._hbatch, K, C.byref(m), None if sc is None else C.byref(sc), C.byref(hs), 0, 0, 5.0, env._st, env._out, env._auto_cfg,
                                             env._episode.data_ptr(), env._lift_failed.data_ptr(), None, None, None, None, stream), 'gq_rollout_policy_hist')


def test_nothing_else_moved_reset_checkpoint_and_refusals():
    from gym_quadruped_amd import _lib
    n = 64
    a, b = _env(n=n, seed=5), _env(n=n, seed=5)
    a.reset(random=True); b.reset(random=True)
    p = _policy(3, 13)
    L, F = 3, p.hist_words
    r = b.rollout_policy(8, p, KP, KD, action_scale=SCALE, record_obs=True, record_actions=True)
    assert b.closed_loop_status()[2] == n * 8
    _replay_flags(a, b, r, 8, STATE)
    hist = b.policy_history.clone()
    assert hist.shape == (n, L, F) and float(hist.abs().max()) > 0
    # a history-less MlpPolicy, a GruPolicy and the mailbox rollout on the same batch still equal the step loop, and leave the history alone
    r = b.rollout_policy(8, PR.make_policy('odd', 'elu'), KP, KD, action_scale=SCALE, record_obs=True, record_actions=True)
    assert b.closed_loop_status()[2] == n * 8
    _replay_flags(a, b, r, 8, STATE)
    r = b.rollout_policy(8, G.make_policy('odd', 'elu'), KP, KD, action_scale=SCALE, record_obs=True, record_actions=True)
    assert b.closed_loop_status()[2] == n * 8
    _replay_flags(a, b, r, 8, STATE)
    r = b.rollout_closed_loop(10, KP, KD, mode='mailbox', record_obs=True, record_actions=True)
    assert b.closed_loop_status()[2] == n * 10
    _replay_flags(a, b, r, 10, STATE)
    assert _same(b.policy_history, hist)
    # reset of a mask empties exactly those envs' histories; the checkpoint carries the state; another (L, F) is refused until it is reassigned
    b.policy_history = torch.arange(1, n * L * F + 1, device=DEV).reshape(n, L, F).float()
    keep = b.policy_history.clone()
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[[0, 5, 63]] = True
    b.reset(env_ids=mask)
    assert (b.policy_history[mask] == 0).all() and torch.equal(b.policy_history[~mask], keep[~mask])
    sd = b.state_dict()
    assert torch.equal(sd['_policy_history'], b.policy_history)
    b.reset(random=True)
    assert (b.policy_history == 0).all()
    b.load_state_dict(sd)
    assert torch.equal(b.policy_history, sd['_policy_history'])
    with pytest.raises(ValueError, match='frames of'):
        b.rollout_policy(4, _policy(2, 13), KP, KD)
    with pytest.raises(ValueError, match='frames of'):
        b.rollout_policy(4, _policy(3, 24), KP, KD)
    b.policy_history = torch.zeros(n, 2, F, device=DEV)
    b.rollout_policy(4, _policy(2, 13), KP, KD)
    assert b.closed_loop_status()[2] == n * 4 and b.policy_history.shape == (n, 2, F) and float(b.policy_history.abs().max()) > 0
    # the library's refusals through the raw entry point; the batch steps normally after each
    a, b = _env(n=n, seed=6), _env(n=n, seed=6)
    a.reset(random=True); b.reset(random=True)
    state, ctl = torch.zeros(n, 2, L, F, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)

    def blocks(**hk):
        m = b._policy_struct(p)
        m.decimation = 4
        hs = p._hist_struct(state, ctl)
        for k, v in hk.items():
            setattr(hs, k, v)
        return m, hs
    act = torch.randn(n, 12, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 20
    for hk, msg in ((dict(struct_size=8), 'GqPolicyHist.struct_size'), (dict(frames=0), 'frames = 0'), (dict(cols=0), 'cols = 0'), (dict(cols=25), 'cols = 25'),
                    (dict(in_dim=112), 'in_dim = 112'), (dict(frames=9, in_dim=36 + 9 * 25), 'columns'), (dict(state=None), 'state'), (dict(ctl=None), 'ctl')):
        with pytest.raises(_lib.GqError, match=msg):
            _raw(b, *blocks(**hk))
        a.step(act); b.step(act)
        for f in STATE:
            assert torch.equal(getattr(a, f), getattr(b, f)), (msg, f)
    assert not state.any() and not ctl.any(), 'a refused call writes nothing'
    _raw(b, *blocks())
    assert b.closed_loop_status()[2] == n * 4 and bool(((ctl & 2) != 0).all()) and float(state.abs().max()) > 0
