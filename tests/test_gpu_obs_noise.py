"""GPU tests of the sensor noise on the in-loop policy's input row (include/gq.h gq_rollout_policy_noise / gq_obs_noise_eval,
QuadrupedEnv.rollout_policy(obs_noise=ObsNoise(...)) / obs_noise_eval, csrc/gq_policy_noise.h), bit for bit, on 70 envs (full 16-row tiles, a
partial one, lanes beyond one wavefront pass), K = 16, D = 4, with an action scale under which robots fall and re-spawn inside the call:

* the law on the device is the numpy reference (tests/obs_noise_ref.py);
* 'policy_obs_clean' is the true row, 'policy_obs' the law on it under (step0 + s D, env id), 'policy_means' the network on 'policy_obs';
* the recorded torques are the joint law on the TRUE joint state, and replayed through `step` on a twin they leave the same state, flags and
  observations; rewards and dones are the reference windows on the true rows;
* ObsNoise(0.0) is the call without noise, in every record;
* a history's frames - in the row and in env.policy_history - hold the noisy current blocks, zero where dones says so.
"""
import numpy as np
import pytest
import torch

import height_scan_ref as HS
import obs_noise_ref as R
import policy_gru_ref as G
import policy_mlp_ref as PR
import reward_ref as RW
from learn_windows import _replay_flags, _same
from test_gpu_closed_loop import STATE, _env, _twin

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, K, D = 70, 16, 4
S = K // D
KP, KD, SCALE = 25.0, 0.8, 2.0   # (four times the scale of the other policy tests: robots fall inside the call)
MODES = [('plain', 'uniform'), ('plain', 'normal'), ('learn', 'uniform'), ('learn', 'normal'), ('gru', 'normal'), ('scan', 'uniform'), ('hist', 'normal')]


def _np(t):
    return t.detach().cpu().numpy()


def _t(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


def _amp(in_obs):
    """the first and the last observation column noised, zeros in between, joint angles and velocities at different amplitudes"""
    a = np.zeros(in_obs, dtype=np.float32)
    a[0:12:2], a[12:24], a[0], a[-1] = 0.02, 0.5, 0.05, 0.25
    a[1] = a[13] = 0.0
    return a


def _setup(mode):
    """(a, b, policy, maps of a and b or None, rollout keywords) of a mode: twins in the same state after 60 steps of random torques"""
    from gym_quadruped_amd.policy import HeightScan
    if mode == 'scan':
        from test_gpu_policy_scan import _scan_twin
        a, b, hm_a, hm_b = _scan_twin(N, 'perlin', 3, 5)
        return a, b, HS.make_mlp(24, HeightScan(3, 5, offset=0.3, clip=0.1, scale=5.0)), (hm_a, hm_b), dict(record_transitions=True)
    if mode == 'hist':
        from test_gpu_policy_hist import _policy
        a, b = _twin('mini_cheetah', N, warm=60, state_obs_names=RW.OBS_NAMES)
        return a, b, _policy(2, 13), None, dict(record_transitions=True, reward=RW.specs()['all'])
    a, b = _twin('mini_cheetah', N, warm=60, state_obs_names=RW.OBS_NAMES)
    if mode == 'gru':
        return a, b, G.make_policy('odd'), None, dict(record_transitions=True)
    kw = dict(record_transitions=True, reward=RW.specs()['all']) if mode == 'learn' else {}
    return a, b, PR.make_policy('odd', 'elu'), None, kw


def _noise(p, kind):
    from gym_quadruped_amd.policy import ObsNoise
    return ObsNoise(_amp(p.in_obs), kind=kind, scan_amp=0.03 if getattr(p, 'height_scan', None) is not None else 0.0)


def _amps(p, nz):
    cells = p.height_scan.cells if getattr(p, 'height_scan', None) is not None else 0
    return R.amp_row(nz.table(p), p.in_obs, cells, p.in_dim, nz.scan_amp)


def _torque(env, a_held, row):
    q0 = env._key_qpos[7:19].float()
    return KP * ((q0 + SCALE * a_held) - row[:, 0:12]) + KD * (0 - row[:, 12:24]) + 0


@pytest.mark.parametrize('kind', ['uniform', 'normal'])
def test_the_law_on_the_device_is_the_reference(kind):
    """gq_obs_noise_eval against numpy, bit for bit, at 1, 15, 16, 17 and 131 rows: an MLP row with the fed-back action and a row with a scan"""
    from gym_quadruped_amd.policy import HeightScan, ObsNoise
    env = _env(n=4, seed=5)
    rng = np.random.default_rng(2)
    for p in (PR.make_policy('odd', 'elu'), HS.make_mlp(24, HeightScan(3, 5))):
        nz = _noise(p, kind)
        amps = _amps(p, nz)
        for n in (1, 15, 16, 17, 131):
            rows = rng.standard_normal((n, p.in_dim)).astype(np.float32)
            rows[0, 1] = -0.0   # an amplitude of 0: the word, the sign of a zero included, is untouched
            steps = rng.integers(0, 2 ** 31 - 1, n)
            ids = rng.integers(0, 2 ** 20, n)
            steps[0], ids[0] = 2 ** 31 - 1, 0
            got = _np(env.obs_noise_eval(p, nz, _t(rows), steps, ids))
            want = R.apply(rows, amps, kind, int(env._seed), steps, ids)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, p.in_dim, n)
            assert (got != rows)[:, amps > 0].mean() > 0.99 and np.array_equal(got[:, amps == 0].view(np.uint32), rows[:, amps == 0].view(np.uint32))
    with pytest.raises(ValueError, match='in_obs = 37'):
        env.obs_noise_eval(PR.make_policy('odd', 'elu'), ObsNoise(np.ones(36)), torch.zeros(1, 49, device=DEV), [0], [0])


@pytest.mark.parametrize('mode,kind', MODES)
def test_the_noisy_rollout_feeds_the_law_and_leaves_the_step_loops_state(mode, kind):
    a, b, p, maps, kw = _setup(mode)
    nz, learn, gids = _noise(p, kind), 'reward' in kw, np.arange(N)
    amps = _amps(p, nz)
    if mode == 'hist':
        b.policy_history = torch.rand(N, 2, p.hist_words, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV) + 0.5
    before, pending = b._obs_buf.clone(), b._terminated.clone().bool()
    step0, seed = int(b._launches) & 0x7fffffff, int(b._seed)
    if maps is not None:
        hits0 = maps[0].update_height_map().clone()   # the twin is in the same state: its rays, cast apart from the rollout
    r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, record_obs=True, record_actions=True, obs_noise=nz, **kw)
    code, _, played = b.closed_loop_status()
    assert code == 0 and played == N * K
    want_keys = {'obs', 'obs_seq', 'actions', 'policy_actions'}
    if kw:
        want_keys |= {'policy_obs', 'policy_obs_clean', 'policy_means'} | ({'rewards', 'dones'} if learn else set()) | ({'policy_hidden'} if mode == 'gru' else set())
    assert set(r) == want_keys
    # 5. the recorded torques through `step` on the twin: the same state, flags and observation bits, re-spawns included
    if maps is not None:
        from test_gpu_policy_scan import _replay
        rows, term, hit_seq = _replay(a, maps[0], b, r, K)
    else:
        rows, term = _replay_flags(a, b, r, K, STATE)
    win = term.view(S, D, N).any(dim=1)
    assert bool(win.any()) and bool((~win).any()), 'the workload must hold a window with a termination and one without'
    assert bool(term[:K - 1].any()), 'an env re-spawns inside the call'
    pol, acts = r['policy_actions'], r['actions']
    true_row = lambda s: before if s == 0 else rows[D * s - 1]
    # ... and every torque is the joint law on the TRUE joint state (columns that carry noise in the row the network is fed)
    for k in range(K):
        assert _same(acts[k], _torque(b, pol[k // D], before if k == 0 else rows[k - 1])), k
    if learn:
        from test_gpu_learn_rollout import _windows
        want_r, want_d = _windows(b, kw['reward'], rows, term, acts, pol, pending, D)
        assert torch.equal(r['dones'], want_d) and _same(r['rewards'], want_r), 'rewards and dones read the true rows'
        assert torch.equal(r['dones'], win) and bool(r['dones'].any()) and bool((~r['dones']).any())
    for s in range(S):
        steps = np.full(N, step0 + s * D)
        if not kw:   # the plain kernel keeps no record of the row: rebuilt from the replayed loop, the network on it is the action
            clean = torch.cat([true_row(s)[:, :p.in_obs], torch.zeros(N, 12, device=DEV) if s == 0 else pol[s - 1]], dim=1)
            fed = _t(R.apply(_np(clean), amps, kind, seed, steps, gids))
            assert not _same(fed, clean) and _same(pol[s], b.policy_eval(p, fed)), s
            continue
        clean, noisy = r['policy_obs_clean'][s], r['policy_obs'][s]
        # 2. the clean record is the true row on the fed columns (and the clean scan, the fed-back action)
        assert _same(clean[:, :p.in_obs], true_row(s)[:, :p.in_obs]), s
        at = p.in_obs
        if mode == 'scan':
            from test_gpu_policy_scan import ZCOL
            hits = hits0 if s == 0 else hit_seq[D * s - 1]
            assert _same(clean[:, at:at + 15], _t(HS.scan_of(p.height_scan, _np(hits), _np(true_row(s)[:, ZCOL])))), s
            at += 15
        assert _same(clean[:, at:at + 12], torch.zeros(N, 12, device=DEV) if s == 0 else pol[s - 1]), s
        # 3. the fed record is the law on the clean one
        assert _same(noisy, _t(R.apply(_np(clean), amps, kind, seed, steps, gids))), s
        changed = _np(noisy).view(np.uint32) != _np(clean).view(np.uint32)
        assert changed[:, amps > 0].mean() > 0.99 and not changed[:, amps == 0].any(), s
        # 4. the network on the fed record is the recorded mean
        if mode == 'gru':
            want, _ = b.policy_eval(p, noisy, hidden=r['policy_hidden'][s])
        else:
            want = b.policy_eval(p, noisy)
        assert _same(r['policy_means'][s], want) and _same(pol[s], want), s
    if mode == 'hist':
        # 7. the frames: in the row, frame_i at step s is the NOISY current block of step s - i, zero from a termination on; after the call
        # env.policy_history holds the blocks of the last policy steps, zero where dones says so (the closing visit included)
        pobs, dones, c, col0, F = r['policy_obs'], r['dones'], p.hist_cols, p.in_obs + 12, p.hist_words
        cur = torch.cat([pobs[:, :, :c], pobs[:, :, p.in_obs:p.in_obs + 12]], dim=2)   # [S, N, F] as fed
        assert not _same(cur[:, :, :c], r['policy_obs_clean'][:, :, :c])
        zero = torch.zeros(N, F, device=DEV)
        for s in range(1, S):
            f1 = torch.where(dones[s - 1][:, None], zero, cur[s - 1])
            assert _same(pobs[s][:, col0:col0 + F], f1), s
            if s >= 2:
                f2 = torch.where((dones[s - 1] | dones[s - 2])[:, None], zero, cur[s - 2])
                assert _same(pobs[s][:, col0 + F:], f2), s
        after = b.policy_history
        assert _same(after[:, 0], torch.where(dones[S - 1][:, None], zero, cur[S - 1]))
        assert _same(after[:, 1], torch.where((dones[S - 1] | dones[S - 2])[:, None], zero, cur[S - 2]))


@pytest.mark.parametrize('mode', ['plain', 'learn', 'gru', 'scan', 'hist'])
def test_zero_amplitude_is_the_call_without_noise_in_every_record(mode):
    from gym_quadruped_amd.policy import ObsNoise
    a, b, p, maps, kw = _setup(mode)
    if mode == 'hist':
        a.policy_history = torch.rand(N, 2, p.hist_words, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV) + 0.5
        b.policy_history = a.policy_history.clone()
    call = dict(action_scale=SCALE, decimation=D, noise_sigma=0.3, record_obs=True, record_actions=True, **kw)
    ra = a.rollout_policy(K, p, KP, KD, **call)
    rb = b.rollout_policy(K, p, KP, KD, obs_noise=ObsNoise(0.0, kind='normal'), **call)
    assert a.closed_loop_status()[2] == N * K and b.closed_loop_status()[2] == N * K
    assert set(rb) - set(ra) == ({'policy_obs_clean'} if kw else set()) and set(ra) <= set(rb)
    for key, v in ra.items():
        if key != 'obs':
            assert v.dtype == rb[key].dtype and (torch.equal(v, rb[key]) if v.dtype == torch.bool else _same(v, rb[key])), key
    if kw:
        assert _same(rb['policy_obs_clean'], rb['policy_obs'])
    for f in STATE:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    if mode == 'hist':
        assert _same(a.policy_history, b.policy_history)
    if mode == 'gru':
        assert _same(a.policy_hidden, b.policy_hidden)


def test_refusals_leave_the_batch_usable():
    from gym_quadruped_amd import _lib
    from gym_quadruped_amd.policy import ObsNoise
    a, b = _env(n=16, seed=6), _env(n=16, seed=6)
    a.reset(random=True); b.reset(random=True)
    p = PR.make_policy('odd', 'elu', in_obs=24)
    for bad, msg in ((ObsNoise(np.ones(23)), 'in_obs = 24'), (ObsNoise(1.0, scan_amp=0.5), 'no height scan'), (0.5, 'ObsNoise')):
        with pytest.raises(ValueError, match=msg):
            b.rollout_policy(4, p, KP, KD, obs_noise=bad)
    nz = ObsNoise(0.1)
    st = nz._struct(p, b.device)
    import ctypes as C
    stream = torch.cuda.current_stream(b.device).cuda_stream

    def raw(**hk):
        m = b._policy_struct(p)
        m.decimation = 4
        blk = nz._struct(p, b.device)
        for k, v in hk.items():
            setattr(blk, k, v)
        _lib.check(b._L.gq_rollout_policy_noise(b._hbatch, 4, C.byref(m), None, None, None, C.byref(blk), 0, 0, 5.0, b._st, b._out, b._auto_cfg, b._episode.data_ptr(),
                                                b._lift_failed.data_ptr(), None, None, None, None, stream), 'gq_rollout_policy_noise')
    act = torch.randn(16, 12, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 20
    for hk, msg in ((dict(struct_size=8), 'GqPolicyNoise.struct_size'), (dict(kind=2), 'kind is 2'), (dict(n_amp=23), 'n_amp = 23'), (dict(amp=None), 'amp'),
                    (dict(scan_amp=-1.0), 'scan_amp'), (dict(scan_amp=float('nan')), 'scan_amp'), (dict(scan_amp=0.5), 'no height scan'), (dict(policy_obs_clean=act.data_ptr()), 'policy_obs_clean')):
        with pytest.raises(_lib.GqError, match=msg):
            raw(**hk)
        a.step(act); b.step(act)
        for f in STATE:
            assert torch.equal(getattr(a, f), getattr(b, f)), (msg, f)
    assert st.n_amp == 24
    raw()
    assert b.closed_loop_status()[2] == 16 * 4
