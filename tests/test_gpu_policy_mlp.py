"""GPU tests of the MLP policy inside the closed-loop rollout (include/gq.h gq_rollout_policy / gq_policy_mlp_eval,
QuadrupedEnv.rollout_policy / policy_eval, csrc/gq_policy_mlp.h):

* the matrix-core form of the network (mlp_tile_forward) and the plain fmaf loop that defines it (mlp_row_forward) give the same bits
  on the device - and, for relu networks, the bits of the host program; a row's result does not depend on its tile;
* the loop is closed: every recorded policy action is the network on the recorded observation row and the previous action, every
  recorded torque the joint-impedance law on the held action, bit for bit;
* the recorded torques replayed through the step loop leave the same state, flags and observation rows, bit for bit - re-spawns
  included, at the batch sizes that put 15, 16 and 17 envs into one policy tile, with far more step wavefronts than envs;
* the exploration noise is sigma * z of the documented Philox stream; everything that cannot be done is refused with a message and
  leaves the batch usable.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_mlp_ref as R
from test_gpu_closed_loop import STATE, _env, _twin

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KP, KD, SCALE = 25.0, 0.8, 0.25
ROW_COUNTS = (1, 15, 16, 17, 131)


@pytest.fixture(scope='module')
def handle():
    env = _env(n=16, seed=1)
    env.reset(random=True)
    return env


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('act,out', [('relu', None), ('elu', 'tanh'), ('tanh', None)])
@pytest.mark.parametrize('shape', ['odd', 'wide'])
def test_tile_and_scalar_forms_have_the_same_bits(handle, shape, act, out):
    p = R.make_policy(shape, act, out)
    rows = R.rows_for(p, max(ROW_COUNTS))
    dev_rows = torch.from_numpy(rows).to(DEV)
    host = torch.from_numpy(np.ascontiguousarray(R.host_forward(p, rows)[-1])).to(DEV) if act == 'relu' else None
    ref, bound = R.network_bound(p, rows)
    for n in ROW_COUNTS:
        tile, scalar = handle.policy_eval(p, dev_rows[:n], impl='tile'), handle.policy_eval(p, dev_rows[:n], impl='scalar')
        assert tile.shape == (n, 12) and _same(tile, scalar), (n, float((tile - scalar).abs().max()))
        if host is not None:
            assert _same(tile, host[:n]), n
        err = np.abs(tile.cpu().numpy().astype(np.float64) - ref[:n])
        print(f'{shape} {act} n={n}: worst error / bound {float((err / bound[:n]).max()):.3f}')
        assert (err <= bound[:n]).all()


@pytest.mark.parametrize('shape,act', [('odd', 'elu'), ('wide', 'relu')])
def test_a_row_s_result_does_not_depend_on_its_tile(handle, shape, act):
    p = R.make_policy(shape, act)
    mine = torch.from_numpy(R.rows_for(p, 17, seed=2)).to(DEV)
    alone = handle.policy_eval(p, mine)
    for at in (0, 5, 19, 114):   # across tile boundaries, in other slots, at the ragged end
        rows = torch.from_numpy(R.rows_for(p, 131, seed=3 + at)).to(DEV) * 5
        rows[at:at + 17] = mine
        assert _same(handle.policy_eval(p, rows)[at:at + 17], alone), at
    perm = torch.randperm(17, device=DEV)
    assert _same(handle.policy_eval(p, mine[perm]), alone[perm])


def _torque(env, a_held, row):
    q0 = env._key_qpos[7:19].float()
    q, qd = row[:, 0:12], row[:, 12:24]
    return KP * ((q0 + SCALE * a_held) - q) + KD * (0 - qd) + 0


def test_the_loop_is_closed():
    n, K, D = 200, 12, 4
    env = _env(n=n, seed=7)
    env.reset(random=True)
    p = R.make_policy('odd', 'elu')
    before = env._obs_buf.clone()
    r = env.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, record_obs=True, record_actions=True)
    code, _, played = env.closed_loop_status()
    assert code == 0 and played == n * K
    obs, acts, pol = r['obs_seq'], r['actions'], r['policy_actions']
    assert pol.shape == (K // D, n, 12) and acts.shape == (K, n, 12) and obs.shape == (K, n, env._obs_dim)
    for s in range(K // D):
        row = before if s == 0 else obs[D * s - 1]
        prev = torch.zeros(n, 12, device=DEV) if s == 0 else pol[s - 1]
        want = env.policy_eval(p, torch.cat([row[:, :p.in_obs], prev], dim=1))
        assert _same(pol[s], want), s
    for k in range(K):
        assert _same(acts[k], _torque(env, pol[k // D], before if k == 0 else obs[k - 1])), k
    assert torch.isfinite(pol).all() and float(pol.abs().max()) > 0.01


def _replay(a, b, r, K):
    rows = []
    for k in range(K):
        a.step(r['actions'][k])
        rows.append(a._obs_buf.clone())
    torch.cuda.synchronize()
    for f in STATE:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    if r['obs_seq'] is not None:
        assert torch.equal(torch.stack(rows), r['obs_seq'])


@pytest.mark.parametrize('robot,n,K', [('mini_cheetah', 131, 24), ('go2', 1000, 20)])
def test_rollout_equals_the_step_loop_with_the_recorded_torques(robot, n, K):
    a, b = _twin(robot, n)
    p = R.make_policy('odd', 'elu')
    r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=4, record_obs=True, record_actions=True)
    code, _, played = b.closed_loop_status()
    assert code == 0 and played == n * K
    _replay(a, b, r, K)
    assert torch.isfinite(b.qpos).all()
    print(f'{robot} n={n}: episodes max {int(b._episode.max())}')
    if n == 1000:
        assert int(b._episode.max()) > 1, 'the rollout must contain auto-resets'
    # and the batch is an ordinary batch afterwards
    a.step(r['actions'][0]); b.step(r['actions'][0])
    torch.cuda.synchronize()
    assert torch.equal(a._qpos, b._qpos) and torch.equal(a._obs_buf, b._obs_buf)


@pytest.mark.parametrize('D', [1, 4])
@pytest.mark.parametrize('n,step_waves', [(1, 0), (7, 0), (120, 0), (128, 0), (136, 0), (9, 2048)])
def test_edge_sizes_and_single_policy_steps(n, step_waves, D):
    """15, 16 and 17 envs in a queue (n = 120, 128, 136 over 8 queues), fewer envs than XCDs, one policy step per call, and pop
    tickets far ahead of the pushes"""
    a, b = _env(n=n, seed=3), _env(n=n, seed=3)
    a.reset(random=True); b.reset(random=True)
    p = R.make_policy('odd', 'relu')
    for K in (D, 2 * D):
        before = b._obs_buf.clone()
        r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, decimation=D, record_obs=True, record_actions=True, step_waves=step_waves)
        code, _, played = b.closed_loop_status()
        assert code == 0 and played == n * K
        want = b.policy_eval(p, torch.cat([before[:, :p.in_obs], torch.zeros(n, 12, device=DEV)], dim=1))
        assert _same(r['policy_actions'][0], want)
        assert _same(r['actions'][0], _torque(b, want, before))
        _replay(a, b, r, K)


def test_noise_is_sigma_z_of_the_documented_stream_and_the_clip_holds():
    """a = net(x) + sigma * z, each operation rounded: the recorded action equals float32(net(x)) + float32(sigma * z) bit for bit (the
    difference a - net(x) itself is that product only up to the rounding of the sum, so the sum is what is compared)"""
    n, K, D, sigma = 40, 8, 4, 0.3
    a, b = _twin('mini_cheetah', n)
    p = R.make_policy('odd', 'tanh')
    for clip in (None, 0.2):
        before, step0, seed = b._obs_buf.clone(), int(b._launches) & 0x7fffffff, int(b._seed)
        r = b.rollout_policy(K, p, KP, KD, action_scale=SCALE, action_clip=clip, decimation=D, noise_sigma=sigma, record_obs=True, record_actions=True)
        assert b.closed_loop_status()[2] == n * K
        pol, obs = r['policy_actions'], r['obs_seq']
        for s in range(K // D):
            row = before if s == 0 else obs[D * s - 1]
            prev = torch.zeros(n, 12, device=DEV) if s == 0 else pol[s - 1]
            net = b.policy_eval(p, torch.cat([row[:, :p.in_obs], prev], dim=1))
            z = torch.from_numpy(R.policy_noise(seed, step0 + D * s, n)).to(DEV)
            want = net + torch.tensor(sigma, dtype=torch.float32, device=DEV) * z
            if clip is not None:
                want = want.clamp(-clip, clip)
            assert _same(pol[s], want), (clip, s)
            assert float(z.std()) > 0.8 and float((pol[s] - net).abs().max()) > 0.05
        _replay(a, b, r, K)


def _raw(env, m, K=4):
    from gym_quadruped_amd import _lib
    stream = torch.cuda.current_stream(env.device).cuda_stream
    _lib.check(env._L.gq_rollout_policy(env._hbatch, K, C.byref(m), 0, 0, 5.0, env._st, env._out, env._auto_cfg, env._episode.data_ptr(), env._lift_failed.data_ptr(),
                                        None, None, stream), 'gq_rollout_policy')


def test_what_cannot_be_done_is_refused_and_the_batch_stays_usable():
    from gym_quadruped_amd import _lib
    from gym_quadruped_amd.policy import MlpPolicy
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    n = 64
    a, env = _env(n=n, seed=5), _env(n=n, seed=5)
    a.reset(random=True); env.reset(random=True)
    p = R.make_policy('odd', 'relu')
    z = np.zeros
    with pytest.raises(ValueError, match='linear layers'):   # more than 4 layers
        MlpPolicy([z((24, 24), np.float32)] * 4 + [z((24, 12), np.float32)], [z(24, np.float32)] * 4 + [z(12, np.float32)])
    with pytest.raises(ValueError, match='256'):             # a width out of range
        MlpPolicy([z((24, 300), np.float32), z((300, 12), np.float32)], [z(300, np.float32), z(12, np.float32)])
    with pytest.raises(ValueError, match='12'):              # an output width other than 12
        MlpPolicy([z((24, 11), np.float32)], [z(11, np.float32)])

    def struct(**kw):   # the same refusals from the library, for a binding that does not go through MlpPolicy
        m = env._policy_struct(p)
        m.decimation = 4
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    for kw, msg in ((dict(n_layers=5), 'linear layers'), (dict(width=(C.c_int32 * 4)(20, 300, 12, 0)), 'outputs'), (dict(width=(C.c_int32 * 4)(20, 33, 11, 0)), '12'),
                    (dict(in_obs=env._obs_dim + 1), 'in_obs'), (dict(blob=None), 'blob is null'), (dict(decimation=3), 'multiple'), (dict(blob_floats=7), 'blob_floats'),
                    (dict(struct_size=8), 'stale')):
        with pytest.raises(_lib.GqError, match=msg):
            _raw(env, struct(**kw))
    with pytest.raises(ValueError, match='observation columns'):   # in_obs beyond the user's row (39 columns)
        env.rollout_policy(4, R.make_policy('wide', 'relu'), KP, KD)
    with pytest.raises(ValueError, match='multiple'):
        env.rollout_policy(6, p, KP, KD, decimation=4)
    with pytest.raises(_lib.GqError, match='qpos_js'):       # missing joint columns
        e2 = _env(n=8, state_obs_names=('base_pos', 'base_lin_vel', 'base_ang_vel'))
        e2.reset(random=True)
        e2.rollout_policy(4, R.make_policy('single', 'relu', in_obs=9), KP, KD)
    with pytest.raises(_lib.GqError, match='Newton'):        # PGS
        e3 = QuadrupedEnv('mini_cheetah', num_envs=8, device=DEV, solver='pgs', auto_reset='next_step', state_obs_names=env.state_obs_names)
        e3.reset(random=True)
        e3.rollout_policy(4, p, KP, KD)
    with pytest.raises(_lib.GqError, match='next-step'):     # same-step auto-reset
        e4 = QuadrupedEnv('mini_cheetah', num_envs=8, device=DEV, solver='newton', auto_reset='same_step', state_obs_names=env.state_obs_names)
        e4.reset(random=True)
        e4.rollout_policy(4, p, KP, KD)
    # the batch steps normally afterwards, the MLP rollout works on it, and a plain closed-loop rollout still equals the step loop
    act = torch.randn(n, 12, device=DEV) * 20
    a.step(act); env.step(act)
    r = env.rollout_policy(8, p, KP, KD, record_obs=True, record_actions=True)
    _replay(a, env, r, 8)
    r = env.rollout_closed_loop(10, KP, KD, mode='mailbox', record_obs=True, record_actions=True)
    assert env.closed_loop_status()[2] == n * 10
    _replay(a, env, r, 10)
