"""The sensor noise on the in-loop policy's input row without a GPU (gym_quadruped_amd/policy.py ObsNoise, csrc/gq_policy_noise.h, include/gq.h
GqPolicyNoise): policy_row_value<.., NOISE = true> played on the host (tests/obs_noise_host.cpp) against the numpy restatement of the law
(tests/obs_noise_ref.py) bit for bit, histories over four policy steps, the independence of the draws, a sanity bound on the reference's
draws, ObsNoise's refusals, and the new struct and entry points of the ABI."""
import ctypes

import numpy as np
import pytest

import obs_noise_ref as R
from height_scan_ref import scan_law
from philox_ref import philox4x32

SEED = 0x1234_5678_9abc_def1
SCAN_LAW = (0.3, 0.8, 2.5)   # offset, clip, scale


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _play(in_obs, cells, feed_last, L, cols, kind, amp, scan_amp=0.0, steps=1, n=5, seed=3, step0=1000, D=4, reverse=False, obs=None):
    """random inputs through the host program, and everything the checks need next to its answer"""
    rng = np.random.default_rng(seed)
    od = min(in_obs + 3, 256)
    col_z = od - 1   # the base's z may lie beyond in_obs
    F = cols + (12 if feed_last else 0) if L else 0
    gids = (7 + 3 * np.arange(n)).astype(np.uint32)
    shift, scale = rng.standard_normal(in_obs).astype(np.float32), (0.5 + rng.random(in_obs)).astype(np.float32)
    if obs is None:
        obs = rng.standard_normal((steps, n, od)).astype(np.float32)
    last = rng.standard_normal((steps, n, 12)).astype(np.float32)
    hits = rng.standard_normal((steps, n, cells, 3)).astype(np.float32)
    store = rng.standard_normal((n, 2, L, F)).astype(np.float32)
    ctl = (2 | (np.arange(n) & 1)).astype(np.float32)   # VALID, both parities
    got = R.host_play(in_obs, od, col_z, cells, feed_last, L, cols, kind, SEED, step0, D, gids, amp, scan_amp, shift, scale, SCAN_LAW, store, ctl, obs, last, hits,
                      reverse=reverse)
    in_dim = got['rec'].shape[2]
    amps = R.amp_row(amp, in_obs, cells, in_dim, scan_amp)
    return dict(got=got, obs=obs, last=last, hits=hits, store=store, ctl=ctl.astype(np.int32), gids=gids, shift=shift, scale=scale, amps=amps, in_dim=in_dim,
                col_z=col_z, F=F, step0=step0, D=D)


def _check_step(p, s, in_obs, cells, feed_last, L, cols, kind, frames_before):
    """step s of a play against the reference: the clean record is the row's true words, the noisy one the law on it, the words fed shift / scale
    of the noisy one.  frames_before [n, L, F]: the frames the step is fed.  Returns the frames fed at the next step."""
    got, n = p['got'], p['obs'].shape[1]
    f12 = 12 if feed_last else 0
    clean = np.zeros((n, p['in_dim']), dtype=np.float32)
    clean[:, :in_obs] = p['obs'][s][:, :in_obs]
    if cells:
        clean[:, in_obs:in_obs + cells] = scan_law(p['obs'][s][:, p['col_z']][:, None], p['hits'][s][:, :, 2], *SCAN_LAW)
    if feed_last:
        clean[:, in_obs + cells:in_obs + cells + 12] = p['last'][s]
    col0 = in_obs + cells + f12
    if L:
        clean[:, col0:] = frames_before.reshape(n, -1)
    assert np.array_equal(bits(got['clean'][s]), bits(clean)), f'step {s}: the clean record holds the true words'
    steps = np.full(n, p['step0'] + s * p['D'])
    want = R.apply(clean, p['amps'], kind, SEED, steps, p['gids'])
    assert np.array_equal(bits(got['rec'][s]), bits(want)), f'step {s}: the record is the law on the true row, bit for bit'
    fed = want.copy()
    fed[:, :in_obs] = (want[:, :in_obs] - p['shift']) * p['scale']
    for i in range(L):
        c = col0 + i * p['F']
        fed[:, c:c + cols] = (want[:, c:c + cols] - p['shift'][:cols]) * p['scale'][:cols]
    assert np.array_equal(bits(got['fed'][s][:, :p['in_dim']]), bits(fed)), f'step {s}: shift / scale act on the noisy word'
    assert not got['fed'][s][:, p['in_dim']:].any()
    if not L:
        return None
    cur = np.concatenate([want[:, :cols], want[:, in_obs + cells:in_obs + cells + f12]], axis=1)   # the current block AS FED: noisy
    return np.concatenate([cur[:, None, :], frames_before[:, :-1]], axis=1)


def _frames(store, ctl):
    """the frames [n, L, F] a store feeds: buffer ctl & 1, zeros without VALID"""
    n = store.shape[0]
    f = store[np.arange(n), ctl & 1].copy()
    f[(ctl & 2) == 0] = 0
    return f


@pytest.mark.parametrize('kind', ['uniform', 'normal'])
@pytest.mark.parametrize('in_obs', [1, 45, 244])
def test_host_row_equals_the_reference_bit_for_bit(in_obs, kind):
    """the first and the last observation column noised, a zero amplitude in between (in_obs = 1: the one column), with the fed-back action"""
    amp = np.zeros(in_obs, dtype=np.float32)
    amp[0], amp[-1] = 0.75, 1.5 if in_obs > 1 else 0.75
    if in_obs > 4:
        amp[2] = 1e-3
    for reverse in (False, True):
        p = _play(in_obs, 0, True, 0, 0, kind, amp, reverse=reverse)
        _check_step(p, 0, in_obs, 0, True, 0, 0, kind, None)
        rec, clean = p['got']['rec'][0], p['got']['clean'][0]
        changed = bits(rec) != bits(clean)
        assert changed[:, :in_obs][:, amp > 0].all() and not changed[:, :in_obs][:, amp == 0].any() and not changed[:, in_obs:].any()


@pytest.mark.parametrize('kind', ['uniform', 'normal'])
def test_host_row_with_scan_and_history_at_256_columns(kind):
    in_obs, cells, L, cols = 45, 15, 4, 34
    amp = np.zeros(in_obs, dtype=np.float32)
    amp[[0, 7, 33, 34, 44]] = (0.5, 0.0625, 2.0, 1.0, 0.25)   # columns inside and outside the frames' cols
    p = _play(in_obs, cells, True, L, cols, kind, amp, scan_amp=0.125)
    assert p['in_dim'] == 256
    _check_step(p, 0, in_obs, cells, True, L, cols, kind, _frames(p['store'], p['ctl']))
    rec, clean = p['got']['rec'][0], p['got']['clean'][0]
    changed = bits(rec) != bits(clean)
    assert changed[:, in_obs:in_obs + cells].all(), 'every scan column is noised'
    assert not changed[:, in_obs + cells:].any(), 'the fed-back action and the frames are not'


@pytest.mark.parametrize('kind', ['uniform', 'normal'])
def test_a_negative_zero_under_zero_amplitude_stays_negative_zero(kind):
    in_obs = 6
    obs = np.full((1, 3, in_obs + 3), -0.0, dtype=np.float32)
    amp = np.array([1.0, 0, 0, 0, 0, 1.0], dtype=np.float32)
    p = _play(in_obs, 0, False, 0, 0, kind, amp, n=3, obs=obs)
    rec = bits(p['got']['rec'][0])
    assert (rec[:, 1:5] == 0x80000000).all(), 'amplitude 0: the word is untouched, not o + 0'
    assert (rec[:, [0, 5]] != 0x80000000).all()
    # the law's sum itself would have lost the sign: -0.0 + 0 * n = +0.0
    assert bits(np.float32(-0.0) + np.float32(0.0) * np.float32(0.5)) == 0


@pytest.mark.parametrize('kind', ['uniform', 'normal'])
@pytest.mark.parametrize('cells', [0, 15])
def test_history_over_four_policy_steps_holds_the_noisy_block_and_is_not_noised_twice(cells, kind):
    in_obs, L, cols, steps = 9, 2, 5, 4
    amp = np.array([0.5, 0, 1.0, 0.25, 0.125, 0, 0, 0, 2.0], dtype=np.float32)
    p = _play(in_obs, cells, True, L, cols, kind, amp, scan_amp=0.5 if cells else 0.0, steps=steps, n=7)
    frames = _frames(p['store'], p['ctl'])
    ctl = p['ctl'].copy()
    for s in range(steps):
        nxt = _check_step(p, s, in_obs, cells, True, L, cols, kind, frames)
        ctl = ((ctl & 1) ^ 1) | 2
        assert np.array_equal(p['got']['ctl'][s].astype(np.int32), ctl)
        assert np.array_equal(bits(_frames(p['got']['store'][s], ctl)), bits(nxt)), f'after step {s} the store holds the noisy current block, newest first'
        frames = nxt
    rec, clean = p['got']['rec'], p['got']['clean']
    col0 = in_obs + cells + 12
    for s in range(steps - 1):
        # frame_1 fed at s + 1 is the NOISY current block of step s, word for word - and both records of step s + 1 agree on it: no second draw
        assert np.array_equal(bits(rec[s + 1][:, col0:col0 + cols]), bits(rec[s][:, :cols]))
        assert np.array_equal(bits(rec[s + 1][:, col0:]), bits(clean[s + 1][:, col0:]))
        assert not np.array_equal(bits(rec[s][:, :cols]), bits(clean[s][:, :cols]))


def test_the_headers_philox_is_the_references():
    cols, steps, gids = np.array([0, 1, 44, 255]), np.array([0, 5, 2 ** 31 - 1]), np.array([0, 69, 2 ** 32 - 1])
    got = R.host_words(SEED, cols, steps, gids)
    vec = R.philox_blocks(R.counters(cols, steps, gids), SEED)
    assert np.array_equal(got, vec[..., :2])
    for i in range(3):
        for j, c in enumerate(cols):
            w = philox4x32((int(c), int(steps[i]), int(gids[i]), R.STREAM), (SEED & 0xffffffff, SEED >> 32))
            assert list(vec[i, j]) == w


def test_draws_of_two_columns_steps_and_env_ids_differ_and_share_no_block_with_the_action_noise():
    assert R.STREAM not in R.OTHER_STREAMS
    cols, steps, gids = np.arange(45), np.repeat(np.arange(100, 132, 4), 70), np.tile(np.arange(70), 8)
    for kind in ('uniform', 'normal'):
        n = R.draws(kind, SEED, cols, steps, gids).reshape(8, 70, 45)
        assert (n[:, :, :-1] != n[:, :, 1:]).mean() > 0.999 and (n[:-1] != n[1:]).mean() > 0.999 and (n[:, :-1] != n[:, 1:]).mean() > 0.999
        assert len(np.unique(bits(n))) > 0.99 * n.size
        other = R.draws(kind, SEED + 1, cols, steps, gids).reshape(8, 70, 45)
        assert (n != other).mean() > 0.999, 'another seed, other noise'
    # the counters of the two streams over the same (step, env) keys - the action noise's 12 joints against the first 12 columns included
    mine = R.counters(cols, steps, gids).reshape(-1, 4)
    act = R.action_counters(steps, gids).reshape(-1, 4)
    key = lambda c: set(map(tuple, c.tolist()))
    assert len(key(mine)) == mine.shape[0], 'one block per (column, step, env)'
    assert not key(mine) & key(act)
    wm, wa = R.philox_blocks(R.counters(np.arange(12), steps, gids), SEED), R.philox_blocks(R.action_counters(steps, gids), SEED)
    assert (wm[..., :2] != wa[..., :2]).all(axis=-1).mean() > 0.999


def test_the_references_draws_have_the_moments_of_their_law():
    """a sanity bound on the reference (the device is held to it by bits): six standard errors of the mean and of the variance over M draws"""
    cols, steps, gids = np.arange(45), np.repeat(100 + 4 * np.arange(8), 70), np.tile(np.arange(70), 8)
    M = 70 * 8 * 45
    u = R.draws('uniform', SEED, cols, steps, gids).astype(np.float64)
    assert u.size == M and u.min() >= -1.0 and u.max() < 1.0
    # U(-1, 1): var 1/3, var of x^2 = 1/5 - 1/9 = 4/45
    assert abs(u.mean()) <= 6 / np.sqrt(3 * M)
    assert abs(u.var() - 1 / 3) <= 6 * np.sqrt(4 / (45 * M))
    z = R.draws('normal', SEED, cols, steps, gids).astype(np.float64)
    # N(0, 1): var 1, var of x^2 = 2
    assert abs(z.mean()) <= 6 / np.sqrt(M)
    assert abs(z.var() - 1.0) <= 6 * np.sqrt(2 / M)
    assert np.isfinite(z).all() and np.abs(z).max() < 6.0   # |z| <= sqrt(2 * 25 ln 2) = 5.89 from u1 >= 2^-25


def test_the_law_rounds_a_product_and_a_sum():
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((16, 45)).astype(np.float32)
    amps = R.amp_row((0.1 + rng.random(45)).astype(np.float32), 45, 0, 45)
    steps, gids = np.arange(16) * 4, np.arange(16)
    for kind in ('uniform', 'normal'):
        got = R.apply(rows, amps, kind, SEED, steps, gids).astype(np.float64)
        ref = R.apply64(rows, amps, kind, SEED, steps, gids)
        scale = np.abs(rows) + amps[None, :] * np.abs(R.draws(kind, SEED, np.arange(45), steps, gids))
        assert (np.abs(got - ref) <= 2.0 ** -23 * scale).all(), 'two roundings: the product, then the sum'


def _mlp(in_dim, **kw):
    from gym_quadruped_amd.policy import MlpPolicy
    return MlpPolicy([np.zeros((in_dim, 12), dtype=np.float32)], [np.zeros(12, dtype=np.float32)], **kw)


def test_obs_noise_validation_and_from_names():
    from gym_quadruped_amd.policy import HeightScan, ObsNoise
    p = _mlp(45 + 12, feed_last_action=True)
    assert np.array_equal(ObsNoise(0.5).table(p), np.full(45, 0.5, dtype=np.float32))
    assert ObsNoise(np.arange(45), kind='normal').table(p).dtype == np.float32
    for bad in (np.ones(44), np.ones(46), np.ones(57)):
        with pytest.raises(ValueError, match='in_obs = 45'):
            ObsNoise(bad).table(p)
    for bad in (-1.0, np.nan, np.inf, [0.1, -0.1], [0.1, np.nan]):
        with pytest.raises(ValueError, match='amp'):
            ObsNoise(bad)
    with pytest.raises(ValueError, match='kind'):
        ObsNoise(1.0, kind='gauss')
    for bad in (-0.5, np.nan, np.inf):
        with pytest.raises(ValueError, match='scan_amp'):
            ObsNoise(1.0, scan_amp=bad)
    with pytest.raises(ValueError, match='no height scan'):
        ObsNoise(1.0, scan_amp=0.1)._check(p)
    ps = _mlp(45 + 15 + 12, feed_last_action=True, height_scan=HeightScan(3, 5))
    assert ObsNoise(1.0, scan_amp=0.1)._check(ps).shape == (45,)

    class Env:
        state_obs_names = ('base_lin_vel:base', 'base_ang_vel:base', 'gravity_vector:base', 'qpos_js', 'qvel_js', 'base_pos')   # 3 + 3 + 3 + 12 + 12 + 3
    nz = ObsNoise.from_names(Env, {'qvel_js': 1.5, 'base_ang_vel:base': [0.2, 0.2, 0.1]}, kind='normal')
    want = np.zeros(36, dtype=np.float32)
    want[3:6], want[21:33] = (0.2, 0.2, 0.1), 1.5
    assert nz.kind == 'normal' and np.array_equal(nz.amp, want)
    assert np.array_equal(nz.table(_mlp(33)), want[:33]), 'the policy reads the leading 33 columns: base_pos carries no noise'
    with pytest.raises(ValueError, match='behind'):
        nz.table(_mlp(30))
    with pytest.raises(ValueError, match='feet_pos'):
        ObsNoise.from_names(Env, {'feet_pos': 0.1})


def test_policy_noise_struct_and_exports_are_in_the_abi_and_the_version_stays():
    from gym_quadruped_amd import _lib, cabi
    # (layout and export against the header: tests/test_host_and_abi.py discovers every struct and symbol)
    assert 'gq_rollout_policy_noise' in _lib.EXPORTS and 'gq_obs_noise_eval' in _lib.EXPORTS
    g = cabi.GqPolicyNoise
    assert [f[0] for f in g._fields_] == ['struct_size', 'kind', 'n_amp', 'scan_amp', 'amp', 'policy_obs_clean'] and ctypes.sizeof(g) == 32
    assert (g.kind.offset, g.n_amp.offset, g.scan_amp.offset, g.amp.offset, g.policy_obs_clean.offset) == (4, 8, 12, 16, 24)
    assert cabi.GQ_OBS_NOISE == dict(uniform=0, normal=1)
    assert len(_lib.ABI['gq_rollout_policy_noise'][1]) == len(_lib.ABI['gq_rollout_policy_hist'][1]) + 2
    assert _lib.LIB_PATH.exists(), 'build the HIP extension first (__graft_entry__.build())'
    L = ctypes.CDLL(str(_lib.LIB_PATH))
    assert L.gq_version() == 660 and cabi.GQ_ABI_VERSION == 660
    # the eight pinned sizes are what they were
    sizes = (ctypes.c_int32 * 8)()
    assert L.gq_struct_sizes(sizes) == 0 and list(sizes) == [ctypes.sizeof(t) for t in _lib.SIZED_STRUCTS] and len(_lib.SIZED_STRUCTS) == 8
    assert cabi.GqPolicyNoise not in _lib.SIZED_STRUCTS
    # a stale binding is refused before anything else is looked at (no device is touched: the handle is never reached)
    L.gq_last_error.restype = ctypes.c_char_p
    L.gq_rollout_policy_noise.argtypes = _lib.ABI['gq_rollout_policy_noise'][1]
    L.gq_obs_noise_eval.argtypes = _lib.ABI['gq_obs_noise_eval'][1]
    m = cabi.GqPolicyMlp(struct_size=ctypes.sizeof(cabi.GqPolicyMlp), n_layers=1)
    stale = g(struct_size=ctypes.sizeof(g) - 8, kind=0, n_amp=1)
    args = (0, 0, 0.0, cabi.GqState(), cabi.GqObsOut(), None, None, None, None, None, None, None, None)
    assert L.gq_rollout_policy_noise(None, 0, ctypes.byref(m), None, None, None, ctypes.byref(stale), *args) == -1
    assert b'GqPolicyNoise' in L.gq_last_error() and b'stale binding' in L.gq_last_error()
    assert L.gq_rollout_policy_noise(None, 0, ctypes.byref(m), None, None, None, None, *args) == -1 and b'gq_rollout_policy_noise' in L.gq_last_error()
    assert L.gq_obs_noise_eval(None, ctypes.byref(stale), 1, 0, 1, 0, None, None, None, 0, None, None) == -1
    assert b'GqPolicyNoise' in L.gq_last_error() and b'stale binding' in L.gq_last_error()
