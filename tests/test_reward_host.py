"""The reward of the learning rollout without a GPU (gym_quadruped_amd/reward.py, csrc/gq_reward.h, include/gq.h GqLearn): the law's
definition (reward_step in tests/reward_host.cpp, a stand-alone g++ program) against the float64 evaluation, RewardSpec's validation and
column resolution, and the new struct and entry points of the ABI."""
import ctypes

import numpy as np
import pytest

import reward_ref as R

SPECS = R.specs()


@pytest.fixture(scope='module')
def steps():
    """random steps and the edge steps, once for every spec"""
    rnd, edge = R.random_steps(6000, seed=11), R.edge_steps()
    return tuple(np.concatenate([a, b]) for a, b in zip(rnd, edge)), rnd[0].shape[0]


@pytest.mark.parametrize('name', list(SPECS))
def test_host_law_is_within_the_bound_of_the_float64_reference(name, steps):
    """the issue's bound c 2^-24 (dt sum |w_i term_i| + |w_termination|) with the measured c of profiles/reward_law_error.txt - which the
    two exp terms make wide - and, for every spec, the first-order bound of the law's own roundings (reward_ref.first_order_bound)"""
    spec = SPECS[name]
    st, n_rnd = steps
    got = R.host_reward(spec, *st).astype(np.float64)
    ref, bound = R.issue_bound(spec, st)
    fin = np.isfinite(ref) & np.isfinite(bound)   # (1e10)^2 12 w overflows float32 and is inf in both
    assert fin[:n_rnd].all() and fin.sum() >= fin.size - 3
    err = np.abs(got - ref)
    tight = R.first_order_bound(spec, st)
    print(f'{name}: worst error / issue bound {float((err[fin] / np.maximum(bound[fin], 1e-300)).max()):.3e}, / first-order bound {float((err[fin] / np.maximum(tight[fin], 1e-300)).max()):.3f}')
    assert (err[fin] <= bound[fin]).all()
    assert (err[fin] <= tight[fin]).all()
    assert not np.isfinite(got[~fin]).any() or (np.abs(got[~fin]) > 1e30).all(), 'where float64 leaves the float32 range the law does not come back small'


def test_edge_rows_have_the_values_the_law_states(steps):
    rows, u, a, ap, term = R.edge_steps()
    full = SPECS['all']
    got = R.host_reward(full, rows, u, a, ap, term)
    dt = np.float32(R.DT)
    w = {k: np.float32(v) for k, v in full.weights.items()}
    # the all-zero row: exp(0) twice, the height term, alive
    s = np.float32(0)
    for t, v in (('track_lin_vel', 1.0), ('track_ang_vel', 1.0), ('base_height', np.float32(0.3) * np.float32(0.3)), ('alive', 1.0)):
        s = np.float32(np.float64(w[t]) * np.float64(np.float32(v)) + np.float64(s))   # fmaf: one rounding
    assert got[0] == dt * s
    assert got[-1] == np.float32(dt * s + w['termination']), 'termination is added after dt'
    # beyond the clamp the exp terms are exactly 0: the argument stops at 87 and expm1(-87) rounds to -1
    lin = R.host_reward(SPECS['track_lin_vel'], rows, u, a, ap, term)
    assert lin[0] == dt * np.float32(1.0) and (lin[[1, 3, 4, 5, 6]] == 0).all() and lin[2] == 0
    # huge torques: 12 x 1e36 stays finite in float32
    tq = R.host_reward(SPECS['torques'], rows, u, a, ap, term)
    assert np.isfinite(tq).all() and tq[7] < -1e28
    # a term that is off does not look at its words: NaN everywhere else leaves `alive` alone
    nan = np.full_like(rows, np.nan)
    assert (R.host_reward(SPECS['alive'], nan, nan[:, :12], nan[:, :12], nan[:, :12], term) == dt * w['alive']).all()


def test_required_obs_of_every_term():
    from gym_quadruped_amd.reward import TERMS, RewardSpec
    want = dict(track_lin_vel=('base_lin_vel_err:base',), track_ang_vel=('base_ang_vel_err:base',), lin_vel_z=('base_lin_vel:base',), ang_vel_xy=('base_ang_vel:base',),
                orientation=('gravity_vector:base',), base_height=('base_pos',), torques=(), joint_vel=('qvel_js',), power=('qvel_js',), action_rate=(), alive=(),
                termination=())
    assert set(want) == set(TERMS)
    for t in TERMS:
        assert RewardSpec(**{t: -0.5}).required_obs() == want[t], t
    assert RewardSpec().required_obs() == ()
    assert RewardSpec(joint_vel=1.0, power=1.0, track_lin_vel=2.0).required_obs() == ('base_lin_vel_err:base', 'qvel_js')
    assert set(SPECS['all'].required_obs()) <= set(R.OBS_NAMES)


def test_spec_refuses_what_the_library_would():
    from gym_quadruped_amd.reward import RewardSpec
    for bad in (dict(alive=float('nan')), dict(torques=float('inf')), dict(track_lin_vel=1.0, sigma_lin=0.0), dict(track_ang_vel=1.0, sigma_ang=-1.0),
                dict(feet_air_time=1.0), dict(track_lin_vel=1.0, sigma_lin=float('nan')), dict(base_height_target=float('inf'))):
        with pytest.raises(ValueError):
            RewardSpec(**bad)
    s = RewardSpec(track_ang_vel=1.0, sigma_lin=0.0)   # sigma_lin is not read: its term is off
    assert s.sigma_lin == 0.0 and s.track_ang_vel == 1.0 and s.track_lin_vel == 0.0
    with pytest.raises(ValueError, match='feet_air_time'):
        RewardSpec(feet_air_time=1.0)


def test_columns_are_resolved_by_observable_name():
    from gym_quadruped_amd.reward import RewardSpec
    full = SPECS['all']
    cols = full.columns(R.OBS_NAMES)
    assert cols['joint_vel'] == cols['power'] == tuple(range(12, 24))
    assert cols['base_height'] == (26,) and cols['lin_vel_z'] == (29,) and cols['ang_vel_xy'] == (30, 31)
    assert cols['track_lin_vel'] == (33, 34) and cols['track_ang_vel'] == (38,) and cols['orientation'] == (39, 40)
    assert 'torques' not in cols and 'alive' not in cols
    # another order, qvel in the place of qvel_js
    other = ('gravity_vector:base', 'qpos', 'qvel', 'base_pos')
    assert RewardSpec(joint_vel=1.0, orientation=1.0, base_height=1.0).columns(other) == {'orientation': (0, 1), 'base_height': (3 + 19 + 18 + 2,), 'joint_vel': tuple(range(3 + 19 + 6, 3 + 19 + 18))}
    with pytest.raises(ValueError, match='base_lin_vel:base'):
        RewardSpec(lin_vel_z=1.0).columns(other)
    assert RewardSpec(lin_vel_z=0.0, alive=1.0).columns(other) == {}
    assert R.law_columns(RewardSpec(power=1.0)) == [-1] * 9 + list(range(12, 24))


def test_reference_is_the_formula():
    full = SPECS['all']
    rows, u, a, ap, term = R.random_steps(50, seed=3)
    x = rows.astype(np.float64)
    w = {k: float(np.float32(v)) for k, v in full.weights.items()}
    qd = x[:, 12:24]
    s = (w['track_lin_vel'] * np.exp(-np.minimum((x[:, 33] ** 2 + x[:, 34] ** 2) / 0.25, 87)) + w['track_ang_vel'] * np.exp(-np.minimum(x[:, 38] ** 2 / 0.25, 87))
         + w['lin_vel_z'] * x[:, 29] ** 2 + w['ang_vel_xy'] * (x[:, 30] ** 2 + x[:, 31] ** 2) + w['orientation'] * (x[:, 39] ** 2 + x[:, 40] ** 2)
         + w['base_height'] * (x[:, 26] - float(np.float32(0.3))) ** 2 + w['torques'] * (u.astype(np.float64) ** 2).sum(1) + w['joint_vel'] * (qd ** 2).sum(1)
         + w['power'] * np.abs(u * qd).sum(1) + w['action_rate'] * ((a.astype(np.float64) - ap) ** 2).sum(1) + w['alive'])
    want = float(np.float32(R.DT)) * s + w['termination'] * term
    got = full.reference(rows, u, a, ap, term, full.columns(R.OBS_NAMES), R.DT)
    assert np.allclose(got, want, rtol=1e-13, atol=0)


def test_learn_struct_layout_matches_header_and_the_abi_keeps_its_version():
    from gym_quadruped_amd import _lib
    from gym_quadruped_amd.cabi import GqLearn
    from gym_quadruped_amd.reward import TERMS
    fields = [n for n, _ in GqLearn._fields_]
    assert fields[2:14] == ['w_' + t for t in TERMS], 'the weights stand in the order of the law\'s sum'
    # (layout and export: tests/test_host_and_abi.py, for every struct and symbol) both entry points are in the binding's table, with arguments
    assert _lib.ABI['gq_rollout_policy_learn'][1] and _lib.ABI['gq_reward_eval'][1]
    assert _lib.LIB_PATH.exists(), 'build the HIP extension first (__graft_entry__.build())'
    L = ctypes.CDLL(str(_lib.LIB_PATH))
    assert L.gq_version() == 660
    assert L.gq_rollout_policy_learn and L.gq_reward_eval
    # a stale binding is refused before anything else is looked at (no device is touched: the handle is never reached)
    L.gq_last_error.restype = ctypes.c_char_p
    g = GqLearn(struct_size=ctypes.sizeof(GqLearn) - 8)
    L.gq_reward_eval.argtypes = _lib.ABI['gq_reward_eval'][1]
    assert L.gq_reward_eval(None, ctypes.byref(g), None, None, None, None, None, 0, None, None) == -1 and b'stale binding' in L.gq_last_error()
    spec_struct = SPECS['all']._struct()
    assert spec_struct.struct_size == ctypes.sizeof(GqLearn) and spec_struct.w_termination == -2.0 and abs(spec_struct.base_height_target - 0.3) < 1e-7
