"""What the foot-reward tests share (tests/test_foot_reward_host.py, tests/test_gpu_foot_reward.py): the host program around the law's
definition (tests/foot_reward_host.cpp, built with g++ on first use), the test specs, rows and sequences, and the derived error bound.

Run as a script it prints the measured error of the law against float64 (profiles/foot_reward_law_error.txt)."""
import functools
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

import policy_mlp_ref as PR  # noqa: E402
import reward_ref as R  # noqa: E402

ROOT, U, DT = R.ROOT, R.U, R.DT
# the twelve terms' observables, then the feet's: contact_state is canonical in the row, the others follow legs_order
OBS_NAMES = R.OBS_NAMES + ('contact_state', 'contact_forces', 'feet_vel', 'feet_pos:base')
OBS_DIM = R.OBS_DIM + 4 + 12 * 3
LEGS = ('FL', 'FR', 'RL', 'RR')
LEGS_PERMUTED = ('RR', 'FL', 'RL', 'FR')
_TMP = None


def foot_full(**kw):
    """every foot term on"""
    from gym_quadruped_amd.reward import FootRewardSpec
    args = dict(air_time=1.0, slip=-0.1, impact=-0.01, clearance=-5.0, air_time_target=0.2, min_cmd_speed=0.5, impact_limit=1.0, clearance_target=-0.2)
    args.update(kw)
    return FootRewardSpec(**args)


def foot_specs():
    """name -> FootRewardSpec: each foot term alone, air_time without its gate, and all together"""
    from gym_quadruped_amd.reward import FootRewardSpec
    return {'air_time': FootRewardSpec(air_time=1.0, air_time_target=0.2, min_cmd_speed=0.5), 'air_time_ungated': FootRewardSpec(air_time=1.0, air_time_target=0.2, min_cmd_speed=0.0),
            'slip': FootRewardSpec(slip=-0.1), 'impact': FootRewardSpec(impact=-0.01, impact_limit=1.0), 'clearance': FootRewardSpec(clearance=-5.0, clearance_target=-0.2),
            'all': foot_full()}


def with_feet(feet, weights=None, **kw):
    """a RewardSpec of `weights` (default: every one of the twelve terms) with the foot terms `feet`"""
    from gym_quadruped_amd.reward import RewardSpec
    kw.setdefault('base_height_target', 0.3)
    return RewardSpec(**(R.weights_full() if weights is None else weights), feet=feet, **kw)


@functools.lru_cache(maxsize=None)
def host_program(sanitize=False):
    global _TMP
    if _TMP is None:
        _TMP = tempfile.TemporaryDirectory()
    exe = Path(_TMP.name) / ('foot_reward_host_san' if sanitize else 'foot_reward_host')
    flags = ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] if sanitize else ['-O2']
    subprocess.run(['g++', *flags, '-std=c++17', '-ffp-contract=off', '-w', '-I', str(ROOT / 'tests' / 'simt_emu'), '-I', str(ROOT / 'gym_quadruped_amd' / 'csrc'),
                    '-o', str(exe), str(ROOT / 'tests' / 'foot_reward_host.cpp')], check=True)
    return exe


def foot_columns(spec, names=OBS_NAMES, legs_order=LEGS):
    """the 24 columns of the foot law's block (csrc/gq_reward_feet.h FootLaw), -1 where nothing that is on reads them"""
    cols = spec.feet.columns(names, legs_order) if spec.feet is not None else {}
    four = lambda k: list(cols.get(k, (-1,) * 4))
    return four('feet:contact') + four('feet:vx') + four('feet:vy') + four('feet:fz') + four('feet:zb') + list(cols.get('feet:cmd_err', (-1, -1))) + list(cols.get('feet:cmd_vel', (-1, -1)))


def host_sequence(spec, rows, torques, a, a_prev, terminated, air=None, D=0, pending=None, dt=DT, names=OBS_NAMES, legs_order=LEGS, sanitize=False):
    """the host program (tests/foot_reward_host.cpp: learn_step and learn_visit of csrc/gq_learn.h, the definition) over K steps of S
    sequences with the state carried: rows [K, S, od], torques / a / a_prev [K, S, 12], terminated [K, S], air [S, 4] (None: zeros) -> dict
    of reward [K, S] f32, air [K, S, 4] f32 (the state after every step), gate [K, S] bool, impact [K, S, 4] bool (the law's threshold
    decisions).  D = 0: the step law alone, whatever `terminated` says.  D >= 1: the window law with decimation D and pending [S] (None:
    nobody waits for a re-spawn); the dict gains rewards [K // D, S] f32, dones [K // D, S] bool and air_final [S, 4]."""
    from gym_quadruped_amd.reward import FOOT_TERMS, TERMS, FootRewardSpec
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    K, S, od = rows.shape
    ft = spec.feet if spec.feet is not None else FootRewardSpec()
    head = np.asarray([spec.weights[t] for t in TERMS] + [spec.sigma_lin, spec.sigma_ang, spec.base_height_target, dt] + [ft.weights[t] for t in FOOT_TERMS]
                      + [ft.air_time_target, ft.min_cmd_speed, ft.impact_limit or 0.0, ft.clearance_target or 0.0], dtype=np.float32)
    ints = np.asarray([S, K, od, D, *R.law_columns(spec, names), *foot_columns(spec, names, legs_order)], dtype=np.int32)
    air0 = np.zeros((S, 4), dtype=np.float32) if air is None else np.ascontiguousarray(air, dtype=np.float32).reshape(S, 4)
    pend = np.zeros(S, dtype=np.float32) if pending is None else np.asarray(pending).reshape(S).astype(np.float32)
    flag = lambda v: np.zeros((K, S, 1), dtype=np.float32) if v is None else np.asarray(v).reshape(K, S, 1).astype(np.float32)
    f12 = lambda v: np.asarray(v, dtype=np.float32).reshape(K, S, 12)
    body = np.concatenate([rows, f12(torques), f12(a), f12(a_prev), flag(terminated)], axis=2)
    with tempfile.TemporaryDirectory() as d:
        src, dst = Path(d) / 'in.bin', Path(d) / 'out.bin'
        np.concatenate([head.view(np.uint32), ints.view(np.uint32), air0.reshape(-1).view(np.uint32), pend.view(np.uint32),
                        np.ascontiguousarray(body).reshape(-1).view(np.uint32)]).tofile(src)
        subprocess.run([str(host_program(sanitize)), str(src), str(dst)], check=True)
        raw = np.fromfile(dst, dtype=np.float32)
    out, tail = raw[:K * S * 7].reshape(K, S, 7), raw[K * S * 7:]
    mask = out[..., 6].astype(np.int64)
    res = dict(reward=out[..., 0].copy(), air=out[..., 1:5].copy(), gate=out[..., 5] != 0, impact=np.stack([(mask >> i) & 1 for i in range(4)], axis=-1).astype(bool))
    if D > 0:
        W = K // D
        assert tail.size == 2 * W * S + 4 * S
        res.update(rewards=tail[:W * S].reshape(W, S).copy(), dones=tail[W * S:2 * W * S].reshape(W, S) != 0, air_final=tail[2 * W * S:].reshape(S, 4).copy())
    return res


def host_rows(spec, rows, torques, a, a_prev, terminated, air=None, **kw):
    """n independent steps (what reward_eval(..., feet_air=) computes): -> (reward [n], air_next [n, 4])"""
    lift = lambda v: None if v is None else np.asarray(v)[None]
    out = host_sequence(spec, lift(rows), lift(torques), lift(a), lift(a_prev), lift(terminated), air=air, **kw)
    return out['reward'][0], out['air'][0]


def contact_columns(names=OBS_NAMES):
    from gym_quadruped_amd.reward import FootRewardSpec
    return list(FootRewardSpec(slip=1.0).columns(names)['feet:contact'])


def random_rows(n, seed=0, names=OBS_NAMES, od=OBS_DIM):
    """reward_ref.random_steps at this module's row width, the contact columns drawn 0 / 1; and random air times, a third of them 0"""
    rng = np.random.default_rng(seed + 1000)
    rows, u, a, ap, term = R.random_steps(n, seed=seed, od=od)
    rows[:, contact_columns(names)] = rng.integers(0, 2, (n, 4)).astype(np.float32)
    air = (rng.uniform(0.0, 0.6, (n, 4)) * (rng.uniform(size=(n, 4)) > 1 / 3)).astype(np.float32)
    return (rows, u, a, ap, term), air


def edge_rows(names=OBS_NAMES, od=OBS_DIM):
    """reward_ref.edge_steps at this module's row width (every column one value: the feet are in contact wherever it is not 0), air times 0.1"""
    steps = R.edge_steps(od=od)
    return steps, np.full((steps[0].shape[0], 4), 0.1, dtype=np.float32)


def random_sequences(S=64, T=200, seed=0, toggle=0.1, names=OBS_NAMES, od=OBS_DIM):
    """S independent sequences of T steps, [T, S, ...]: values over four decades as reward_ref.random_steps, contacts that toggle with
    probability `toggle` per step (flights of about 1 / toggle steps)"""
    rng = np.random.default_rng(seed + 2000)
    rows, u, a, ap, term = R.random_steps(S * T, seed=seed, od=od)
    c = np.zeros((T, S, 4), dtype=np.float32)
    state = rng.integers(0, 2, (S, 4))
    for k in range(T):
        state = np.where(rng.uniform(size=(S, 4)) < toggle, 1 - state, state)
        c[k] = state
    rows = rows.reshape(T, S, od)
    rows[:, :, contact_columns(names)] = c
    return rows, u.reshape(T, S, 12), a.reshape(T, S, 12), ap.reshape(T, S, 12), term.reshape(T, S)


def sequence_reference(spec, seq, host, air=None, dt=DT, names=OBS_NAMES, legs_order=LEGS):
    """float64 reference and DERIVED bound of every step's reward over sequences `seq` ([T, S, ...]); the law's threshold decisions (gate,
    fz above the limit) are the float32 evaluation's (`host`: host_sequence's result); c_i and t_i > 0 are the same on both sides by
    construction (exact words; a sum of positive dt).  First-order count of the float32 law's roundings, u = 2^-24, as
    reward_ref.first_order_bound:
      the twelve terms: 14 u of each term's value; the foot terms: FootRewardSpec.sequence64's 'roundings' - air_time: the air time tn behind
        a landing is a chain of (steps in the air + 1) additions, each rounding at most u tn, then the difference (u) and the sum over up
        to four feet (3 u); slip: 8 fmaf; impact: the difference and 3 adds; clearance: d (1), d d (2 + 1), the speed (2), 4 fmaf = 9 u;
      the sum S: now at most 15 fmaf, each rounding a partial sum of at most M = sum |w_i term_i| over ALL terms; dt S and the
        termination's add: 2 u;  14 + 15 + 2 = 31: 32 u (dt M + |w_termination|) is allowed, plus dt u times the foot terms' own count,
      plus the exp terms' absolute allowance, as there."""
    from gym_quadruped_amd.reward import TERMS
    rows, u, a, ap, term = seq
    T, S, od = rows.shape
    cols = spec.columns(names, legs_order)
    flat = lambda v: np.asarray(v).reshape(T * S, -1)
    with np.errstate(over='ignore', invalid='ignore'):
        terms = spec.terms64(flat(rows).astype(np.float64), flat(u), flat(a), flat(ap), np.asarray(term).reshape(T * S), cols)
        dt64 = np.float64(np.float32(dt))
        wt = np.float64(np.float32(spec.weights['termination']))
        flag = terms['termination'].reshape(T, S) if 'termination' in terms else np.zeros((T, S))
        s_base, m_base = np.zeros((T, S)), np.zeros((T, S))                 # the twelve terms' S, as RewardSpec._sum64 forms it
        for t in TERMS[:-1]:
            if t in terms:
                wv = np.float64(np.float32(spec.weights[t])) * terms[t].reshape(T, S)
                s_base += wv
                m_base += np.abs(wv)
        ft = spec.feet.sequence64(rows.astype(np.float64), cols, dt, air=air, decisions=dict(gate=host['gate'], impact=host['impact']))
        ref = dt64 * (s_base + ft['sum']) + wt * flag
        w_exp = abs(np.float32(spec.weights['track_lin_vel'])) + abs(np.float32(spec.weights['track_ang_vel']))
        bound = U * (32.0 * (dt64 * (m_base + ft['magnitude']) + abs(wt)) + dt64 * ft['roundings']) + dt64 * w_exp * (PR.activation_allowance('elu') + 3.0) * U
    return ref, bound, ft['air']


def measured_ratio(spec, seq):
    host = host_sequence(spec, *seq)
    ref, bound, _ = sequence_reference(spec, seq, host)
    ok = np.isfinite(ref) & np.isfinite(bound) & (bound > 0)
    return float((np.abs(host['reward'].astype(np.float64) - ref)[ok] / bound[ok]).max()) if ok.any() else 0.0


if __name__ == '__main__':
    print('Error of the reward law with its foot terms (csrc/gq_reward_feet.h: foot_reward_step, float32, contraction off, IEEE operations and')
    print('fmaf; host build g++ -O2 -ffp-contract=off, tests/foot_reward_host.cpp) against the float64 restatement (RewardSpec._sum64 +')
    print('FootRewardSpec.sequence64, the state carried through): largest |f32 - f64| / bound over 64 sequences of 200 steps (values over four')
    print('decades, contacts toggling with probability 0.1 per step; tests/foot_reward_ref.py random_sequences), where bound is the DERIVED')
    print('first-order count of the law\'s roundings (sequence_reference) that tests/test_foot_reward_host.py asserts.  dt = 0.002.')
    worst = 0.0
    seq = random_sequences()
    for name, feet in foot_specs().items():
        for tag, spec in (('feet alone', with_feet(feet, weights={})), ('with the twelve terms', with_feet(feet))):
            r = measured_ratio(spec, seq)
            worst = max(worst, r)
            print(f'{name:18s} {tag:22s} {r:8.4f}')
    print(f'worst measured ratio to the bound: {worst:.4f} (the test asserts <= 1)')
