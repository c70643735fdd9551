"""What the reward tests share (tests/test_reward_host.py, tests/test_gpu_learn_rollout.py): the host program around the law's definition
(tests/reward_host.cpp, built with g++ on first use), the test specs and rows, and the error bounds.

Run as a script it prints the measured error of the law against float64 (profiles/reward_law_error.txt)."""
import functools
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import policy_mlp_ref as PR  # noqa: E402

U = 2.0 ** -24
OBS_NAMES = ('qpos_js', 'qvel_js', 'base_pos', 'base_lin_vel:base', 'base_ang_vel:base', 'base_lin_vel_err:base', 'base_ang_vel_err:base', 'gravity_vector:base')
OBS_DIM = 12 + 12 + 3 * 6
DT = 0.002
# profiles/reward_law_error.txt: 4 x the largest ratio of 60 000 random rows per spec, rounded up to a power of two.  The ratio is that
# large because exp(-x) = expm1(-x) + 1 carries an ABSOLUTE error of a few 2^-24 whatever its value: alone, at x >= 17, the term's value is
# below that error.  first_order_bound() below is the bound that says so, and the one that pins the other terms.
C_BOUND = 2.0 ** 26
_TMP = None


def weights_full():
    """every term on, with the signs and sizes a locomotion task gives them"""
    return dict(track_lin_vel=1.0, track_ang_vel=0.5, lin_vel_z=-2.0, ang_vel_xy=-0.05, orientation=-0.2, base_height=-30.0, torques=-1e-5,
                joint_vel=-1e-3, power=-2e-5, action_rate=-0.01, alive=0.25, termination=-2.0)


def spec_of(weights, **kw):
    from gym_quadruped_amd.reward import RewardSpec
    kw.setdefault('base_height_target', 0.3)
    return RewardSpec(**weights, **kw)


def specs():
    """name -> spec: each term alone, and all together"""
    full = weights_full()
    out = {name: spec_of({name: w}) for name, w in full.items()}
    out['all'] = spec_of(full)
    return out


def spec_no_exp():
    w = weights_full()
    w['track_lin_vel'] = w['track_ang_vel'] = 0.0
    return spec_of(w)


@functools.lru_cache(maxsize=None)
def host_program():
    global _TMP
    _TMP = tempfile.TemporaryDirectory()
    exe = Path(_TMP.name) / 'reward_host'
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-w', '-I', str(ROOT / 'tests' / 'simt_emu'), '-I', str(ROOT / 'gym_quadruped_amd' / 'csrc'),
                    '-o', str(exe), str(ROOT / 'tests' / 'reward_host.cpp')], check=True)
    return exe


def law_columns(spec, names=OBS_NAMES):
    """the 21 columns of the law's block (csrc/gq_reward.h RewardLaw), -1 where the term is off"""
    cols = spec.columns(names)
    one = lambda t, i: cols[t][i] if t in cols else -1
    qd = cols.get('joint_vel', cols.get('power', (-1,) * 12))
    return [one('track_lin_vel', 0), one('track_lin_vel', 1), one('track_ang_vel', 0), one('lin_vel_z', 0), one('ang_vel_xy', 0), one('ang_vel_xy', 1),
            one('orientation', 0), one('orientation', 1), one('base_height', 0), *qd]


def host_reward(spec, rows, torques, a, a_prev, terminated, dt=DT, names=OBS_NAMES):
    """reward_step (the definition) over n steps, float32 [n]"""
    from gym_quadruped_amd.reward import TERMS
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, od = rows.shape
    head = np.asarray([spec.weights[t] for t in TERMS] + [spec.sigma_lin, spec.sigma_ang, spec.base_height_target, dt], dtype=np.float32)
    ints = np.asarray([n, od, *law_columns(spec, names)], dtype=np.int32)
    body = np.concatenate([rows, np.asarray(torques, dtype=np.float32).reshape(n, 12), np.asarray(a, dtype=np.float32).reshape(n, 12),
                           np.asarray(a_prev, dtype=np.float32).reshape(n, 12), np.asarray(terminated).reshape(n, 1).astype(np.float32)], axis=1)
    with tempfile.TemporaryDirectory() as d:
        src, dst = Path(d) / 'in.bin', Path(d) / 'out.bin'
        np.concatenate([head.view(np.uint32), ints.view(np.uint32), np.ascontiguousarray(body).reshape(-1).view(np.uint32)]).tofile(src)
        subprocess.run([str(host_program()), str(src), str(dst)], check=True)
        return np.fromfile(dst, dtype=np.float32)


def random_steps(n, seed=0, od=OBS_DIM):
    """(rows, torques, a, a_prev, terminated): normal values over four decades of scale, so that every term is met small and large - the
    arguments of exp from 1e-4 to far beyond its clamp"""
    rng = np.random.default_rng(seed)
    scaled = lambda shape, lo, hi: (rng.normal(size=shape) * 10.0 ** rng.uniform(lo, hi, size=(shape[0], 1))).astype(np.float32)
    return scaled((n, od), -2.5, 1.5), scaled((n, 12), -1.0, 2.5), scaled((n, 12), -2.0, 0.5), scaled((n, 12), -2.0, 0.5), rng.integers(0, 2, n).astype(np.uint8)


def edge_steps(od=OBS_DIM):
    """all zero; the exp arguments exactly at / just below / beyond the clamp (sigma = 0.25: x = 4 e^2); huge torques; a terminated zero row"""
    e_clamp = np.sqrt(np.float32(87.0) / np.float32(4.0))
    vals = [0.0, float(e_clamp), float(np.nextafter(np.float32(e_clamp), np.float32(0))), float(np.nextafter(np.float32(e_clamp), np.float32(10))), 5.0, 100.0, 1e10]
    rows = np.zeros((len(vals) + 2, od), dtype=np.float32)
    for i, v in enumerate(vals):
        rows[i] = v
    u = np.zeros((rows.shape[0], 12), dtype=np.float32)
    u[len(vals)] = 1e18
    u[len(vals), ::2] = -1e18
    rows[len(vals)] = 1.5
    term = np.zeros(rows.shape[0], dtype=np.uint8)
    term[-1] = 1
    a = np.zeros_like(u)
    a[len(vals)] = 3.0
    return rows, u, a, np.zeros_like(u), term


def issue_bound(spec, steps, dt=DT, names=OBS_NAMES):
    """(float64 reference, C_BOUND 2^-24 (dt sum |w_i term_i| + |w_termination|))"""
    cols = spec.columns(names)
    with np.errstate(over='ignore'):
        return spec.reference(*steps, cols, dt), C_BOUND * U * spec.magnitude(*steps, cols, dt)


def first_order_bound(spec, steps, dt=DT, names=OBS_NAMES):
    """The law's own error to first order, in float32 roundings (u = 2^-24) - what a correct implementation keeps, from the order of the
    operations alone:
      a term: a chain of at most 12 fmaf over non-negative products (12 u of its value), its operands rounded once or twice before (the
        difference a - a_prev or z - target, the product e e): 14 u of the term's value;
      the sum S: at most 11 fmaf, each rounding a partial sum that is at most M = sum |w_i term_i|: 11 u M;  dt S and the termination's add: 2 u;
      together 27 u (dt M + |w_termination|); 32 u is allowed.
      exp(-x) = expm1(-x) + 1: expm1's error is measured in units of 2^-24 max(1, |y|), |y| <= 1 here (policy_mlp_ref.activation_allowance: 4 x
        the measured ratio), the add is exact (Sterbenz: expm1 in [-1, -1/2]) or rounds to u; x itself carries 4 roundings (e e, the fmaf,
        inv_sigma, the product), worth 4 u x exp(-x) <= 1.5 u: (allowance + 3) u ABSOLUTE per exp term, times dt |w|."""
    cols = spec.columns(names)
    with np.errstate(over='ignore'):
        mag = spec.magnitude(*steps, cols, dt)
    w_exp = abs(np.float32(spec.weights['track_lin_vel'])) + abs(np.float32(spec.weights['track_ang_vel']))
    return 32.0 * U * mag + float(np.float32(dt)) * w_exp * (PR.activation_allowance('elu') + 3.0) * U


def measured_ratio(spec, steps):
    ref, _ = issue_bound(spec, steps)
    got = host_reward(spec, *steps).astype(np.float64)
    with np.errstate(over='ignore'):
        mag = spec.magnitude(*steps, spec.columns(OBS_NAMES), DT)
    ok = np.isfinite(ref) & (mag > 0)
    return float((np.abs(got - ref)[ok] / (U * mag[ok])).max()) if ok.any() else 0.0


if __name__ == '__main__':
    print('Error of the reward law (csrc/gq_reward.h: reward_step, float32, contraction off, IEEE operations and fmaf; host build g++ -O2')
    print('-ffp-contract=off, tests/reward_host.cpp) against RewardSpec.reference (numpy float64): largest |f32 - f64| / (2^-24 (dt sum |w_i term_i|')
    print('+ |w_termination|)) over 60 000 random steps per spec (tests/reward_ref.py random_steps: normal values over four decades of scale),')
    print('each term alone and all together; dt = 0.002, sigma = 0.25.')
    worst = 0.0
    steps = random_steps(60_000)
    for name, spec in specs().items():
        r = measured_ratio(spec, steps)
        worst = max(worst, r)
        print(f'{name:14s} {r:14.3f}')
    c = 4 * worst
    print(f'largest: {worst:.3f}; x 4 = {c:.3f}; rounded up to a power of two: C_BOUND = 2^{int(np.ceil(np.log2(c)))}')
    print('The two exp terms alone set it: exp(-x) = mlp_expm1(-min(x, 87)) + 1 has an absolute error of a few 2^-24 (the rounding of a number')
    print('next to -1), so from x = 17 on the term\'s value is all error - a ratio of 2^24 and more.  Every other term, and the full sum, stays')
    print('below 32: the tests also hold the law to that first-order bound, with the absolute allowance for the exp terms (first_order_bound).')
