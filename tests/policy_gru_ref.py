"""What the recurrent-policy tests share (tests/test_policy_gru_host.py, tests/test_gpu_policy_gru.py): the host program around the law's
definition and the episode rule (tests/policy_gru_host.cpp, built with g++ on first use), the test policies, and the DERIVED error bound of
one step against float64.

Run as a script it prints the measured activation ratios and the worst error / bound of every shape (profiles/gru_policy_law_error.txt)."""
import functools
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

import policy_mlp_ref as M

ROOT = M.ROOT
U = M.U
_TMP = None


@functools.lru_cache(maxsize=None)
def host_program():
    global _TMP
    _TMP = tempfile.TemporaryDirectory()
    exe = Path(_TMP.name) / 'policy_gru_host'
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-w', '-I', str(ROOT / 'tests' / 'simt_emu'), '-I', str(ROOT / 'gym_quadruped_amd' / 'csrc'),
                    '-o', str(exe), str(ROOT / 'tests' / 'policy_gru_host.cpp')], check=True)
    return exe


def _run(args, data):
    with tempfile.TemporaryDirectory() as d:
        src, dst = Path(d) / 'in.bin', Path(d) / 'out.bin'
        data.tofile(src)
        subprocess.run([str(host_program()), *args, str(src), str(dst)], check=True)
        return np.fromfile(dst, dtype=np.float32)


def host_sig(x):
    return _run(['sig'], np.ascontiguousarray(x, dtype=np.float32))


def obs_in(policy, rows):
    return M.obs_in(policy, rows)   # (o - shift) * scale in float32 on the first in_obs columns


def host_forward(policy, rows, h):
    """gru_row_forward on the packed blob over raw rows and states: (actions [n, 12], h' WITH its padding [n, Hp]), float32"""
    x = obs_in(policy, rows)
    h = np.ascontiguousarray(h, dtype=np.float32).reshape(x.shape[0], policy.hidden)
    widths = policy.widths + [0] * (4 - len(policy.widths))
    head = np.asarray([policy.in_dim, policy.hidden, len(policy.widths), M.ACT_ID[policy.activation], M.ACT_ID[policy.out_activation], *widths, x.shape[0]], dtype=np.int32)
    out = _run(['forward'], np.concatenate([head.view(np.float32), policy.pack(), x.reshape(-1), h.reshape(-1)]))
    hp = (policy.hidden + 15) & ~15
    out = out.reshape(x.shape[0], 12 + hp)
    return out[:, :12], out[:, 12:]


def host_rule(pending, terminated, H, D, closing):
    """gru_episode_rule played over consecutive calls.  pending: [calls][n] (the flag before each call), terminated: [calls][K][n] (the byte
    after each step) -> (fed [calls][K // D][n][H], after [calls][n][H]): the rows as fed at every policy step and after each call"""
    pending, terminated = np.asarray(pending, dtype=np.int32), np.asarray(terminated, dtype=np.int32)
    calls, K, n = terminated.shape
    body = np.concatenate([np.concatenate([pending[c].reshape(-1), terminated[c].reshape(-1)]) for c in range(calls)])
    out = _run(['rule'], np.concatenate([np.asarray([n, H, D, K, calls, int(closing)], dtype=np.int32), body]).view(np.float32))
    out = out.reshape(calls, K // D + 1, n, H)
    return out[:, :-1], out[:, -1]


SHAPES = {
    # no width a multiple of 4 or 16; shift / scale; the last action fed back
    'odd': dict(in_obs=37, hidden=20, head=(33,), feed_last_action=True, shift=True),
    'wide': dict(in_obs=256, hidden=128, head=(256, 256), feed_last_action=False, shift=False),
    'minimal': dict(in_obs=24, hidden=1, head=(), feed_last_action=False, shift=False),
}


def make_policy(shape, activation='elu', out_activation=None, seed=0, in_obs=None, hidden=None, head=None):
    from gym_quadruped_amd.policy import GruPolicy
    s = SHAPES[shape]
    rng = np.random.default_rng(seed + 31 * len(shape))
    n_obs = s['in_obs'] if in_obs is None else in_obs
    H = s['hidden'] if hidden is None else hidden
    k = n_obs + (12 if s['feed_last_action'] else 0)
    w_ih = (rng.uniform(-1, 1, (k, 3 * H)) * np.sqrt(3.0 / k)).astype(np.float32)
    w_hh = (rng.uniform(-1, 1, (H, 3 * H)) * np.sqrt(3.0 / H)).astype(np.float32)
    b_ih, b_hh = rng.uniform(-0.3, 0.3, 3 * H).astype(np.float32), rng.uniform(-0.3, 0.3, 3 * H).astype(np.float32)
    dims = [H, *(s['head'] if head is None else head), 12]
    ws = [(rng.uniform(-1, 1, (a, b)) * np.sqrt(3.0 / a)).astype(np.float32) for a, b in zip(dims[:-1], dims[1:])]
    bs = [rng.uniform(-0.3, 0.3, b).astype(np.float32) for b in dims[1:]]
    kw = {}
    if s['shift']:
        kw = dict(obs_shift=rng.uniform(-0.5, 0.5, n_obs).astype(np.float32), obs_scale=rng.uniform(0.5, 2.0, n_obs).astype(np.float32))
    return GruPolicy(w_ih, w_hh, b_ih, b_hh, ws, bs, activation=activation, out_activation=out_activation, feed_last_action=s['feed_last_action'], **kw)


def rows_for(policy, n, seed=1):
    """x in [-2, 2], h in [-1, 1]"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, (n, policy.in_dim)).astype(np.float32), rng.uniform(-1.0, 1.0, (n, policy.hidden)).astype(np.float32)


def sig_error(n=200_001):
    """largest |gru_sig - float64 sigmoid| / (2^-24 max(1, |y|)): activation_error's arguments and measure, for the header's sigmoid"""
    from gym_quadruped_amd.policy import sig64
    rng = np.random.default_rng(5)
    x = np.concatenate([np.linspace(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-1, 1, n), rng.normal(0, 1e-3, 1000)]).astype(np.float32)
    y = sig64(x.astype(np.float64))
    return float((np.abs(host_sig(x).astype(np.float64) - y) / (U * np.maximum(1.0, np.abs(y)))).max())


@functools.lru_cache(maxsize=None)
def sig_allowance():
    return 4.0 * sig_error()


def step_bound(policy, rows, h):
    """(reference(): (a, h'), the allowed errors (ea [n, 12], eh [n, H])) of ONE step, to first order:
      a chain      (Kp + 2) 2^-24 (|b| + sum |x_k w_k|) (layer_bounds' term), and an error e on its inputs reaches it as e |W|
      s = gi + gh  one rounding, 2^-24 |s|;  sig is 1/4-Lipschitz and adds its allowance (4 x the measured ratio, |sig| <= 1)
      t = fmaf(r, gh_n, gi_n)   e_r |gh_n| + |r| e_gh + e_gi + 2^-24 |t|;  tanh is 1-Lipschitz and adds its allowance
      d = h - n    e_n + 2^-24 |d|;   h' = fmaf(z, d, n)   e_z |d| + |z| e_d + e_n + 2^-24 |h'|
    then through the head with network_bound's rule; the factor 1 + 2^-10 covers the higher orders."""
    from gym_quadruped_amd.policy import _ACT64, sig64
    f64 = lambda v: v.astype(np.float64)
    x = np.array(rows, dtype=np.float64)
    ex = np.zeros_like(x)
    if policy.obs_shift is not None:
        x[:, :policy.in_obs] -= f64(policy.obs_shift)
    if policy.obs_scale is not None:
        x[:, :policy.in_obs] *= f64(policy.obs_scale)
    if policy.obs_shift is not None or policy.obs_scale is not None:
        ex[:, :policy.in_obs] = 2 * U * np.abs(x[:, :policy.in_obs])   # the two float32 roundings of (o - shift) * scale
    h = np.array(h, dtype=np.float64)
    H = policy.hidden
    kpx, kph = (policy.in_dim + 3) & ~3, (H + 3) & ~3
    gates = policy._gates()   # ir, hr, iz, hz, in, hn
    gi, gh, egi, egh = [], [], [], []
    for g in range(3):
        (wi, bi), (wh, bh) = gates[2 * g], gates[2 * g + 1]
        wi, bi, wh, bh = f64(wi), f64(bi), f64(wh), f64(bh)
        gi.append(x @ wi + bi)
        gh.append(h @ wh + bh)
        egi.append(ex @ np.abs(wi) + (kpx + 2) * U * (np.abs(bi) + (np.abs(x) + ex) @ np.abs(wi)))
        egh.append((kph + 2) * U * (np.abs(bh) + np.abs(h) @ np.abs(wh)))
    a_sig, a_tanh = sig_allowance(), M.activation_allowance('tanh')

    def gate(g):
        s = gi[g] + gh[g]
        return sig64(s), 0.25 * (egi[g] + egh[g] + U * np.abs(s)) + a_sig * U
    r, er = gate(0)
    z, ez = gate(1)
    t = gi[2] + r * gh[2]
    n = np.tanh(t)
    en = er * np.abs(gh[2]) + np.abs(r) * egh[2] + egi[2] + U * np.abs(t) + a_tanh * U * np.maximum(1.0, np.abs(n))
    d = h - n
    ed = en + U * np.abs(d)
    hn = n + z * d
    eh = ez * np.abs(d) + np.abs(z) * ed + en + U * np.abs(hn)
    y, err = hn, eh
    for l, (w, b) in enumerate(zip(policy.head_weights, policy.head_biases)):
        w64, b64 = f64(w), f64(b)
        kp = (w.shape[0] + 3) & ~3
        act = policy.out_activation if l == len(policy.head_weights) - 1 else policy.activation
        nxt = _ACT64[act](y @ w64 + b64)
        err = err @ np.abs(w64) + (kp + 2) * U * (np.abs(b64) + (np.abs(y) + err) @ np.abs(w64)) + M.activation_allowance(act) * U * np.maximum(1.0, np.abs(nxt))
        y = nxt
    return (y, hn), (err * (1 + 2.0 ** -10), eh * (1 + 2.0 ** -10))


def worst_ratio(shape, activation='elu', out_activation=None, n=24):
    """largest error / bound of gru_row_forward against reference() over n rows: (actions, hidden)"""
    p = make_policy(shape, activation, out_activation)
    rows, h = rows_for(p, n)
    a, hn = host_forward(p, rows, h)
    (ra, rh), (ea, eh) = step_bound(p, rows, h)
    return float((np.abs(a - ra) / ea).max()), float((np.abs(hn[:, :p.hidden] - rh) / eh).max())


def rule_expectation(pending, terminated, D, closing):
    """the episode rule as a loop: (zero_fed [calls][K // D][n], zero_after [calls][n]) - is the row zero where host_rule reports it"""
    pending, terminated = np.asarray(pending, dtype=bool), np.asarray(terminated, dtype=bool)
    calls, K, n = terminated.shape
    fed, after = np.zeros((calls, K // D, n), dtype=bool), np.zeros((calls, n), dtype=bool)
    zero = np.zeros(n, dtype=bool)
    for c in range(calls):
        for k in range(K + int(closing)):
            zero |= pending[c] if k == 0 else terminated[c, k - 1]
            if k % D == 0 and k < K:
                fed[c, k // D] = zero
                zero[:] = False   # the cell's output is not zero
        after[c] = zero
    return fed, after


if __name__ == '__main__':
    print('Error of the recurrent policy\'s law (csrc/gq_policy_gru.h) against numpy float64, host, g++ -O2 -ffp-contract=off.')
    print('Activations: largest |f32 - f64| / (2^-24 max(1, |y|)) over 601 003 arguments (a grid of 200 001 and 200 001 random ones in')
    print('[-20, 20], 200 001 random ones in [-1, 1], 1000 normal ones of scale 1e-3); the tests allow 4 x the ratio they measure.')
    print(f'sig   {sig_error():.4f}   (gru_sig = fmaf(0.5, mlp_tanh(0.5 v), 0.5))')
    print(f'tanh  {M.activation_error("tanh"):.4f}')
    print(f'elu   {M.activation_error("elu"):.4f}')
    print('One step of gru_row_forward from x in [-2, 2], h in [-1, 1] (24 rows) against GruPolicy.reference: worst error / derived first-order')
    print('bound (tests/policy_gru_ref.py step_bound) of the 12 actions and of h\':')
    for shape in SHAPES:
        for act, out in (('elu', None), ('tanh', 'tanh'), ('relu', None)):
            ra, rh = worst_ratio(shape, act, out)
            print(f'{shape:8s} head {act:4s} out {str(out):4s}  actions {ra:.2e}  hidden {rh:.2e}')
