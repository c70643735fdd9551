"""What the MLP-policy tests share (tests/test_policy_mlp_host.py, tests/test_gpu_policy_mlp.py): the host program around the law's
definition (tests/policy_mlp_host.cpp, built with g++ on first use), the test networks, the error bounds, and a numpy restatement of the
policy's noise.

Run as a script it prints the measured error of the header's elu / tanh (profiles/mlp_policy_law_error.txt)."""
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

U = 2.0 ** -24   # unit roundoff of float32
ACT_ID = dict(none=0, relu=1, elu=2, tanh=3)
_TMP = None


@functools.lru_cache(maxsize=None)
def host_program():
    global _TMP
    _TMP = tempfile.TemporaryDirectory()
    exe = Path(_TMP.name) / 'policy_mlp_host'
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-w', '-I', str(ROOT / 'tests' / 'simt_emu'), '-I', str(ROOT / 'gym_quadruped_amd' / 'csrc'),
                    '-o', str(exe), str(ROOT / 'tests' / 'policy_mlp_host.cpp')], check=True)
    return exe


def _run(args, data, dtype=np.float32):
    with tempfile.TemporaryDirectory() as d:
        src, dst = Path(d) / 'in.bin', Path(d) / 'out.bin'
        data.tofile(src)
        subprocess.run([str(host_program()), *args, str(src), str(dst)], check=True)
        return np.fromfile(dst, dtype=dtype)


def host_activation(name, x):
    return _run(['act', str(ACT_ID[name])], np.ascontiguousarray(x, dtype=np.float32))


def host_normal(x0, x1):
    w = np.stack([np.asarray(x0, dtype=np.uint32), np.asarray(x1, dtype=np.uint32)], axis=1)
    return _run(['normal'], np.ascontiguousarray(w))


def obs_in(policy, rows):
    """the network's input rows from raw rows: (o - shift) * scale in float32, each operation rounded (mlp_obs_in)"""
    x = np.array(rows, dtype=np.float32)
    if policy.obs_shift is not None:
        x[:, :policy.in_obs] = x[:, :policy.in_obs] - policy.obs_shift
    if policy.obs_scale is not None:
        x[:, :policy.in_obs] = x[:, :policy.in_obs] * policy.obs_scale
    return x


def host_forward(policy, rows):
    """mlp_row_forward on the packed blob over raw rows: the list of every layer's outputs [n, N_l] (float32), the last one the result"""
    x = obs_in(policy, rows)
    widths = policy.widths + [0] * (4 - len(policy.widths))
    head = np.asarray([len(policy.widths), policy.in_dim, ACT_ID[policy.activation], ACT_ID[policy.out_activation], *widths, x.shape[0]], dtype=np.int32)
    out = _run(['forward'], np.concatenate([head.view(np.float32), policy.pack(), x.reshape(-1)]))
    pads = [(n + 15) & ~15 for n in policy.widths]
    out = out.reshape(x.shape[0], sum(pads))
    layers, at = [], 0
    for n, p in zip(policy.widths, pads):
        assert not out[:, at + n:at + p].any(), 'the padding outputs of a layer are zero'
        layers.append(out[:, at:at + n])
        at += p
    return layers


SHAPES = {
    # no width a multiple of 4 or 16; shift / scale; the last action fed back
    'odd': dict(in_obs=37, hidden=(20, 33), feed_last_action=True, shift=True),
    'wide': dict(in_obs=256, hidden=(256, 256, 256), feed_last_action=False, shift=False),
    'single': dict(in_obs=24, hidden=(), feed_last_action=False, shift=False),
}


def make_policy(shape, activation, out_activation=None, seed=0, in_obs=None, gain=1.0):
    from gym_quadruped_amd.policy import MlpPolicy
    s = SHAPES[shape]
    rng = np.random.default_rng(seed + 17 * len(shape))
    n_obs = s['in_obs'] if in_obs is None else in_obs
    dims = [n_obs + (12 if s['feed_last_action'] else 0), *s['hidden'], 12]
    ws = [(rng.uniform(-1, 1, (k, n)) * gain * np.sqrt(3.0 / k)).astype(np.float32) for k, n in zip(dims[:-1], dims[1:])]
    bs = [rng.uniform(-0.3, 0.3, n).astype(np.float32) for n in dims[1:]]
    kw = {}
    if s['shift']:
        kw = dict(obs_shift=rng.uniform(-0.5, 0.5, n_obs).astype(np.float32), obs_scale=rng.uniform(0.5, 2.0, n_obs).astype(np.float32))
    return MlpPolicy(ws, bs, activation=activation, out_activation=out_activation, feed_last_action=s['feed_last_action'], **kw)


def rows_for(policy, n, seed=1):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, (n, policy.in_dim)).astype(np.float32)


def activation_error(name, n=200_001):
    """largest |header's activation - float64 activation| / (2^-24 max(1, |y|)) over n arguments in [-20, 20] (a grid and random ones)"""
    from gym_quadruped_amd.policy import _ACT64
    rng = np.random.default_rng(5)
    x = np.concatenate([np.linspace(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-1, 1, n), rng.normal(0, 1e-3, 1000)]).astype(np.float32)
    y = _ACT64[name](x.astype(np.float64))
    got = host_activation(name, x).astype(np.float64)
    return float((np.abs(got - y) / (U * np.maximum(1.0, np.abs(y)))).max())


@functools.lru_cache(maxsize=None)
def activation_allowance(name):
    """the activation's own error a test allows: 4 x the measured ratio (the factor of profiles/foot_cmd_law_error.txt), in units of 2^-24 max(1, |y|)"""
    return 0.0 if name in ('none', 'relu') else 4.0 * activation_error(name)


def layer_bounds(policy, layers, rows):
    """Per layer: (float64 evaluation of that ONE layer on the float32 inputs the program gave it, the allowed error).  Linear part: the
    first-order bound of a Kp-long fma chain, (Kp + 2) 2^-24 (|b| + sum |x_k w_k|); the activation is 1-Lipschitz and adds its own error."""
    from gym_quadruped_amd.policy import _ACT64
    x = obs_in(policy, rows).astype(np.float64)
    res = []
    for l, (w, b) in enumerate(zip(policy.weights, policy.biases)):
        w64, b64 = w.astype(np.float64), b.astype(np.float64)
        kp = (w.shape[0] + 3) & ~3
        act = policy.out_activation if l == len(policy.weights) - 1 else policy.activation
        y = _ACT64[act](x @ w64 + b64)
        bound = (kp + 2) * U * (np.abs(b64) + np.abs(x) @ np.abs(w64)) + activation_allowance(act) * U * np.maximum(1.0, np.abs(y))
        res.append((y, bound))
        x = layers[l].astype(np.float64)
    return res


def network_bound(policy, rows):
    """(reference(), allowed error) of the whole network's 12 outputs: the per-layer bound carried through the following layers (an error e on
    a layer's outputs reaches the next layer's as at most e |W|, activations being 1-Lipschitz); evaluated on the float64 activations, to
    first order like the per-layer bound itself, with the factor 1 + 2^-10 for the higher orders."""
    from gym_quadruped_amd.policy import _ACT64
    x = np.array(rows, dtype=np.float64)
    err = np.zeros_like(x)
    if policy.obs_shift is not None:
        x[:, :policy.in_obs] -= policy.obs_shift.astype(np.float64)
    if policy.obs_scale is not None:
        x[:, :policy.in_obs] *= policy.obs_scale.astype(np.float64)
    if policy.obs_shift is not None or policy.obs_scale is not None:
        err[:, :policy.in_obs] = 2 * U * np.abs(x[:, :policy.in_obs])   # the two float32 roundings of (o - shift) * scale
    for l, (w, b) in enumerate(zip(policy.weights, policy.biases)):
        w64, b64 = w.astype(np.float64), b.astype(np.float64)
        kp = (w.shape[0] + 3) & ~3
        act = policy.out_activation if l == len(policy.weights) - 1 else policy.activation
        y = _ACT64[act](x @ w64 + b64)
        err = err @ np.abs(w64) + (kp + 2) * U * (np.abs(b64) + (np.abs(x) + err) @ np.abs(w64)) + activation_allowance(act) * U * np.maximum(1.0, np.abs(y))
        x = y
    return x, err * (1 + 2.0 ** -10)


def normal_ref(x0, x1):
    """mlp_normal (csrc/gq_policy_mlp.h) restated line by line in numpy float64: the same IEEE operations in the same order, hence the same
    bits.  x0, x1: words 0, 1 of the Philox blocks (uint32 arrays)."""
    x0, x1 = np.asarray(x0, dtype=np.uint64), np.asarray(x1, dtype=np.uint64)
    v = 2 * (x0 >> np.uint64(8)) + 1
    e = np.frexp(v.astype(np.float64))[1].astype(np.int64) - 1   # position of the top bit (v < 2^25 is exact in float64)
    m = v.astype(np.float64) / (2.0 ** e)
    big = m > 1.4142135623730951
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    p = np.full_like(s, 1.0 / 15.0)
    for d in (13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * s2 + 1.0 / d
    p = p * s2 + 1.0
    ln_u1 = (e - 25).astype(np.float64) * 0.6931471805599453 + 2.0 * s * p
    u2 = (x1 >> np.uint64(8)).astype(np.float64) * (1.0 / 16777216.0)
    w = u2 - 0.5
    a = np.abs(w)
    fold = a > 0.25
    b = np.where(fold, 0.5 - a, a)
    th = 6.283185307179586 * b
    t2 = th * th
    c = np.full_like(t2, 1.0 / 20922789888000.0)
    for d in (87178291200.0, 479001600.0, 3628800.0, 40320.0, 720.0, 24.0):
        c = 1.0 / d - c * t2
    c = 0.5 - c * t2
    c = 1.0 - c * t2
    z = np.sqrt(-2.0 * ln_u1) * np.where(fold, c, -c)
    return z.astype(np.float32)


def policy_noise(seed, step, n_envs, env_id_offset=0):
    """z [n_envs, 12] of the MLP policy at step `step` (noise_step0 + k): Philox block (joint, step, global env id, 0x3b1f), key = seed"""
    from philox_ref import philox4x32
    x0, x1 = np.zeros((n_envs, 12), dtype=np.uint32), np.zeros((n_envs, 12), dtype=np.uint32)
    for e in range(n_envs):
        for j in range(12):
            w = philox4x32((j, step, e + env_id_offset, 0x3b1f), (seed & 0xffffffff, seed >> 32))
            x0[e, j], x1[e, j] = w[0], w[1]
    return normal_ref(x0.reshape(-1), x1.reshape(-1)).reshape(n_envs, 12)


if __name__ == '__main__':
    print('Error of the MLP policy\'s activations (csrc/gq_policy_mlp.h: mlp_elu, mlp_tanh - IEEE operations and fmaf, no library call)')
    print('against numpy float64: largest |f32 - f64| / (2^-24 max(1, |y|)) over 601 003 arguments (a grid of 200 001 and 200 001 random')
    print('ones in [-20, 20], 200 001 random ones in [-1, 1], 1000 normal ones of scale 1e-3), g++ -O2 -ffp-contract=off, host.')
    print('The tests allow 4 x the ratio they measure themselves (tests/policy_mlp_ref.py activation_allowance).')
    for name in ('elu', 'tanh'):
        print(f'{name:5s} {activation_error(name):.4f}')
