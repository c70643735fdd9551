"""What the height-scan tests share (tests/test_height_scan_host.py, tests/test_gpu_policy_scan.py): the scan law of
csrc/gq_policy_scan.h restated in numpy float32, the host program around the header's routine (tests/height_scan_host.cpp, built with g++ on
first use), and small policies with a scan in their input row."""
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

_TMP = None


def scan_law(z_base, z_hit, offset, clip, scale):
    """s = clamp((z_base - offset) - z_hit, -clip, +clip) * scale in float32: two subtractions in that order, fmax, fmin, one multiply, each
    rounded once (numpy's float32 arithmetic rounds every operation; broadcasting as numpy's)"""
    f = lambda v: np.asarray(v, dtype=np.float32)
    z_base, z_hit, offset, clip, scale = f(z_base), f(z_hit), f(offset), f(clip), f(scale)
    zr = z_base - offset
    d = zr - z_hit
    c = np.fmin(np.fmax(d, -clip), clip)
    return (c * scale).astype(np.float32)


def scan_of(spec, hits, z):
    """the scan [n, cells] of a ``HeightScan`` from hit points [n, rows, cols, 1, 3] (or [n, cells, 3]) and the rows' base z [n]: numpy float32"""
    hits, z = np.asarray(hits, dtype=np.float32), np.asarray(z, dtype=np.float32)
    z_hit = hits.reshape(hits.shape[0], spec.cells, 3)[:, :, 2]
    return scan_law(z[:, None], z_hit, spec.offset, spec.clip, spec.scale)


@functools.lru_cache(maxsize=None)
def host_program():
    global _TMP
    _TMP = tempfile.TemporaryDirectory()
    exe = Path(_TMP.name) / 'height_scan_host'
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-w', '-I', str(ROOT / 'tests' / 'simt_emu'), '-I', str(ROOT / 'gym_quadruped_amd' / 'csrc'),
                    '-o', str(exe), str(ROOT / 'tests' / 'height_scan_host.cpp')], check=True)
    return exe


def host_law(records):
    """height_scan_cell of the header over records [n, 5] = (z_base, z_hit, offset, clip, scale)"""
    rec = np.ascontiguousarray(records, dtype=np.float32).reshape(-1, 5)
    with tempfile.TemporaryDirectory() as d:
        src, dst = Path(d) / 'in.bin', Path(d) / 'out.bin'
        rec.tofile(src)
        subprocess.run([str(host_program()), str(src), str(dst)], check=True)
        return np.fromfile(dst, dtype=np.float32)


def make_mlp(in_obs, spec, hidden=(32, 16), feed_last_action=True, activation='elu', seed=0, shift=True, gain=1.0):
    """an MlpPolicy over in_obs observation columns, the scan of ``spec`` (None: no scan) and, with feed_last_action, the last action"""
    from gym_quadruped_amd.policy import MlpPolicy
    rng = np.random.default_rng(seed)
    in_dim = in_obs + (spec.cells if spec is not None else 0) + (12 if feed_last_action else 0)
    dims = [in_dim, *hidden, 12]
    ws = [(rng.uniform(-1, 1, (k, n)) * gain * np.sqrt(3.0 / k)).astype(np.float32) for k, n in zip(dims[:-1], dims[1:])]
    bs = [rng.uniform(-0.3, 0.3, n).astype(np.float32) for n in dims[1:]]
    kw = dict(obs_shift=rng.uniform(-0.5, 0.5, in_obs).astype(np.float32), obs_scale=rng.uniform(0.5, 2.0, in_obs).astype(np.float32)) if shift else {}
    return MlpPolicy(ws, bs, activation=activation, feed_last_action=feed_last_action, height_scan=spec, **kw)


def make_gru(in_obs, spec, hidden=20, head=(33,), feed_last_action=True, activation='elu', seed=0):
    from gym_quadruped_amd.policy import GruPolicy
    rng = np.random.default_rng(seed + 5)
    in_dim = in_obs + (spec.cells if spec is not None else 0) + (12 if feed_last_action else 0)
    u = lambda k, n: (rng.uniform(-1, 1, (k, n)) * np.sqrt(3.0 / k)).astype(np.float32)
    dims = [hidden, *head, 12]
    return GruPolicy(u(in_dim, 3 * hidden), u(hidden, 3 * hidden), rng.uniform(-0.3, 0.3, 3 * hidden).astype(np.float32), rng.uniform(-0.3, 0.3, 3 * hidden).astype(np.float32),
                     [u(k, n) for k, n in zip(dims[:-1], dims[1:])], [rng.uniform(-0.3, 0.3, n).astype(np.float32) for n in dims[1:]], activation=activation,
                     feed_last_action=feed_last_action, height_scan=spec, obs_shift=rng.uniform(-0.5, 0.5, in_obs).astype(np.float32),
                     obs_scale=rng.uniform(0.5, 2.0, in_obs).astype(np.float32))
