"""TEST INFRASTRUCTURE shared by the CPU and GPU tests of the sensor noise on the in-loop policy's input row (csrc/gq_policy_noise.h): the
law restated in numpy float32 / float64 on tests/philox_ref.py's Philox, and the host program around policy_row_value<.., NOISE = true>
(tests/obs_noise_host.cpp, built with g++ on first use)."""
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

from philox_ref import M0, M1, W0, W1   # noqa: E402
from policy_mlp_ref import normal_ref                # noqa: E402

STREAM = 0x0b5e          # GQ_OBS_NOISE_STREAM
ACTION_STREAM = 0x3b1f   # GQ_MLP_NOISE_STREAM
OTHER_STREAMS = (0x3b1f, 0x9011, 0xc0de, 0xd157, 0x5eed)
KIND = dict(uniform=0, normal=1)
_TMP = None


def counters(cols, steps, gids):
    """the Philox counters (c, step, gid, STREAM) of every (row, column): cols [C], steps / gids [n] -> uint32 [n, C, 4]"""
    cols, steps, gids = (np.asarray(v, dtype=np.int64) & 0xffffffff for v in (cols, steps, gids))
    n, C = steps.shape[0], cols.shape[0]
    ctr = np.empty((n, C, 4), dtype=np.uint32)
    ctr[..., 0] = cols[None, :]
    ctr[..., 1] = steps[:, None]
    ctr[..., 2] = gids[:, None]
    ctr[..., 3] = STREAM
    return ctr


def philox_blocks(ctr, seed):
    """philox_ref.philox4x32 over an array of counters [..., 4] (uint32): the same ten rounds, vectorised -> uint32 [..., 4]"""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint64(seed & 0xffffffff), np.uint64((seed >> 32) & 0xffffffff)
    lo, s32 = np.uint64(0xffffffff), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & lo, (p0 >> s32) ^ c[3] ^ k1, p0 & lo]
        k0, k1 = (k0 + np.uint64(W0)) & lo, (k1 + np.uint64(W1)) & lo
    return np.stack(c, axis=-1).astype(np.uint32)


def unit(kind, x0, x1):
    """n of the law from words 0, 1 of the blocks: float32"""
    if kind == 'normal':
        return normal_ref(np.asarray(x0).reshape(-1), np.asarray(x1).reshape(-1)).reshape(np.shape(x0))
    u = (np.asarray(x0, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u + u) - np.float32(1.0)


def draws(kind, seed, cols, steps, gids):
    """n [n, C] float32 of columns `cols` for rows keyed by (steps, gids)"""
    w = philox_blocks(counters(cols, steps, gids), seed)
    return unit(kind, w[..., 0], w[..., 1])


def amp_row(amp, in_obs, cells, in_dim, scan_amp=0.0):
    """the amplitude of every column of the input row: amp on the observation columns, scan_amp on the scan's, 0 behind them"""
    a = np.zeros(in_dim, dtype=np.float32)
    a[:in_obs] = np.broadcast_to(np.asarray(amp, dtype=np.float32), (in_obs,))
    a[in_obs:in_obs + cells] = np.float32(scan_amp)
    return a


def apply(rows, amps, kind, seed, steps, gids):
    """THE LAW over raw input rows [n, in_dim] (float32) with per-column amplitudes `amps` [in_dim] (amp_row): o + amp * n, the product and the
    sum each rounded to float32; a column with amplitude 0 passes bit for bit"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    out = rows.copy()
    on = np.flatnonzero(amps > 0)
    if on.size:
        n = draws(kind, seed, on, steps, gids)
        d = (amps[on][None, :] * n).astype(np.float32)
        out[:, on] = (rows[:, on] + d).astype(np.float32)
    return out


def apply64(rows, amps, kind, seed, steps, gids):
    """the same in float64 arithmetic on the float32 draws: what the law rounds"""
    out = np.array(rows, dtype=np.float64)
    on = np.flatnonzero(amps > 0)
    if on.size:
        out[:, on] += amps[on].astype(np.float64)[None, :] * draws(kind, seed, on, steps, gids).astype(np.float64)
    return out


def action_counters(steps, gids):
    """the counters of the action noise (gq_policy_mlp.h: (joint, step, gid, 0x3b1f)) for the same keys: uint32 [n, 12, 4]"""
    ctr = counters(np.arange(12), steps, gids)
    ctr[..., 3] = ACTION_STREAM
    return ctr


@functools.lru_cache(maxsize=None)
def host_program():
    global _TMP
    _TMP = tempfile.TemporaryDirectory()
    exe = Path(_TMP.name) / 'obs_noise_host'
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-w', '-I', str(ROOT / 'tests' / 'simt_emu'), '-I', str(ROOT / 'gym_quadruped_amd' / 'csrc'),
                    '-o', str(exe), str(ROOT / 'tests' / 'obs_noise_host.cpp')], check=True)
    return exe


def host_play(in_obs, od, col_z, cells, feed_last, L, cols, kind, seed, step0, D, gids, amp, scan_amp, shift, scale, scan_law, store, ctl, obs, last, hits,
              reverse=False):
    """tests/obs_noise_host.cpp: `steps` consecutive policy steps of n envs through policy_row_value<SCAN, HIST, LearnPlain, true>, policy step s
    keyed by (step0 + s D, gids[e]).  obs [steps, n, od], last [steps, n, 12], hits [steps, n, cells, 3]; store [n, 2, L, F] / ctl [n] the
    history before the first step (ignored with L = 0).  Returns dict(fed [steps, n, Kp], rec, clean [steps, n, in_dim], store [steps, n, 2, L, F],
    ctl [steps, n])."""
    steps, n = obs.shape[0], obs.shape[1]
    F = (cols + (12 if feed_last else 0)) if L else 0
    in_dim = in_obs + cells + (12 if feed_last else 0) + L * F
    kp = (in_dim + 3) & ~3
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    head = np.array([n, in_obs, od, col_z, cells, int(feed_last), L, cols, steps, int(reverse), KIND[kind], seed & 0xffffffff, (seed >> 32) & 0xffffffff, step0, D],
                    dtype=np.uint32)
    parts = [head.view(np.float32), np.asarray(gids, dtype=np.uint32).view(np.float32), f32(np.broadcast_to(np.asarray(amp, dtype=np.float32), (in_obs,))),
             f32([scan_amp]), f32(shift), f32(scale), f32(scan_law)]
    if L:
        parts += [f32(store), f32(ctl)]
    for s in range(steps):
        parts += [f32(obs[s]), f32(last[s])] + ([f32(hits[s])] if cells else [])
    with tempfile.TemporaryDirectory() as d:
        src, dst = Path(d) / 'in.bin', Path(d) / 'out.bin'
        np.concatenate(parts).tofile(src)
        subprocess.run([str(host_program()), str(src), str(dst)], check=True)
        res = np.fromfile(dst, dtype=np.float32)
    per = n * (kp + 2 * in_dim + 2 * L * F + (1 if L else 0))
    assert res.size == steps * per, (res.size, steps, per)
    res = res.reshape(steps, per)
    out, at = {}, 0
    for name, shape in (('fed', (n, kp)), ('rec', (n, in_dim)), ('clean', (n, in_dim)), ('store', (n, 2, L, F)), ('ctl', (n,) if L else (0,))):
        size = int(np.prod(shape))
        out[name] = res[:, at:at + size].reshape((steps,) + shape)
        at += size
    return out


def host_words(seed, cols, steps, gids):
    """words 0, 1 of the header's own Philox (noise_philox01) for every (row, column): the `philox` mode of the host program -> uint32 [n, C, 2]"""
    ctr = counters(cols, steps, gids).reshape(-1, 4)
    with tempfile.TemporaryDirectory() as d:
        src, dst = Path(d) / 'in.bin', Path(d) / 'out.bin'
        np.concatenate([np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff, ctr.shape[0]], dtype=np.uint32), ctr.reshape(-1)]).tofile(src)
        subprocess.run([str(host_program()), 'philox', str(src), str(dst)], check=True)
        return np.fromfile(dst, dtype=np.uint32).reshape(len(np.atleast_1d(steps)), len(np.atleast_1d(cols)), 2)

