"""The in-loop policy's input row without a GPU (csrc/gq_policy_dev.h policy_row_value, the row's one definition): the routine the kernel's tile
stage calls, played by a stand-alone g++ program (tests/policy_row_host.cpp, built on first use) over every combination of height scan, last
action and observation history, against a numpy row assembled from the references the feature tests already have - bit for bit."""
import functools
import itertools
import subprocess
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import height_scan_ref
import policy_hist_ref
import policy_mlp_ref

ROOT = Path(__file__).resolve().parent.parent
_TMP = None

N, IN_OBS, OD, COL_Z, STEPS = 3, 5, 9, 7, 3       # the z column lies beyond in_obs; STEPS = L + 1: both buffers are read and written, the oldest frame drops out
SCAN = (2, 3)                                      # rows x cols of the scan
L, COLS = 2, 3                                     # frames, leading observation words of a frame
SCAN_LAW = (0.3, 0.25, 2.5)                        # offset, clip, scale


@functools.lru_cache(maxsize=None)
def host_program():
    global _TMP
    _TMP = tempfile.TemporaryDirectory()
    exe = Path(_TMP.name) / 'policy_row_host'
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-w', '-I', str(ROOT / 'tests' / 'simt_emu'), '-I', str(ROOT / 'gym_quadruped_amd' / 'csrc'),
                    '-o', str(exe), str(ROOT / 'tests' / 'policy_row_host.cpp')], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def _inputs():
    """what every case shares: tables, rows, actions, hit points (a third of the cells saturates on either side), and the store before step 0"""
    rng = np.random.default_rng(11)
    f = np.float32
    d = SimpleNamespace()
    d.shift, d.scale = rng.uniform(-0.5, 0.5, IN_OBS).astype(f), rng.uniform(0.5, 2.0, IN_OBS).astype(f)
    d.obs = rng.standard_normal((STEPS, N, OD)).astype(f)
    d.obs[:, :, COL_Z] = rng.uniform(0.2, 0.6, (STEPS, N))
    d.last = rng.uniform(-1, 1, (STEPS, N, 12)).astype(f)
    cells = SCAN[0] * SCAN[1]
    d.hits = rng.standard_normal((STEPS, N, cells, 3)).astype(f)
    d.hits[..., 2] = (d.obs[:, :, COL_Z, None] - f(SCAN_LAW[0])) - rng.uniform(-1.5, 1.5, (STEPS, N, cells)).astype(f) * f(SCAN_LAW[1])
    return d


def _store0(F):
    """env 0: VALID clear over a store full of 777 (every frame reads as zero); env 1: a marked, valid store in buffer 1 (hist0 of
    policy_hist_ref.marks) and 777 in buffer 0; env 2: the same in buffer 0"""
    hist0, _ = policy_hist_ref.marks(N, L, F, 1)
    state = np.full((N, 2, L, F), 777.0, dtype=np.float32)
    state[1, 1], state[2, 0] = hist0[1], hist0[2]
    return state, np.asarray([1, 1 | 2, 0 | 2], dtype=np.int64)   # bit 0 the parity, bit 1 VALID


def _play(scan, feed_last, hist, reverse):
    d = _inputs()
    cells = SCAN[0] * SCAN[1] if scan else 0
    F = (COLS + (12 if feed_last else 0)) if hist else 0
    head = np.asarray([N, IN_OBS, OD, COL_Z, cells, int(feed_last), L if hist else 0, COLS if hist else 0, STEPS, int(reverse)], dtype=np.int32)
    parts = [d.shift, d.scale, np.asarray(SCAN_LAW, dtype=np.float32)]
    state0 = ctl0 = None
    if hist:
        state0, ctl0 = _store0(F)
        parts += [state0.reshape(-1), ctl0.astype(np.float32)]
    for s in range(STEPS):
        parts += [d.obs[s].reshape(-1), d.last[s].reshape(-1), d.hits[s, :, :cells].reshape(-1)]
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = Path(tmp) / 'in.bin', Path(tmp) / 'out.bin'
        src.write_bytes(head.tobytes() + np.concatenate(parts).astype(np.float32).tobytes())
        subprocess.run([str(host_program()), str(src), str(dst)], check=True)
        out = np.fromfile(dst, dtype=np.float32)
    in_dim = IN_OBS + cells + (12 if feed_last else 0) + (L * F if hist else 0)
    kp = (in_dim + 3) & ~3
    per = N * (kp + in_dim + 2 * (L if hist else 0) * F + (1 if hist else 0))
    out = out.reshape(STEPS, per)
    a, b, c = N * kp, N * (kp + in_dim), N * (kp + in_dim + 2 * (L if hist else 0) * F)
    got = SimpleNamespace(fed=out[:, :a].reshape(STEPS, N, kp), rec=out[:, a:b].reshape(STEPS, N, in_dim),
                          state=out[:, b:c].reshape(STEPS, N, 2, L, F) if hist else None, ctl=out[:, c:].astype(np.int64) if hist else None)
    return got, SimpleNamespace(cells=cells, F=F, in_dim=in_dim, kp=kp, state0=state0, ctl0=ctl0)


def _obs_in(words, cols):
    """(o - shift) * scale over the leading `cols` columns, by policy_mlp_ref.obs_in's float32 arithmetic"""
    d = _inputs()
    law = SimpleNamespace(in_obs=cols, obs_shift=d.shift[:cols], obs_scale=d.scale[:cols])
    return policy_mlp_ref.obs_in(law, np.asarray(words, dtype=np.float32).reshape(-1, words.shape[-1])).reshape(words.shape)


def _reference(scan, feed_last, hist, g):
    """the rows fed and recorded [STEPS, N, in_dim] and the store and control words after every step, in numpy"""
    d = _inputs()
    scan_words = height_scan_ref.scan_law(d.obs[:, :, COL_Z, None], d.hits[..., 2], *SCAN_LAW)[:, :, :g.cells]
    tail = [d.last] if feed_last else []
    fed = [_obs_in(d.obs[:, :, :IN_OBS], IN_OBS), scan_words] + tail
    rec = [d.obs[:, :, :IN_OBS], scan_words] + tail
    states, ctls = [], []
    if hist:
        cur = np.concatenate([d.obs[:, :, :COLS]] + tail, axis=2)                      # the raw current frame of every step [STEPS, N, F]
        hist0 = policy_hist_ref.store_view(g.state0, g.ctl0)
        quiet = np.zeros((STEPS, N), dtype=bool)
        frames, after = policy_hist_ref.fed_history(cur, hist0, np.zeros(N, dtype=bool), quiet, 1, False)   # [STEPS, N, L, F]
        rec.append(frames.reshape(STEPS, N, L * g.F))
        fed.append(_obs_in(frames, COLS).reshape(STEPS, N, L * g.F))
        # the store word for word: a step reads buffer p and writes buffer 1 - p (current block to slot 0, frame_i to slot i), then flips p
        state, ctl = g.state0.copy(), g.ctl0.copy()
        for s in range(STEPS):
            for e in range(N):
                q = 1 - (ctl[e] & 1)
                state[e, q, 0], state[e, q, 1:] = cur[s, e], frames[s, e, :-1]
                ctl[e] = q | 2
            states.append(state.copy()), ctls.append(ctl.copy())
            view = policy_hist_ref.store_view(state, ctl)
            assert np.array_equal(view, frames[s + 1] if s + 1 < STEPS else after)     # (the two models of the store agree)
    return np.concatenate(fed, axis=2), np.concatenate(rec, axis=2), states, ctls


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('scan,feed_last,hist', list(itertools.product([False, True], repeat=3)))
def test_the_row_routine_equals_the_numpy_row_bit_for_bit_in_any_staging_order(scan, feed_last, hist):
    got, g = _play(scan, feed_last, hist, reverse=False)
    rev, _ = _play(scan, feed_last, hist, reverse=True)
    fed, rec, states, ctls = _reference(scan, feed_last, hist, g)
    assert fed.shape == (STEPS, N, g.in_dim) and g.in_dim == IN_OBS + 6 * scan + 12 * feed_last + hist * L * (COLS + 12 * feed_last)
    for name, play in (('lane order', got), ('reverse order', rev)):
        assert np.array_equal(_bits(play.fed[:, :, :g.in_dim]), _bits(fed)), f'{name}: the words fed'
        assert np.array_equal(_bits(play.fed[:, :, g.in_dim:]), np.zeros((STEPS, N, g.kp - g.in_dim), dtype=np.uint32)), f'{name}: +0 behind in_dim'
        assert np.array_equal(_bits(play.rec), _bits(rec)), f'{name}: the recorded raw row'
        if hist:
            assert np.array_equal(_bits(play.state), _bits(np.stack(states))), f'{name}: the store after each step'
            assert np.array_equal(play.ctl, np.stack(ctls)), f'{name}: the control words after each step'
    if not hist:
        return
    # frame_i at step s is the current block of step s - i: its raw words in the record, shift / scale by their ORIGINAL column in the row fed
    col0, a0 = IN_OBS + g.cells + 12 * feed_last, IN_OBS + g.cells
    for s, i in itertools.product(range(STEPS), range(1, L + 1)):
        at = col0 + (i - 1) * g.F
        if s - i < 0:
            assert (got.rec[s, 0, at:at + g.F] == 0).all(), 'the frames of the env without VALID are zero (raw) until its own steps fill them'
            continue
        was = got.rec[s - i]
        assert np.array_equal(_bits(got.rec[s, :, at:at + COLS]), _bits(was[:, :COLS]))
        assert np.array_equal(_bits(got.fed[s, :, at:at + COLS]), _bits(got.fed[s - i, :, :COLS])), 'shift / scale by the original column'
        assert np.array_equal(_bits(got.fed[s, :, at:at + COLS]), _bits(_obs_in(was[:, :COLS], COLS)))
        if feed_last:
            assert np.array_equal(_bits(got.fed[s, :, at + COLS:at + g.F]), _bits(was[:, a0:a0 + 12])), 'the action words as they were'
    assert (got.rec[0, 1:, col0:] < 0).all(), 'the marked stores (negative words) are fed at step 0'
    assert not np.array_equal(got.state[-1], g.state0) and (got.state[-1] != 777).all(), 'both buffers of every env have been written'
