"""Test infrastructure of the observation history (gym_quadruped_amd/csrc/gq_policy_hist.h): the law as a ten-line numpy loop, the store's
view as the env reads it, and the header's routines played on the host (tests/policy_hist_host.cpp, built with g++ on first use)."""
import functools
import subprocess
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
_TMP = None


def fed_history(cur, hist0, pending, term, D, closing):
    """THE REFERENCE.  cur [S, n, F]: the current block of every policy step; hist0 [n, L, F]: the frames before the call, newest first;
    pending [n]: the env waits for its re-spawn before the call; term [S * D, n]: the `terminated` byte after every step; closing: the
    learning modes' visit at k = K.  -> (fed [S, n, L, F], the frames fed at every policy step; after [n, L, F], what would be fed next)"""
    hist, S = np.array(hist0, dtype=np.float32), len(cur)
    term, fed = np.asarray(term, dtype=bool), np.zeros((len(cur),) + np.shape(hist0), dtype=np.float32)
    for s in range(S):
        seen = np.asarray(pending, dtype=bool) if s == 0 else term[(s - 1) * D:s * D].any(axis=0)
        hist[seen] = 0.0                                                      # the rule, before anything of the visit is staged
        fed[s] = hist
        hist = np.concatenate([np.asarray(cur[s])[:, None], hist[:, :-1]], axis=1)  # the push: the current block is the newest, the oldest drops out
    hist[term[(S - 1) * D:S * D - (0 if closing else 1)].any(axis=0)] = 0.0   # the visits after the last push (k = K with closing only)
    return fed, hist


def store_view(state, ctl):
    """[n, 2, L, F] and the control words [n] -> [n, L, F]: the buffer of the word's parity, all zero without VALID (env.policy_history)"""
    state, ctl = np.asarray(state, dtype=np.float32), np.asarray(ctl).astype(np.int64)
    return np.where((((ctl >> 1) & 1) != 0)[:, None, None], state[np.arange(len(ctl)), ctl & 1], np.float32(0.0))


@functools.lru_cache(maxsize=None)
def host_program():
    global _TMP
    _TMP = tempfile.TemporaryDirectory()
    exe = Path(_TMP.name) / 'policy_hist_host'
    subprocess.run(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-w', '-I', str(ROOT / 'tests' / 'simt_emu'), '-I', str(ROOT / 'gym_quadruped_amd' / 'csrc'),
                    '-o', str(exe), str(ROOT / 'tests' / 'policy_hist_host.cpp')], check=True)
    return exe


def _run(args, data):
    with tempfile.TemporaryDirectory() as d:
        src, dst = Path(d) / 'in.bin', Path(d) / 'out.bin'
        data.tofile(src)
        subprocess.run([str(host_program()), *args, str(src), str(dst)], check=True)
        return np.fromfile(dst, dtype=np.float32)


def host_div_mismatches():
    return int(_run(['div'], np.zeros(1, dtype=np.float32))[0])


def marks(n, L, F, S_total):
    """the words of tests/policy_hist_host.cpp: (hist0 [n, L, F], cur [S_total, n, F]) - every word names its env, its step and its place"""
    e, w = np.arange(n)[:, None], np.arange(F)[None, :]
    hist0 = np.stack([-(4096.0 * (i + 1) + 64 * e + w + 1) for i in range(L)], axis=1).astype(np.float32)
    cur = np.stack([4096.0 * (g + 1) + 64 * e + w + 1 for g in range(S_total)]).astype(np.float32)
    return hist0, cur


def host_play(pending, terminated, L, F, D, closing):
    """the header's routines over consecutive calls.  pending [calls][n], terminated [calls][K][n] -> (cur [calls][K // D][n][F],
    fed [calls][K // D][n][L][F], after [calls][n][L][F] through store_view, ctl [calls][n])"""
    pending, terminated = np.asarray(pending, dtype=np.int32), np.asarray(terminated, dtype=np.int32)
    calls, K, n = terminated.shape
    body = np.concatenate([np.concatenate([pending[c].reshape(-1), terminated[c].reshape(-1)]) for c in range(calls)])
    out = _run(['play'], np.concatenate([np.asarray([n, L, F, D, K, calls, int(closing)], dtype=np.int32), body]).view(np.float32))
    S, per = K // D, 2 * L * F
    out = out.reshape(calls, S * n * (F + L * F) + n * per + n)
    rows = out[:, :S * n * (F + L * F)].reshape(calls, S, n, F + L * F)
    state = out[:, S * n * (F + L * F):-n].reshape(calls, n, 2, L, F)
    ctl = out[:, -n:].astype(np.int64)
    after = np.stack([store_view(state[c], ctl[c]) for c in range(calls)])
    return rows[..., :F], rows[..., F:].reshape(calls, S, n, L, F), after, ctl
