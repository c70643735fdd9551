"""The early publication of convex self pairs (csrc/gq_exchange.h "published early") under the host emulator: a first step leaves the
prediction words in the axis cache, the second step publishes those pairs between the smooth stages and the floor pass and takes them up in
pass B as published - and is held to the fp64 oracle by the one-step parity helper like any other step."""
import numpy as np

from helpers import dbg, emu_lib, emu_step, marshalled, random_states, self_contact_states
import step_parity as sp
from contact_list import Shapes
from step_parity import ParityTally, emu_record
from oracle.oracle import Oracle


def test_second_step_with_predicted_pairs_matches_oracle():
    n_t = 6
    mm = marshalled('mini_cheetah', solver=1, iterations=100, tolerance=1e-10, noise_floor=0.0)
    o = Oracle(marshalled('mini_cheetah', solver=1, iterations=100, tolerance=1e-12))
    rng = np.random.default_rng(23)
    qpos, qvel = self_contact_states(mm.md, n_t, rng, o, want_cross=True)
    # two envs in the key posture in front, one per window of the emulator's 256-slot table: owners publish only while such envs pass by
    q0, v0 = random_states(mm.md, 2, rng, z_range=(0.6, 0.7))
    q0[:, 7:] = mm.md.key_qpos[0][7:]; q0[:, 3:7] = [1, 0, 0, 0]
    qpos, qvel = np.concatenate([q0, qpos]), np.concatenate([0 * v0, 0.2 * qvel]).astype(np.float32)
    n = n_t + 2
    fr = np.full(n, 0.7, np.float32)
    ctrl = (rng.normal(0, 1, (2, n, 12)) * 5).astype(np.float32)
    L = emu_lib()
    runs = {}
    for on in (0, 1):
        L.emu_set_exchange(on)
        try:
            a = emu_step(mm, ctrl[0], qpos.copy(), qvel.copy(), debug_envs=n, friction=fr)
            s1 = {k: a[k].copy() for k in ('qpos', 'qvel', 'warm', 'time')}
            b = emu_step(mm, ctrl[1], s1['qpos'].copy(), s1['qvel'].copy(), warm=s1['warm'].copy(), time=s1['time'].copy(), debug_envs=n, friction=fr, rows=True)
        finally:
            L.emu_set_exchange(0)
        runs[on] = (s1, b)
    s1, b = runs[1]
    early = np.array([dbg(b['debug'][e], 'xq')[10] for e in range(n)])
    print('pairs published early in the second step, per env:', early.tolist())
    assert early[2:].sum() >= 1, 'no pair was published early: the test does not reach the early block'
    assert early[:2].sum() == 0
    # the exchange - early publication included - changes nothing, bit for bit
    for k in ('qpos', 'qvel', 'warm', 'obs'):
        assert np.array_equal(runs[0][1][k], b[k]), k
    for e in range(n):
        for f in ('ncon', 'nefc', 'efc_J', 'efc_aref', 'contact_dist', 'contact_geom', 'qacc'):
            assert np.array_equal(dbg(runs[0][1]['debug'][e], f), dbg(b['debug'][e], f)), (e, f)
    # ... and the second step is the oracle's
    tally = ParityTally(mm.md.cone == 1, 3e-7, shapes=Shapes(mm))
    held_early = 0
    for e in range(2, n):
        cls = tally.step_env(e, o, (s1['qpos'][e], s1['qvel'][e], s1['warm'][e], np.zeros(18), float(s1['time'][e]), 0.7), ctrl[1][e],
                             emu_record(b, e, contacts=True), sp.SELF_STEP)
        held_early += int(cls in sp.COMPARED and early[e] > 0)
    tally.finish_count('emulated second step with early-published pairs', n_t // 2)
    assert held_early >= 1, 'no env that published early was compared by value'
