"""Start states that reach the branches of the step's observation stage (csrc/gq_step_body.h S11) the whole-step digests do not: the gimbal
pole of the Euler angles, a foot body with several contacts, the elliptic-cone force decode with many contacts, observation layouts that
skip blocks.  One set of builders, two backends: the GPU digests of tests/test_gpu_obs_lanes.py (recorded before the epilogue was rescheduled)
and the emulated one-step parity of tests/test_obs_lanes_emulated.py.  Everything is drawn from seeded generators and filtered by the fp64
oracle alone, so both backends - and the recorded digests - see the same states.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

from helpers import marshalled, oracle_fits_self_budget, random_states, self_contact_states

CMD = (0.4, -0.2, 0.0, 0.3)   # base velocity command of every case (lin x, lin y, lin z, yaw rate): the error observables are not the velocities


def hip_height(robot):
    from gym_quadruped_amd.robot_cfgs import get_robot_config
    return float(get_robot_config(robot).hip_height)


def _oracle(robot, **kw):
    from oracle.oracle import Oracle
    return Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-12, **kw))


def gimbal_states(n):
    """mini_cheetah in the air (z = 1 m), at rest, nose straight down (even envs) or up (odd envs): base quaternion (sqrt(1/2), 0, +-sqrt(1/2), 0),
    R[2][0] = -+1, so that as_euler('xyz') is at its pole."""
    md = marshalled('mini_cheetah').md
    q = np.tile(md.key_qpos[0], (n, 1))
    q[:, 2] = 1.0
    s = np.sqrt(0.5)
    q[:, 3:7] = [s, 0.0, s, 0.0]
    q[1::2, 5] = -s
    return q, np.zeros((n, 18), np.float32)


def calf_contacts(o, calf_bodies):
    """The oracle's world contacts per calf body after its last forward pass"""
    if not o.ncon:
        return {b: 0 for b in calf_bodies}
    b1, b2 = o.get('contact_body1').astype(int), o.get('contact_body').astype(int)
    return {b: int(((b1 <= 0) & (b2 == b)).sum()) for b in calf_bodies}


def folded_states(n, seed=29):
    """mini_cheetah folded onto itself near the floor (helpers.self_contact_states, the generator of the early-publish tests), kept when the
    oracle also finds two or more floor contacts on one calf body: contact_forces of that foot is a sum over several contacts."""
    o = _oracle('mini_cheetah')
    md = o.mm.md
    hip = hip_height('mini_cheetah')
    rng = np.random.default_rng(seed)
    calves = [4 + 3 * leg for leg in range(4)]   # (MuJoCo body ids: world 0, trunk 1, then hip / thigh / calf per leg)
    Q, V = [], []
    for _ in range(40):
        q, v = self_contact_states(md, 2 * n, rng, o, z=(0.5 * hip, 1.1 * hip))
        for e in range(len(q)):
            o.set_state(q[e], v[e], np.zeros(18), np.zeros(18), 0.0, -1.0)
            o.forward(np.zeros(12), stage=1)
            if max(calf_contacts(o, calves).values()) >= 2 and oracle_fits_self_budget(o, False) and len(Q) < n:   # (within the row budget: no contact is cut)
                Q.append(q[e]); V.append(0.2 * v[e])
        if len(Q) == n:
            break
    assert len(Q) == n, f'only {len(Q)} of {n} folded states with two contacts on a calf'
    return np.stack(Q), np.stack(V).astype(np.float32)


def crouch_states(robot, n, seed=31, min_ncon=8):
    """Even envs stand in the key posture, lowered until the four feet touch the floor; odd envs are crouched onto trunk, thighs and calves
    with the legs folded at random - drawn until the oracle finds at least min_ncon contacts, none deeper than 3 cm, that still fit the
    kernel's row budget (a condim-6 foot takes 11 of the 64 rows an elliptic env has, so eight contacts are mostly link contacts): the
    elliptic decode runs over a long contact list and nothing is cut.  Returns (qpos, qvel, the oracle's contact count per env)."""
    o = _oracle(robot)
    md = o.mm.md
    hip = hip_height(robot)
    rng = np.random.default_rng(seed)
    q = np.tile(md.key_qpos[0], (n, 1))
    v = np.zeros((n, 18))
    q[:, 0:2] = rng.uniform(-2, 2, (n, 2))
    ncon = []
    for e in range(n):
        found = None
        if e % 2 == 0:
            for z in np.arange(1.2 * hip, 0.05 * hip, -0.002):
                o.set_state(np.r_[q[e, :2], z, q[e, 3:]], v[e], np.zeros(18), np.zeros(18), 0.0, -1.0)
                o.forward(np.zeros(12), stage=1)
                if o.ncon >= 4:
                    found = (np.r_[q[e, :2], z, q[e, 3:]], o.ncon)
                    break
        else:
            for _ in range(20000):
                qe = random_states(md, 1, rng, z_range=(0.04, 0.2))[0][0]
                qe[7:] = md.key_qpos[0][7:] + rng.uniform(-1.2, 1.2, 12)
                o.set_state(qe, v[e], np.zeros(18), np.zeros(18), 0.0, -1.0)
                o.forward(np.zeros(12), stage=1)
                if o.ncon >= min_ncon and oracle_fits_self_budget(o, md.cone == 1) and o.get('contact_dist').min() > -0.03:
                    found = (qe, o.ncon)
                    break
        assert found is not None, (robot, e, 'no pose with enough contacts')
        q[e] = found[0]
        ncon.append(found[1])
    v[:, 0:6] = rng.normal(0, 0.1, (n, 6))
    return q, v.astype(np.float32), ncon


def floor_states(robot, n, seed=37, z=(0.7, 1.3)):
    """random_states around the standing height (z: the range in hip heights): some envs in flight, some on the floor - from 0.7 hip heights
    most of them pressed into it, over the row budget (the digests); the parity test, which can compare only envs within the budget, starts higher"""
    md = marshalled(robot).md
    hip = hip_height(robot)
    q, v = random_states(md, n, np.random.default_rng(seed), z_range=(z[0] * hip, z[1] * hip))
    return q, v.astype(np.float32)


def controls(n, steps, seed=41, sigma=10.0):
    return (np.random.default_rng(seed).normal(0, 1, (steps, n, 12)) * sigma).astype(np.float32)
