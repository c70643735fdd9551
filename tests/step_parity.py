"""The one-step parity check shared by tests/test_kernel_emulated.py, tests/test_gpu_parity.py and tests/test_gpu_boundary.py: step one env in
the fp64 oracle, classify it (ParityTally), hold the kernel's values for that env to the oracle's (compare) under a NAMED tolerance set.
The kernel side is a plain mapping name -> ndarray made by emu_record (host emulator) or gpu_records (QuadrupedEnv).  TEST INFRASTRUCTURE."""
from __future__ import annotations

from pathlib import Path
from typing import NamedTuple

import numpy as np

from helpers import ALL_OBS, DBG, GQ_MAXEFC, dbg, oracle_fits_self_budget, split_obs, tally_note


class Tol(NamedTuple):
    """|got - ref| < atol * S + rtol * |ref| elementwise (<= when not strict); S = max(1, max|ref|, weight * 9.81 * mass) when scaled, else 1."""
    atol: float
    rtol: float = 0.0
    scaled: bool = False
    weight: float = 0.0     # floor of S as a fraction of the robot's weight (contact-force observables)
    strict: bool = True

    def check(self, got, ref, what, mass=0.0):
        ref = np.asarray(ref, dtype=np.float64)
        err = np.abs(np.asarray(got) - ref)
        s = max(1.0, np.abs(ref).max(initial=0.0), self.weight * 9.81 * mass) if self.scaled else 1.0
        bound = self.atol * s + self.rtol * np.abs(ref)
        assert (err < bound if self.strict else err <= bound).all(), (what, float(err.max(initial=0.0)), float(np.max(bound, initial=0.0)))


def close(rtol, atol=0.0):
    """numpy's assert_allclose(rtol, atol)"""
    return Tol(atol, rtol, strict=False)


def close_scaled(c):
    """numpy's assert_allclose(atol=c * max(1, max|ref|)) with its default rtol"""
    return Tol(c, 1e-7, scaled=True, strict=False)


def below(c, weight=0.0):
    """max|got - ref| < c * max(1, max|ref|, weight of the robot * `weight`)"""
    return Tol(c, scaled=True, weight=weight)


def pick(tols, *names):
    return {k: tols[k] for k in names}


EXACT = Tol(0.0, strict=False)
_FORCE_OBS = ('contact_forces', 'contact_forces:base', 'contact_state')
FLAGS = {'flags': ('terminated', 'invalid')}

# The named tolerance sets: quantity -> Tol, 'obs' -> {observable -> Tol}, 'flags' -> the termination flags held to the oracle's.
# PGS kernel against the oracle's PGS after the same sweeps, the rows of the stage-by-stage tests (emulator: same arithmetic order; GPU: fma contraction)
EMU_STAGE_ROWS = {'efc_J': close(1e-5, 1e-5), 'efc_R': close(1e-5), 'efc_aref': close(1e-4, 1e-2)}
GPU_STAGE_ROWS = {'efc_J': close(1e-4, 1e-5), 'efc_R': close(1e-4), 'efc_aref': close(2e-4, 2e-2)}
GPU_FORWARD_ROWS = pick(GPU_STAGE_ROWS, 'efc_J', 'efc_aref')
# Newton kernel (tolerance 1e-8, fp32) against the oracle's Newton converged to 1e-12 .. 1e-13
ELLIPTIC_STEP = {'efc_J': close_scaled(2e-5), 'efc_R': close(2e-4), 'efc_aref': close_scaled(2e-4), 'qacc': below(2e-4), 'efc_force': below(2e-3),
                 'qvel': Tol(5e-4), 'qpos': Tol(2e-6), 'obs': {k: below(2e-3) for k in _FORCE_OBS + ('feet_vel',)}}
TERRAIN_NEWTON_STEP = {'efc_J': close_scaled(3e-5), 'efc_R': close(3e-4), 'efc_aref': close_scaled(3e-4), 'qacc': below(2e-4), 'qvel': Tol(5e-4),
                       'obs': {**{k: below(1e-2, weight=0.1) for k in ('contact_forces', 'contact_forces:base', 'feet_vel')}, 'contact_state': below(1e-2)},
                       'flags': ('terminated',)}   # (contact_state: bits; under the weight floor a flipped bit of a robot above 100 kg went unnoticed)
IMPEDANCE_STEP = pick(TERRAIN_NEWTON_STEP, 'efc_R', 'efc_aref', 'qacc')
PLANE_PREFIX = {**pick(TERRAIN_NEWTON_STEP, 'efc_J', 'efc_R', 'efc_aref'), **FLAGS}   # the rows the kernel kept against the oracle's first rows
PLANE_STEP = {**PLANE_PREFIX, 'qacc': below(2e-4), 'efc_force': below(2e-3), 'qvel': Tol(5e-4), 'qpos': Tol(2e-6),
              'obs': {k: below(2e-3, weight=0.05) for k in _FORCE_OBS}}
# PGS on world geoms and self-collision rows against the oracle's PGS (no efc_R: the rows are the Newton variant's)
TERRAIN_PGS_STEP = {**pick(TERRAIN_NEWTON_STEP, 'efc_J', 'efc_aref', 'qvel', 'flags'), 'qacc': below(3e-4),
                    'obs': {k: below(1e-2, weight=0.1) for k in _FORCE_OBS}}
TERRAIN_PGS_STEP_GPU = {**pick(TERRAIN_PGS_STEP, 'efc_J', 'efc_aref', 'qacc', 'flags'), 'obs': pick(TERRAIN_PGS_STEP['obs'], 'contact_forces', 'contact_state')}
# robot-robot contacts: deep random interpenetrations, |aref| up to 1e5
SELF_STEP = {'ncon': EXACT, 'efc_J': close(2e-4, 2e-5), 'efc_R': close(2e-4), 'efc_aref': close(2e-4, 5e-2), 'qacc': below(2e-4), 'efc_force': below(2e-3),
             'qvel': Tol(5e-4), 'qpos': Tol(2e-6)}
SELF_STEP_ELLIPTIC = {**SELF_STEP, 'efc_force': below(2e-2)}
CAPSULE_PROXY_STEP = pick(SELF_STEP, 'ncon', 'efc_J', 'qacc')
SELF_STEP_GPU = {'ncon': EXACT, 'obs': {k: below(5e-3) for k in ('contact_state', 'feet_vel', 'base_lin_acc')}, **FLAGS}
CONTACT_COUNT = {'ncon': EXACT}
ROLLOUT_STATE_STEP = {'qacc': below(3e-4), 'qvel': Tol(1e-3)}
HARD_STATE = {'qacc': Tol(2e-5, scaled=True, strict=False)}   # spot (condim 6, impratio 100): 8e-6; the others below 1e-6
# an env over the row budget: the rows the kernel kept and the flags (ParityTally.check_budget_prefix)
BUDGET_PREFIX = {'efc_J': Tol(3e-5, scaled=True, strict=False), 'efc_R': close(3e-4), 'efc_aref': Tol(3e-4, scaled=True, strict=False), **FLAGS}

_ROWS = ('efc_J', 'efc_R', 'efc_aref', 'efc_force')


def compare(o, kern, tols, e=None, cmd=(0, 0, 0, 0), legs_order=(0, 1, 2, 3), mass=0.0):
    """Hold the kernel's values of one env (`kern`: name -> ndarray) to the oracle's after its step, quantity by quantity as `tols` names them.
    Constraint rows are compared over the kernel's first `nefc` rows (all of them when the row counts agree)."""
    k = int(kern['nefc'][0]) if any(name in _ROWS for name in tols) else 0
    for name, tol in tols.items():
        if name in ('obs', 'flags'):
            continue
        ref, got = np.asarray(getattr(o, name), dtype=np.float64), np.asarray(kern[name])
        if name == 'efc_J':
            got = got.reshape(64, 18)
        got, ref = (got[:k], ref[:k]) if name in _ROWS else (got.reshape(ref.shape), ref)
        tol.check(got, ref, (e, name), mass)
    if 'obs' in tols or 'flags' in tols:
        ref, term, inv = o.get_obs(ALL_OBS, cmd, legs_order)
        for name, tol in tols.get('obs', {}).items():
            tol.check(kern['obs'][name], ref[name], (e, name), mass)
        for name in tols.get('flags', ()):
            assert bool(kern[name]) == {'terminated': term, 'invalid': inv}[name], (e, name)


def has_tie(o, threshold):
    """Two hull vertices of (numerically) equal depth, or a convex contact whose point is not determined: fp32 and fp64 may pick either."""
    return bool(o.ncon) and o.get('contact_tiegap').min() < threshold


def emu_record(st, e):
    """The kernel-side mapping of env e out of emu_step's state (its debug record, state rows, observations and flags)."""
    rec = st['debug'][e]
    kern = {name: dbg(rec, name) for name in DBG}
    kern.update(qpos=st['qpos'][e], qvel=st['qvel'][e], obs=split_obs(st['obs'][e], st['obs_names']), terminated=st['terminated'][e], invalid=st['invalid'][e])
    return kern


def gpu_records(env, n, names):
    """The kernel-side mappings of the first n envs of a QuadrupedEnv after a step taken with enable_debug(n): debug_internals(names) plus
    the env's own tensors ('dropped': info['contacts_dropped'])."""
    import torch
    torch.cuda.synchronize()
    d = env.debug_internals(n, names)
    qp, qv, ob = env.qpos.cpu().numpy(), env.qvel.cpu().numpy(), env._obs_buf.cpu().numpy()
    tg, ig, dr = env._terminated.cpu().numpy(), env._invalid.cpu().numpy(), env._contacts_dropped.cpu().numpy()
    obs_names = list(env.state_obs_names) + list(env._extra_names)
    return [dict(d[e], qpos=qp[e], qvel=qv[e], obs=split_obs(ob[e], obs_names), terminated=tg[e], invalid=ig[e], dropped=int(dr[e])) for e in range(n)]


class ParityTally:
    """Why an env was (not) compared value-by-value, and the per-env driver of the one-step parity tests (step_env).

    The strict rule (default): `mismatch` - kernel and oracle disagree on the number of constraint rows although the oracle's set fits
    the kernel's budget and no deepest-vertex tie explains it - is a FAILURE, never a skip: that is what a contact-detection bug looks like.

    lenient_rows=True, the older inline rule `tie or nefc != o.nefc: continue`: an env whose row count differs from the oracle's is SKIPPED
    instead of failing the test, whatever the reason (over the budget or not), and a tie is skipped without holding its rows to the oracle's.
    The skipped mismatches are still counted and printed by report(), so the number is on record."""

    def __init__(self, cone, tie_threshold, lenient_rows=False):
        self.cone, self.tie_threshold, self.lenient_rows = bool(cone), tie_threshold, lenient_rows
        self.n = self.checked = self.tie = self.point = self.budget = self.budget_prefix_checked = 0
        self.mismatch = []

    def classify(self, e, o, nefc_kernel):
        self.n += 1
        gaps = o.get('contact_tiegap') if o.ncon else np.ones(1)
        if self.lenient_rows:
            if gaps.min() < self.tie_threshold:
                self.tie += 1
                return 'tie'
            if int(nefc_kernel) != o.nefc:
                self.mismatch.append((e, int(nefc_kernel), o.nefc))
                return 'mismatch'
            self.checked += 1
            return 'ok'
        if gaps.min() < self.tie_threshold:
            if (gaps[gaps < self.tie_threshold] == -1.0).all():
                # convex contacts whose POINT is not determined (two faces, a face and an edge, parallel edges: every point of the overlap is a
                # valid witness and the polytope's last triangle picks one - gq_oracle.c cvx_point_tie): depth, normal and therefore the number
                # of rows ARE determined and are held to the oracle's; J / forces / qacc of the env are out of reach like a tie's
                self.point += 1
                if oracle_fits_self_budget(o, self.cone):
                    assert int(nefc_kernel) == o.nefc, (e, 'rows of an env with an undetermined contact point', int(nefc_kernel), o.nefc)
                return 'tie'
            self.tie += 1          # two hull vertices of (numerically) equal depth: fp32 / fp64 may pick either
            return 'tie'
        if not oracle_fits_self_budget(o, self.cone):
            self.budget += 1       # robot lying on the ground with more contacts than one wave's 63 rows
            assert nefc_kernel <= GQ_MAXEFC and nefc_kernel < o.nefc, (e, nefc_kernel, o.nefc)
            return 'budget'
        if int(nefc_kernel) != o.nefc:
            self.mismatch.append((e, int(nefc_kernel), o.nefc))
            return 'mismatch'
        self.checked += 1
        return 'ok'

    def step_env(self, e, o, state, ctrl, kern, tols, prefix=False, **kw):
        """The shared sequence for one env: set the oracle to `state` (set_state's arguments), step it with `ctrl`, classify the env by the
        kernel's row count, and hold an 'ok' env to the oracle under `tols` (compare; **kw goes there).  prefix=True also holds an over-budget
        env to the prefix rule, and info['contacts_dropped'] to exactly the contacts of MuJoCo's list the kernel did not take (none of an 'ok' env).
        Returns the class; the caller counts what it needs on the 'ok' envs."""
        o.set_state(*state)
        o.step(np.asarray(ctrl, dtype=np.float64))
        cls = self.classify(e, o, int(kern['nefc'][0]))
        if cls == 'ok':
            compare(o, kern, tols, e, **kw)
            assert not prefix or kern['dropped'] == 0, (e, kern['dropped'])
        elif cls == 'budget' and prefix:
            self.check_budget_prefix(e, o, kern)
            assert kern['dropped'] == o.ncon - int(kern['ncon'][0]) > 0, (e, kern['dropped'], o.ncon, int(kern['ncon'][0]))
        return cls

    def check_budget_prefix(self, e, o, kern):
        """An env over the row budget is not skipped altogether: the kernel keeps a PREFIX of MuJoCo's constraint list
        (friction-loss rows, limit rows, whole contacts in order), so its rows must equal the oracle's first `nefc_kernel`
        rows, and the termination flags - taken from the uncapped contact list - must be the oracle's.  Only the solution
        (forces, qacc) of such an env is out of reach of the comparison."""
        compare(o, kern, BUDGET_PREFIX, (e, 'prefix of an over-budget env'))
        self.budget_prefix_checked += 1

    def report(self, what):
        if self.lenient_rows:
            msg = (f'{what} [lenient rows]: {self.n} envs, {self.checked} compared, {self.tie} ties (rows not held), '
                   f'{len(self.mismatch)} row-count mismatches SKIPPED {self.mismatch[:8]}')
        else:
            msg = (f'{what}: {self.n} envs, {self.checked} compared, {self.tie} deepest-vertex ties, {self.point} with an undetermined contact point (rows held to the oracle), {self.budget} over the row '
                   f'budget ({self.budget_prefix_checked} of them held to the prefix rule), {len(self.mismatch)} MISMATCHED {self.mismatch[:8]}')
        tally_note(msg)
        return msg

    def finish(self, what, min_checked, max_tie, max_budget):
        msg = self.report(what)
        assert not self.mismatch, msg
        nd = self.n - self.point   # the shares are taken among the envs whose contacts are all determined
        assert self.checked >= min_checked * nd and self.tie <= max_tie * self.n and self.budget <= max_budget * self.n and nd >= 0.3 * self.n, msg

    def finish_count(self, what, min_compared):
        """The closing assertion of the tests that ask for a number of compared envs: at least `min_compared`, and (strict rule) no mismatch."""
        msg = self.report(what)
        assert self.lenient_rows or not self.mismatch, msg
        assert self.checked >= min_compared, msg


def hard_states(robot):
    """States captured from benchmark rollouts on which the fp32 Newton solver once ran into the iteration cap (tests/golden/newton_stagnation_*.npz)."""
    return np.load(Path(__file__).parent / 'golden' / f'newton_stagnation_{robot}.npz')


def hold_hard_states(z, o, kern):
    """Every captured state ends within the order of the fp64 oracle's iteration count, at the oracle's solution (kern[e]: 'niter', 'qacc', 'nefc')."""
    for e in range(len(z['qpos'])):
        o.set_state(z['qpos'][e], z['qvel'][e], z['warm'][e], z['applied'][e], 0.0, float(z['friction'][e]))
        o.step(z['ctrl'][e].astype(np.float64))
        nit = int(kern[e]['niter'][0])
        assert nit <= 20, (e, nit, o.solver_niter)
        compare(o, kern[e], HARD_STATE, (e, nit))
