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
# go1's cylinder geoms are regular 32-vertex prisms: by the oracle alone (tools/contact_pose_sensitivity.py: its own normal jumps under one fp32
# rounding of the geom poses) 47 of the self-collision test's 160 envs hold a contact whose minimum translation has two directions - the share of
# contacts per env that hold_contact_list may accept as the other direction on go1; every other robot: none
GO1_NORMAL_TIES = 0.3
COMPARED = ('ok', 'point_held', 'tie_held')   # ParityTally.step_env: the classes of an env that was held to the caller's tolerance set


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


def emu_record(st, e, contacts=False):
    """The kernel-side mapping of env e out of emu_step's state (its debug record, state rows, observations and flags; contacts=True: its
    contact row as well, decoded - kern['contacts'])."""
    rec = st['debug'][e]
    kern = {name: dbg(rec, name) for name in DBG}
    if contacts:
        from contact_list import contact_env, decode_contact_rows
        kern['contacts'] = contact_env(decode_contact_rows(st['contacts'][e:e + 1]), 0)
    kern.update(qpos=st['qpos'][e], qvel=st['qvel'][e], obs=split_obs(st['obs'][e], st['obs_names']), terminated=st['terminated'][e], invalid=st['invalid'][e])
    return kern


def gpu_records(env, n, names):
    """The kernel-side mappings of the first n envs of a QuadrupedEnv after a step taken with enable_debug(n): debug_internals(names) plus
    the env's own tensors ('dropped': info['contacts_dropped'])
    and, from an env built with accessors=True, env.contacts() ('contacts')."""
    import torch
    torch.cuda.synchronize()
    d = env.debug_internals(n, names)
    qp, qv, ob = env.qpos.cpu().numpy(), env.qvel.cpu().numpy(), env._obs_buf.cpu().numpy()
    tg, ig, dr = env._terminated.cpu().numpy(), env._invalid.cpu().numpy(), env._contacts_dropped.cpu().numpy()
    obs_names = list(env.state_obs_names) + list(env._extra_names)
    recs = [dict(d[e], qpos=qp[e], qvel=qv[e], obs=split_obs(ob[e], obs_names), terminated=tg[e], invalid=ig[e], dropped=int(dr[e])) for e in range(n)]
    if getattr(env, '_contacts', None) is not None:   # an env built with accessors=True: the contact list, through env.contacts()
        from contact_list import contact_env, contacts_numpy
        con = contacts_numpy(env.contacts())
        for e in range(n):
            recs[e]['contacts'] = contact_env(con, e)
    return recs


class ParityTally:
    """Why an env was (not) compared value-by-value, and the per-env driver of the one-step parity tests (step_env).

    With the kernel's contact list in the records (kern['contacts']) the list itself is held to the oracle's contact by contact, and an env
    whose contact POINTS alone are undecided is compared by value after the oracle has taken the kernel's points (step_env_with_list);
    without it such an env is held to the oracle's row count only (classify).

    The strict rule (default): `mismatch` - kernel and oracle disagree on the number of constraint rows although the oracle's set fits
    the kernel's budget and no deepest-vertex tie explains it - is a FAILURE, never a skip: that is what a contact-detection bug looks like.

    lenient_rows=True, the older inline rule `tie or nefc != o.nefc: continue`: an env whose row count differs from the oracle's is SKIPPED
    instead of failing the test, whatever the reason (over the budget or not), and a tie is skipped without holding its rows to the oracle's.
    The skipped mismatches are still counted and printed by report(), so the number is on record."""

    def __init__(self, cone, tie_threshold, lenient_rows=False, shapes=None):
        """shapes: contact_list.Shapes of the model, needed where the kernel records carry the contact list"""
        self.cone, self.tie_threshold, self.lenient_rows, self.shapes = bool(cone), tie_threshold, lenient_rows, shapes
        self.n = self.checked = self.tie = self.point = self.budget = self.budget_prefix_checked = self.point_held = self.tie_held = self.capped = self.budget_tie = 0
        self.mismatch = []
        from contact_list import ListStats
        self.list_stats = ListStats()

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
        kern['contacts'] (contact_list.contact_env: the kernel's contact row; strict rule only) adds the contact list, contact by contact, and
        the value comparison of the envs with an undetermined point (step_env_with_list).
        Returns the class; COMPARED names the classes that were held to `tols`, on which the caller counts what it needs."""
        o.set_state(*state)
        o.step(np.asarray(ctrl, dtype=np.float64))
        if kern.get('contacts') is not None and not self.lenient_rows:
            return self.step_env_with_list(e, o, state, ctrl, kern, tols, prefix, **kw)
        cls = self.classify(e, o, int(kern['nefc'][0]))
        if cls == 'ok':
            compare(o, kern, tols, e, **kw)
            assert not prefix or kern['dropped'] == 0, (e, kern['dropped'])
        elif cls == 'budget' and prefix:
            self.check_budget_prefix(e, o, kern)
            assert kern['dropped'] == o.ncon - int(kern['ncon'][0]) > 0, (e, kern['dropped'], o.ncon, int(kern['ncon'][0]))
        return cls

    def step_env_with_list(self, e, o, state, ctrl, kern, tols, prefix=False, **kw):
        """step_env once the oracle has stepped, for a kernel record that carries the contact list.  Every env but one with a capped convex
        pair has its list held to the oracle's (contact_list.hold_contact_list).  An env whose only undecided quantities are contact POINTS
        (tiegap -1: two faces, a face and an edge, parallel edges; or two vertices of equal depth) - or the direction of a minimum translation
        that has two of equal depth - is then compared by value all the same: the oracle steps again from the same state with the kernel's
        points (that normal) substituted for exactly those contacts (Oracle.set_contact_pos) - its contact and row counts must not move -
        and the env is held to `tols` like an 'ok' env.  mj_contactForce of the row is held to the oracle's under tols['efc_force']
        (below(2e-3) where the set has none)."""
        from contact_list import hold_contact_forces, hold_contact_list
        con, nefc_k, mass = kern['contacts'], int(kern['nefc'][0]), kw.get('mass', 0.0)
        ftol = tols.get('efc_force', below(2e-3))
        hold = lambda: hold_contact_list(o, con, np.asarray(state[0])[:2], self.shapes, self.cone, self.tie_threshold, e, self.list_stats)
        assert int(con['nefc']) == nefc_k, (e, 'row count of the contact row', int(con['nefc']), nefc_k)
        gaps = o.get('contact_tiegap') if o.ncon else np.ones(1)
        low = gaps < self.tie_threshold
        self.n += 1
        if (low & (gaps == 0.0) & (o.get('contact_cvx') == 1.0)).any():
            self.capped += 1       # a convex pair at the shared iteration cap: both sides hold an unfinished iteration's state - its dist is held to
            if oracle_fits_self_budget(o, self.cone) and nefc_k == o.nefc:   # capped_dist and the other contacts of the list in full where the two
                hold()                                                        # states still gave the same list; rows and solution stay out
            return 'capped'
        if not oracle_fits_self_budget(o, self.cone):
            self.budget += 1       # robot lying on the ground with more contacts than one wave's 63 rows: the list and - where no contact has to be
            assert nefc_k <= GQ_MAXEFC and nefc_k < o.nefc, (e, nefc_k, o.nefc)   # substituted - the rows are held to the prefix rule
            if not hold() and prefix:
                self.check_budget_prefix(e, o, kern)
                assert kern['dropped'] == o.ncon - int(kern['ncon'][0]) > 0, (e, kern['dropped'], o.ncon, int(kern['ncon'][0]))
                return 'budget'
            self.budget_tie += int(low.any())
            return 'budget' if not low.any() else 'budget_tie'
        point = bool((gaps[low] == -1.0).all())
        if not point and (nefc_k != o.nefc or int(con['ncon']) != o.ncon):
            self.tie += 1          # two hull vertices of equal depth against the floor: the other choice changes the manifold of the geom
            return 'tie'
        if nefc_k != o.nefc:
            assert not low.any(), (e, 'rows of an env with an undetermined contact point', nefc_k, o.nefc)
            self.mismatch.append((e, nefc_k, o.nefc))
            return 'mismatch'
        subst = hold()
        if subst:
            ncon, nefc, idx = o.ncon, o.nefc, sorted(subst)
            o.set_state(*state)
            o.set_contact_pos(idx, [subst[c][0] for c in idx], [np.full(3, np.nan) if subst[c][1] is None else subst[c][1] for c in idx])
            o.step(np.asarray(ctrl, dtype=np.float64))
            assert (o.ncon, o.nefc) == (ncon, nefc), (e, 'the substituted points changed the oracle\'s list', o.ncon, o.nefc, ncon, nefc)
        compare(o, kern, tols, e, **kw)
        hold_contact_forces(o, con, ftol, e, mass, self.list_stats)
        assert not prefix or kern['dropped'] == 0, (e, kern['dropped'])
        if not subst:
            self.checked += 1
            return 'ok'
        if all(gaps[c] == -1.0 for c in subst):
            self.point_held += 1
            return 'point_held'
        self.tie_held += 1         # a vertex tie, or a minimum translation with two directions
        return 'tie_held'

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
            if self.list_stats.n['contacts']:
                msg += (f'; with the contact list: {self.point_held} with an undetermined point and {self.tie_held} with a vertex tie compared by value after substituting the '
                        f'kernel\'s points (point_held, tie_held), {self.capped} with a capped convex pair left out, {self.budget_tie} of the over-budget ones with such a point; ' + self.list_stats.line(what))
        tally_note(msg)
        return msg

    def finish(self, what, min_checked, max_tie, max_budget):
        msg = self.report(what)
        assert not self.mismatch, msg
        nd = self.n - self.point   # the shares are taken among the envs whose contacts are all determined
        assert self.checked >= min_checked * nd and self.tie <= max_tie * self.n and self.budget <= max_budget * self.n and nd >= 0.3 * self.n, msg

    def finish_held(self, what, min_checked, max_uncompared, max_budget, min_compared=0.9, max_normal_tie=0.0):
        """finish() for a tally whose records carried the contact list: the envs compared by value - 'ok' ones and the ones held by substitution -
        make up at least min_compared of all, the ones left out (capped convex pairs, vertex ties that changed a manifold) at most
        max_uncompared; min_checked is finish()'s share of 'ok' envs among the ones that had nothing to substitute; max_normal_tie: contacts
        accepted as the other of two minimum translations, per env of the tally (0 unless the robot has regular prisms)."""
        msg = self.report(what)
        assert not self.mismatch, msg
        held = self.point_held + self.tie_held
        assert self.checked + held >= min_compared * self.n and self.tie + self.capped + self.point <= max_uncompared * self.n, msg
        # a second minimum translation of equal depth (contact_list.hold_contact_list) is a property of regular prisms: none elsewhere
        assert self.list_stats.n['normal_tie'] <= max_normal_tie * self.n, msg
        assert self.checked >= min_checked * (self.n - held) and self.budget - self.budget_tie <= max_budget * self.n, msg   # (max_budget: of the envs without a tie, as in finish)

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
