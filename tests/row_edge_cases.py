"""Constraint rows outside the box the whole-step parity tests draw from: joint-limit rows (random_states never puts a joint past its range)
and contacts at low ground friction (the suite steps at 0.55 - 0.8), with the checks that hold a backend's records to the fp64 oracle.  One
set of builders, two backends: the step kernel under the host emulator (tests/test_row_edges_emulated.py) and on the GPU
(tests/test_gpu_row_edges.py); tests/reports/low_friction_sweep.py prints the friction table from the same states.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

import step_parity as sp
from contact_list import Shapes
from helpers import budgeted_states, marshalled, oracle_fits_self_budget, random_states, tally_note
from step_parity import ParityTally, below

TIMESTEP = 0.002
OVERSHOOT = (1e-5, 1e-3, 0.02, 0.2)   # rad past the range; nothing below 1e-5: fp32 qj against an fp32 range decides differently from fp64 within ~3e-7 rad
INSIDE = 1e-5                          # rad inside the range: no row (jnt_margin is 0 on every model)
LIMIT_ROBOTS = ('aliengo', 'b2', 'go2', 'spot')   # partial `limited` mask, pyramidal / pyramidal, all limited / 12 friction-loss rows + condim-6 feet, elliptic / implicitfast
FRICTIONS = (0.0, 1e-3, 3e-3, 5e-3, 1e-2, 2e-2, 3e-2, 0.05, 0.1, 0.2, 3.0)
Z_LOW = (0.3, 1.6)    # base height of the envs near the floor, in hip heights: drawn until the oracle finds a floor contact (limit_states)
N_FRICTION = len(FRICTIONS) * 12
# (robot, solver): pyramidal Newton - the cases with a floor -, elliptic Newton, PGS
FRICTION_CASES = (('aliengo', 'newton'), ('mini_cheetah', 'newton'), ('b2', 'newton'), ('go2', 'newton'), ('hyqreal1', 'newton'), ('aliengo', 'pgs'))
PGS_SWEEPS = 50


def hip_height(robot):
    from gym_quadruped_amd.robot_cfgs import get_robot_config
    return float(get_robot_config(robot).hip_height)


def limited_joints(md):
    """The hinges 0..11 (joint 0 is the free joint) that have a range"""
    return np.where(np.asarray(md.jnt_limited)[1:13] != 0)[0]


def expected_limit_rows(md, qpos_env):
    """MuJoCo's limit rows of one env from qpos and jnt_range in fp64, in its order: joint by joint, the lower side before the upper.
    [(hinge, sign of the row's single Jacobian entry)]: dist = q - lo, J = +1 on the lower side; dist = hi - q, J = -1 on the upper."""
    rg, mg = np.asarray(md.jnt_range, dtype=np.float64)[1:13], np.asarray(md.jnt_margin, dtype=np.float64)[1:13]
    rows = []
    for j in limited_joints(md):
        q = float(qpos_env[7 + j])
        if q - rg[j, 0] < mg[j]:
            rows.append((int(j), 1.0))
        if rg[j, 1] - q < mg[j]:
            rows.append((int(j), -1.0))
    return rows


def limit_states(md, n, rng, hip, o):
    """random_states with joints placed past their range.  Env e: k = (1, 2, 4, every limited joint)[e % 4] joints, each one of OVERSHOOT past a
    random side; the envs with e % 8 == 5 have their k = (1, 2, 4, all)[(e // 8) % 4] joints INSIDE the range by 1e-5 instead and must
    give no row.  Half of the envs (at random) have the base at 2 - 3 hip heights: no floor contact, limit and friction-loss rows only.
    The others are near the floor, where limit rows and contacts share the row budget.  Legs folded to the ends of their ranges do not reach
    the floor from a standing height, and a robot lying on its links is over the budget (0.8 - 1.6 hip heights, by the oracle `o` alone:
    0 - 7 of 48 envs with limit rows and contacts, 18 - 100 % of the envs in contact over budget on the four robots).  So the height of such an
    env is drawn from Z_LOW hip heights up to 40 times, until the oracle finds a contact and the constraint set fits the budget; the first
    max(3, n // 16) envs with every limited joint's row are drawn until it does NOT fit instead (held to the prefix rule: their limit rows come in
    front of the contacts that are cut).
    Returns (qpos, qvel, rows, inside): rows[e] = expected_limit_rows of env e, inside[e] = it is one of the no-row envs."""
    qpos, qvel = random_states(md, n, rng, z_range=(2.0 * hip, 3.0 * hip))
    high = rng.permutation(n) < n // 2
    lim, rg = limited_joints(md), np.asarray(md.jnt_range, dtype=np.float64)[1:13]
    ks = (1, 2, 4, len(lim))
    inside = np.arange(n) % 8 == 5
    over = 0
    for e in range(n):
        k = ks[(e // 8) % 4] if inside[e] else ks[e % 4]
        for j in rng.permutation(lim)[:k]:
            side, d = int(rng.integers(2)), -INSIDE if inside[e] else OVERSHOOT[int(rng.integers(len(OVERSHOOT)))]
            qpos[e, 7 + j] = rg[j, 0] - d if side == 0 else rg[j, 1] + d
        if high[e]:
            continue
        want_over = k == len(lim) and not inside[e] and over < max(3, n // 16)
        found = None
        for _ in range(40):
            z = rng.uniform(Z_LOW[0] * hip, Z_LOW[1] * hip)
            o.set_state(np.r_[qpos[e, :2], z, qpos[e, 3:]], qvel[e], np.zeros(18), np.zeros(18), 0.0, 0.8)
            o.forward(np.zeros(12), stage=1)
            fits = oracle_fits_self_budget(o, md.cone == 1)
            if o.ncon and fits != want_over:
                found = (z, fits)
                break
            if o.ncon and fits and found is None:
                found = (z, fits)   # (no over-budget height in 40 draws: the first that fits)
        if found is not None:
            qpos[e, 2] = found[0]
            over += not found[1]
        else:
            qpos[e, 2] = 2.5 * hip   # (nothing found: in flight)
    return qpos, qvel, [expected_limit_rows(md, qpos[e]) for e in range(n)], inside


def limit_case(robot, n, seed=5):
    """The inputs of one joint-limit launch and the oracle's model (Newton at tolerance 1e-12).  Robot-robot contacts are off on both sides, so
    that the rows are friction loss, limits and floor contacts, the ones PLANE_STEP / ELLIPTIC_STEP were set for: legs folded to the ends of
    their ranges interpenetrate by centimetres, and those contacts miss the floor sets for reasons of their own.  Measured on the emulator with
    robot-robot contacts on: efc_J 3.4e-5 off on box pairs 2 - 5 cm deep (SELF_STEP allows 2e-4); two mirrored legs (hips at opposite ends of
    their range, equal thigh angles) make box_box's edge axis pass through both centres, t . n = 5e-17, and the sign of that normal is a coin
    toss in fp64 as well; b2's knee 0.2 rad past its lower limit puts the foot sphere's centre inside the thigh's cylinder, on its mid-plane,
    where the kernel's convex routine returns a depth of 0.7 - 4.8 cm for the oracle's 5.66 cm in about half of the draws - an open finding
    about cvx_pair_wave on a sphere swallowed by its partner, not about limit rows.
    The limit rows are assembled before any contact in every kernel variant."""
    from oracle.oracle import Oracle
    mmN = marshalled(robot, solver=1, iterations=100, tolerance=1e-12, self_collision=False)
    rng = np.random.default_rng(seed)
    qpos, qvel, rows, inside = limit_states(mmN.md, n, rng, hip_height(robot), Oracle(mmN))
    return dict(robot=robot, n=n, mmN=mmN, qpos=qpos, qvel=qvel.astype(np.float32), warm=rng.normal(0, 5, (n, 18)).astype(np.float32),
                ctrl=(rng.normal(0, 1, (n, 12)) * 40).astype(np.float32), friction=np.full(n, 0.8, np.float32), rows=rows, inside=inside)


def contact_rows(o, ncon, cone):
    """Rows of the first ncon contacts of the oracle's list (the kernel keeps a prefix of it)"""
    dims = o.get('contact_dim').astype(int)[:ncon] if ncon else np.zeros(0, int)
    return int(sum(1 if d == 1 else (d if cone else 2 * (d - 1)) for d in dims))


def scaled_qvel_check(tol, kern, o, e):
    """tols['qvel'] on dqvel / max(1, timestep * max|qacc of the oracle|): the velocity error is h * (acceleration error), and a joint 0.2 rad
    past its range makes |qacc| large (test_step_parity_on_benchmark_rollout_states divides the same way)"""
    s = max(1.0, TIMESTEP * np.abs(o.qacc).max())
    tol.check(np.asarray(kern['qvel']) / s, o.qvel / s, (e, 'qvel / max(1, h max|qacc|)'))


def hold_limit_case(case, kern, what):
    """Hold the records `kern` (one per env: emu_record / gpu_records, with efc_type and efc_force) of a launch over limit_case's inputs to the
    oracle: the whole step under PLANE_STEP / ELLIPTIC_STEP, the count and the exact +-1 Jacobian of the limit rows, and the coverage the
    case was built for."""
    from oracle.oracle import Oracle
    md, n, robot = case['mmN'].md, case['n'], case['robot']
    cone = md.cone == 1
    nfl = int((np.asarray(md.dof_frictionloss) > 0).sum())
    nlimited = len(limited_joints(md))
    o = Oracle(case['mmN'])
    tols = dict(sp.ELLIPTIC_STEP if cone else sp.PLANE_STEP)
    qvel_tol = tols.pop('qvel')
    tally = ParityTally(cone, 3e-7, shapes=Shapes(case['mmN']))
    with_rows = all_rows = with_contacts = in_contact = over_in_contact = over_full = left_out = 0
    seen_sides = set()
    for e in range(n):
        k, rows = kern[e], case['rows'][e]
        state = (case['qpos'][e], case['qvel'][e], case['warm'][e], np.zeros(18), 0.0, float(case['friction'][e]))
        cls = tally.step_env(e, o, state, case['ctrl'][e], k, tols, mass=md.total_mass)
        in_contact += o.ncon > 0
        if cls == 'budget':
            tally.check_budget_prefix(e, o, k)
            over_in_contact += 1
            over_full += len(rows) == nlimited
        if cls not in sp.COMPARED + ('budget',):
            left_out += 1
            continue
        # the limit rows sit between the friction-loss rows and the contacts: their count, kind and single Jacobian entry
        nefc, ncon = int(k['nefc'][0]), int(k['ncon'][0])
        nl = nefc - nfl - contact_rows(o, ncon, cone)
        assert nl == len(rows), (e, 'limit rows', nl, len(rows), nefc, nfl, ncon)
        assert not case['inside'][e] or nl == 0, (e, 'a joint 1e-5 inside its range gave a row')
        J = np.asarray(k['efc_J']).reshape(64, 18)[nfl:nfl + nl]
        want = np.zeros((nl, 18))
        for r, (j, sgn) in enumerate(rows):
            want[r, 6 + j] = sgn
        assert np.array_equal(J, want), (e, 'limit rows of efc_J', rows, [(int(np.argmax(np.abs(x))), float(x[np.argmax(np.abs(x))])) for x in J])
        assert (np.asarray(k['efc_type'])[nfl:nfl + nl] == 2).all(), (e, 'efc_type of the limit rows', np.asarray(k['efc_type'])[:nefc])
        if cls == 'budget':
            continue
        scaled_qvel_check(qvel_tol, k, o, e)   # (efc_aref of the limit rows: the first nefc rows, under the set)
        with_rows += nl > 0
        all_rows += nl == nlimited
        with_contacts += nl > 0 and o.ncon > 0
        seen_sides |= {s for _, s in rows}
    msg = tally.report(f'joint limits {what} {robot}')
    msg = (f'  {with_rows} compared envs with limit rows, {all_rows} with every limited joint\'s, {with_contacts} with contacts as well, sides {sorted(seen_sides)}, '
            f'{in_contact} in contact, {over_in_contact} over budget ({over_full} of them with all {nlimited} limit rows), {left_out} left out')
    tally_note(msg)
    assert not tally.mismatch, msg
    assert with_rows >= 0.6 * n and seen_sides == {1.0, -1.0} and all_rows >= 8 and with_contacts >= 10, msg
    assert left_out <= 0.1 * n and over_in_contact <= 0.25 * max(in_contact, 1), msg
    assert robot != 'go2' or over_full >= 3, msg   # 12 friction-loss + 12 limit rows in front of four condim-6 feet: held to the prefix rule
    return tally


# ------------------------------------------------------------------------------------------------ low ground friction

def friction_models(robot, solver):
    """(kernel model, oracle model at iteration cap 300, at cap 1200).  Newton: the product's settings against the oracle at tolerance 1e-12,
    which it cannot formally meet on pyramidal cones at low friction - its solutions at the two caps are compared instead; PGS: the same
    PGS_SWEEPS sweeps on both sides."""
    if solver == 'pgs':
        mm = marshalled(robot, solver=0, iterations=PGS_SWEEPS, tolerance=0.0)
        return mm, mm, mm
    return (marshalled(robot, solver=1, iterations=100, tolerance=1e-8, noise_floor=1e-5),
            marshalled(robot, solver=1, iterations=300, tolerance=1e-12), marshalled(robot, solver=1, iterations=1200, tolerance=1e-12))


def friction_states(md, n, rng, o, hip):
    """random_states at 0.6 - 1.4 hip heights with at most 8 % of the envs over the row budget, the tangential base velocity scaled up so
    that feet slide, kept when the oracle finds a contact; env j steps at FRICTIONS[j % len(FRICTIONS)].  Returns (qpos, qvel, friction)."""
    def draw(k):
        q, v = random_states(md, k, rng, z_range=(0.6 * hip, 1.4 * hip))
        v[:, 0:2] *= 4.0
        touching = []
        for e in range(k):   # (a state in flight has no row that friction enters)
            o.set_state(q[e], v[e], np.zeros(18), np.zeros(18), 0.0, 0.8)
            o.forward(np.zeros(12), stage=1)
            touching.append(o.ncon > 0)
        return q[touching], v[touching]
    qpos, qvel = budgeted_states(n, draw, o, md.cone == 1, max_over=0.08)
    return qpos, qvel, np.asarray([FRICTIONS[j % len(FRICTIONS)] for j in range(n)], np.float32)


def friction_case(robot, solver, n=N_FRICTION, seed=7):
    from oracle.oracle import Oracle
    mm, m300, m1200 = friction_models(robot, solver)
    rng = np.random.default_rng(seed)
    qpos, qvel, fric = friction_states(m300.md, n, rng, Oracle(m300), hip_height(robot))
    return dict(robot=robot, solver=solver, n=n, mm=mm, m300=m300, m1200=m1200, qpos=qpos, qvel=qvel.astype(np.float32),
                warm=rng.normal(0, 5, (n, 18)).astype(np.float32), ctrl=(rng.normal(0, 1, (n, 12)) * 40).astype(np.float32), friction=fric)


def friction_tols(md, solver):
    """The existing named set of the case, with qacc at below(2e-4)"""
    base = sp.TERRAIN_PGS_STEP if solver == 'pgs' else (sp.ELLIPTIC_STEP if md.cone == 1 else sp.PLANE_STEP)
    return {**base, 'qacc': below(2e-4)}


def has_floor(md, solver):
    """The pyramidal-cone Newton kernel: R of an edge row goes with mu^2, and the primal Hessian M + J^T D J leaves fp32's reach"""
    return solver == 'newton' and md.cone == 0


def hold_friction_case(case, kern, what, floor, tols=None):
    """Hold the records of a launch over friction_case's inputs to the oracle at cap 300: every env at a friction at or above `floor` (any
    friction where the case has no floor) under friction_tols, an env below it to finite values only.  An env counts only if the oracle's
    qacc at caps 300 and 1200 agree to 1e-9 max(1, |qacc|).  Returns {friction: [(qacc error / max(1, max|qacc|), kernel niter)]} over the
    compared envs in contact - the rows of tests/reports/low_friction_sweep.py."""
    from oracle.oracle import Oracle
    md, n, solver = case['m300'].md, case['n'], case['solver']
    cone = md.cone == 1
    o, o2 = Oracle(case['m300']), Oracle(case['m1200'])
    tols = friction_tols(md, solver) if tols is None else tols
    rows_only = sp.pick(tols, 'efc_J', 'efc_aref')
    tally = ParityTally(cone, 3e-7)
    by = {f: [] for f in FRICTIONS}
    unsettled = []
    for e in range(n):
        k, f = kern[e], float(case['friction'][e])
        state = (case['qpos'][e], case['qvel'][e], case['warm'][e], np.zeros(18), 0.0, f)
        for name in ('qacc', 'qvel', 'qpos'):
            assert np.isfinite(np.asarray(k[name])).all(), (e, f, name)
        held = not has_floor(md, solver) or FRICTIONS[e % len(FRICTIONS)] >= floor
        if solver == 'newton':
            o2.set_state(*state); o2.step(case['ctrl'][e].astype(np.float64))
            ref2 = o2.qacc
            o.set_state(*state); o.step(case['ctrl'][e].astype(np.float64))
            if not (np.abs(o.qacc - ref2) <= 1e-9 * np.maximum(1.0, np.abs(ref2))).all():
                unsettled.append((e, f, float(np.abs(o.qacc - ref2).max())))
                continue
        cls = tally.step_env(e, o, state, case['ctrl'][e], k, tols if held else rows_only, mass=md.total_mass)
        if cls in sp.COMPARED and o.ncon:
            by[FRICTIONS[e % len(FRICTIONS)]].append((float(np.abs(np.asarray(k['qacc']) - o.qacc).max() / max(1.0, np.abs(o.qacc).max())), int(k['niter'][0])))
    msg = tally.report(f'low friction {what} {case["robot"]} {solver}')
    for f in FRICTIONS:
        if by[f]:
            err = np.asarray([x[0] for x in by[f]])
            tally_note(f'  friction {f:g}: n {len(err)} p50 {np.median(err):.1e} p99 {np.percentile(err, 99):.1e} max {err.max():.1e} niter {sorted(x[1] for x in by[f])}')
    assert not tally.mismatch, msg
    assert not unsettled, (msg, 'the oracle at caps 300 and 1200 disagrees', unsettled)
    assert min(len(v) for v in by.values()) >= 6, (msg, {f: len(v) for f, v in by.items()})
    return by


# ------------------------------------------------------------------------------------------------ the two backends

NAMES = ['qacc', 'niter', 'nefc', 'ncon', 'efc_J', 'efc_R', 'efc_aref', 'efc_force', 'efc_type']


def emu_case_records(mm, case, contacts=False):
    """One emulated launch over a case's inputs.  contacts=True: with the contact row - an env whose contact POINTS alone are undecided is
    then compared too"""
    from helpers import emu_step
    from step_parity import emu_record
    n = case['n']
    st = emu_step(mm, case['ctrl'], case['qpos'].copy(), case['qvel'].copy(), warm=case['warm'].copy(), friction=case['friction'].copy(), debug_envs=n, rows=contacts)
    return [emu_record(st, e, contacts=contacts) for e in range(n)]


def gpu_case_records(case, solver, iterations, tolerance, contacts=False, **kw):
    """One GPU launch over a case's inputs: a QuadrupedEnv of case['n'] envs with the state written into its tensors"""
    import torch
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    from helpers import ALL_OBS
    from step_parity import gpu_records
    n = case['n']
    env = QuadrupedEnv(case['robot'], state_obs_names=tuple(ALL_OBS), num_envs=n, device='cuda:0', solver=solver, solver_iterations=iterations,
                       solver_tolerance=tolerance, seed=0, accessors=contacts, **kw)
    env._qpos.copy_(torch.as_tensor(case['qpos'])); env._qvel.copy_(torch.as_tensor(case['qvel'])); env._warm.copy_(torch.as_tensor(case['warm']))
    env._friction.copy_(torch.as_tensor(case['friction']))   # (the state tensors themselves: the sweep steps below QuadrupedEnv's floor on purpose)
    env.enable_debug(n)
    env.step(torch.as_tensor(case['ctrl']))
    kern = gpu_records(env, n, NAMES)
    env.close()
    return kern


def gpu_friction_records(case):
    return gpu_case_records(case, case['solver'], PGS_SWEEPS if case['solver'] == 'pgs' else 100, 0.0 if case['solver'] == 'pgs' else 1e-8)
