"""How well "the pair touched a step ago" predicts where the convex narrow phase's work falls (the early publication of DESIGN 7 item 0):
the state distribution of tools/convex_census.py (N envs of the CPU oracle, 50 N(0,1) N.m random torques, re-spawn on termination), every
convex self pair that passes the bounding spheres run once more through the oracle's routine (gqo_test_convex) on the poses the step
collided at.  Two predictors, both remembered per pair across a re-spawn as the kernel's axis cache would:
  narrow  the pair yielded a contact one step earlier;
  wide    the pair's gap one step earlier was below its margin + the model's largest pair margin (the kernel's self_margin).
Per predictor: the share of this step's convex contact work it covers - weighted by EPA iterations, by support queries, and counted
over the contacts of >= 12 EPA iterations alone - and the publications per env-step it costs (useless ones apart).
TEST / MEASUREMENT AID (uses the oracle)."""
from __future__ import annotations

import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / 'tests'))
from helpers import marshalled, random_states   # noqa: E402
from oracle.oracle import Oracle, lib           # noqa: E402


def convex_pairs(mm):
    """the self pairs the oracle hands to its convex routine: not capsule / sphere against each other, no box against a primitive"""
    md = mm.md
    out = []
    for g1, g2 in np.asarray(mm.self_pairs).reshape(-1, 2):
        t = [int(md.geom_type[g]) for g in (g1, g2)]
        caps = [x in (2, 3) for x in t]
        box = [x == 6 for x in t]
        if (caps[0] and caps[1]) or (box[0] and (caps[1] or box[1])) or (box[1] and caps[0]):
            continue
        out.append((int(g1), int(g2)))
    return out


def main(robot='mini_cheetah', n_envs=48, n_steps=250):
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-8)
    md = mm.md
    L = lib()
    D = C.POINTER(C.c_double)
    L.gqo_test_convex.argtypes = [D, C.c_int, D, D, D, C.c_double, D, C.c_int, D, D, D, C.c_double, C.c_double, D]
    pairs = convex_pairs(mm)
    g1s, g2s = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    margin = np.maximum(np.asarray(md.geom_margin)[g1s], np.asarray(md.geom_margin)[g2s])
    self_margin = float(max(max(md.geom_margin[a], md.geom_margin[b]) for a, b in np.asarray(mm.self_pairs).reshape(-1, 2)))
    reach = np.asarray(md.geom_rbound)[g1s] + np.asarray(md.geom_rbound)[g2s] + margin
    vert = np.ascontiguousarray(md.vert_pos, dtype=np.float64).reshape(-1, 3)
    cl = np.asarray(md.geom_cloudid)

    def run(o_xpos, o_xmat, k, marg):
        a, b = g1s[k], g2s[k]
        out = np.zeros(9)
        args = []
        for g in (a, b):
            c = int(cl[g]); V = vert[int(md.cloud_vertadr[c]):int(md.cloud_vertadr[c]) + int(md.cloud_vertnum[c])]
            args += [V.ctypes.data_as(D), int(md.cloud_vertnum[c]), None, np.ascontiguousarray(o_xmat[g]).ctypes.data_as(D),
                     np.ascontiguousarray(o_xpos[g]).ctypes.data_as(D), float(md.cloud_radius[c])]
        rc = L.gqo_test_convex(*args, float(marg), out.ctypes.data_as(D))
        return rc, out[0], int(out[7]), int(out[8])

    rng = np.random.default_rng(0)
    hip = float(mm.desc.key_qpos[2])
    names = ('narrow', 'wide')
    tot = dict(epa=0, queries=0, deep=0, contacts=0, steps=0, term=0, mismatch=0)
    cov = {n: dict(epa=0, queries=0, deep=0, contacts=0, pubs=0, useless=0) for n in names}
    for e in range(n_envs):
        o = Oracle(mm)
        q, v = random_states(md, 1, rng, z_range=(1.0 * hip, 1.2 * hip))
        o.set_state(q[0], 0 * v[0], np.zeros(18), np.zeros(18))
        pred = {n: np.zeros(len(pairs), dtype=bool) for n in names}
        for _ in range(n_steps):
            o.step(50.0 * rng.normal(size=12))
            xpos, xmat = o.geom_xpos, o.geom_xmat
            n = int(o.ncon)
            cg1, cg2 = o.get('contact_geom1')[:n].astype(int), o.get('contact_geom')[:n].astype(int)
            truth = {(a, b) for a, b in zip(cg1, cg2) if a >= 0}
            near = np.nonzero(np.linalg.norm(xpos[g2s] - xpos[g1s], axis=1) <= reach + self_margin)[0]
            now = {nm: np.zeros(len(pairs), dtype=bool) for nm in names}
            for k in near:
                rc, dist, gjk, epa = run(xpos, xmat, k, margin[k] + self_margin)
                hit = bool(rc) and dist < margin[k]
                now['narrow'][k] = hit
                now['wide'][k] = bool(rc)
                if hit != ((pairs[k][0], pairs[k][1]) in truth) and n < 12:
                    tot['mismatch'] += 1
                if hit:
                    w = dict(epa=epa, queries=1 + gjk + epa, deep=int(epa >= 12), contacts=1)
                    for key, val in w.items():
                        tot[key] += val
                        for nm in names:
                            if pred[nm][k]:
                                cov[nm][key] += val
            for nm in names:
                cov[nm]['pubs'] += int(pred[nm].sum())
                cov[nm]['useless'] += int((pred[nm] & ~now['narrow']).sum())
                # a pair out of reach keeps no word of its own: the kernel's cull rejects it before the routine, its sentinel stays
                # until the routine next runs on it - one useless publication per step until then, counted above
                keep = pred[nm].copy(); keep[near] = False
                pred[nm] = now[nm] | keep
            tot['steps'] += 1
            bodies = md.geom_bodyid[cg2]
            if np.any((cg1 < 0) & ((bodies < 2) | ((bodies - 2) % 3 != 2))):
                tot['term'] += 1
                q, v = random_states(md, 1, rng, z_range=(1.0 * hip, 1.2 * hip))
                o.set_state(q[0], 0 * v[0], np.zeros(18), np.zeros(18))
    s = tot['steps']
    print(f"{robot}: {s} env-steps, {tot['term']} terminations, {len(pairs)} convex self pairs, convex contacts / step {tot['contacts'] / s:.3f}, "
          f"EPA its / contact {tot['epa'] / max(tot['contacts'], 1):.2f}, contacts of >= 12 EPA its {tot['deep']}, "
          f"pairs whose replay disagrees with the step's list {tot['mismatch']}")
    for nm in names:
        c = cov[nm]
        print(f"  {nm:6s}: covers {100 * c['epa'] / max(tot['epa'], 1):.1f} % of the EPA iterations, {100 * c['queries'] / max(tot['queries'], 1):.1f} % of the contacts' support queries, "
              f"{100 * c['deep'] / max(tot['deep'], 1):.1f} % of the >= 12-iteration contacts, {100 * c['contacts'] / max(tot['contacts'], 1):.1f} % of the contacts; "
              f"early publications / env-step {c['pubs'] / s:.3f} ({c['useless'] / s:.3f} of them for a pair that no longer touches)")


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'mini_cheetah', n_envs=int(sys.argv[2]) if len(sys.argv) > 2 else 48,
         n_steps=int(sys.argv[3]) if len(sys.argv) > 3 else 250)
