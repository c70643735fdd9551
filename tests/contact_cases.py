"""Case tables for the contact routines of csrc/gq_pairs.h (capsule_box, box_box) and csrc/gq_convex.h (cvx_pair_wave) with the fp64 oracle's
outputs and its classification of every case, and the checks that hold a backend's outputs to them.  One table, two backends (the precedent is
tests/camera_caster.py): the routines called directly under the host emulator (tests/test_kernel_emulated.py) and on the GPU through the probe
library (tests/test_gpu_device_probe.py).  The generators, asserts, tolerances and coverage counts are those of the emulated tests.
TEST INFRASTRUCTURE."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

PAIR_MARGIN = 0.001
PAIR_TOL = dict(dist=2e-6, pos=5e-6, nrm=2e-4)
CVX_MARGIN = 0.01
CVX_TOL = dict(dist=1e-6, angle_deg=0.1, pos=2e-5, capped_dist=1e-4)


@functools.lru_cache(None)
def pair_cases():
    """1500 random and resting configurations, capsule - box and box - box in turn.  Each case: kind ('capsule' | 'box'), args (the fp32 inputs, in
    the routine's argument order), no / oo (the oracle's contact count and its [4][7] rows dist, pos, normal), deep (the oracle sees more than
    0.02 m of overlap: decisions between nearly equal axes / deepest samples may differ, so the case is not compared)."""
    from scipy.spatial.transform import Rotation
    from test_oracle_invariants import _pair_lib, _np_ptr
    Lo = _pair_lib()
    rng = np.random.default_rng(12)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    cases = []
    for trial in range(1500):
        h = rng.uniform(0.02, 0.3, 3); R = Rotation.random(random_state=int(rng.integers(1 << 30))).as_matrix(); c = rng.uniform(-1, 1, 3)
        margin = PAIR_MARGIN
        if trial % 2 == 0:   # capsule - box
            r = rng.uniform(0.005, 0.05)
            if trial % 8 == 0:
                a = np.array([rng.uniform(-h[0], h[0]), rng.uniform(-h[1], h[1]), h[2] + r + rng.uniform(-0.002, 0.0005)])
                b = np.array([rng.uniform(-h[0], h[0]), rng.uniform(-h[1], h[1]), a[2] + rng.uniform(-2e-4, 2e-4)])
                p0, p1 = c + R @ a, c + R @ b
            else:
                p0 = c + R @ (rng.uniform(-1.3, 1.3, 3) * h); p1 = p0 + rng.normal(0, 0.1, 3)
            # fp32 inputs for both, so that the comparison is about the arithmetic only
            p0, p1, cc, Rc, hc = (f32(x).astype(np.float64) for x in (p0, p1, c, R, h))
            rr = float(np.float32(r))
            oo = np.zeros(28)
            Rc = np.ascontiguousarray(Rc)
            no = Lo.gqo_test_capsule_box(_np_ptr(p0), _np_ptr(p1), rr, _np_ptr(cc), _np_ptr(Rc), _np_ptr(hc), margin, _np_ptr(oo))
            cases.append(dict(trial=trial, kind='capsule', args=(f32(p0), f32(p1), rr, f32(cc), f32(Rc), f32(hc)), no=no, oo=oo))
        else:
            hb = rng.uniform(0.02, 0.3, 3)
            if trial % 6 == 1:
                hb[:2] = rng.uniform(0.2, 0.9, 2) * h[:2]
                Rb = R @ Rotation.from_euler('z', rng.uniform(-0.3, 0.3)).as_matrix()
                cb = c + R @ np.array([*(rng.uniform(-0.05, 0.05, 2) * h[:2]), h[2] + hb[2] + rng.uniform(-0.003, 0.0008)])
            else:
                Rb = Rotation.random(random_state=int(rng.integers(1 << 30))).as_matrix()
                cb = c + rng.normal(0, 1, 3) * (h + hb) * 0.8
            cc, Rc, hc, cb, Rb, hb = (f32(x).astype(np.float64) for x in (c, R, h, cb, Rb, hb))
            oo = np.zeros(28)
            Rc, Rb = np.ascontiguousarray(Rc), np.ascontiguousarray(Rb)
            no = Lo.gqo_test_box_box(_np_ptr(cc), _np_ptr(Rc), _np_ptr(hc), _np_ptr(cb), _np_ptr(Rb), _np_ptr(hb), margin, _np_ptr(oo))
            cases.append(dict(trial=trial, kind='box', args=(f32(cc), f32(Rc), f32(hc), f32(cb), f32(Rb), f32(hb)), no=no, oo=oo))
        cases[-1]['deep'] = bool(no and abs(oo[0::7][:no]).max() > 0.02)
    return cases


def check_pairs(cases, outputs, tol=PAIR_TOL):
    """outputs: per case (count, [28] rows) of the backend.  Same number of points, same order, distances / positions / normals to fp32 accuracy;
    returns the worst errors seen (dist, pos, nrm) with their trials."""
    ncap = nbox = multi = 0
    worst = dict(dist=(0.0, -1), pos=(0.0, -1), nrm=(0.0, -1))
    for cs, (ne, oe) in zip(cases, outputs):
        trial, no, oo = cs['trial'], cs['no'], cs['oo']
        if cs['kind'] == 'capsule':
            ncap += no > 0
        else:
            nbox += no > 0
        if cs['deep']:
            continue   # centimetres of overlap: decisions between nearly equal axes / deepest samples may differ; contacts are created at the margin
        assert no == ne, (trial, no, ne, oo[:7], oe[:7])
        multi += no > 1
        for q in range(no):
            for key, e in (('dist', abs(oo[7 * q] - oe[7 * q])), ('pos', np.abs(oe[7 * q + 1:7 * q + 4] - oo[7 * q + 1:7 * q + 4]).max()),
                           ('nrm', np.abs(oe[7 * q + 4:7 * q + 7] - oo[7 * q + 4:7 * q + 7]).max())):
                if e > worst[key][0]:
                    worst[key] = (float(e), trial)
            assert abs(oo[7 * q] - oe[7 * q]) < tol['dist'], (trial, q, oo[7 * q:7 * q + 7], oe[7 * q:7 * q + 7])
            np.testing.assert_allclose(oe[7 * q + 1:7 * q + 4], oo[7 * q + 1:7 * q + 4], atol=tol['pos'], err_msg=f'trial {trial} point {q} pos')
            np.testing.assert_allclose(oe[7 * q + 4:7 * q + 7], oo[7 * q + 4:7 * q + 7], atol=tol['nrm'], err_msg=f'trial {trial} point {q} normal')
    assert ncap > 100 and nbox > 100 and multi > 60, (ncap, nbox, multi)
    return worst


@functools.lru_cache(None)
def convex_cases(robot):
    """Random polytopes (robot None) or the robot's own mesh / cylinder clouds, against an analytic box and against each other, from 12 mm apart to
    30 mm deep, with and without an inflation radius.  Each case: the fp32 inputs (VA, RA, rA, VB | hB, RB, tB; A sits at the origin), the
    oracle's outputs (rc, dist, pos, nrm, eit) and its classification: at_margin (only such a pair may be seen by one side alone), capped (the
    shared iteration cap), determined (the support sets along the normal: not two faces, a face and an edge, parallel edges)."""
    from scipy.spatial.transform import Rotation as Rot
    from helpers import marshalled
    from test_oracle_invariants import _box_corners, _support, convex_oracle
    rng = np.random.default_rng(0)
    md = marshalled(robot, solver=1).md if robot else None
    clouds = [c for c in range(len(md.cloud_vertnum)) if md.cloud_vertnum[c] >= 8] if md else None
    cloud = lambda c: md.vert_pos[md.cloud_vertadr[c]:md.cloud_vertadr[c] + md.cloud_vertnum[c]]
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)   # both sides see the same (fp32) inputs
    cases = []
    for trial in range(240 if robot is None else 120):
        if md is None:
            VA = rng.normal(size=(rng.integers(4, 60), 3)) * rng.uniform(0.02, 0.15, size=3)
            VB, hB = (None, rng.uniform(0.05, 0.5, size=3)) if trial % 2 == 0 else (rng.normal(size=(rng.integers(4, 60), 3)) * rng.uniform(0.02, 0.15, size=3), None)
        else:
            VA = cloud(clouds[trial % len(clouds)])
            VB, hB = (None, rng.uniform(0.1, 0.6, size=3)) if trial % 2 == 0 else (cloud(clouds[int(rng.integers(len(clouds)))]), None)
        VA = f32(VA); VB = None if VB is None else f32(VB); hB = None if hB is None else f32(hB)
        RA, RB = (f32(Rot.random(random_state=int(rng.integers(1 << 30))).as_matrix()) for _ in range(2))
        WA, WB0 = VA @ RA.T, (_box_corners(hB) if VB is None else VB) @ RB.T
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        want = rng.uniform(-0.03, 0.012)
        tB = u * (_support(WA, u) + _support(WB0, -u) + 0.05)
        rc0, d0, _, n0, _, _ = convex_oracle(VA, None, RA, np.zeros(3), 0.0, VB, hB, RB, tB, 0.0, 10.0)
        tB = f32(tB - (d0 - want) * n0)
        rA = float(np.float32(rng.choice([0.0, 0.01])))
        rc, dist, pos, nrm, git, eit = convex_oracle(VA, None, RA, np.zeros(3), rA, VB, hB, RB, tB, 0.0, CVX_MARGIN)
        WB = WB0 + tB
        da = int((WA @ nrm > (WA @ nrm).max() - 1e-6).sum()); db = int((WB @ -nrm > (WB @ -nrm).max() - 1e-6).sum())
        cases.append(dict(trial=trial, VA=VA, RA=RA, rA=rA, VB=VB, hB=hB, RB=RB, tB=tB, rc=rc, dist=dist, pos=pos, nrm=nrm, eit=eit,
                          at_margin=bool(rc and abs(dist - CVX_MARGIN) < 2e-6), capped=eit >= 24, da=da, db=db,
                          determined=min(da, db) == 1 or (da == 2 and db == 2)))
    return cases


def check_convex(cases, outputs, tol=CVX_TOL):
    """outputs: per case (rc, dist, pos [3], nrm [3]) of the backend.  Same contacts; distance, normal and - where the oracle says it is determined -
    point within tol, wherever the polytope did not run into the iteration cap both sides share; returns the worst errors with their trials."""
    n = capped = deep = 0
    worst = dict(dist=(0.0, -1), angle_deg=(0.0, -1), pos=(0.0, -1))
    for cs, (rk, dk, pk, nk) in zip(cases, outputs):
        trial, rc, dist, pos, nrm = cs['trial'], cs['rc'], cs['dist'], cs['pos'], cs['nrm']
        if rc != rk:
            assert cs['at_margin'], (trial, rc, rk, dist)   # only a pair AT the margin may be seen by one side alone
            continue
        if not rc:
            continue
        n += 1; deep += dist < -1e-3
        if cs['capped']:   # the shared iteration cap: both sides report the state of an unfinished iteration, which round-off steers
            capped += 1
            assert abs(dk - dist) < tol['capped_dist']
            continue
        ang = np.degrees(np.arccos(np.clip(nk @ nrm, -1, 1)))
        for key, e in (('dist', abs(dk - dist)), ('angle_deg', ang)) + ((('pos', np.linalg.norm(pk - pos)),) if cs['determined'] else ()):
            if e > worst[key][0]:
                worst[key] = (float(e), trial)
        assert abs(dk - dist) < tol['dist'], (trial, dk, dist)
        assert ang < tol['angle_deg'], (trial, nk, nrm)
        # the point: compared where it is determined (support sets along the normal: not two faces, a face and an edge, parallel edges)
        if cs['determined']:
            assert np.linalg.norm(pk - pos) < tol['pos'], (trial, pk, pos, cs['da'], cs['db'])
    assert n >= 80 and deep >= 30 and capped <= 0.05 * n, (n, deep, capped)
    return worst


# ----------------------------------------------------------------------------------------------------------------- backends
def emu_pairs(cases):
    from helpers import emu_lib
    Le = emu_lib()
    P = C.c_void_p
    Le.emu_capsule_box.argtypes = [P, P, C.c_float, P, P, P, C.c_float, P]
    Le.emu_box_box.argtypes = [P, P, P, P, P, P, C.c_float, P]
    out = []
    for cs in cases:
        oe = np.zeros(28, np.float32)
        a = [x if isinstance(x, float) else x.ctypes.data for x in cs['args']]
        ne = (Le.emu_capsule_box if cs['kind'] == 'capsule' else Le.emu_box_box)(*a, PAIR_MARGIN, oe.ctypes.data)
        out.append((ne, oe))
    return out


def emu_convex(cases):
    from helpers import emu_lib
    Le = emu_lib()
    P = C.c_void_p
    Le.emu_convex.argtypes = [P, C.c_int, P, P, P, C.c_float] * 2 + [C.c_float, P]
    res = []
    for cs in cases:
        arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.float32) for x in (cs['VA'], None, cs['RA'], np.zeros(3), cs['VB'], cs['hB'], cs['RB'], cs['tB'])]
        p = [None if a is None else a.ctypes.data_as(P) for a in arrs]
        out = np.zeros(7, np.float32)
        rc = Le.emu_convex(p[0], 0 if arrs[0] is None else len(arrs[0]), p[1], p[2], p[3], cs['rA'], p[4], 0 if arrs[4] is None else len(arrs[4]), p[5], p[6], p[7], 0.0,
                           CVX_MARGIN, out.ctypes.data_as(P))
        res.append((rc, float(out[0]), out[1:4].astype(float), out[4:7].astype(float)))
    return res


def probe_pairs(be, cases):
    """capsule_box and box_box through the probe library: one case per lane, every case of a kind in one launch"""
    outs = [None] * len(cases)
    for kind, fn in (('capsule', 'capsule_box'), ('box', 'box_box')):
        idx = [i for i, cs in enumerate(cases) if cs['kind'] == kind]
        rows = np.stack([np.concatenate([np.atleast_1d(np.asarray(x, np.float32)).ravel() for x in cases[i]['args']]) for i in idx]).astype(np.float32)
        from device_cases import Out
        cnt, out = be.run(fn, rows, PAIR_MARGIN, len(idx), Out((len(idx),), np.int32), Out((len(idx), 28), np.float32))
        for k, i in enumerate(idx):
            outs[i] = (int(cnt[k]), out[k])
    return outs


def probe_convex(be, cases):
    """cvx_pair_wave through the probe library: one pair per block, the clouds concatenated into one SoA array with a per-case adr / num, the two
    shape descriptors in CvxShape's field order (as the emulator's emu_convex fills them)"""
    from device_cases import Out
    V, desc = [], np.zeros((len(cases), 2, 20), np.float32)
    di = desc.view(np.int32)
    adr = 0
    for k, cs in enumerate(cases):
        for s, (Vs, hs, R, t, r) in enumerate(((cs['VA'], None, cs['RA'], np.zeros(3), cs['rA']), (cs['VB'], cs['hB'], cs['RB'], cs['tB'], 0.0))):
            num = 0 if Vs is None else len(Vs)
            di[k, s, 0], di[k, s, 1], di[k, s, 2], di[k, s, 3] = (0 if Vs is not None else 1), adr, num, -1
            desc[k, s, 4:13] = np.asarray(R, np.float32).ravel(); desc[k, s, 13:16] = t
            desc[k, s, 16:19] = 0.0 if hs is None else hs; desc[k, s, 19] = r
            if num:
                V.append(np.asarray(Vs, np.float32)); adr += num
    V = np.concatenate(V + [np.zeros((1, 3), np.float32)])
    assert ((di[:, :, 1] + di[:, :, 2]) <= len(V)).all() and (di[:, :, 1] >= 0).all()   # every cloud lies inside the vertex arrays
    vx, vy, vz = (np.ascontiguousarray(V[:, a]) for a in range(3))
    hit, out = be.run('convex', vx, vy, vz, desc, CVX_MARGIN, len(cases), Out((len(cases),), np.int32), Out((len(cases), 7), np.float32))
    return [(int(hit[k]), float(out[k, 0]), out[k, 1:4].astype(float), out[k, 4:7].astype(float)) for k in range(len(cases))]
