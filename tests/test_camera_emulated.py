"""The camera ray caster (csrc/gq_camera.h) under the host SIMT emulator: whole images of every robot of the registry against the fp64
caster (camera_caster.py: the cases, the acceptance rule and the coverage conditions the GPU tests share), the height-field walk on a small
synthetic grid against brute-force Moeller-Trumbore, and each ray primitive at its own branches against an fp64 evaluation of the same
geometry.  No GPU: the kernel text is compiled unmodified by g++ (tests/simt_emu)."""
import numpy as np
import pytest

import camera_caster as cc
from helpers import emu_camera, marshalled


def _emu_case(case):
    qpos, cam, _, _, _ = cc.case_reference(case)
    sc = cc._scene(case.robot, case.scene)
    mm = marshalled(case.robot, solver=1, boxes=sc.get('boxes'), hfield=sc.get('hfield'))
    return emu_camera(mm, qpos, cam['body'], cam['pos'], cam['quat'], cam['fovy'], case.W, case.H, cc.ZNEAR, cc.ZFAR, case.flags | (4 if cam['track'] else 0))


def test_cases_cover_what_they_claim():
    cc.check_coverage()


@pytest.mark.parametrize('case', cc.CASES, ids=repr)
def test_emulated_camera_matches_numpy_caster(case):
    out = _emu_case(case)
    worst, nbad = cc.check_case(case, out['depth'], out['seg'], out['xpos'], out['xmat'])
    print(f'{case}: worst depth error {worst:.3f} of the tolerance, {nbad} ids differ')
    if case.scene == 'random_boxes':   # the second half of the box walk: asserted on the reference (check_coverage), then on the result
        assert (cc.box_ids_seen(case, out['seg']) >= 64).any()
    if case.flags == 1:
        assert (out['seg'] < cc._model(case.robot)[0].ngeom).all()
    if case.flags == 2:
        assert not ((out['seg'] >= 0) & (out['seg'] < cc._model(case.robot)[0].ngeom)).any()


def test_go1_last_slot_is_drawn():
    g, _ = cc.last_link_geom('go1')
    seen = 0
    for case in cc.CASES:
        if case.robot == 'go1':
            ref = np.stack([r[3] for r in cc.case_reference(case)[4]]).reshape(-1)
            got = _emu_case(case)['seg'].reshape(-1)
            assert ((got == g) == (ref == g)).mean() > 0.995
            seen += int(((got == g) & (ref == g)).sum())
    assert seen > 0


# ---- b. the height-field walk on a small synthetic grid
NR, NC, SX, SY = 9, 7, 0.75, 1.0   # 0.25 m cells: every grid line is exact in binary, so border and vertex rays meet the DDA's ties exactly


def _grid():
    rng = np.random.default_rng(5)
    H = rng.uniform(0.0, 0.3, (NR, NC)).astype(np.float32)
    xs, ys = np.linspace(-SX, SX, NC), np.linspace(-SY, SY, NR)
    P = np.stack([np.tile(xs, (NR, 1)), np.tile(ys[:, None], (1, NC)), H.astype(np.float64)], -1)
    tris, ids, verts = [], [], []
    for r in range(NR - 1):
        for c in range(NC - 1):
            tris.append([P[r, c], P[r, c + 1], P[r + 1, c]]); ids.append(2 * (r * NC + c)); verts.append({(r, c), (r, c + 1), (r + 1, c)})
            tris.append([P[r + 1, c + 1], P[r + 1, c], P[r, c + 1]]); ids.append(2 * (r * NC + c) + 1); verts.append({(r + 1, c + 1), (r + 1, c), (r, c + 1)})
    return H, P, np.asarray(tris), np.asarray(ids), dict(zip(ids, verts))


def _brute(tris, o, d, tmin):
    """first Moeller-Trumbore hit >= tmin over all triangles, fp64, with the kernel's 1e-9 barycentric slack: (t or -1, index)"""
    a, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    pv = np.cross(d, e2); det = (e1 * pv).sum(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        inv = 1.0 / det; tv = o - a; u = (tv * pv).sum(1) * inv; qv = np.cross(tv, e1); v = (qv @ d) * inv; t = (e2 * qv).sum(1) * inv
    ok = (np.abs(det) >= 1e-14) & (u >= -1e-9) & (u <= 1 + 1e-9) & (v >= -1e-9) & (u + v <= 1 + 1e-9) & (t >= 0) & (t >= tmin)
    if not ok.any():
        return -1.0, -1
    k = int(np.argmin(np.where(ok, t, np.inf)))
    return float(t[k]), k


def _hfield_rays():
    rng = np.random.default_rng(6)
    H, P, _, _, _ = _grid()
    fam = {}
    n = 300
    inside = lambda m: np.stack([rng.uniform(-SX + 0.01, SX - 0.01, m), rng.uniform(-SY + 0.01, SY - 0.01, m)], 1)
    aim = lambda o, m: np.c_[inside(m), rng.uniform(0.0, 0.3, m)] - o
    o = np.c_[inside(n), rng.uniform(0.5, 1.0, n)]
    fam['from above'] = (o, np.c_[rng.uniform(-1, 1, (n, 2)), -rng.uniform(0.2, 1.0, n)])
    o = np.c_[rng.choice([-2.0, 2.0], n), rng.uniform(-SY, SY, n), rng.uniform(0.05, 0.6, n)]
    fam['outside in x'] = (o, aim(o, n))
    o = np.c_[rng.uniform(-SX, SX, n), rng.choice([-2.5, 2.5], n), rng.uniform(0.05, 0.6, n)]
    fam['outside in y'] = (o, aim(o, n))
    o = np.c_[rng.uniform(-2, 2, (n, 2)), np.full(n, 2.0)]
    fam['above zmax'] = (o, aim(o, n))
    o = np.c_[inside(n), rng.uniform(0.31, 0.8, n)]
    fam['d[0] = 0'] = (o, np.c_[np.zeros(n), rng.choice([-1.0, 1.0], n), -rng.uniform(0.1, 1, n)])
    fam['d[1] = 0'] = (o, np.c_[rng.choice([-1.0, 1.0], n), np.zeros(n), -rng.uniform(0.1, 1, n)])
    fam['straight down'] = (o, np.tile([0.0, 0.0, -1.0], (n, 1)))
    gx, gy = -SX + 0.25 * rng.integers(1, NC - 1, n), -SY + 0.25 * rng.integers(1, NR - 1, n)
    fam['along a border in y'] = (np.c_[gx, rng.uniform(-SY, SY, n), np.full(n, 0.6)], np.c_[np.zeros(n), rng.choice([-1.0, 1.0], n), -rng.uniform(0.1, 0.6, n)])
    fam['along a border in x'] = (np.c_[rng.uniform(-SX, SX, n), gy, np.full(n, 0.6)], np.c_[rng.choice([-1.0, 1.0], n), np.zeros(n), -rng.uniform(0.1, 0.6, n)])
    s = rng.choice([-1.0, 1.0], (n, 2))
    fam['cell diagonals'] = (np.c_[gx, gy, np.full(n, 0.5)], np.c_[s, -rng.uniform(0.05, 0.5, n)])   # from a vertex along (+-1, +-1): tx == ty at every step
    r, c = rng.integers(1, NR - 1, n), rng.integers(1, NC - 1, n)
    o = np.c_[inside(n), rng.uniform(0.5, 1.0, n)]
    fam['through a vertex'] = (o, P[r, c] - o)
    o = np.c_[inside(n), rng.uniform(0.2, 0.29, n)]
    fam['grazing out of the field'] = (o, np.c_[rng.uniform(-1, 1, (n, 2)), rng.uniform(0.0, 0.1, n)])
    o = np.c_[np.full(n, -2.0), rng.uniform(-SY, SY, n), rng.uniform(0.05, 0.25, n)]
    fam['low and level'] = (o, np.c_[np.ones(n), rng.uniform(-0.2, 0.2, n), rng.uniform(-0.02, 0.02, n)])
    return fam


def test_hfield_walk_matches_brute_force():
    from helpers import emu_ray_hfield
    H, _, tris, ids, verts = _grid()
    nmiss = nsecond = 0
    for name, (o, d) in _hfield_rays().items():
        tmin = np.zeros(len(o))
        ref = [_brute(tris, o[i], d[i], 0.0) for i in range(len(o))]
        if name in ('low and level', 'from above', 'outside in x'):   # again with tmin beyond the first crossing: the next one is returned
            first = np.array([r[0] for r in ref])
            keep = first >= 0
            o, d, tmin = np.r_[o, o[keep]], np.r_[d, d[keep]], np.r_[tmin, first[keep] + 1e-3]
            ref += [_brute(tris, o[i], d[i], tmin[i]) for i in range(len(first), len(o))]
            nsecond += sum(1 for r in ref[len(first):] if r[0] >= 0)
        t, tri = emu_ray_hfield(H, SX, SY, o, d, tmin)
        hits = 0
        for i, (tr, k) in enumerate(ref):
            if tr < 0:
                assert t[i] == -1.0, (name, i, t[i], o[i], d[i])
                nmiss += 1
                continue
            hits += 1
            assert t[i] >= tmin[i] and abs(t[i] - tr) <= 1e-9 * (1 + tr), (name, i, t[i], tr, o[i], d[i])
            # the same triangle or one that shares a grid vertex with it: at an edge or a vertex both are hit within the barycentric slack
            assert verts[int(tri[i])] & verts[int(ids[k])], (name, i, int(tri[i]), int(ids[k]))
        assert hits >= 30 or name == 'grazing out of the field', (name, hits)   # no family's value comparison is an empty one
        print(f'{name}: {len(ref)} rays, {hits} hits')
    assert nmiss >= 100 and nsecond >= 100, (nmiss, nsecond)


# ---- c. the primitives at their own branches.  The fp64 side takes the same fp32-rounded rays and sizes and finds the entry into the convex
# solid directly: the solid is {lo <= t <= hi} (the slab along the axis) cut by {f(t) <= 0}, f a quadratic; the entry is the first of lo and
# f's roots after which the ray is inside.  No case split on the sign of a, the discriminant or a generator, so it does not share the
# kernel's branches.
TOL = lambda t: 1e-4 * np.abs(t) + 1e-5   # the project's depth tolerance


def _entry(lo, hi, qa, qb, qc):
    """first t in [lo, hi] from which a t^2 + 2 b t + c <= 0 holds: (t, on_quadric) or None"""
    f = lambda t: (qa * t + 2 * qb) * t + qc
    cand = [(lo, False)]
    if abs(qa) > 1e-300:
        disc = qb * qb - qa * qc
        if disc >= 0:
            cand += [((-qb - np.sqrt(disc)) / qa, True), ((-qb + np.sqrt(disc)) / qa, True)]
    elif abs(qb) > 1e-300:
        cand.append((-0.5 * qc / qb, True))
    cand = sorted(x for x in cand if lo <= x[0] <= hi)
    for i, (t, on) in enumerate(cand):
        nxt = cand[i + 1][0] if i + 1 < len(cand) else hi
        if nxt > t and f(0.5 * (t + nxt)) <= 0:
            return t, on
    return None


def _slab64(oz, dz, z0, z1):
    if dz == 0:
        return (-1e30, 1e30) if z0 <= oz <= z1 else None
    a, b = (z0 - oz) / dz, (z1 - oz) / dz
    return min(a, b), max(a, b)


def _ref_quadric(kind, o, d, par):
    """fp64 entry (t, part) or None of one ray; sphere / cylinder / cone.  part as the kernel's: cylinder 0 side 1 cap, cone 0 side 1 base"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    if kind == 'sphere':
        r = par[0]
        e = _entry(-1e30, 1e30, d @ d, o @ d, o @ o - r * r)
        return None if e is None else (e[0], 0)
    if kind == 'cylinder':
        r, h = par
        sl = _slab64(o[2], d[2], -h, h)
        e = None if sl is None else _entry(sl[0], sl[1], d[0] ** 2 + d[1] ** 2, o[0] * d[0] + o[1] * d[1], o[0] ** 2 + o[1] ** 2 - r * r)
        return None if e is None else (e[0], 0 if e[1] else 1)
    rb, zb, zt = par
    sl = _slab64(o[2], d[2], zb, zt)
    k2, hz = (rb / (zt - zb)) ** 2, zt - o[2]
    e = None if sl is None else _entry(sl[0], sl[1], d[0] ** 2 + d[1] ** 2 - k2 * d[2] ** 2, o[0] * d[0] + o[1] * d[1] + k2 * hz * d[2], o[0] ** 2 + o[1] ** 2 - k2 * hz * hz)
    return None if e is None else (e[0], 0 if e[1] else 1)


def _ref_capsule(o, d, par):
    """nearest positive entry of the cylinder and the two cap spheres; origin inside: None.  part 0 cylinder, 1 cap at +h, 2 cap at -h"""
    r, h = par
    o = np.asarray(o, np.float64)
    zc = min(max(o[2], -h), h)
    if o[0] ** 2 + o[1] ** 2 + (o[2] - zc) ** 2 <= r * r:
        return None
    c = [_ref_quadric('cylinder', o, d, (r, h)), _ref_quadric('sphere', o - [0, 0, h], d, (r,)), _ref_quadric('sphere', o + [0, 0, h], d, (r,))]
    c = [(x[0], k) for k, x in enumerate(c) if x is not None and x[0] > 0]
    return min(c) if c else None


def _ref(kind, o, d, par, scale=1.0):
    par = tuple(np.float64(np.float32(p)) for p in par)
    if kind == 'capsule':
        return _ref_capsule(o, d, (par[0] * scale, par[1]))
    if kind == 'cone':
        return _ref_quadric(kind, o, d, (par[0] * scale, par[1], par[2]))
    return _ref_quadric(kind, o, d, (par[0] * scale,) + ((par[1] * scale,) if kind == 'cylinder' else ()))


def _random_rays(rng, n, reach):
    """rays from around the shape towards it (and some past it), fp32"""
    o = rng.normal(size=(n, 3)); o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(1.5, 4.0, (n, 1)) * reach
    d = rng.uniform(-1.1, 1.1, (n, 3)) * reach - o
    return o.astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)


def _compare(kind, o, d, par, max_grazing=0.01, need_parts=()):
    """kernel against fp64 on the rays; returns the share of grazing rays left out.  A ray is grazing if the fp64 verdict (hit or miss, or
    the part) changes when the radius / half size is scaled by 1 +- 1e-5 (the depth atol); those are left out of the verdict comparison."""
    from helpers import emu_cam_prim
    t, part = emu_cam_prim(kind, o, d, par)
    graze = 0
    seen = set()
    for i in range(len(o)):
        r0, rm, rp = (_ref(kind, o[i], d[i], par, s) for s in (1.0, 1 - 1e-5, 1 + 1e-5))
        key = lambda r: None if r is None else r[1]
        hitk = t[i] != -1.0
        if (r0 is None) != (rm is None) or (r0 is None) != (rp is None) or key(r0) != key(rm) or key(r0) != key(rp):
            graze += 1
            continue
        if r0 is None:
            assert t[i] == -1.0, (kind, i, t[i], o[i], d[i])
            continue
        if kind == 'sphere' and r0[0] < 0 and (np.float64(o[i]) @ np.float64(o[i])) <= np.float64(np.float32(par[0])) ** 2:
            assert t[i] == -1.0, (kind, 'origin inside', i)
            continue
        assert hitk, (kind, i, r0, o[i], d[i])
        assert abs(t[i] - r0[0]) <= TOL(r0[0]), (kind, i, t[i], r0, o[i], d[i])
        assert (t[i] < 0) == (r0[0] < 0), (kind, 'sign of the entry', i, t[i], r0[0])
        if kind != 'sphere':
            # the part where the runner-up surface is farther than the depth tolerance: scaling by 1 +- 1e-5 did not change it
            assert int(part[i]) == r0[1], (kind, 'part', i, int(part[i]), r0, o[i], d[i])
            seen.add(r0[1])
    assert set(need_parts) <= seen, (kind, seen)
    share = graze / len(o)
    assert share <= max_grazing, (kind, share)
    return share


PRIMS = [('sphere', (0.07,), ()), ('cylinder', (0.058, 0.125), (0, 1)), ('capsule', (0.02, 0.1), (0, 1, 2)), ('cone', (0.05, 0.1, 0.25), (0, 1))]


@pytest.mark.parametrize('kind,par,parts', PRIMS, ids=[p[0] for p in PRIMS])
def test_primitive_random_rays(kind, par, parts):
    o, d = _random_rays(np.random.default_rng(11), 3000, max(par))
    share = _compare(kind, o, d, par, need_parts=parts)
    print(f'{kind}: {100 * share:.2f} % grazing rays left out')


@pytest.mark.parametrize('kind,par,parts', PRIMS, ids=[p[0] for p in PRIMS])
def test_primitive_constructed_rays(kind, par, parts):
    from helpers import emu_cam_prim
    rng = np.random.default_rng(12)
    n = 200
    r = par[0]
    zmid = 0.5 * (par[1] + par[2]) if kind == 'cone' else 0.0
    top = par[2] if kind == 'cone' else (par[1] + (r if kind == 'capsule' else 0.0) if kind != 'sphere' else r)
    # parallel to the axis (a == 0 exactly), inside and outside the radius, from above and from below
    xy = rng.uniform(-2 * r, 2 * r, (n, 2))
    o = np.c_[xy, rng.choice([-1.0, 1.0], n) * 3 * top].astype(np.float32)
    d = np.c_[np.zeros((n, 2)), -np.sign(o[:, 2])].astype(np.float32)
    _compare(kind, o, d, par)
    # perpendicular to the axis (d.z == 0 exactly), at heights inside and outside the shape
    ang = rng.uniform(0, 2 * np.pi, n)
    o = np.c_[3 * r * np.cos(ang), 3 * r * np.sin(ang), zmid + rng.uniform(-1.5, 1.5, n) * (top - zmid)].astype(np.float32)
    tgt = rng.uniform(-1.2 * r, 1.2 * r, (n, 2))
    d = np.c_[tgt - o[:, :2], np.zeros(n)].astype(np.float32)
    _compare(kind, o, d, par)
    # the origin inside: no front face is seen.  The sphere and the capsule return -1; the cylinder and the cone return their (negative) entry
    # behind the origin, which the caller's znear test rejects
    o = np.c_[rng.uniform(-0.3, 0.3, (n, 2)) * r * (0.3 if kind == 'cone' else 1.0), zmid + rng.uniform(-0.3, 0.3, n) * (top - zmid)].astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    t, _ = emu_cam_prim(kind, o, d, par)
    assert (t == -1.0).all() if kind in ('sphere', 'capsule') else (t < 0).all(), (kind, t[t >= 0])
    # beyond the shape and pointing away: the entry lies behind the origin
    m = 10 * n if kind == 'cone' else n   # the cone is slim: fewer of the random rays meet it
    o, d = _random_rays(rng, m, max(par))
    keep = np.array([(x := _ref(kind, o[i], d[i], par)) is not None and x[0] > 0 for i in range(m)])
    t, _ = emu_cam_prim(kind, o[keep] + 3.0 * d[keep] / np.linalg.norm(d[keep], axis=1, keepdims=True) * 4 * max(par), d[keep], par)
    assert keep.sum() > 20 and (t < 0).all(), (kind, keep.sum(), t[t >= 0])
    if kind == 'capsule':
        assert (t == -1.0).all()   # its parts are taken only from in front of the origin


def test_cone_generator_parallel_and_a_negative():
    rb, zb, zt = 0.05, 0.1, 0.25
    k = rb / (zt - zb)
    rng = np.random.default_rng(13)
    n = 300
    # directions (cos, sin, -1 / k) rounded to fp32, kept where a, evaluated in fp32 as cam_cone evaluates it, lies inside the band
    # |a| <= 1e-7 (d.x^2 + d.y^2 + k^2 d.z^2) in which the kernel takes the ray for parallel to a generator
    f = np.float32
    kf = f(rb) / (f(zt) - f(zb)); k2 = kf * kf
    ang = rng.uniform(0, 2 * np.pi, 40000)
    d = np.c_[np.cos(ang), np.sin(ang), np.full(len(ang), -1.0 / k)].astype(f)
    xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], k2 * d[:, 2] * d[:, 2]
    band = np.abs(xx + yy - zz) <= f(1e-7) * (xx + yy + zz)
    assert xx.dtype == f and band.sum() >= 100, band.sum()
    d = d[band][:n]
    print(f'cone: {band.sum()} of {len(ang)} rounded generator directions take the parallel branch, {len(d)} compared')
    ang, n = ang[band][:n], len(d)
    o = (np.c_[rng.uniform(-1, 1, (n, 2)) * rb, np.full(n, zt + 0.3)]).astype(f)
    _compare('cone', o, d, (rb, zb, zt))
    # steeper than a generator (a < 0), from above the apex and from below through the base disc
    d = np.c_[0.3 * k * np.cos(ang), 0.3 * k * np.sin(ang), -np.ones(n)].astype(np.float32)
    _compare('cone', o, d, (rb, zb, zt))
    o2 = np.c_[rng.uniform(-0.8, 0.8, (n, 2)) * rb, np.full(n, zb - 0.2)].astype(np.float32)
    d2 = (d * np.float32([1, 1, -1])).astype(np.float32)
    _compare('cone', o2, d2, (rb, zb, zt), need_parts=(1,))


def _ref_hull(P, o, d):
    o, d, P = np.float64(o), np.float64(d), np.float64(P)
    den, num = P[:, :3] @ d, P[:, 3] - P[:, :3] @ o
    if ((den == 0) & (num < 0)).any():
        return None
    with np.errstate(divide='ignore', invalid='ignore'):
        tk = num / den
    tin, tout = np.where(den < 0, tk, -np.inf), np.where(den > 0, tk, np.inf)
    return (float(tin.max()), int(tin.argmax())) if tin.max() <= tout.min() else None


def _hull_case(P, o, d, max_grazing=0.01):
    from helpers import emu_cam_prim
    P = np.asarray(P, np.float32)
    t, part = emu_cam_prim('hull', o, d, planes=P)
    graze = 0
    for i in range(len(o)):
        refs = [_ref_hull(np.c_[P[:, :3], np.float64(P[:, 3]) * s], o[i], d[i]) for s in (1.0, 1 - 1e-5, 1 + 1e-5)]
        if len({r is None for r in refs}) > 1:
            graze += 1
            continue
        if refs[0] is None:
            assert t[i] == -1.0, (i, t[i])
            continue
        assert abs(t[i] - refs[0][0]) <= TOL(refs[0][0]), (i, t[i], refs[0])
        if refs[0][1] == refs[1][1] == refs[2][1]:
            nk = np.float64(P[int(part[i]), :3])   # the entry plane, or one through the same point (an edge)
            assert abs(nk @ (np.float64(o[i]) + refs[0][0] * np.float64(d[i])) - P[int(part[i]), 3]) <= 2e-5 * (1 + abs(refs[0][0])), (i, int(part[i]), refs[0])
    assert graze <= max_grazing * len(o), graze / len(o)
    return graze / len(o)


def test_hull_box_and_real_cloud():
    from gym_quadruped_amd.cabi import hull_planes
    rng = np.random.default_rng(14)
    s = np.array([0.12, 0.05, 0.03])
    box = np.array([[1, 0, 0, s[0]], [-1, 0, 0, s[0]], [0, 1, 0, s[1]], [0, -1, 0, s[1]], [0, 0, 1, s[2]], [0, 0, -1, s[2]]], np.float64)
    o, d = _random_rays(rng, 3000, 0.12)
    g1 = _hull_case(box, o, d)
    # parallel to a face (den == 0 exactly for two or four planes), inside and outside its slab
    o2 = o.copy(); d2 = d.copy()
    d2[:, 2] = 0.0; d2[::2, 1] = 0.0
    o2[:, 2] = rng.uniform(-2, 2, len(o2)) * s[2]
    _hull_case(box, o2, d2)
    md = cc._model('mini_cheetah')[0]
    P, adr = hull_planes(md)
    cl = int(np.argmax(np.diff(adr)))
    Pc = P[adr[cl]:adr[cl + 1]]
    assert len(Pc) >= 8
    ext = float(np.abs(Pc[:, 3]).max())
    o, d = _random_rays(rng, 3000, ext)
    g2 = _hull_case(Pc, o, d)
    # parallel to a face of the cloud: directions in the plane of a random face
    nk = np.float64(np.float32(Pc[rng.integers(0, len(Pc), len(d)), :3]))
    d3 = np.float64(d) - (np.float64(d) * nk).sum(1, keepdims=True) * nk
    _hull_case(Pc, o, d3.astype(np.float32))
    print(f'hull: {100 * g1:.2f} % (box) and {100 * g2:.2f} % (cloud of {len(Pc)} planes) grazing rays left out')


def test_ray_slab_and_triangle():
    from helpers import emu_ray_slab, emu_ray_triangle
    rng = np.random.default_rng(15)
    s = np.float32([0.3, 0.2, 0.1])
    o, d = _random_rays(rng, 3000, 0.3)
    for k in range(3):   # d[k] == 0 exactly, inside and outside slab k
        o[k::6, k] = rng.uniform(-2, 2, len(o[k::6])).astype(np.float32) * s[k]; d[k::6, k] = 0.0
    hit, tin, tout, ax = emu_ray_slab(o, d, s)
    graze = 0
    for i in range(len(o)):
        refs = []
        for sc in (1.0, 1 - 1e-5, 1 + 1e-5):
            lo, hi, axis, ok = -1e30, 1e30, -1, True
            for k in range(3):
                ok_, dk, s_ = np.float64(o[i, k]), np.float64(d[i, k]), np.float64(s[k]) * sc
                if dk == 0:
                    ok = ok and abs(ok_) <= s_
                    continue
                a, b = sorted(((-s_ - ok_) / dk, (s_ - ok_) / dk))
                if a > lo:
                    lo, axis = a, k
                hi = min(hi, b)
            refs.append((lo, axis) if ok and lo <= hi else None)
        if len({r is None for r in refs}) > 1:
            graze += 1
            continue
        assert bool(hit[i]) == (refs[0] is not None), (i, o[i], d[i])
        if refs[0] is not None:
            assert abs(tin[i] - refs[0][0]) <= TOL(refs[0][0]), (i, tin[i], refs[0])
            if refs[0][1] == refs[1][1] == refs[2][1]:
                assert int(ax[i]) == refs[0][1], (i, int(ax[i]), refs[0])
    assert graze <= 0.01 * len(o), graze / len(o)
    # ray_triangle in both precisions against fp64 Moeller-Trumbore, rays aimed inside and outside one triangle
    tri = np.float32([[0.0, 0.0, 0.1], [0.5, 0.0, 0.2], [0.0, 0.4, 0.05]])
    n = 2000
    o = np.c_[rng.uniform(-1, 1, (n, 2)), rng.uniform(0.5, 1.5, n)].astype(np.float32)
    w = rng.uniform(-0.3, 1.3, (n, 2))
    tgt = tri[0] + w[:, :1] * (tri[1] - tri[0]) + w[:, 1:] * (tri[2] - tri[0])
    d = (tgt - o).astype(np.float32)
    for dt, slack in ((np.float32, 1e-5), (np.float64, 1e-9)):
        hit, t = emu_ray_triangle(o, d, tri[0], tri[1], tri[2], dt)
        nedge = 0
        for i in range(n):
            tr, _ = _brute(np.float64(tri)[None], np.float64(o[i]), np.float64(d[i]), 0.0)
            u, v = w[i]
            if min(u, v, 1 - u - v) < slack * 10 and min(u, v, 1 - u - v) > -slack * 10:
                nedge += 1
                continue
            assert bool(hit[i]) == (tr >= 0), (dt, i, u, v)
            if tr >= 0:
                assert abs(t[i] - tr) <= (TOL(tr) if dt == np.float32 else 1e-9 * (1 + tr)), (dt, i, t[i], tr)
        assert nedge <= 0.01 * n
