"""Case tables for the height-field narrow phase of csrc/gq_boxes.h (closest_on_triangle, hf_triangle_under, sphere_hfield): four grids that are
rough or mild, coarse or fine, never square and away from the origin; sphere and triangle queries on them; and three evaluators that see the same
fp32-rounded inputs - (a) the truth, a numpy fp64 brute force over every triangle near the query with no culling and no rule about which triangle
may speak, (b) the fp64 oracle's routines (oracle/gq_oracle.c through gqo_test_closest_on_triangle / gqo_test_sphere_hfield), (c) the kernel's
routines, under the host emulator (emu_*) and on the GPU through the probe library (probe_*), one case per lane.  The precedent is
tests/contact_cases.py: generators, references, checks and coverage counts in one module.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from contact_cases import PAIR_TOL

TIE_WIDTH = 3e-7          # two candidates this close in distance: fp32 and fp64 may pick either (the project's tie width)
MAX_TIE_SHARE = 0.05      # per grid, counted from the reference's side
ORACLE_TOL = 1e-9         # oracle against truth: metres, and per normal component (tests/test_oracle_invariants.py)
MARGINS = (0.0, 0.002)
SLIVER = 0.1            # height of a sliver triangle over its long edge (triangle_cases)

# name: (rows, cols, dx, dy, amplitude, pos, seed)
GRIDS = {
    'mild_coarse': (41, 57, 0.11, 0.07, 0.03, (40.0, -35.0, 0.4), 101),
    'rough_coarse': (41, 57, 0.11, 0.07, 0.12, (40.0, -35.0, 0.4), 102),
    'mild_fine': (161, 193, 0.012, 0.009, 0.004, (-1.5, 2.5, 0.0), 103),
    'rough_fine': (161, 193, 0.012, 0.009, 0.02, (-1.5, 2.5, 0.0), 104),
}


@functools.lru_cache(None)
def grid(name):
    """The grid as generate_terrain returns it under 'hfield': data float32 in [0, 1] (uniform noise, fixed seed), size = (rx, ry, elevation, base)."""
    from gym_quadruped_amd.terrain import _BOX_DEFAULT
    nr, nc, dx, dy, amp, pos, seed = GRIDS[name]
    hf = dict(_BOX_DEFAULT)
    data = np.random.default_rng(seed).uniform(0.0, 1.0, (nr, nc)).astype(np.float32)
    hf.update(data=data, size=(dx * (nc - 1) / 2.0, dy * (nr - 1) / 2.0, float(amp), 0.01), pos=tuple(float(v) for v in pos))
    return hf


def cell_sizes(hf):
    nr, nc = hf['data'].shape
    return 2 * hf['size'][0] / (nc - 1), 2 * hf['size'][1] / (nr - 1)


def limits(hf, inset):
    """terrain limits (x max, x min, y max, y min) `inset` inside the grid's border"""
    sx, sy = hf['size'][0], hf['size'][1]
    px, py = hf['pos'][0], hf['pos'][1]
    return (px + sx - inset, px - sx + inset, py + sy - inset, py - sy + inset)


@functools.lru_cache(None)
def foot_radii():
    """the foot radii of aliengo and hyqreal1"""
    from helpers import marshalled
    out = []
    for robot in ('aliengo', 'hyqreal1'):
        mm = marshalled(robot, solver=1)
        out += [float(mm.md.cloud_radius[mm.md.geom_cloudid[int(g)]]) for g in mm.desc.feet_geomid]
    return tuple(sorted(set(out)))


# ----------------------------------------------------------------------------------------------------------------- the surface, fp64
def _heights(hf):
    return hf['size'][2] * np.asarray(hf['data'], dtype=np.float64)


def surface(hf, x, y):
    """Height (relative to pos z) and unit normal of the triangle under the hfield-local points (x, y): triangle interpolation with the kernel's
    diagonal (from (c, r+1) to (c+1, r)); also `inside` (the point lies over the grid) and `edge`, the distance of the point's cell coordinates
    from the nearest cell line or diagonal in cells (where fp32 and fp64 may take different triangles)."""
    Hm = _heights(hf)
    nr, nc = Hm.shape
    dx, dy = cell_sizes(hf)
    fx, fy = (np.asarray(x, np.float64) + hf['size'][0]) / dx, (np.asarray(y, np.float64) + hf['size'][1]) / dy
    inside = (fx >= 0) & (fy >= 0) & (fx <= nc - 1) & (fy <= nr - 1)
    c = np.clip(np.floor(fx).astype(int), 0, nc - 2); r = np.clip(np.floor(fy).astype(int), 0, nr - 2)
    u, v = fx - c, fy - r
    h00, h10, h01, h11 = Hm[r, c], Hm[r, c + 1], Hm[r + 1, c], Hm[r + 1, c + 1]
    up = u + v > 1.0
    gx = np.where(up, h11 - h01, h10 - h00) / dx
    gy = np.where(up, h11 - h10, h01 - h00) / dy
    h = np.where(up, h11 + (u - 1) * (h11 - h01) + (v - 1) * (h11 - h10), h00 + u * (h10 - h00) + v * (h01 - h00))
    inv = 1 / np.sqrt(gx * gx + gy * gy + 1)
    n = np.stack([-gx * inv, -gy * inv, inv], -1)
    edge = np.minimum.reduce([u, 1 - u, v, 1 - v, np.abs(u + v - 1)])
    return h, n, inside, edge


def _closest_on_triangles(P, A, B, Cc):
    """Closest points of triangles to points, broadcast over leading axes, NOT by Ericson's region walk (that is the routine under test): the
    orthogonal projection where it falls inside the triangle, else the nearest of the three edges' closest points.  Returns q, the unit normal
    (n.z >= 0 for a height-field triangle), the barycentric coordinates of the projection, interior, and the feature of q (0-2 corner a / b / c,
    3-5 edge ab / bc / ca, 6 interior)."""
    AB, AC = B - A, Cc - A
    N = np.cross(AB, AC)
    nn = N / np.linalg.norm(N, axis=-1, keepdims=True)
    nn = np.where(nn[..., 2:3] < 0, -nn, nn)
    side = np.sum((P - A) * nn, -1, keepdims=True)
    proj = P - side * nn
    area = np.sum(np.cross(AB, AC) * nn, -1)
    wa = np.sum(np.cross(B - proj, Cc - proj) * nn, -1) / area
    wb = np.sum(np.cross(Cc - proj, A - proj) * nn, -1) / area
    wc = np.sum(np.cross(A - proj, B - proj) * nn, -1) / area
    bary = np.stack([wa, wb, wc], -1)
    interior = (bary >= 0).all(-1)
    best_q, best_d, feat = proj.copy(), np.full(interior.shape, np.inf), np.full(interior.shape, 6)
    for k, (S, E) in enumerate(((A, B), (B, Cc), (Cc, A))):
        D = E - S
        t = np.clip(np.sum((P - S) * D, -1) / np.sum(D * D, -1), 0.0, 1.0)
        qs = S + t[..., None] * D
        ds = np.linalg.norm(P - qs, axis=-1)
        better = ds < best_d
        f = np.where(t == 0.0, k, np.where(t == 1.0, (k + 1) % 3, 3 + k))
        best_q = np.where(better[..., None], qs, best_q); feat = np.where(better, f, feat); best_d = np.where(better, ds, best_d)
    q = np.where(interior[..., None], proj, best_q)
    feat = np.where(interior, 6, feat)
    return q, nn, bary, interior, feat


# ----------------------------------------------------------------------------------------------------------------- sphere queries
@functools.lru_cache(None)
def sphere_cases(name):
    """1000 queries over the grid's interior and 100 within r + reach of its border, inside and just outside.  Every evaluator sees the same
    numbers: base (x, y of a robot's base, float64 holding fp32 values), rel (the centre's x, y relative to the base and its world z, fp32), r,
    reach (fp32); the hfield-local centre `p` is base + rel - float32(pos) in fp64, exactly what the kernel's coordinates stand for."""
    hf = grid(name)
    rng = np.random.default_rng(GRIDS[name][6] + 1000)
    sx, sy = hf['size'][0], hf['size'][1]
    pos = np.asarray(hf['pos'], np.float32).astype(np.float64)
    n_in, n_bd = 1000, 100
    n = n_in + n_bd
    r = rng.choice(foot_radii(), n)
    reach = np.maximum(rng.choice(MARGINS, n), 0.0) + 1e-4
    R = r + reach
    x = rng.uniform(-sx + R, sx - R, n); y = rng.uniform(-sy + R, sy - R, n)
    # the border queries: one coordinate within R of a border line, on either side of it; the other anywhere (corners included)
    k = np.arange(n_in, n)
    off = rng.uniform(-1.0, 1.0, n_bd) * R[k]
    which = rng.integers(0, 4, n_bd)
    x[k] = np.where(which == 0, -sx + off, np.where(which == 1, sx + off, rng.uniform(-sx - R[k], sx + R[k])))
    y[k] = np.where(which == 2, -sy + off, np.where(which == 3, sy + off, rng.uniform(-sy - R[k], sy + R[k])))
    h, _, _, _ = surface(hf, np.clip(x, -sx, sx), np.clip(y, -sy, sy))
    z = h + rng.uniform(0.2 * r, r + reach)
    f32 = lambda a: np.asarray(a, np.float32)
    world = np.stack([x + pos[0], y + pos[1], z + pos[2]], -1)
    base = f32(world[:, :2] + rng.uniform(-0.3, 0.3, (n, 2))).astype(np.float64)
    rel = f32(np.concatenate([world[:, :2] - base, world[:, 2:3]], -1))
    r32, reach32 = f32(r), f32(reach)
    p = np.concatenate([base + rel[:, :2].astype(np.float64) - pos[:2], rel[:, 2:3].astype(np.float64) - pos[2]], -1)
    hs, ns, inside, edge = surface(hf, p[:, 0], p[:, 1])
    return dict(name=name, hf=hf, n=n, base=base, rel=rel, r=r32, reach=reach32, p=p, surf_h=hs, surf_n=ns, inside=inside, edge=edge,
                above=inside & (p[:, 2] > hs), border=np.arange(n) >= n_in)


@functools.lru_cache(None)
def sphere_truth(name):
    """(a) per query: the smallest exact point-triangle distance over every triangle within r + reach (+ a cell) of the centre minus r, and the
    candidates within TIE_WIDTH of it: their normals (p - q) / |p - q|, the face normal where p lies on the triangle.  `second`: the query has a
    candidate within TIE_WIDTH whose normal is another one (more than PAIR_TOL's normal tolerance away)."""
    cs = sphere_cases(name)
    hf, p = cs['hf'], cs['p']
    Hm = _heights(hf)
    nr, nc = Hm.shape
    dx, dy = cell_sizes(hf)
    sx, sy = hf['size'][0], hf['size'][1]
    Rmax = float((cs['r'] + cs['reach']).max())
    wx, wy = int(np.ceil(Rmax / dx)) + 1, int(np.ceil(Rmax / dy)) + 1
    c0 = np.floor((p[:, 0] + sx) / dx).astype(int); r0 = np.floor((p[:, 1] + sy) / dy).astype(int)
    oc, orr, up = np.meshgrid(np.arange(-wx, wx + 1), np.arange(-wy, wy + 1), np.arange(2), indexing='ij')
    c = c0[:, None] + oc.ravel()[None, :]; rr = r0[:, None] + orr.ravel()[None, :]; up = np.broadcast_to(up.ravel()[None, :], c.shape)
    valid = (c >= 0) & (rr >= 0) & (c <= nc - 2) & (rr <= nr - 2)
    cc, rc = np.clip(c, 0, nc - 2), np.clip(rr, 0, nr - 2)
    x0, y0 = -sx + dx * cc, -sy + dy * rc
    B = np.stack([x0 + dx, y0, Hm[rc, cc + 1]], -1); Cc = np.stack([x0, y0 + dy, Hm[rc + 1, cc]], -1)
    A = np.where(up[..., None] == 1, np.stack([x0 + dx, y0 + dy, Hm[rc + 1, cc + 1]], -1), np.stack([x0, y0, Hm[rc, cc]], -1))
    P = p[:, None, :]
    q, nn, _, _, feat = _closest_on_triangles(P, A, B, Cc)
    d = P - q
    l = np.linalg.norm(d, axis=-1)
    nrm = np.where(l[..., None] > 1e-12, d / np.maximum(l, 1e-300)[..., None], nn)
    l = np.where(valid, l, np.inf)
    best = l.min(1)
    cand = l <= best[:, None] + TIE_WIDTH
    first = l.argmin(1)
    n0 = nrm[np.arange(len(p)), first]
    other = cand & (np.abs(nrm - n0[:, None, :]).max(-1) > PAIR_TOL['nrm'])
    return dict(dist=best - cs['r'].astype(np.float64), nrm=n0, cand=cand, cand_nrm=nrm, second=other.any(1),
                face=feat[np.arange(len(p)), first] == 6)


def _desc(hf):
    from helpers import GqModelDesc
    d = GqModelDesc()
    data = np.ascontiguousarray(hf['data'], dtype=np.float32)
    d.hfield_nrow, d.hfield_ncol = data.shape
    d.hfield_data = data.ctypes.data_as(C.POINTER(C.c_float))
    d.hfield_size = (C.c_double * 4)(*[float(v) for v in hf['size']])
    return d, data


@functools.lru_cache(None)
def sphere_oracle(name):
    """(b) oracle/gq_oracle.c's sphere_hfield on the hfield-local centres"""
    from oracle.oracle import lib
    cs = sphere_cases(name)
    L = lib()
    P = C.c_void_p
    L.gqo_test_sphere_hfield.argtypes = [P, C.c_int, P, P, P, P, P]
    L.gqo_test_sphere_hfield.restype = None
    d, keep = _desc(cs['hf'])
    p = np.ascontiguousarray(cs['p']); r = cs['r'].astype(np.float64); reach = cs['reach'].astype(np.float64)
    hit, out = np.zeros(cs['n'], np.int32), np.zeros((cs['n'], 4))
    L.gqo_test_sphere_hfield(C.byref(d), cs['n'], p.ctypes.data, r.ctypes.data, reach.ctypes.data, hit.ctypes.data, out.ctypes.data)
    return dict(hit=hit.astype(bool), dist=out[:, 0], nrm=out[:, 1:4])


def _grid_words(hf):
    nr, nc = hf['data'].shape
    pos = np.asarray(hf['pos'], np.float64)
    return np.array([nr, nc, hf['size'][0], hf['size'][1], hf['size'][2], *pos], np.float64)


def backend_spheres(be, name):
    """(c) the kernel's sphere_hfield and hf_triangle_under through `be` (device_cases.Backend over the emulator library or the probe library)"""
    from device_cases import Out
    cs = sphere_cases(name)
    q = np.concatenate([cs['rel'], cs['r'][:, None], cs['reach'][:, None]], -1).astype(np.float32)
    n = cs['n']
    hit, out, under = be.run('sphere_hfield', _grid_words(cs['hf']), np.ascontiguousarray(cs['hf']['data'], dtype=np.float32), cs['base'], q, n,
                             Out((n,), np.int32), Out((n, 4), np.float32), Out((n, 5), np.float32))
    return dict(hit=hit.astype(bool), dist=out[:, 0].astype(np.float64), nrm=out[:, 1:4].astype(np.float64), under=under.astype(np.float64))


def compared(cs, truth):
    """the queries the oracle is held to the truth on: the centre lies above the surface and the true distance is below reach"""
    return cs['above'] & (truth['dist'] < cs['reach'])


def tie_share(name):
    cs, t = sphere_cases(name), sphere_truth(name)
    m = compared(cs, t)
    return float((t['second'] & m).sum()) / max(int(m.sum()), 1), int(m.sum())


def _normal_error(nrm, truth, i):
    """distance (largest component) of a normal to the nearest of the truth's candidates of query i"""
    return float(np.abs(truth['cand_nrm'][i][truth['cand'][i]] - nrm[None, :]).max(-1).min())


def check_oracle_spheres(name):
    """(b) against (a): every compared query is a contact of the brute-force distance, with the normal of one of the nearest candidates.
    Returns (compared, worst distance error, worst normal error, queries with a second candidate, face / non-face contacts)."""
    cs, t, o = sphere_cases(name), sphere_truth(name), sphere_oracle(name)
    idx = np.flatnonzero(compared(cs, t))
    wd = wn = 0.0
    bad = []
    for i in idx:
        ed = abs(o['dist'][i] - t['dist'][i]) if o['hit'][i] or t['dist'][i] > cs['reach'][i] - ORACLE_TOL else np.inf
        en = _normal_error(o['nrm'][i], t, i)
        wd, wn = max(wd, ed), max(wn, en)
        if not (ed < ORACLE_TOL and en < ORACLE_TOL):
            bad.append((int(i), float(o['dist'][i]), float(t['dist'][i]), en))
    nface = int(t['face'][idx].sum())
    assert len(idx) >= 300 and len(idx) - nface >= (20 if 'rough' in name else 0), (name, len(idx), nface)
    assert int(cs['border'][idx].sum()) >= 10, (name, int(cs['border'][idx].sum()))
    assert not bad, (name, f'{len(bad)} of {len(idx)} queries disagree with the brute-force distance', bad[:6])
    return len(idx), wd, wn, int(t['second'][idx].sum()), nface, len(idx) - nface


def check_backend_spheres(name, got, tol=PAIR_TOL):
    """(c) against (b), every query (those beside and beyond the border too).  Presence agrees unless the true distance (the oracle's, where the
    centre is not over the grid) is within tol['dist'] of reach; distances agree; the normal is the oracle's or - ties - that of a candidate whose
    distance is within TIE_WIDTH of the smallest.  The triangle under the centre (hf_triangle_under): on or off the grid as the fp64 surface
    says, its height to tol['dist'], its normal to tol['nrm'] away from cell lines and diagonals.  Returns the worst errors."""
    cs, t, o = sphere_cases(name), sphere_truth(name), sphere_oracle(name)
    worst = dict(dist=(0.0, -1), nrm=(0.0, -1), height=(0.0, -1))
    nhit = nfar = ntie = 0
    for i in range(cs['n']):
        ref_d = t['dist'][i] if cs['above'][i] else o['dist'][i]
        if got['hit'][i] != o['hit'][i]:
            assert abs(ref_d - cs['reach'][i]) < tol['dist'], (name, i, 'presence', bool(got['hit'][i]), bool(o['hit'][i]), ref_d, float(cs['reach'][i]))
            continue
        if not o['hit'][i]:
            nfar += 1
            continue
        nhit += 1
        ed = abs(got['dist'][i] - o['dist'][i])
        en = float(np.abs(got['nrm'][i] - o['nrm'][i]).max())
        if en >= tol['nrm'] and cs['above'][i] and t['second'][i]:
            ntie += 1
            en = _normal_error(got['nrm'][i], t, i)
        for key, e in (('dist', ed), ('nrm', en)):
            if e > worst[key][0]:
                worst[key] = (float(e), i)
        assert ed < tol['dist'], (name, i, 'dist', got['dist'][i], o['dist'][i])
        assert en < tol['nrm'], (name, i, 'normal', got['nrm'][i], o['nrm'][i])
    u = got['under']
    on_line = cs['edge'] < 1e-4
    dx, dy = cell_sizes(cs['hf'])
    at_border = np.minimum(np.abs(np.abs(cs['p'][:, 0]) - cs['hf']['size'][0]), np.abs(np.abs(cs['p'][:, 1]) - cs['hf']['size'][1])) < 1e-5
    for i in range(cs['n']):
        if at_border[i]:
            continue
        assert bool(u[i, 0]) == bool(cs['inside'][i]), (name, i, 'triangle under', u[i], cs['p'][i])
        if not cs['inside'][i]:
            continue
        eh = abs(u[i, 1] - cs['surf_h'][i])
        if eh > worst['height'][0]:
            worst['height'] = (float(eh), i)
        assert eh < tol['dist'], (name, i, 'height under', u[i, 1], cs['surf_h'][i])
        if not on_line[i]:
            np.testing.assert_allclose(u[i, 2:5], cs['surf_n'][i], atol=tol['nrm'], err_msg=f'{name} query {i} normal under')
    assert nhit >= 300 and nfar >= 5 and int(cs['inside'].sum()) < cs['n'], (name, nhit, nfar)
    return dict(worst, hits=nhit, ties=ntie)


# ----------------------------------------------------------------------------------------------------------------- triangle queries
_FEATURES = ('corner a', 'corner b', 'corner c', 'edge ab', 'edge bc', 'edge ca', 'interior')


@functools.lru_cache(None)
def triangle_cases():
    """Random triangles and slivers (the third corner SLIVER of the long edge off it) with points spread over all seven Voronoi regions,
    and triangles on a dyadic lattice with points EXACTLY over a corner and exactly over an edge.  fp32 inputs; the fp64 reference of
    _closest_on_triangles: q, the barycentric coordinates of the projection, interior, the feature.
    How thin: a height-field triangle's thinness is |dh| / cell size, at most 0.12 / 0.07 = 1.7 and 0.02 / 0.009 = 2.2 on the grids above;
    1 : 10 is five times thinner than anything they hold.  The barycentric weights are differences of products that cancel to the fraction
    area / L^2, so the closest point's fp32 error grows with the aspect - between eps32 x aspect x size and eps32 x aspect^2 x size, 2e-7 to
    2e-6 m at 1 : 10 and 0.3 m, under PAIR_TOL['pos'] = 5e-6; at 1 : 50 the emulator was measured at 9e-6, so no fp32 evaluation of the
    formula holds that tolerance there.  A random triangle that happens to be thinner than the slivers is drawn again."""
    rng = np.random.default_rng(77)
    rows = []
    for trial in range(2400):
        a = rng.uniform(-0.5, 0.5, 3)
        b = a + rng.normal(0, 1, 3) * rng.uniform(0.01, 0.3)
        if trial % 3 == 2:   # sliver
            w = rng.normal(0, 1, 3); w -= w @ (b - a) * (b - a) / ((b - a) @ (b - a)); w /= np.linalg.norm(w)
            c = a + rng.uniform(0.1, 0.9) * (b - a) + SLIVER * np.linalg.norm(b - a) * w
        else:
            c = a + rng.normal(0, 1, 3) * rng.uniform(0.01, 0.3)
            while max(np.linalg.norm(b - a), np.linalg.norm(c - b), np.linalg.norm(a - c)) ** 2 * SLIVER > 2 * np.linalg.norm(np.cross(b - a, c - a)):
                c = a + rng.normal(0, 1, 3) * rng.uniform(0.01, 0.3)
        n = np.cross(b - a, c - a); n /= np.linalg.norm(n)
        w3 = rng.uniform(-1.0, 2.0, 3); w3 /= w3.sum() if abs(w3.sum()) > 0.2 else 1.0
        p = w3[0] * a + w3[1] * b + w3[2] * c + n * rng.normal(0, 0.05)
        rows.append(np.concatenate([p, a, b, c]))
    exact = 0
    for trial in range(60):   # dyadic lattice, the triangle in a plane z = const: the point sits exactly over a corner / an edge's midpoint
        g = lambda: rng.integers(-64, 64, 2) / 128.0
        z0 = float(rng.integers(-32, 32)) / 64.0
        a, b, c = (np.array([*g(), z0]) for _ in range(3))
        if abs(np.cross(b - a, c - a)[2]) < 1e-3:
            continue
        hgt = float(rng.integers(1, 32)) / 256.0 * (1 if trial % 2 else -1)
        for foot in (a, b, c, (a + b) / 2, (b + c) / 2, (c + a) / 2):
            rows.append(np.concatenate([foot + [0, 0, hgt], a, b, c])); exact += 1
    inp = np.asarray(rows, np.float32)
    D = inp.astype(np.float64)
    q, _, bary, interior, feat = _closest_on_triangles(D[:, 0:3], D[:, 3:6], D[:, 6:9], D[:, 9:12])
    counts = np.bincount(feat, minlength=7)
    assert (counts >= 50).all() and exact >= 200, dict(zip(_FEATURES, counts))
    return dict(inp=inp, q=q, bary=bary, interior=interior, feat=feat, counts=counts, exact=exact)


def oracle_triangles():
    from oracle.oracle import lib
    cs = triangle_cases()
    L = lib()
    L.gqo_test_closest_on_triangle.argtypes = [C.c_void_p] * 5
    D = np.ascontiguousarray(cs['inp'].astype(np.float64))
    q, inside = np.zeros((len(D), 3)), np.zeros(len(D), bool)
    for i in range(len(D)):
        inside[i] = bool(L.gqo_test_closest_on_triangle(D[i, 0:3].ctypes.data, D[i, 3:6].ctypes.data, D[i, 6:9].ctypes.data, D[i, 9:12].ctypes.data, q[i].ctypes.data))
    return q, inside


def backend_triangles(be):
    from device_cases import Out
    cs = triangle_cases()
    n = len(cs['inp'])
    q, inside = be.run('closest_on_triangle', cs['inp'], n, Out((n, 3), np.float32), Out((n,), np.int32))
    return q.astype(np.float64), inside.astype(bool)


def check_triangles(q, inside, pos_tol):
    """the closest point to pos_tol; the `interior` flag agrees unless a reference barycentric coordinate is within 1e-6 of 0"""
    cs = triangle_cases()
    err = np.abs(q - cs['q']).max(-1)
    i = int(err.argmax())
    assert err[i] < pos_tol, ('closest point', i, q[i], cs['q'][i], _FEATURES[cs['feat'][i]])
    clear = np.abs(cs['bary']).min(-1) > 1e-6
    bad = np.flatnonzero(clear & (inside != cs['interior']))
    assert not len(bad), ('interior flag', bad[:8], cs['bary'][bad[:8]])
    assert int(clear.sum()) >= 0.8 * len(clear)
    return float(err[i]), i


# ----------------------------------------------------------------------------------------------------------------- the report
REPORT_HEAD = ('Height-field routines of csrc/gq_boxes.h against the fp64 oracle\'s (tests/hfield_cases.py): worst errors per grid and backend; '
               'the oracle itself against the brute-force distance')


def write_report(backend, lines):
    """profiles/hfield_cases_report.txt: the lines of `backend` ('oracle', 'emulator', 'gpu') replaced, the other backends' kept"""
    import os
    from helpers import ROOT
    path = os.environ.get('GQ_HFIELD_REPORT', str(ROOT / 'profiles' / 'hfield_cases_report.txt'))
    try:
        old = [ln for ln in open(path).read().splitlines()[1:] if ln and not ln.startswith(backend + ' ')] if os.path.exists(path) else []
        order = {'oracle': 0, 'emulator': 1, 'gpu': 2}
        body = sorted(old + [f'{backend} {ln}' for ln in lines], key=lambda ln: order.get(ln.split(' ', 1)[0], 3))
        text = REPORT_HEAD + '\n' + '\n'.join(body) + '\n'
        if not os.path.exists(path) or open(path).read() != text:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, 'w') as fh:
                fh.write(text)
    except OSError:
        pass


def fmt_spheres(name, w, tol=PAIR_TOL):
    return (f'sphere_hfield {name:<13s} contacts {w["hits"]:>5d}   max error vs fp64 oracle: dist {w["dist"][0]:.3g} (query {w["dist"][1]}, tolerance {tol["dist"]:g}), '
            f'nrm {w["nrm"][0]:.3g} (query {w["nrm"][1]}, tolerance {tol["nrm"]:g}), height under {w["height"][0]:.3g} (query {w["height"][1]}); '
            f'{w["ties"]} normals settled among tied candidates')


def run_backend(be, label):
    """every check of a kernel backend, the report lines written; returns them"""
    lines = []
    e, i = check_triangles(*backend_triangles(be), PAIR_TOL['pos'])
    lines.append(f'closest_on_triangle cases {len(triangle_cases()["inp"]):>5d}   max point error vs fp64 reference {e:.3g} (case {i}, tolerance {PAIR_TOL["pos"]:g})')
    for name in GRIDS:
        lines.append(fmt_spheres(name, check_backend_spheres(name, backend_spheres(be, name))))
    for ln in lines:
        print(label, ln)
    write_report(label, lines)
    return lines


# ----------------------------------------------------------------------------------------------------------------- whole steps on the grids
STEP_ROBOTS = ('aliengo', 'hyqreal1')   # primitive geoms and pyramidal cones / hulls and elliptic cones


def scene(name):
    """(scene description, terrain limits) as generate_terrain returns them, with the grid for height field"""
    from gym_quadruped_amd.terrain import _FLOOR_DEFAULT
    hf = grid(name)
    return {'name': name, 'floor': dict(_FLOOR_DEFAULT), 'boxes': [], 'hfield': hf}, limits(hf, 0.0)


def assert_foot_form(mm, hf, name, robot):
    """Which foot form hfield_item_scan takes holds by construction: on the coarse grids 2 (r + reach) < min(dx, dy) for every foot of aliengo, a
    footprint of at most 2 x 2 cells (the parallel form; hyqreal1's feet of 0.036 m span 0.074 m, a shade over the 0.07 m rows, so a foot that
    straddles two grid lines sends its step through the serial form: at most 3 rows, either form may run); on the fine grids max(dx, dy) <=
    every foot radius, so c1 - c0 >= 2 (the serial form)."""
    dx, dy = cell_sizes(hf)
    md = mm.md
    for g in mm.desc.feet_geomid:
        r = float(md.cloud_radius[md.geom_cloudid[int(g)]])
        reach = max(float(max(hf['margin'], md.geom_margin[int(g)])), 0.0) + 1e-4
        if 'coarse' in name:
            assert 2 * (r + reach) < (2 if robot == 'hyqreal1' else 1) * min(dx, dy), (name, r, reach, dx, dy)
        else:
            assert max(dx, dy) <= r, (name, r, dx, dy)


def step_states(mm, robot, name, n, rng, o):
    """n states of robots dropped at a drawn height over the local surface of the grid, at most 8 % of them over the kernel's row budget; a
    quarter of the envs with the base within one body length of the grid's border (feet and links hang over it)."""
    from helpers import budgeted_states, random_states
    from gym_quadruped_amd.robot_cfgs import get_robot_config
    hf, md = grid(name), mm.md
    hip = float(get_robot_config(robot).hip_height)
    sx, sy = hf['size'][0], hf['size'][1]
    body = float(np.ptp(np.asarray(md.body_pos)[[2, 5, 8, 11], 0])) + 2 * float(np.abs(np.asarray(md.body_pos)[[2, 5, 8, 11], 1]).max())
    body = min(body, 0.9 * min(sx, sy))

    hips = np.asarray(md.body_pos)[[2, 5, 8, 11]]
    reach_xy = 0.5 * float(np.hypot(np.ptp(hips[:, 0]), 2 * np.abs(hips[:, 1]).max())) + 0.08   # the circle the feet of a standing robot stay in

    def draw_coarse(k):
        q, v = random_states(md, k, rng, z_range=(0.65 * hip, 0.98 * hip))
        x, y = rng.uniform(-sx + body, sx - body, k), rng.uniform(-sy + body, sy - body, k)
        edge = np.arange(k) % 4 == 0
        side = rng.integers(0, 4, k)
        d = rng.uniform(0.0, body, k)
        x = np.where(edge & (side == 0), -sx + d, np.where(edge & (side == 1), sx - d, np.where(edge, rng.uniform(-sx, sx, k), x)))
        y = np.where(edge & (side == 2), -sy + d, np.where(edge & (side == 3), sy - d, np.where(edge, rng.uniform(-sy, sy, k), y)))
        h, _, _, _ = surface(hf, x, y)
        q[:, 0], q[:, 1] = x + hf['pos'][0], y + hf['pos'][1]
        q[:, 2] += h + hf['pos'][2]
        # every second robot away from the border stands on the surface instead (draw_fine): feet that rest on the ridges, centres above them
        qs, vs = draw_fine(k)
        stand = (np.arange(k) % 2 == 1) & ~edge
        q[stand], v[stand] = qs[stand], vs[stand]
        keep = np.ones(k, bool)
        for e in range(k):   # feet that keep their lever (min_lever); the other draws are left out
            o.set_state(q[e], np.zeros(18), np.zeros(18), np.zeros(18), 0.0, 0.8); o.forward(np.zeros(12), stage=1)
            keep[e] = min_lever(o, mm, hf) >= MIN_LEVER and not _tie(o)
        return q[keep], v[keep]

    def draw_fine(k):
        """The fine grids are hardly larger than the robots and lie in the floor's plane, so whatever sinks into them meets the floor as well and
        the row budget is spent twice: a standing robot (small joint noise and tilt, all feet over the grid) is lowered in steps of 2 mm until
        the oracle sees four height-field contacts, then a drawn 0 - 4 mm further."""
        from scipy.spatial.transform import Rotation
        q, v = random_states(md, k, rng)
        v *= 0.3
        for e in range(k):
            for attempt in range(30):   # a pose whose feet keep their lever (min_lever): drawn again otherwise
                q[e, 7:] = md.key_qpos[0][7:] + rng.uniform(-0.05, 0.05, 12)
                q[e, 3:7] = Rotation.from_euler('xyz', [rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(-np.pi, np.pi)]).as_quat(scalar_first=True)
                q[e, 0] = hf['pos'][0] + rng.uniform(-sx + reach_xy, sx - reach_xy); q[e, 1] = hf['pos'][1] + rng.uniform(-sy + reach_xy, sy - reach_xy)
                for z in np.arange(1.1 * hip, 0.8 * hip, -0.002):
                    q[e, 2] = hf['pos'][2] + z
                    o.set_state(q[e], np.zeros(18), np.zeros(18), np.zeros(18), 0.0, 0.8); o.forward(np.zeros(12), stage=1)
                    if count_contacts(o, mm, hf)[0] >= 4:
                        break
                q[e, 2] -= rng.uniform(0.0, 0.004)
                o.set_state(q[e], np.zeros(18), np.zeros(18), np.zeros(18), 0.0, 0.8); o.forward(np.zeros(12), stage=1)
                if count_contacts(o, mm, hf)[0] >= 4 and min_lever(o, mm, hf) >= MIN_LEVER and not _tie(o):
                    break
        return q, v

    draw = draw_coarse if 'coarse' in name else draw_fine
    qpos, qvel = budgeted_states(n, draw, o, md.cone == 1, max_over=0.08)
    dist = np.minimum(sx - np.abs(qpos[:, 0] - hf['pos'][0]), sy - np.abs(qpos[:, 1] - hf['pos'][1]))
    assert (dist <= body).sum() >= n // 4 - 1, (name, int((dist <= body).sum()), n)
    for e in range(n):
        o.set_state(qpos[e], np.zeros(18), np.zeros(18), np.zeros(18), 0.0, 0.8); o.forward(np.zeros(12), stage=1)
        assert min_lever(o, mm, hf) >= MIN_LEVER, (name, e, min_lever(o, mm, hf))
    return qpos, qvel.astype(np.float32)


MIN_LEVER = 0.01   # metres; see min_lever


def _tie(o):
    """two cloud vertices of numerically equal depth (ParityTally's tie, 3e-6): the env would be skipped, not compared - hyqreal1's finely
    tessellated hulls tie in more than half of the drawn poses - so such a draw is left out, as budgeted_states leaves out over-budget ones"""
    return bool(o.ncon) and float(o.get('contact_tiegap').min()) < 3e-6


def min_lever(o, mm, hf):
    """The smallest distance |p - q| = r + dist between a foot's centre and the edge or corner it touches, over the oracle's current contacts
    (inf without one).  The normal of such a contact is (p - q) / |p - q|; the kernel's fp32 kinematics place p to about the project's tie width
    (3e-7 m), so the normal - and with it the contact's rows of efc_J - carries an error of 3e-7 / |p - q|.  TERRAIN_NEWTON_STEP holds efc_J to
    3e-5: out of reach of any fp32 kernel once the centre is closer than 3e-7 / 3e-5 = 0.01 m to the feature, i.e. once a foot of 0.0265 m has
    sunk 0.0165 m into a ridge - no state a simulation comes to rest in.  The whole-step states keep every such lever at 0.01 m or more by
    construction (a face contact's normal does not depend on p and has no lever).  A state that did not was measured at 1.06e-4 in efc_J, on
    the emulator and the GPU alike: the robot had been lowered until its feet sat 0.9 and 3.8 mm from ridges."""
    if not o.ncon:
        return np.inf
    md = mm.md
    feet = {int(g) for g in mm.desc.feet_geomid}
    nrm, pos, dist, geom = o.contact_frame[:, 0, :], o.contact_pos, o.get('contact_dist'), o.get('contact_geom').astype(int)
    world = o.get('contact_body1').astype(int) == 0
    out = np.inf
    for c in range(o.ncon):
        if not world[c] or abs(nrm[c, 2] - 1.0) <= 1e-9 or geom[c] not in feet:
            continue
        q = pos[c] - 0.5 * dist[c] * nrm[c] - np.asarray(hf['pos'], np.float64)
        _, ns, _, _ = surface(hf, q[0], q[1])
        if np.abs(ns - nrm[c]).max() > 1e-6:
            out = min(out, float(md.cloud_radius[md.geom_cloudid[geom[c]]]) + float(dist[c]))
    return out


def count_contacts(o, mm, hf):
    """From the oracle's side, after its step: (height-field contacts, those of feet whose normal is not the face normal of the triangle under
    the contact's surface point - the closest feature is an edge or a corner -, link-geom contacts with the height field)"""
    if not o.ncon:
        return 0, 0, 0
    md = mm.md
    feet = {int(g) for g in mm.desc.feet_geomid}
    nrm, pos, dist, geom = o.contact_frame[:, 0, :], o.contact_pos, o.get('contact_dist'), o.get('contact_geom').astype(int)
    world = o.get('contact_body1').astype(int) == 0
    nhf = nonface = nlink = 0
    for c in range(o.ncon):
        if not world[c] or abs(nrm[c, 2] - 1.0) <= 1e-9:
            continue   # robot-robot, or the floor
        nhf += 1
        if geom[c] not in feet:
            nlink += 1
            continue
        q = pos[c] - 0.5 * dist[c] * nrm[c] - np.asarray(hf['pos'], np.float64)   # the point on the surface
        _, ns, inside, _ = surface(hf, q[0], q[1])
        nonface += bool(np.abs(ns - nrm[c]).max() > 1e-6)
    return nhf, nonface, nlink

