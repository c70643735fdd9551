"""The kernel's contact list (the contact row of gq_batch_set_outputs: QuadrupedEnv.contacts(), or the row the host emulator fills) held to the
fp64 oracle's, contact by contact: one decoder of the row, one comparison (hold_contact_list) shared by tests/test_kernel_emulated.py and
tests/test_gpu_parity.py, and the signed distances (Shapes) that say whether the point of a contact whose position is not determined - two
faces, a face and an edge, parallel edges: every point of the overlap is a valid witness - lies on the contact feature.  TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

from contact_cases import CVX_TOL, PAIR_TOL
from gym_quadruped_amd.accessors import AccessorsMixin
from gym_quadruped_amd.cabi import GQ_CON_MAX
from helpers import oracle_fits_self_budget

FRAME_ORTHO, MU_RTOL = 1e-6, 1e-6
# Tangents: 2e-5 (the accessor test's bound on the flat floor) where the normal is exact on both sides - the floor plane.  Elsewhere the tangents are
# mju_makeFrame of a computed normal and inherit its error, so two things are held: the kernel's tangents are mju_makeFrame (fp64, make_frame below)
# of the kernel's OWN normal to 2e-5 - the construction itself - and they are the oracle's to 4 x 4.09e-5: under one fp32 rounding of the geom poses
# the oracle's own tangents move by up to 4.09e-5 on the six robots whose convex pairs have no two-direction ties (tools/contact_pose_sensitivity.py,
# profiles/contact_list_parity.md); 4 x that movement and no more.
FRAME_TOL, FRAME_TOL_COMPUTED_NORMAL = 2e-5, 4 * 4.09e-5
FIELDS = ('ncon', 'nefc', 'geom1', 'geom2', 'dist', 'pos', 'frame', 'dim', 'force', 'mu')


class _Rows(AccessorsMixin):
    """AccessorsMixin.contacts() over host rows: the record layout stays the product's (gym_quadruped_amd/accessors.py), in one place"""

    def __init__(self, rows):
        import torch
        self._contacts, self.num_envs = torch.as_tensor(np.ascontiguousarray(rows, dtype=np.float32)), len(rows)


def decode_contact_rows(rows):
    """Contact rows [N][GQ_CON_STRIDE] (the row the host emulator fills) through the product's own decoder, AccessorsMixin.contacts(), as host
    arrays: ncon, nefc [N]; per slot geom1 (-1: a world geom), geom2, dist, pos (x / y relative to the pre-step base), frame [3][3], dim, force [6], mu."""
    return contacts_numpy(_Rows(rows).contacts())


def contacts_numpy(con):
    """env.contacts() (tensors on the device) as the host arrays decode_contact_rows returns"""
    return {k: con[k].detach().cpu().numpy() for k in FIELDS}


def contact_env(con, e):
    """env e of either: the mapping hold_contact_list takes"""
    return {k: con[k][e] for k in FIELDS}


def make_frame(n):
    """mju_makeFrame without a tangent hint, fp64: rows normal, tangent 1 (y or z made orthogonal to the normal), tangent 2 = n x t1"""
    n = np.asarray(n, dtype=np.float64) / np.linalg.norm(n)
    t = np.array([0.0, 1.0, 0.0]) if -0.5 < n[1] < 0.5 else np.array([0.0, 0.0, 1.0])
    t = t - (n @ t) * n
    t /= np.linalg.norm(t)
    return np.stack([n, t, np.cross(n, t)])


# ----------------------------------------------------------------------------------------------------------------- signed distances
def _seg_dist(q, a, b):
    ab = b - a
    t = np.clip(((q - a) * ab).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300), 0.0, 1.0)
    return np.linalg.norm(q - (a + t[..., None] * ab), axis=-1)


def _tri_dist(q, A, B, C):
    """distance of the point q to every triangle (A, B, C) [T][3]"""
    n = np.cross(B - A, C - A)
    n /= np.linalg.norm(n, axis=1)[:, None]
    d = ((q - A) * n).sum(1)
    p = q - d[:, None] * n
    inside = np.ones(len(A), bool)
    for U, W in ((A, B), (B, C), (C, A)):
        inside &= (np.cross(W - U, p - U) * n).sum(1) >= 0.0
    edges = np.minimum(np.minimum(_seg_dist(q, A, B), _seg_dist(q, B, C)), _seg_dist(q, C, A))
    return np.where(inside, np.abs(d), edges)


class Shapes:
    """Signed distance of a world point to a collision shape of the model, from the model's own tables: a robot geom is its vertex cloud
    (one vertex: sphere; two: capsule; 8: box; 32: the cylinder's prism; a hull's vertices) inflated by the cloud's radius and placed by the
    geom poses handed in (the oracle's fp64 ones); a world geom is the floor plane z = 0 or a box of the scene."""

    def __init__(self, mm):
        self.md, self.boxes, self._hull = mm.md, list(mm.boxes), {}

    def cloud(self, cl):
        md = self.md
        return np.asarray(md.vert_pos[md.cloud_vertadr[cl]:md.cloud_vertadr[cl] + md.cloud_vertnum[cl]], dtype=np.float64)

    def _hull_of(self, cl):
        if cl not in self._hull:
            from scipy.spatial import ConvexHull
            V = self.cloud(cl)
            h = ConvexHull(V)
            self._hull[cl] = (h.equations.copy(), V[h.simplices[:, 0]], V[h.simplices[:, 1]], V[h.simplices[:, 2]])
        return self._hull[cl]

    def sd_cloud(self, cl, q):
        """signed distance of q (geom frame) to the convex hull of cloud cl: the deepest face plane inside, the closest face outside"""
        V = self.cloud(cl)
        if len(V) == 1:
            return float(np.linalg.norm(q - V[0]))
        if len(V) == 2:
            return float(_seg_dist(q, V[0], V[1]))
        eq, A, B, C = self._hull_of(cl)
        s = float((eq[:, :3] @ q + eq[:, 3]).max())
        return s if s <= 0.0 else float(_tri_dist(q, A, B, C).min())

    def sd_geom(self, g, xpos, xmat, p):
        """robot geom g placed at xpos [3] / xmat [3][3]"""
        cl = int(self.md.geom_cloudid[g])
        return self.sd_cloud(cl, np.asarray(xmat).reshape(3, 3).T @ (np.asarray(p) - xpos)) - float(self.md.cloud_radius[cl])

    def sd_world(self, w, p):
        """world geom w: -1 the floor plane, else box w of the scene"""
        if w < 0:
            return float(p[2])
        from scipy.spatial.transform import Rotation
        assert w < len(self.boxes), f'world geom {w}: the height field has no signed distance here (boxes 0..{len(self.boxes) - 1} and the floor do)'
        b = self.boxes[w]
        R = Rotation.from_quat(np.asarray(b['quat'], float), scalar_first=True).as_matrix()
        d = np.abs(R.T @ (np.asarray(p) - np.asarray(b['pos'], float))) - np.asarray(b['size'], float)
        return float(np.linalg.norm(np.maximum(d, 0.0)) + min(d.max(), 0.0))

    def sd_pair(self, o, c, p):
        """the signed distances of p to the two shapes of the oracle's contact c (after its forward pass or step: the poses of that pass)"""
        g1, g2, w = int(o.get('contact_geom1')[c]), int(o.get('contact_geom')[c]), int(o.get('contact_wgeom')[c])
        xp, xm = o.geom_xpos, o.geom_xmat
        first = self.sd_geom(g1, xp[g1], xm[g1], p) if g1 >= 0 else self.sd_world(w, p)
        return first, self.sd_geom(g2, xp[g2], xm[g2], p)

    def _world_verts(self, o, c):
        """the vertices (and inflation radii) of the two shapes of the oracle's contact c: a robot geom's cloud, a world box's corners"""
        g1, g2, w = int(o.get('contact_geom1')[c]), int(o.get('contact_geom')[c]), int(o.get('contact_wgeom')[c])
        md, xp, xm = self.md, o.geom_xpos, o.geom_xmat
        geom = lambda g: (self.cloud(int(md.geom_cloudid[g])) @ xm[g].T + xp[g], float(md.cloud_radius[md.geom_cloudid[g]]))
        if g1 >= 0:
            return geom(g1), geom(g2)
        from scipy.spatial.transform import Rotation
        assert 0 <= w < len(self.boxes), f'world geom {w}: only the boxes of the scene have vertices here (not the floor, not the height field)'
        b = self.boxes[w]
        R = Rotation.from_quat(np.asarray(b['quat'], float), scalar_first=True).as_matrix()
        corners = np.array([[i, j, k] for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)], float) * np.asarray(b['size'], float)
        return (corners @ R.T + np.asarray(b['pos'], float), 0.0), geom(g2)

    def penetrating_polytopes(self, o, c):
        """Is contact c a pair of polytopes without inflation radius that penetrate?  Only then is the overlap along a direction piecewise linear
        in the direction, so that equal overlap along a second direction that is a local minimum proves a second minimum translation."""
        (A, ra), (B, rb) = self._world_verts(o, c)
        return ra == 0.0 and rb == 0.0 and len(A) >= 4 and len(B) >= 4 and float(o.get('contact_dist')[c]) < -CVX_TOL['dist']

    def depth_along(self, o, c, n):
        """the separation of the two shapes of contact c along the unit direction n (first shape -> second): the distance of the convex pair is
        the maximum of this over all directions when they are apart, and minus the least overlap when they penetrate"""
        (A, ra), (B, rb) = self._world_verts(o, c)
        return float((B @ n).min() - rb - (A @ n).max() - ra)

    def on_feature(self, o, c, p, dist):
        """(b): p lies on the contact feature - within half the depth (+ CVX_TOL['pos']) of both shapes.  Returns (holds, the two distances)."""
        sd = self.sd_pair(o, c, p)
        return max(sd) <= 0.5 * abs(dist) + CVX_TOL['pos'], sd


# ----------------------------------------------------------------------------------------------------------------- the comparison
class ListStats:
    """Worst per-contact errors seen by hold_contact_list and what it counted, for the tallies of profiles/contact_list_parity.md"""

    def __init__(self):
        self.worst = dict(dist_cvx=0.0, dist_prim=0.0, angle_deg=0.0, nrm_prim=0.0, tangent=0.0, tangent_own=0.0, pos_cvx=0.0, pos_prim=0.0, midplane=0.0, feature=-1.0, force=0.0)
        self.n = dict(contacts=0, cvx=0, undetermined=0, vertex_tie=0, normal_tie=0, capped=0, undetermined_moved=0)

    def see(self, key, v):
        self.worst[key] = max(self.worst[key], float(v))

    def line(self, what):
        return f'contact lists {what}: ' + ', '.join(f'{k} {v}' for k, v in self.n.items()) + '; worst ' + ', '.join(f'{k} {v:.2e}' for k, v in self.worst.items())


def hold_contact_list(o, con, base_xy, shapes, cone, tie_threshold, e=None, stats=None):
    """Hold the kernel's contact list of one env (`con`: contact_env's mapping) to the oracle's after the oracle has stepped from the same
    state.  base_xy: the pre-step base x / y the row's points are relative to.  An env whose oracle set fits the kernel's budget: every
    contact; an over-budget env: the kernel's contacts against the oracle's first ncon_kernel (the prefix rule).  Per contact: geoms, dim
    (equal), mu, dist, the frame, and the point - or, where the point is not determined, its component along the normal and that it lies
    on the contact feature.  Contacts of a pair the convex routine capped (tiegap == 0) are held to capped_dist only and counted.

    A convex normal further than CVX_TOL['angle_deg'] from the oracle's is accepted in one case only: two polytopes without inflation radius
    that PENETRATE (the overlap is then piecewise linear in the direction - for cores that are apart it falls off like a cosine, and equal
    overlap would prove nothing), whose minimum translation has two directions of equal depth, of which the kernel took the other - the
    shapes, placed by the oracle's fp64 poses, overlap along the kernel's normal by the oracle's depth to CVX_TOL['dist'] (Shapes.depth_along)
    AND no tilt of 0.1 degree away from it lessens the overlap.  The callers bound how many such contacts a robot may have.  (Regular
    prisms - go1's cylinder geoms - meet such ties by symmetry: under one fp32 rounding of its geom poses the oracle's own normal jumps
    between the two, profiles/contact_list_parity.md.)  Its point is then held to the contact feature.

    Returns {contact: (the kernel's world point, the kernel's normal or None)} for the contacts the oracle has to take from the kernel
    before the env can be compared by value: a point below the tie threshold, such a normal."""
    stats = stats if stats is not None else ListStats()
    nk = int(con['ncon'])
    if oracle_fits_self_budget(o, cone):
        assert nk == o.ncon, (e, 'contacts', nk, o.ncon)
    else:
        assert nk <= o.ncon and nk <= GQ_CON_MAX, (e, 'contacts of an over-budget env', nk, o.ncon)
    if nk == 0:
        return {}
    get = lambda name: o.get(name)[:nk]
    assert (con['geom1'][:nk] == get('contact_geom1').astype(int)).all() and (con['geom2'][:nk] == get('contact_geom').astype(int)).all(), \
        (e, 'geoms', con['geom1'][:nk], con['geom2'][:nk], get('contact_geom1'), get('contact_geom'))
    assert (con['dim'][:nk] == get('contact_dim').astype(int)).all(), (e, 'dim', con['dim'][:nk], get('contact_dim'))
    mu = o.get('contact_friction').reshape(-1, 5)[:nk, 0]   # the row's last word is mjContact.friction[0] (include/gq.h), not the regularised mjContact.mu
    assert (np.abs(con['mu'][:nk] - mu) <= MU_RTOL * np.abs(mu)).all(), (e, 'mu', con['mu'][:nk], mu)
    gap, cvx, dist_o = get('contact_tiegap'), get('contact_cvx').astype(bool), get('contact_dist')
    on_floor = (get('contact_geom1') < 0) & (get('contact_wgeom') == -1.0)
    pos_o, frame_o = o.contact_pos[:nk], o.contact_frame[:nk]
    pos_k = np.asarray(con['pos'][:nk], dtype=np.float64).copy()
    pos_k[:, :2] += np.asarray(base_xy, dtype=np.float64)
    scale = max(1.0, np.abs(o.contact_pos).max())
    subst = {}
    for c in range(nk):
        stats.n['contacts'] += 1; stats.n['cvx'] += int(cvx[c])
        capped = bool(cvx[c]) and gap[c] == 0.0
        undetermined = gap[c] == -1.0
        vertex_tie = not capped and not undetermined and gap[c] < tie_threshold
        if gap[c] < tie_threshold:
            subst[c] = (pos_k[c], None)
        dk, fk = float(con['dist'][c]), np.asarray(con['frame'][c], dtype=np.float64)
        tol = CVX_TOL['capped_dist'] if capped else (CVX_TOL['dist'] if cvx[c] else PAIR_TOL['dist']) + (tie_threshold if vertex_tie else 0.0)
        if not capped:
            stats.see('dist_cvx' if cvx[c] else 'dist_prim', abs(dk - dist_o[c]))
        assert abs(dk - dist_o[c]) < tol, (e, c, 'dist', dk, dist_o[c], gap[c])
        assert np.abs(fk @ fk.T - np.eye(3)).max() < FRAME_ORTHO, (e, c, 'frame not orthonormal', fk)
        if capped:   # the shared iteration cap: both sides hold the state of an unfinished iteration - normal and point are skipped, and counted
            stats.n['capped'] += 1
            continue
        normal_tie = False
        if cvx[c]:
            ang = np.degrees(np.arccos(np.clip(fk[0] @ frame_o[c][0], -1.0, 1.0)))
            if ang > CVX_TOL['angle_deg']:   # accepted only as the other of two minimum translations of penetrating polytopes
                assert shapes.penetrating_polytopes(o, c), (e, c, 'normal', fk[0], frame_o[c][0], ang)
                along = shapes.depth_along(o, c, fk[0])
                assert abs(along - dist_o[c]) < CVX_TOL['dist'], (e, c, 'normal: not a direction of minimum depth', fk[0], frame_o[c][0], along, dist_o[c])
                for t in (fk[1], fk[2], fk[1] + fk[2], fk[1] - fk[2]):   # ... and a local minimum of the overlap: no tilt of 0.1 deg lessens it
                    for sgn in (-1.0, 1.0):
                        nt = fk[0] + sgn * np.radians(CVX_TOL['angle_deg']) * t / np.linalg.norm(t)
                        tilted = shapes.depth_along(o, c, nt / np.linalg.norm(nt))
                        assert tilted <= along + 1e-9, (e, c, 'normal: not a local minimum of the overlap', fk[0], frame_o[c][0], tilted, along)
                normal_tie = True
                stats.n['normal_tie'] += 1
                subst[c] = (pos_k[c], fk[0])
            else:
                stats.see('angle_deg', ang)
        else:
            stats.see('nrm_prim', np.abs(fk[0] - frame_o[c][0]).max())
            assert np.abs(fk[0] - frame_o[c][0]).max() <= PAIR_TOL['nrm'], (e, c, 'normal', fk[0], frame_o[c][0])
        if not on_floor[c] and abs(abs(fk[0][1]) - 0.5) > 1e-4:   # (at |n_y| = 0.5 mju_makeFrame changes its reference axis)
            stats.see('tangent_own', np.abs(fk - make_frame(fk[0])).max())
            assert np.abs(fk - make_frame(fk[0])).max() <= FRAME_TOL, (e, c, 'tangents are not mju_makeFrame of the normal', fk)
        straddle = (abs(fk[0][1]) - 0.5) * (abs(frame_o[c][0][1]) - 0.5) <= 0.0   # (the two normals on either side of mju_makeFrame's switch of axis)
        if not normal_tie and not straddle:
            stats.see('tangent', np.abs(fk[1:] - frame_o[c][1:]).max())
            assert np.abs(fk[1:] - frame_o[c][1:]).max() <= (FRAME_TOL if on_floor[c] else FRAME_TOL_COMPUTED_NORMAL), (e, c, 'tangents', fk, frame_o[c])
        if undetermined or vertex_tie or normal_tie:
            stats.n['undetermined' if undetermined else 'vertex_tie'] += int(not normal_tie)
            if undetermined and not normal_tie:   # (a) the midplane is determined
                along = abs(frame_o[c][0] @ (pos_k[c] - pos_o[c]))
                stats.see('midplane', along)
                assert along <= CVX_TOL['pos'], (e, c, 'point off the midplane', pos_k[c], pos_o[c])
                stats.n['undetermined_moved'] += int(np.linalg.norm(pos_k[c] - pos_o[c]) > CVX_TOL['pos'] * scale)
            ok, sd = shapes.on_feature(o, c, pos_k[c], dist_o[c])   # (b) on the contact feature
            stats.see('feature', max(sd) - 0.5 * abs(dist_o[c]))
            assert ok, (e, c, 'point off the contact feature', pos_k[c], sd, dist_o[c])
        elif cvx[c]:
            stats.see('pos_cvx', np.linalg.norm(pos_k[c] - pos_o[c]) / scale)
            assert np.linalg.norm(pos_k[c] - pos_o[c]) < CVX_TOL['pos'] * scale, (e, c, 'point', pos_k[c], pos_o[c])
        else:
            stats.see('pos_prim', np.abs(pos_k[c] - pos_o[c]).max() / scale)
            assert np.abs(pos_k[c] - pos_o[c]).max() <= PAIR_TOL['pos'] * scale, (e, c, 'point', pos_k[c], pos_o[c])
    return subst


def hold_contact_forces(o, con, tol, e=None, mass=0.0, stats=None):
    """mj_contactForce of the row against the oracle's, under the tolerance the caller's set gives efc_force; the slots past the list are zero"""
    nk = int(con['ncon'])
    assert nk == o.ncon, (e, nk, o.ncon)
    if nk:
        if stats is not None:
            stats.see('force', np.abs(con['force'][:nk] - o.contact_force).max() / max(1.0, np.abs(o.contact_force).max()))
        tol.check(con['force'][:nk], o.contact_force, (e, 'contact force'), mass)
    assert not np.asarray(con['force'][nk:]).any(), (e, 'force past the list')
