"""Physical invariants that pin the CPU oracle's mj_step restatement (MuJoCo itself is unavailable)."""
import numpy as np
import pytest

from helpers import marshalled, random_states
from gym_quadruped_amd.mjcf import mass_matrix_dense
from oracle.oracle import Oracle

ROBOTS = ['mini_cheetah', 'aliengo', 'hyqreal2', 'b2', 'go1', 'go2', 'hyqreal1', 'spot']
ELLIPTIC = ['go1', 'go2', 'hyqreal1', 'spot']   # cone="elliptic" impratio=100; go1 / go2 / spot feet are condim 6


def _state(md, rng, z=1.0):
    q = md.key_qpos[0].copy() if len(md.key_qpos) else md.qpos0.copy()
    q[7:] += rng.uniform(-0.3, 0.3, 12)
    q[2] = z
    quat = rng.normal(size=4)
    q[3:7] = quat / np.linalg.norm(quat)
    return q, rng.normal(size=18)


@pytest.mark.parametrize('robot', ROBOTS)
def test_mass_matrix_equals_independent_formulation(robot):
    mm = marshalled(robot, solver=1)
    o = Oracle(mm)
    rng = np.random.default_rng(0)
    import copy
    md2 = copy.deepcopy(mm.md)
    md2.qpos0 = np.array([mm.desc.qpos0[i] for i in range(19)])
    for _ in range(5):
        q, v = _state(mm.md, rng)
        o.set_state(q, v, np.zeros(18), np.zeros(18))
        o.forward(np.zeros(12))
        Mref, _, _ = mass_matrix_dense(md2, q)   # sum_b J_b' I_b J_b, no CRBA
        np.testing.assert_allclose(o.M, Mref, rtol=1e-10, atol=1e-12)
        assert np.linalg.eigvalsh(o.M).min() > 0


@pytest.mark.parametrize('robot', ROBOTS)
def test_free_fall_and_gravity_torque(robot):
    mm = marshalled(robot, solver=1)
    md, o = mm.md, Oracle(mm)
    rng = np.random.default_rng(1)
    q, _ = _state(md, rng, z=2.0)
    o.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18))
    o.forward(np.zeros(12))
    assert o.ncon == 0
    np.testing.assert_allclose(o.qacc[:3], [0, 0, -9.81], atol=1e-9)     # base falls with g
    np.testing.assert_allclose(o.qacc[3:], 0, atol=1e-8)                 # no relative motion starts
    bias = o.qfrc_bias.copy()
    assert abs(bias[2] - md.total_mass * 9.81) < 1e-8                    # weight on the base z dof

    def U(qq):
        o.set_state(qq, np.zeros(18), np.zeros(18), np.zeros(18)); o.forward(np.zeros(12), stage=1)
        return 9.81 * np.sum(md.body_mass * o.xipos[:, 2])
    for i in range(12):                                                  # RNE(q,0,0) = dU/dq
        dq = np.zeros(19); dq[7 + i] = 1e-6
        assert abs((U(q + dq) - U(q - dq)) / 2e-6 - bias[6 + i]) < 1e-6


def test_momentum_in_flight():
    """No contacts: joint damping/friction/actuation are internal -> d(p)/dt = m g exactly, integrated by Euler."""
    mm = marshalled('mini_cheetah', solver=1, iterations=100, tolerance=1e-12)
    md, o = mm.md, Oracle(mm)
    rng = np.random.default_rng(2)
    q, v = _state(md, rng, z=3.0)
    o.set_state(q, v, np.zeros(18), np.zeros(18))

    def momentum():
        o.forward(np.zeros(12), stage=1)
        cv, xi, sc = o.cvel, o.xipos, o.subtree_com[1]
        return sum(md.body_mass[b] * (cv[b, 3:] + np.cross(cv[b, :3], xi[b] - sc)) for b in range(1, md.nbody))
    p0 = momentum()
    nstep = 50
    for _ in range(nstep):
        o.step(rng.normal(0, 10, 12))
    p1 = momentum()
    np.testing.assert_allclose(p1 - p0, [0, 0, -md.total_mass * 9.81 * nstep * 0.002], atol=2e-2)


@pytest.mark.parametrize('robot', ['mini_cheetah', 'aliengo', 'go2', 'hyqreal1'])
def test_static_stance_carries_the_weight(robot):
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-10)
    md, o = mm.md, Oracle(mm)
    q = md.key_qpos[0].copy()
    o.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18))
    for _ in range(4000):
        o.step(np.zeros(12))
    fn = []
    for _ in range(200):   # the unactuated robot may still be creeping: average the normal force
        o.step(np.zeros(12)); fn.append(o.contact_force[:o.ncon, 0][o.contact_geom1[:o.ncon] < 0].sum())   # (contacts with the WORLD: robot-robot forces are internal)
    assert np.abs(o.qvel).max() < 1.0
    assert abs(np.mean(fn) - md.total_mass * 9.81) < 0.03 * md.total_mass * 9.81


def test_pgs_converges_to_newton_solution():
    """Both solve the same strictly convex problem: forces and qacc must agree once PGS has converged."""
    rng = np.random.default_rng(3)
    mmN = marshalled('mini_cheetah', solver=1, iterations=100, tolerance=1e-12)
    mmP = marshalled('mini_cheetah', solver=0, iterations=20000, tolerance=1e-14)
    oN, oP = Oracle(mmN), Oracle(mmP)
    qpos, qvel = random_states(mmN.md, 12, rng)
    seen_contact = 0
    for e in range(12):
        ctrl = rng.normal(0, 20, 12)
        for o in (oN, oP):
            o.set_state(qpos[e], qvel[e], np.zeros(18), np.zeros(18)); o.forward(ctrl)
        seen_contact += oN.ncon > 0
        assert np.abs(oN.qacc - oP.qacc).max() < 1e-5 * max(1, np.abs(oN.qacc).max())
        # constraint-space optimality of the Newton solution: KKT residual of the dual
        f, R, J = oN.efc_force, oN.efc_R, oN.efc_J
        jar = J @ oN.qacc - oN.efc_aref
        t = oN.get('efc_type')
        fl = oN.efc_frictionloss
        for i in range(oN.nefc):
            if t[i] == 0:
                expect = np.clip(-jar[i] / R[i], -fl[i], fl[i])
            else:
                expect = max(0.0, -jar[i] / R[i])
            assert abs(f[i] - expect) < 1e-6 * max(1, abs(expect))
    assert seen_contact >= 4


def test_contact_forces_oppose_penetration_and_respect_friction_cone():
    mm = marshalled('mini_cheetah', solver=1, iterations=100, tolerance=1e-10)
    o = Oracle(mm)
    rng = np.random.default_rng(4)
    qpos, qvel = random_states(mm.md, 30, rng, z_range=(0.15, 0.3))
    n = 0
    for e in range(30):
        o.set_state(qpos[e], qvel[e], np.zeros(18), np.zeros(18), friction=0.7); o.forward(rng.normal(0, 10, 12))
        cf = o.contact_force
        for c in range(o.ncon):
            n += 1
            assert cf[c, 0] >= -1e-9
            mu = 0.7 if o.contact_geom[c] in [mm.md.geom_names.index(k) for k in ('FL', 'FR', 'RL', 'RR')] else 0.7
            assert abs(cf[c, 1]) <= mu * cf[c, 0] + 1e-7 and abs(cf[c, 2]) <= mu * cf[c, 0] + 1e-7
    assert n > 20


@pytest.mark.parametrize('robot', ELLIPTIC)
def test_elliptic_cone_solution_is_optimal_and_inside_the_cone(robot):
    """Elliptic friction cones (mj_constraintUpdate, mjCNSTR_CONTACT_ELLIPTIC): the Newton iterate must (i) zero the
    gradient M (qacc - qacc_smooth) - J' f, (ii) be a minimiser of the primal objective (no random perturbation lowers
    it), (iii) give contact forces inside the elliptic cone f_n >= 0, sum_j (f_j / friction_j)^2 <= f_n^2 - the
    cost's middle zone is exactly the dual of the projection onto that cone - and (iv) regularise the friction
    dimensions with R_j = R_n mu^2 / friction_j^2, mu = friction_0 / sqrt(impratio)."""
    mm = marshalled(robot, solver=1, iterations=200, tolerance=1e-14)
    md, o = mm.md, Oracle(mm)
    assert md.cone == 1
    rng = np.random.default_rng(7)
    qpos, qvel = random_states(md, 24, rng, z_range=(0.6 * mm.desc.key_qpos[2], 1.05 * mm.desc.key_qpos[2]))
    ncon = nmiddle = 0
    for e in range(24):
        o.set_state(qpos[e], qvel[e] * 0.5, np.zeros(18), np.zeros(18), friction=0.6 if e % 2 else -1.0)
        o.forward(rng.normal(0, 10, 12))
        if o.ncon == 0:
            continue
        J, f, R = o.efc_J, o.efc_force, o.efc_R
        grad = o.M @ (o.qacc - o.qacc_smooth) - J.T @ f
        assert np.abs(grad).max() < 1e-6 * max(1.0, np.abs(J.T @ f).max())
        c0 = o.primal_cost(o.qacc)
        for _ in range(20):
            d = rng.normal(size=18) * 10.0 ** rng.uniform(-4, -1)
            assert o.primal_cost(o.qacc + d) >= c0 - 1e-9 * max(1.0, abs(c0))
        dims, adr, fri, mu = o.get('contact_dim').astype(int), o.get('contact_efc_address').astype(int), o.get('contact_friction').reshape(-1, 5), o.get('contact_mu')
        cf = o.contact_force
        for c in range(o.ncon):
            ncon += 1
            a, dim = adr[c], dims[c]
            if dim == 1:
                continue
            assert abs(mu[c] - fri[c, 0] / np.sqrt(md.impratio)) < 1e-15
            np.testing.assert_allclose(R[a + 1:a + dim], R[a] * mu[c] ** 2 / fri[c, :dim - 1] ** 2, rtol=1e-12)
            fn, ft = f[a], f[a + 1:a + dim]
            np.testing.assert_allclose(cf[c, :dim], f[a:a + dim])           # mj_contactForce is the identity for elliptic rows
            assert fn >= -1e-12
            assert np.sqrt(np.sum((ft / fri[c, :dim - 1]) ** 2)) <= fn * (1 + 1e-9) + 1e-12
            nmiddle += fn > 1e-9 and np.sqrt(np.sum((ft / fri[c, :dim - 1]) ** 2)) > fn * (1 - 1e-6)   # on the cone surface: sliding
    assert ncon >= 10 and nmiddle >= 1


def test_elliptic_stance_weight_and_cone_at_rest():
    """hyqreal1 (elliptic, condim 3) dropped on its feet and left to settle: the floor carries the weight and every
    contact force stays inside its cone (the unactuated legs splay, so the tangential forces are large)."""
    mm_e = marshalled('hyqreal1', solver=1, iterations=200, tolerance=1e-12)
    oe = Oracle(mm_e)
    oe.set_state(mm_e.md.key_qpos[0].copy(), np.zeros(18), np.zeros(18), np.zeros(18))
    for _ in range(3000):
        oe.step(np.zeros(12))
    fz = oe.contact_force[:oe.ncon, 0][oe.contact_geom1[:oe.ncon] < 0].sum()   # (contacts with the world: robot-robot forces are internal)
    assert abs(fz - mm_e.md.total_mass * 9.81) < 0.05 * mm_e.md.total_mass * 9.81
    fri = oe.get('contact_friction').reshape(-1, 5)
    cf = oe.contact_force
    for c in range(oe.ncon):
        assert np.hypot(cf[c, 1] / fri[c, 0], cf[c, 2] / fri[c, 1]) <= cf[c, 0] * (1 + 1e-9) + 1e-9


def _slab(z_top, half=(6.0, 6.0, 1.0), pos_xy=(0.0, 0.0), euler=(0.0, 0.0, 0.0)):
    from gym_quadruped_amd.terrain import _box
    return _box([pos_xy[0], pos_xy[1], z_top - half[2]], euler, [2 * h for h in half])


@pytest.mark.parametrize('robot', ['mini_cheetah', 'aliengo', 'go2'])
def test_world_box_top_face_is_a_raised_floor(robot):
    """World boxes (terrain.py add_box): a wide slab whose top face is at height H under the robot must give exactly the
    dynamics of the floor plane H lower - same distances, frames (normal +z), mixing with default geom parameters."""
    H = 1.37   # thick slab: random test states sink up to 0.1 m into the ground, the top face must stay the nearest one
    mmF = marshalled(robot, solver=1, iterations=100, tolerance=1e-12)
    mmB = marshalled(robot, solver=1, iterations=100, tolerance=1e-12, boxes=[_slab(H)])
    oF, oB = Oracle(mmF), Oracle(mmB)
    rng = np.random.default_rng(9)
    hip = float(mmF.desc.key_qpos[2])
    qpos, qvel = random_states(mmF.md, 40, rng, z_range=(0.7 * hip, 1.3 * hip))
    ncon = 0
    for e in range(40):
        ctrl = rng.normal(0, 10, 12)
        oF.set_state(qpos[e], qvel[e], np.zeros(18), np.zeros(18)); oF.step(ctrl)
        qb = qpos[e].copy(); qb[2] += H
        oB.set_state(qb, qvel[e], np.zeros(18), np.zeros(18)); oB.step(ctrl)
        if oF.ncon and len(set(oF.get('contact_geom').astype(int))) != oF.ncon:
            continue   # a link geom lies on the floor with several contact points (plane routines); a box pair yields one
        assert oB.ncon == oF.ncon
        ncon += oF.ncon
        np.testing.assert_allclose(oB.qacc, oF.qacc, rtol=1e-7, atol=1e-7 * max(1, np.abs(oF.qacc).max()))
        np.testing.assert_allclose(oB.get('contact_dist'), oF.get('contact_dist'), atol=1e-12)
        np.testing.assert_allclose(oB.contact_frame, oF.contact_frame, atol=1e-12)
    assert ncon > 0


def test_world_box_side_face_and_ramp_normals():
    """Sphere-box narrow phase: a foot next to a box is pushed out through the nearest face (horizontal normal for a side
    face), a foot on a tilted ramp gets the ramp's normal; forces respect the friction pyramid in the contact frame."""
    from gym_quadruped_amd.terrain import generate_terrain
    scene, _ = generate_terrain('ramp', 0.3)
    mm = marshalled('aliengo', solver=1, iterations=200, tolerance=1e-12, boxes=scene['boxes'])
    o = Oracle(mm)
    b = scene['boxes'][0]
    from scipy.spatial.transform import Rotation
    Rb = Rotation.from_quat(np.asarray(b['quat'], float) / np.linalg.norm(b['quat']), scalar_first=True).as_matrix()
    n_top = Rb[:, 2]
    q = mm.md.key_qpos[0].copy()
    # put the robot on the ramp surface: 1 m up-slope of the ramp centre, base raised along the ramp normal
    p_on = np.asarray(b['pos']) + Rb @ np.array([1.0, 0.0, b['size'][2]])
    q[0:3] = p_on + np.array([0, 0, float(mm.desc.key_qpos[2]) * 1.5])
    o.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18)); o.forward(np.zeros(12), stage=1)
    # lower the robot until its deepest foot sinks 2 mm into the ramp (the ramp slab is only 5 cm thick)
    top = np.asarray(b['pos']) + Rb @ np.array([0.0, 0.0, b['size'][2]])
    feet = [mm.md.geom_names.index(k) for k in ('FL', 'FR', 'RL', 'RR')]
    rad = float(mm.md.cloud_radius[mm.md.geom_cloudid[feet[0]]])
    dmin = min(float(n_top @ (o.geom_xpos[g] - top)) - rad for g in feet)
    q[2] -= (dmin + 0.002) / n_top[2]
    o.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18)); o.forward(np.zeros(12))
    assert o.ncon >= 2
    fr = o.contact_frame
    cf = o.contact_force
    for c in range(o.ncon):
        np.testing.assert_allclose(fr[c] @ fr[c].T, np.eye(3), atol=1e-12)
        assert fr[c][0] @ n_top > 0.999                      # ramp normal, not the world z axis
        assert abs(fr[c][0][2] - 1.0) > 1e-3
        assert cf[c, 0] >= -1e-9 and abs(cf[c, 1]) <= cf[c, 0] + 1e-6 and abs(cf[c, 2]) <= cf[c, 0] + 1e-6
    # a foot beside a tall box: nearest face is a side face -> horizontal normal
    tall = _slab(1.0, half=(0.2, 0.2, 0.5), pos_xy=(0.0, 0.0))
    mm2 = marshalled('aliengo', solver=1, iterations=100, tolerance=1e-10, boxes=[tall])
    o2 = Oracle(mm2)
    q = mm2.md.key_qpos[0].copy(); q[2] = 0.6
    o2.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18)); o2.forward(np.zeros(12), stage=1)
    foot = o2.geom_xpos[mm2.md.geom_names.index('FL')]
    q[0] += -foot[0] + 0.2 + 0.02                               # FL foot centre 2 cm outside the +x face
    q[1] += -foot[1]
    o2.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18)); o2.forward(np.zeros(12))
    normals = o2.contact_frame[:, 0]
    assert any(abs(nv[0] - 1.0) < 1e-9 and abs(nv[2]) < 1e-9 for nv in normals), normals


def _plane_hfield(H=0.0, slope=0.0, half=6.0, n=33, elevation=1.0):
    """Height field whose samples lie on the plane z = H + slope * (x + half) (data in [0, 1] x elevation)."""
    x = np.linspace(-half, half, n)
    data = np.tile(slope * (x + half) / elevation, (n, 1)).astype(np.float32)
    assert data.max() <= 1.0
    return dict(data=data, size=(half, half, elevation, 0.01), pos=(0.0, 0.0, H))


@pytest.mark.parametrize('robot', ['aliengo', 'hyqreal1'])
def test_flat_height_field_is_a_raised_floor(robot):
    """A height field with constant elevation H under the robot must give exactly the dynamics of the floor plane H lower
    (sphere-triangle and vertex-plane distances degenerate to the plane's, normal +z, default geom parameters)."""
    H = 1.37
    # (mesh_graph off: a mesh keeps ONE contact with the height field, so the floor side is held to its support vertex as well)
    mmF = marshalled(robot, solver=1, iterations=100, tolerance=1e-12, mesh_graph=False)
    mmH = marshalled(robot, solver=1, iterations=100, tolerance=1e-12, hfield=_plane_hfield(H), mesh_graph=False)
    oF, oH = Oracle(mmF), Oracle(mmH)
    rng = np.random.default_rng(19)
    hip = float(mmF.desc.key_qpos[2])
    qpos, qvel = random_states(mmF.md, 40, rng, z_range=(0.7 * hip, 1.3 * hip))
    ncon = 0
    for e in range(40):
        ctrl = rng.normal(0, 10, 12)
        oF.set_state(qpos[e], qvel[e], np.zeros(18), np.zeros(18)); oF.step(ctrl)
        qb = qpos[e].copy(); qb[2] += H
        oH.set_state(qb, qvel[e], np.zeros(18), np.zeros(18)); oH.step(ctrl)
        if oF.ncon and len(set(oF.get('contact_geom').astype(int))) != oF.ncon:
            continue   # a box / capsule lies on the floor with several contact points; the height-field pair yields one
        assert oH.ncon == oF.ncon
        ncon += oF.ncon
        np.testing.assert_allclose(oH.qacc, oF.qacc, rtol=1e-6, atol=1e-6 * max(1, np.abs(oF.qacc).max()))
        np.testing.assert_allclose(oH.get('contact_dist'), oF.get('contact_dist'), atol=1e-9)
        np.testing.assert_allclose(oH.contact_frame, oF.contact_frame, atol=1e-9)
    assert ncon > 0


def test_sloped_height_field_normals_and_cone():
    """Feet on a height field that is one tilted plane: every contact carries the plane's normal and the sphere's distance
    to it; the forces stay inside the friction pyramid of that frame; a ridge (two planes meeting) is met at its edge."""
    s = 0.25
    mm = marshalled('aliengo', solver=1, iterations=200, tolerance=1e-12, hfield=_plane_hfield(0.5, s, elevation=4.0))
    o = Oracle(mm)
    n_pl = np.array([-s, 0.0, 1.0]) / np.sqrt(1 + s * s)
    q = mm.md.key_qpos[0].copy()
    q[0:2] = (0.37, -0.21)
    q[2] = 3.0
    o.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18)); o.forward(np.zeros(12), stage=1)
    feet = [mm.md.geom_names.index(k) for k in ('FL', 'FR', 'RL', 'RR')]
    rad = float(mm.md.cloud_radius[mm.md.geom_cloudid[feet[0]]])
    p0 = np.array([-6.0, 0.0, 0.5])                                    # a point of the plane
    dmin = min(float(n_pl @ (o.geom_xpos[g] - p0)) - rad for g in feet)
    q[2] -= (dmin + 0.002) / n_pl[2]
    o.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18)); o.forward(np.zeros(12))
    assert o.ncon >= 2
    fr, cf, dist = o.contact_frame, o.contact_force, o.get('contact_dist')
    geoms = o.get('contact_geom').astype(int)
    for c in range(o.ncon):
        np.testing.assert_allclose(fr[c][0], n_pl, atol=1e-9)
        if geoms[c] in feet:
            np.testing.assert_allclose(dist[c], n_pl @ (o.geom_xpos[geoms[c]] - p0) - rad, atol=1e-9)
        assert cf[c, 0] >= -1e-9 and abs(cf[c, 1]) <= cf[c, 0] + 1e-6 and abs(cf[c, 2]) <= cf[c, 0] + 1e-6
    # ridge: z = 1 - |x| sampled on the grid (apex on a grid line): a sphere above the apex touches the edge, normal +z
    x = np.linspace(-2.0, 2.0, 41)
    ridge = dict(data=np.tile(1.0 - np.abs(x) / 2.0, (41, 1)).astype(np.float32), size=(2.0, 2.0, 2.0, 0.01), pos=(0.0, 0.0, 0.0))
    mm2 = marshalled('aliengo', solver=1, iterations=100, tolerance=1e-10, hfield=ridge)
    o2 = Oracle(mm2)
    q = mm2.md.key_qpos[0].copy(); q[2] = 3.0
    o2.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18)); o2.forward(np.zeros(12), stage=1)
    foot = o2.geom_xpos[mm2.md.geom_names.index('FL')]
    q[0] -= foot[0]                                                    # FL foot centre exactly above the ridge line x = 0
    q[2] -= foot[2] - (2.0 + rad - 0.001)                              # 1 mm into the apex (height 2 at x = 0)
    o2.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18)); o2.forward(np.zeros(12))
    c = list(o2.get('contact_geom').astype(int)).index(mm2.md.geom_names.index('FL'))
    np.testing.assert_allclose(o2.contact_frame[c][0], [0, 0, 1], atol=1e-9)
    np.testing.assert_allclose(o2.get('contact_dist')[c], -0.001, atol=1e-9)


def _lying_states(md, n, rng, z):
    """Random orientations at low height: trunk, hips and thighs reach the floor (what the plane routines for boxes,
    capsules and cylinders are for)."""
    from scipy.spatial.transform import Rotation
    q = np.tile(md.key_qpos[0], (n, 1))
    q[:, 7:] += rng.uniform(-0.5, 0.5, (n, 12))
    q[:, 2] = rng.uniform(*z, n)
    q[:, 3:7] = Rotation.random(n, random_state=int(rng.integers(1 << 30))).as_quat(scalar_first=True)
    return q


@pytest.mark.parametrize('robot', ['aliengo', 'go1', 'go2', 'b2', 'hyqreal2'])
def test_plane_routines_against_brute_force_geometry(robot):
    """mjraw_PlaneBox / PlaneCapsule / mjc_PlaneCylinder as restated in gqo_collision, checked against the geometry itself:
    every contact point lies on its geom's surface at the stated distance; a box reports exactly its corners at or below the
    centre that are inside the margin (at most 4); a capsule both end spheres inside the margin, +axis end first, frame
    tangent = the axis projected onto the floor; a cylinder's first point is the lowest point of a densely sampled rim, the
    second the point under it on the other cap, the last two the other corners of the near cap's inscribed triangle."""
    mm = marshalled(robot, solver=1, self_collision=False)
    md, o = mm.md, Oracle(mm)
    rng = np.random.default_rng(17)
    hip = float(mm.desc.key_qpos[2])
    Q = _lying_states(md, 300, rng, (0.05, 0.6 * hip))
    seen = {3: 0, 5: 0, 6: 0}
    multi = {3: 0, 5: 0, 6: 0}
    for q in Q:
        o.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18)); o.forward(np.zeros(12), stage=1)
        if not o.ncon:
            continue
        geoms, dist = o.get('contact_geom').astype(int), o.get('contact_dist')
        pos, frame = o.contact_pos, o.contact_frame
        gx, gm = o.geom_xpos, o.geom_xmat
        world = o.get('contact_geom1') < 0
        for g in np.unique(geoms[world]):
            t = int(md.geom_type[g])
            if t not in seen:
                continue
            idx = np.nonzero((geoms == g) & world)[0]
            assert len(idx) <= (2 if t == 3 else 4) and np.all(np.diff(idx) == 1)
            seen[t] += 1; multi[t] += len(idx) > 1
            R, c = gm[g], gx[g]
            margin = max(md.geom_margin[g], 0.0)
            cl = md.geom_cloudid[g]
            V = md.vert_pos[md.cloud_vertadr[cl]:md.cloud_vertadr[cl] + md.cloud_vertnum[cl]]
            assert np.allclose(frame[idx, 0], [0, 0, 1])
            # the surface point of every contact: midway point pushed back by dist / 2
            surf = pos[idx] + np.outer(0.5 * dist[idx], [0, 0, 1])
            np.testing.assert_allclose(surf[:, 2], dist[idx], atol=1e-12)
            if t == 6:
                corners = c + V @ R.T
                want = [i for i in range(8) if corners[i, 2] <= c[2] and corners[i, 2] < margin][:4]
                np.testing.assert_allclose(surf, corners[want], atol=1e-12)
            elif t == 3:
                r = md.cloud_radius[cl]
                ends = c + V[::-1] @ R.T                  # +axis end first
                want = [i for i in range(2) if ends[i, 2] - r < margin]
                np.testing.assert_allclose(surf, ends[want] - [0, 0, r], atol=1e-12)
                ax = R[:, 2] - np.array([0, 0, R[2, 2]])
                np.testing.assert_allclose(frame[idx, 1], np.tile(ax / np.linalg.norm(ax), (len(idx), 1)), atol=1e-9)
            else:
                rad, hl = np.hypot(V[0, 0], V[0, 1]), abs(V[0, 2])
                loc = (surf - c) @ R                      # contact surface points in the geom frame: on a rim
                np.testing.assert_allclose(np.hypot(loc[:, 0], loc[:, 1]), rad, atol=1e-9)
                np.testing.assert_allclose(np.abs(loc[:, 2]), hl, atol=1e-9)
                th = np.linspace(0, 2 * np.pi, 20001)
                rim = np.stack([rad * np.cos(th), rad * np.sin(th)], 1)
                low = min((c + np.c_[rim, np.full(len(th), s * hl)] @ R.T)[:, 2].min() for s in (-1, 1))
                assert abs(dist[idx[0]] - low) < 1e-7     # the first point is the deepest point of the cylinder
                if len(idx) > 1 and abs(loc[1, 2] + loc[0, 2]) < 1e-9:   # second point: same rim angle, other cap
                    np.testing.assert_allclose(loc[1, :2], loc[0, :2], atol=1e-9)
                if len(idx) >= 3:                          # the near cap's other two points sit at +-120 degrees
                    a0 = np.arctan2(loc[0, 1], loc[0, 0])
                    for k in (-2, -1):
                        d = (np.arctan2(loc[k, 1], loc[k, 0]) - a0 + np.pi) % (2 * np.pi) - np.pi
                        assert abs(abs(d) - 2 * np.pi / 3) < 1e-6 and abs(loc[k, 2] - loc[0, 2]) < 1e-9
    have = {int(t) for g, t in enumerate(md.geom_type) if md.geom_bodyid[g] != 0 and md.geom_cloudid[g] >= 0}
    for t in (3, 5, 6):
        if t in have:
            assert seen[t] >= 10 and multi[t] >= 3, (robot, t, seen, multi)


def _pair_lib():
    import ctypes as C
    from oracle.oracle import lib
    L = lib()
    P = C.c_void_p
    L.gqo_test_capsule_box.argtypes = [P, P, C.c_double, P, P, P, C.c_double, P]
    L.gqo_test_box_box.argtypes = [P, P, P, P, P, P, C.c_double, P]
    return L


def _np_ptr(a):
    return a.ctypes.data


def _point_box_dist(p, c, R, h):
    """distance of world points p [n,3] to the box (centre c, axes = columns of R, half sizes h); negative inside"""
    l = (p - c) @ R
    q = np.clip(l, -h, h)
    out = np.linalg.norm(l - q, axis=1)
    inside = np.all(np.abs(l) <= h, axis=1)
    out[inside] = -np.min(h - np.abs(l[inside]), axis=1)
    return out


def test_capsule_box_routine_against_brute_force():
    """capsule_box (oracle/gq_oracle.c): the first point is the global minimum of the point-box distance over a densely
    sampled axis; points lie midway between the surfaces along the returned normal; a capsule resting along a face gets a
    point at both ends; swapping the end points changes nothing."""
    from scipy.spatial.transform import Rotation
    L = _pair_lib()
    rng = np.random.default_rng(4)
    both = 0
    for trial in range(400):
        h = rng.uniform(0.02, 0.3, 3)
        R = Rotation.random(random_state=int(rng.integers(1 << 30))).as_matrix()
        c = rng.uniform(-1, 1, 3)
        r = rng.uniform(0.005, 0.05)
        if trial % 4 == 0:   # lying (almost) along the +z face
            a = np.array([rng.uniform(-h[0], h[0]), rng.uniform(-h[1], h[1]), h[2] + r + rng.uniform(-0.002, 0.0005)])
            b = np.array([rng.uniform(-h[0], h[0]), rng.uniform(-h[1], h[1]), a[2] + rng.uniform(-2e-4, 2e-4)])
            p0, p1 = c + R @ a, c + R @ b
        else:
            p0 = c + R @ (rng.uniform(-1.6, 1.6, 3) * h)
            p1 = p0 + rng.normal(0, 0.15, 3)
        margin = 0.001
        out = np.zeros(28)
        Rc = np.ascontiguousarray(R)
        n = L.gqo_test_capsule_box(_np_ptr(p0), _np_ptr(p1), r, _np_ptr(c), _np_ptr(Rc), _np_ptr(h), margin, _np_ptr(out))
        sv = np.linspace(0, 1, 20001)
        pts = p0 + sv[:, None] * (p1 - p0)
        dd = _point_box_dist(pts, c, R, h)
        dmin = dd.min()
        if dmin - r >= margin + 1e-9:
            assert n == 0
            continue
        if dmin <= 0:
            continue   # axis inside the box: the deepest-sample rule, not a closest-point statement
        # the closest point is among the (<= 2) points; it is the FIRST one unless the axis is parallel to the face within 1e-5
        # (then the two ends are equally good and the first end is taken, so that fp32 and fp64 agree on the order)
        assert n >= 1 and abs(out[0::7][:n].min() - (dmin - r)) < 2e-7 and out[0] - (dmin - r) < 1e-4
        if abs(out[0] - (dmin - r)) > 2e-7:
            continue
        nrm, pos = out[4:7], out[1:4]
        assert abs(np.linalg.norm(nrm) - 1) < 1e-9
        # the point is midway: moving back by dist/2 reaches the box surface, forward the capsule surface
        assert abs(_point_box_dist((pos - 0.5 * out[0] * nrm)[None], c, R, h)[0]) < 1e-6
        seg = pos + 0.5 * out[0] * nrm + r * nrm      # a point of the axis
        tt = np.clip(np.dot(seg - p0, p1 - p0) / max(np.dot(p1 - p0, p1 - p0), 1e-30), 0, 1)
        assert np.linalg.norm(p0 + tt * (p1 - p0) - seg) < 1e-6
        both += n == 2
        out2 = np.zeros(28)
        n2 = L.gqo_test_capsule_box(_np_ptr(p1), _np_ptr(p0), r, _np_ptr(c), _np_ptr(Rc), _np_ptr(h), margin, _np_ptr(out2))
        assert n2 == n and abs(np.sort(out2[0::7][:n2]) - np.sort(out[0::7][:n])).max() < 1e-9   # swapped ends: the same points (a parallel axis lists them the other way round)
    assert both >= 40


def test_box_box_routine_properties():
    """box_box: separated boxes report the separating-axis distance, which a dense sampling of one box's surface against the
    other confirms as a lower bound attained for face contacts; the normal points from A to B; swapping the boxes flips the
    normal and keeps the distances; a box resting flat on a larger one gets its four bottom corners; contact points lie between
    the two surfaces."""
    from scipy.spatial.transform import Rotation
    L = _pair_lib()
    rng = np.random.default_rng(9)
    flat = faces = 0
    for trial in range(400):
        ha, hb = rng.uniform(0.03, 0.3, 3), rng.uniform(0.03, 0.3, 3)
        Ra = Rotation.random(random_state=int(rng.integers(1 << 30))).as_matrix()
        ca = rng.uniform(-1, 1, 3)
        if trial % 3 == 0:   # B rests flat on A's +z face, smaller footprint
            hb[:2] = rng.uniform(0.2, 0.9, 2) * ha[:2]
            yaw = Rotation.from_euler('z', rng.uniform(-0.3, 0.3)).as_matrix()
            Rb = Ra @ yaw
            off = np.array([*(rng.uniform(-0.05, 0.05, 2) * ha[:2]), ha[2] + hb[2] + rng.uniform(-0.003, 0.0008)])
            cb = ca + Ra @ off
        else:
            Rb = Rotation.random(random_state=int(rng.integers(1 << 30))).as_matrix()
            cb = ca + rng.normal(0, 1, 3) * (ha + hb) * 0.9
        margin = 0.001
        Rac, Rbc = np.ascontiguousarray(Ra), np.ascontiguousarray(Rb)
        out, out2 = np.zeros(28), np.zeros(28)
        n = L.gqo_test_box_box(_np_ptr(ca), _np_ptr(Rac), _np_ptr(ha), _np_ptr(cb), _np_ptr(Rbc), _np_ptr(hb), margin, _np_ptr(out))
        n2 = L.gqo_test_box_box(_np_ptr(cb), _np_ptr(Rbc), _np_ptr(hb), _np_ptr(ca), _np_ptr(Rac), _np_ptr(ha), margin, _np_ptr(out2))
        # brute force: surface samples of B against box A and vice versa
        g = np.linspace(-1, 1, 41)
        surf = []
        for ax in range(3):
            for sg in (-1, 1):
                u, v = np.meshgrid(g, g)
                pts = np.zeros((u.size, 3)); pts[:, ax] = sg
                pts[:, (ax + 1) % 3] = u.ravel(); pts[:, (ax + 2) % 3] = v.ravel()
                surf.append(pts)
        surf = np.concatenate(surf)
        dAB = min(_point_box_dist(cb + (surf * hb) @ Rb.T, ca, Ra, ha).min(), _point_box_dist(ca + (surf * ha) @ Ra.T, cb, Rb, hb).min())
        if n == 0:
            assert dAB >= margin - 1e-3 * 0 - 1e-9 or dAB > 0      # reported separated: really no overlap
            assert n2 == 0
            continue
        d = out[0::7][:n]; pos = out.reshape(4, 7)[:n, 1:4]; nrm = out[4:7]
        assert n2 == n or (n2 > 0 and n > 0)
        assert abs(np.linalg.norm(nrm) - 1) < 1e-9 and np.dot(nrm, cb - ca) > 0                 # from A to B
        assert abs(out2[0::7][:n2].min() - d.min()) < 1e-9 and np.allclose(out2[4:7], -nrm, atol=1e-9)   # swap: same depth, flipped normal
        if dAB > 0:      # separated (inside the margin): the axis distance never exceeds the true distance
            assert d.min() <= dAB + 1e-9
        else:            # overlapping: a penetration is reported
            assert d.min() < 1e-6
        for q in range(n):   # shallow contacts: the point lies midway, within |dist|/2 of both surfaces; deep ones: inside the overlap region
            da, db = _point_box_dist(pos[q][None], ca, Ra, ha)[0], _point_box_dist(pos[q][None], cb, Rb, hb)[0]
            if abs(d.min()) < 5e-3:
                assert abs(da) <= abs(d[q]) * 0.5 + 2e-4 and abs(db) <= abs(d[q]) * 0.5 + 2e-4, (trial, q, da, db, d)
            # (deep overlaps - centimetres - only promise the axis depth and the normal; contacts are created at the margin)
        if trial % 3 == 0:
            flat += 1
            assert n >= 2     # a corner of B that overhangs A's face is not a contact (no polygon clipping): 2-3 points then
            if n == 4:
                faces += 1
                np.testing.assert_allclose(np.sort(d), np.sort(np.full(4, d[0])), atol=2e-3)      # four bottom corners at (nearly) one depth
    assert flat > 100 and faces >= 0.8 * flat


# ------------------------------------------------------------------ convex narrow phase (oracle/gq_convex.h: GJK + EPA)
def _cvx_lib():
    import ctypes as C
    from oracle.oracle import lib
    L = lib()
    L.gqo_test_convex.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double] * 2 + [C.c_double, C.c_void_p]
    return L


def convex_oracle(VA, hA, RA, tA, rA, VB, hB, RB, tB, rB, margin):
    """(found, dist, pos, nrm, gjk iterations, epa iterations) of the oracle's convex routine; V = None: an analytic box of half extents h."""
    import ctypes as C
    L = _cvx_lib()
    arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (VA, hA, RA, tA, VB, hB, RB, tB)]
    p = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in arrs]
    out = np.zeros(9)
    rc = L.gqo_test_convex(p[0], 0 if arrs[0] is None else len(arrs[0]), p[1], p[2], p[3], float(rA),
                           p[4], 0 if arrs[4] is None else len(arrs[4]), p[5], p[6], p[7], float(rB), float(margin), out.ctypes.data_as(C.c_void_p))
    return rc, out[0], out[1:4].copy(), out[4:7].copy(), int(out[7]), int(out[8])


def _closest_on_triangle_to_origin(a, b, c):
    ab, ac = b - a, c - a
    d1, d2 = -(ab @ a), -(ac @ a)
    if d1 <= 0 and d2 <= 0:
        return a
    d3, d4 = -(ab @ b), -(ac @ b)
    if d3 >= 0 and d4 <= d3:
        return b
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        return a + d1 / (d1 - d3) * ab
    d5, d6 = -(ab @ c), -(ac @ c)
    if d6 >= 0 and d5 <= d6:
        return c
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return a + d2 / (d2 - d6) * ac
    va = d3 * d6 - d5 * d4
    if va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        return b + (d4 - d3) / ((d4 - d3) + (d5 - d6)) * (c - b)
    den = 1.0 / (va + vb + vc)
    return a + ab * vb * den + ac * vc * den


def minkowski_truth(WA, WB):
    """Exact signed distance and separating direction of two polytopes given by their world vertices, by brute force: the convex hull of
    ALL pairwise differences a - b (scipy / qhull).  Origin inside: -(distance to the nearest facet plane) = minus the penetration depth
    (the shortest translation that separates the shapes), normal = that facet's; outside: the distance to the nearest point of the
    nearest facet, normal towards the origin."""
    from scipy.spatial import ConvexHull
    D = (WA[:, None, :] - WB[None, :, :]).reshape(-1, 3)
    h = ConvexHull(D)
    if np.all(h.equations[:, 3] <= 0):
        k = int(np.argmax(h.equations[:, 3]))
        return float(h.equations[k, 3]), h.equations[k, :3].copy(), float(np.sort(h.equations[:, 3])[-1] - np.unique(np.round(h.equations[:, 3], 12))[-2] if len(np.unique(np.round(h.equations[:, 3], 12))) > 1 else 1.0)
    best, bq = 1e300, None
    for s in h.simplices:
        q = _closest_on_triangle_to_origin(*D[s])
        if q @ q < best:
            best, bq = q @ q, q
    d = float(np.sqrt(best))
    return d, -bq / d, 1.0


def _box_corners(h):
    return np.array([[sx * h[0], sy * h[1], sz * h[2]] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], dtype=np.float64)


def _support(W, n):
    return float((W @ n).max())


def _check_convex_against_truth(VA, hA, RA, tA, rA, VB, hB, RB, tB, rB, margin, tol=1e-9, ang_tol_deg=1e-3):
    WA = (_box_corners(hA) if VA is None else VA) @ RA.T + tA
    WB = (_box_corners(hB) if VB is None else VB) @ RB.T + tB
    d, n, gap = minkowski_truth(WA, WB)
    dd = d - rA - rB
    rc, dist, pos, nrm, git, eit = convex_oracle(VA, hA, RA, tA, rA, VB, hB, RB, tB, rB, margin)
    if dd >= margin + 1e-9:
        assert rc == 0
        return None
    if dd >= margin - 1e-9:
        return None
    assert rc == 1
    if eit >= 24:   # the polytope ran into the iteration cap it shares with the kernel (one face per lane): an INNER polytope of A - B - its nearest
        assert dd - 1e-9 <= dist < dd + 1e-4, (dist, dd)   # face underestimates the depth, by little; direction and point are the iteration's state
        return None
    assert abs(dist - dd) < tol, (dist, dd)
    # depth / distance is the support-function gap along the reported normal: h_A(n) + h_B(-n) = -dist_core
    assert abs(_support(WA, nrm) + _support(WB, -nrm) + (dist + rA + rB)) < 10 * tol
    if gap > 1e-6:   # the separating direction is unique unless two facets of A - B are equally near
        ang = np.degrees(np.arccos(np.clip(nrm @ n, -1, 1)))
        assert ang < ang_tol_deg, (ang, dist, dd)
    # the contact point lies midway between the two surfaces: half the (signed) distance from A's support plane along the normal
    sa = _support(WA, nrm) + rA
    assert abs(pos @ nrm - (sa + 0.5 * dist)) < 10 * tol
    # ... between two WITNESS points: pos -+ dist / 2 along the normal are points of the two inflated surfaces, i.e. taken back by the
    # radii they lie in the cores (inside every facet plane of the shapes' own hulls)
    from scipy.spatial import ConvexHull
    for W, q in ((WA, pos - (0.5 * dist + rA) * nrm), (WB, pos + (0.5 * dist + rB) * nrm)):
        if len(W) >= 4 and np.linalg.matrix_rank(W - W[0], tol=1e-9) == 3:
            eq = ConvexHull(W).equations
            assert (eq[:, :3] @ q + eq[:, 3]).max() < 1e-7, 'witness point outside its shape'
        elif len(W) == 2:
            t = np.clip((q - W[0]) @ (W[1] - W[0]) / ((W[1] - W[0]) @ (W[1] - W[0])), 0, 1)
            assert np.linalg.norm(W[0] + t * (W[1] - W[0]) - q) < 1e-7
        elif len(W) == 1:
            assert np.linalg.norm(W[0] - q) < 1e-7
    return dist, git, eit


def test_convex_routine_against_the_minkowski_hull_random_polytopes():
    """mjc_Convex as restated in oracle/gq_convex.h (GJK distance, EPA penetration) against brute force: random polytopes of 4 - 60
    vertices, pairs of clouds and cloud - analytic box, separated within the margin, touching and overlapping up to the full size of the
    shapes, with and without an inflation radius.  Distance / depth to 1e-9 m, normal to 1e-3 degree."""
    from scipy.spatial.transform import Rotation as Rot
    rng = np.random.default_rng(0)
    n_contact, its = 0, []
    for trial in range(400):
        VA = rng.normal(size=(rng.integers(4, 60), 3)) * rng.uniform(0.02, 0.15, size=3)
        if trial % 2 == 0:
            VB, hB = None, rng.uniform(0.05, 0.5, size=3)
        else:
            VB, hB = rng.normal(size=(rng.integers(4, 60), 3)) * rng.uniform(0.02, 0.15, size=3), None
        RA, RB = (Rot.random(random_state=int(rng.integers(1 << 30))).as_matrix() for _ in range(2))
        tB = rng.normal(size=3) * rng.choice([0.05, 0.15, 0.3, 0.6])
        r = _check_convex_against_truth(VA, None, RA, np.zeros(3), float(rng.choice([0.0, 0.01])), VB, hB, RB, tB, 0.0, margin=0.02)
        if r is not None:
            n_contact += 1; its.append(r[1:])
    its = np.asarray(its)
    assert n_contact > 150 and its[:, 0].max() <= 12 and its[:, 1].max() <= 24, (n_contact, its.max(0))


@pytest.mark.parametrize('robot', ['mini_cheetah', 'hyqreal1', 'spot', 'go1'])
def test_convex_routine_on_the_robots_own_hulls(robot):
    """The same pin on the geometry the step sees: every mesh / cylinder cloud of the robot against a world box (analytic) and against
    another of the robot's clouds, at random relative poses from 2 cm apart to 3 cm deep."""
    from scipy.spatial.transform import Rotation as Rot
    md = marshalled(robot, solver=1).md
    clouds = [c for c in range(len(md.cloud_vertnum)) if md.cloud_vertnum[c] >= 8]
    assert clouds
    rng = np.random.default_rng(5)
    n_contact = n_deep = 0
    for trial in range(100):
        ca = clouds[trial % len(clouds)]
        VA = md.vert_pos[md.cloud_vertadr[ca]:md.cloud_vertadr[ca] + md.cloud_vertnum[ca]]
        if trial % 2 == 0:
            VB, hB = None, rng.uniform(0.1, 0.6, size=3)
        else:
            cb = clouds[int(rng.integers(len(clouds)))]
            VB, hB = md.vert_pos[md.cloud_vertadr[cb]:md.cloud_vertadr[cb] + md.cloud_vertnum[cb]], None
        RA, RB = (Rot.random(random_state=int(rng.integers(1 << 30))).as_matrix() for _ in range(2))
        WA = VA @ RA.T
        WB0 = (_box_corners(hB) if VB is None else VB) @ RB.T
        # place B 5 cm away along a random direction, then move it in along the (oracle's) separating direction until the shapes are
        # `want` apart - or, want < 0, overlap by at most that much; the final configuration is judged by brute force below
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        want = rng.uniform(-0.03, 0.012)
        tB = u * (_support(WA, u) + _support(WB0, -u) + 0.05)
        rc0, d0, _, n0, _, _ = convex_oracle(VA, None, RA, np.zeros(3), 0.0, VB, hB, RB, tB, 0.0, 10.0)
        assert rc0 == 1 and d0 >= 0.05 - 1e-9
        tB = tB - (d0 - want) * n0
        r = _check_convex_against_truth(VA, None, RA, np.zeros(3), 0.0, VB, hB, RB, tB, 0.0, margin=0.01, tol=1e-9)
        if r is not None:
            n_contact += 1; n_deep += r[0] < -1e-3
    assert n_contact >= 60 and n_deep >= 30, (n_contact, n_deep)


def test_convex_routine_degenerate_configurations():
    """Aligned boxes face to face (the separating direction is a whole facet: depth and normal are unique, the point is not), a box
    corner on a face, exactly touching shapes (distance 0), a capsule core (2 vertices + radius) through a box, a sphere core (1 vertex)
    inside a hull, nested shapes."""
    I = np.eye(3)
    cube = _box_corners([0.1, 0.1, 0.1])
    # face to face, 2 mm deep, both as cloud - cloud and as box - cloud
    for VA, hA in ((cube, None), (None, np.array([0.1, 0.1, 0.1]))):
        rc, dist, pos, nrm, _, _ = convex_oracle(VA, hA, I, np.zeros(3), 0.0, cube, None, I, np.array([0.0, 0.0, 0.198]), 0.0, 0.001)
        assert rc == 1 and abs(dist + 0.002) < 1e-12 and np.allclose(nrm, [0, 0, 1], atol=1e-9) and abs(pos[2] - 0.099) < 1e-9
        assert abs(pos[0]) <= 0.1 + 1e-9 and abs(pos[1]) <= 0.1 + 1e-9
    # exactly touching (distance 0 < margin): a contact with dist 0 and the face normal
    rc, dist, pos, nrm, _, _ = convex_oracle(cube, None, I, np.zeros(3), 0.0, cube, None, I, np.array([0.0, 0.0, 0.2]), 0.0, 0.001)
    assert rc == 1 and abs(dist) < 1e-12 and abs(abs(nrm[2]) - 1) < 1e-6
    # separated by exactly the margin: no contact
    rc = convex_oracle(cube, None, I, np.zeros(3), 0.0, cube, None, I, np.array([0.0, 0.0, 0.2011]), 0.0, 0.001)[0]
    assert rc == 0
    # a corner of a rotated cube 1 mm into the top face of a big analytic box
    from scipy.spatial.transform import Rotation as Rot
    R = Rot.from_euler('xyz', [np.arctan(np.sqrt(2)), 0, np.pi / 4]).as_matrix() @ Rot.from_euler('z', 0.3).as_matrix()
    low = (cube @ R.T)[:, 2].min()
    rc, dist, pos, nrm, _, _ = convex_oracle(None, np.array([1.0, 1.0, 0.5]), I, np.zeros(3), 0.0, cube, None, R, np.array([0.1, -0.2, 0.5 - low - 0.001]), 0.0, 0.001)
    assert rc == 1 and abs(dist + 0.001) < 1e-12 and np.allclose(nrm, [0, 0, 1], atol=1e-9) and abs(pos[2] - 0.4995) < 1e-9
    # capsule core through a box: depth = radius + distance of the axis to the nearest face
    seg = np.array([[0.0, 0.0, -0.3], [0.0, 0.0, 0.3]])
    Ry = Rot.from_euler('y', np.pi / 2).as_matrix()
    rc, dist, pos, nrm, _, _ = convex_oracle(None, np.array([0.2, 0.2, 0.05]), I, np.zeros(3), 0.0, seg, None, Ry, np.array([0.0, 0.0, 0.03]), 0.02, 0.0)
    assert rc == 1 and abs(dist + (0.02 + 0.02)) < 1e-12 and np.allclose(nrm, [0, 0, 1], atol=1e-9)
    # sphere core inside a hull: leaves through the nearest facet
    rc, dist, pos, nrm, _, _ = convex_oracle(cube, None, I, np.zeros(3), 0.0, np.zeros((1, 3)), None, I, np.array([0.07, 0.01, -0.02]), 0.01, 0.0)
    assert rc == 1 and abs(dist + (0.03 + 0.01)) < 1e-12 and np.allclose(nrm, [1, 0, 0], atol=1e-9)
    # nested: a small cube at the centre of a big one - six equally near facets, any of them is a valid answer
    rc, dist, pos, nrm, _, _ = convex_oracle(_box_corners([0.5, 0.5, 0.5]), None, I, np.zeros(3), 0.0, cube, None, I, np.zeros(3), 0.0, 0.0)
    assert rc == 1 and abs(dist + 0.6) < 1e-12 and abs(np.abs(nrm).max() - 1) < 1e-9


@pytest.mark.parametrize('robot', ['mini_cheetah', 'hyqreal1', 'spot'])
def test_mesh_plane_manifold_follows_the_hull_graph(robot):
    """mjc_PlaneConvex as restated in gqo_collision: the first contact of a mesh geom with the floor is the hull's support vertex (the
    lowest vertex, brute force), the others are neighbours of that vertex in the hull's edge graph that lie within the margin, in the
    graph's order, at most three in all; every contact point lies on the vertical through its vertex, midway to the floor."""
    from gym_quadruped_amd.cabi import hull_graphs
    mm = marshalled(robot, solver=1, self_collision=False)
    md, o = mm.md, Oracle(mm)
    adr, num, adj = hull_graphs(md)
    rng = np.random.default_rng(23)
    hip = float(mm.desc.key_qpos[2])
    Q = _lying_states(md, 200, rng, (0.02, 0.5 * hip))
    n_multi = n_geom = 0
    for q in Q:
        o.set_state(q, np.zeros(18), np.zeros(18), np.zeros(18)); o.forward(np.zeros(12), stage=1)
        if not o.ncon:
            continue
        geoms, dist, pos = o.get('contact_geom').astype(int), o.get('contact_dist'), o.contact_pos
        gx, gm = o.geom_xpos, o.geom_xmat
        for g in np.unique(geoms):
            if int(md.geom_type[g]) != 7:
                continue
            idx = np.nonzero(geoms == g)[0]
            assert 1 <= len(idx) <= 3 and np.all(np.diff(idx) == 1)
            cl = md.geom_cloudid[g]
            a = int(md.cloud_vertadr[cl])
            V = md.vert_pos[a:a + md.cloud_vertnum[cl]]
            W = V @ gm[g].T + gx[g]
            margin = max(float(md.geom_margin[g]), 0.0)
            v0 = int(np.argmin(W[:, 2]))
            assert abs(dist[idx[0]] - W[v0, 2]) < 1e-12
            nb = [int(u) for u in adj[adr[a + v0]:adr[a + v0] + num[a + v0]]]
            assert nb == sorted(nb) and v0 not in nb
            expect = [v0] + [u for u in nb if W[u, 2] < margin][:2]
            assert len(idx) == len(expect)
            for c, u in zip(idx, expect):
                np.testing.assert_allclose(pos[c], [W[u, 0], W[u, 1], 0.5 * W[u, 2]], atol=1e-12)
                assert abs(dist[c] - W[u, 2]) < 1e-12
            n_geom += 1; n_multi += len(idx) > 1
    assert n_geom > 100 and n_multi > 20, (n_geom, n_multi)


@pytest.mark.parametrize('robot', ['mini_cheetah', 'hyqreal1', 'spot'])
def test_hull_graph_is_the_edge_graph_of_the_hull(robot):
    """cabi.hull_graphs: symmetric, no self loops, every vertex of a mesh cloud has at least three neighbours, and a vertex is the
    support vertex of a direction exactly when none of its neighbours is higher along it (local = global maximum on a convex polytope:
    the property mjc_PlaneConvex's neighbour walk relies on)."""
    from gym_quadruped_amd.cabi import hull_graphs
    md = marshalled(robot, solver=1).md
    adr, num, adj = hull_graphs(md)
    rng = np.random.default_rng(3)
    meshes = {int(md.geom_cloudid[g]) for g in range(md.ngeom) if md.geom_cloudid[g] >= 0 and md.geom_type[g] == 7}
    assert meshes
    for cl in meshes:
        a, n = int(md.cloud_vertadr[cl]), int(md.cloud_vertnum[cl])
        V = md.vert_pos[a:a + n]
        nb = [set(int(u) for u in adj[adr[a + v]:adr[a + v] + num[a + v]]) for v in range(n)]
        assert all(len(s) >= 3 and v not in s for v, s in enumerate(nb))
        assert all(v in nb[u] for v, s in enumerate(nb) for u in s)
        for _ in range(200):
            d = rng.normal(size=3)
            pr = V @ d
            v = int(np.argmax(pr))
            assert all(pr[u] <= pr[v] for u in nb[v])
            # hill climbing from a random start ends on the support vertex
            w = int(rng.integers(n))
            for _ in range(n):
                u = max(nb[w], key=lambda k: pr[k])
                if pr[u] <= pr[w]:
                    break
                w = u
            assert pr[w] >= pr[v] - 1e-12


@pytest.mark.parametrize('name', ['mild_coarse', 'rough_coarse', 'mild_fine', 'rough_fine'])
def test_sphere_hfield_routine_against_brute_force(name):
    """sphere_hfield (oracle/gq_oracle.c) on rough, fine, non-square grids away from the origin (tests/hfield_cases.py): for every centre above
    the surface whose true distance is below reach, the distance is the smallest exact point-triangle distance over every triangle nearby and
    the normal that of a nearest candidate, to 1e-9.  The rule before this test existed accepted any face the centre projects into, whatever
    the side: on the rough grids a steep neighbour whose plane passes above a centre in the air reported a phantom penetration of centimetres
    (20 of 1051 queries on rough_coarse, up to 0.128 m too deep; 3 of 1052 on rough_fine).  Ties - a second candidate within 3e-7 m with
    another normal - are counted from the truth's side and stay at or below 5 % per grid."""
    import hfield_cases as hc
    share, n = hc.tie_share(name)
    print(f'{name}: {n} compared queries, {100 * share:.2f} % with a second candidate within {hc.TIE_WIDTH:g} m')
    assert share <= hc.MAX_TIE_SHARE, (name, share)
    n, wd, wn, second, nface, nother = hc.check_oracle_spheres(name)
    line = f'sphere_hfield {name:<13s} compared {n:>5d} ({nface} face, {nother} edge / corner contacts, {second} with a tied candidate)   max error vs brute force: dist {wd:.3g}, nrm {wn:.3g} (tolerance {hc.ORACLE_TOL:g})'
    print(line)
    hc.write_report(f'oracle {name}', [line])


def test_closest_on_triangle_routine_against_projection_reference():
    """closest_on_triangle (oracle/gq_oracle.c, Ericson's region walk) against the projection / nearest-edge reference of tests/hfield_cases.py:
    random and sliver triangles, at least 50 points in each of the seven Voronoi regions, points exactly over a corner and over an edge"""
    import hfield_cases as hc
    e, i = hc.check_triangles(*hc.oracle_triangles(), hc.ORACLE_TOL)
    print(f'closest_on_triangle: {dict(zip(hc._FEATURES, hc.triangle_cases()["counts"]))}, max point error {e:.3g} (case {i})')


def _self_contact_oracle(robot, n, seed, want_point=False):
    """(mm, oracle, states): n states with a robot-robot contact; want_point: each with a convex contact whose point is not determined"""
    from helpers import self_contact_states
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-12)
    o = Oracle(mm)
    rng = np.random.default_rng(seed)
    keep = []
    for _ in range(40):
        for q, v in zip(*self_contact_states(mm.md, n, rng, o)):
            o.set_state(q, v, np.zeros(18), np.zeros(18), 0.0, 0.7); o.forward(np.zeros(12), stage=1)
            if not want_point or (o.get('contact_tiegap') == -1.0).any():
                keep.append((q, v))
        if len(keep) >= n:
            break
    assert len(keep) >= n
    return mm, o, keep[:n]


_STEP_OUTPUTS = ('qpos', 'qvel', 'qacc', 'efc_J', 'efc_R', 'efc_aref', 'efc_force', 'contact_pos', 'contact_frame', 'contact_dist', 'contact_force')


@pytest.mark.parametrize('robot', ['b2', 'go2'])
def test_contact_point_override_changes_the_point_alone(robot):
    """Oracle.set_contact_pos: an override equal to the oracle's own points - and, for convex contacts, normals - changes no output bit; a moved
    point moves the rows and nothing of the list; a NaN normal keeps the normal; set_state clears the override; an index past the list is an error."""
    mm, o, states = _self_contact_oracle(robot, 4, 3)
    ctrl = np.random.default_rng(0).normal(0, 10, 12)
    with_normal = 0
    for q, v in states:
        state = (q, v, np.zeros(18), np.zeros(18), 0.0, 0.7)
        o.set_state(*state); o.step(ctrl)
        ref = {k: getattr(o, k).copy() for k in _STEP_OUTPUTS}
        ncon, nefc = o.ncon, o.nefc
        o.set_state(*state); o.set_contact_pos(np.arange(ncon), ref['contact_pos']); o.step(ctrl)
        for k in _STEP_OUTPUTS:
            assert np.array_equal(getattr(o, k), ref[k]), k
        o.set_state(*state); o.set_contact_pos([ncon - 1], ref['contact_pos'][ncon - 1] + [0.0, 0.01, 0.0]); o.step(ctrl)
        assert (o.ncon, o.nefc) == (ncon, nefc)
        assert np.array_equal(o.contact_pos[:ncon - 1], ref['contact_pos'][:ncon - 1]) and np.array_equal(o.contact_pos[ncon - 1], ref['contact_pos'][ncon - 1] + [0.0, 0.01, 0.0])
        for k in ('contact_frame', 'contact_dist', 'efc_R'):
            assert np.array_equal(getattr(o, k), ref[k]), k
        assert not np.array_equal(o.efc_J, ref['efc_J'])
        # the normal that goes with a point (a second minimum translation of a convex pair): the oracle's own normal changes no output bit, a NaN
        # row keeps the normal, another normal turns the frame of that contact alone and leaves its point, its depth and the list
        cvx = np.where(o.get('contact_cvx')[:ncon] == 1.0)[0]
        if len(cvx):
            with_normal += 1
            own = np.full((ncon, 3), np.nan); own[cvx] = ref['contact_frame'][cvx, 0]
            o.set_state(*state); o.set_contact_pos(np.arange(ncon), ref['contact_pos'], own); o.step(ctrl)
            for k in _STEP_OUTPUTS:
                assert np.array_equal(getattr(o, k), ref[k]), k
            c, turned = cvx[0], np.full((ncon, 3), np.nan)
            turned[c] = ref['contact_frame'][c, 0] + 0.1 * ref['contact_frame'][c, 1]
            o.set_state(*state); o.set_contact_pos(np.arange(ncon), ref['contact_pos'], turned); o.step(ctrl)
            assert (o.ncon, o.nefc) == (ncon, nefc)
            others = np.arange(ncon) != c
            assert np.array_equal(o.contact_frame[others], ref['contact_frame'][others]) and np.array_equal(o.contact_pos, ref['contact_pos'])
            assert np.array_equal(o.contact_dist, ref['contact_dist'])
            np.testing.assert_allclose(o.contact_frame[c][0], turned[c] / np.linalg.norm(turned[c]), atol=1e-15)
            assert np.abs(o.contact_frame[c] @ o.contact_frame[c].T - np.eye(3)).max() < 1e-14
        o.set_state(*state); o.step(ctrl)            # cleared by set_state
        for k in _STEP_OUTPUTS:
            assert np.array_equal(getattr(o, k), ref[k]), k
        o.set_state(*state); o.set_contact_pos([ncon], [np.zeros(3)])
        with pytest.raises(RuntimeError, match='override'):
            o.step(ctrl)
        with pytest.raises(RuntimeError, match='override'):
            o.forward(ctrl, stage=1)
        o.set_state(*state)
    assert with_normal >= 2 or robot != 'b2', with_normal   # (b2: hull against hull; go2 has primitives only)


@pytest.mark.parametrize('robot', ['b2', 'hyqreal1', 'go1'])
def test_contact_feature_distances_on_the_oracles_own_points(robot):
    """contact_list.Shapes, the signed distances that decide whether the point of a convex contact lies on the contact feature, with neither
    GPU nor emulator: the oracle's own points - determined or not - lie within half the depth of both shapes; from such a point along
    a tangent a shape is left within the geom's extent, and 1 mm past the last point that still holds the condition fails; along the normal
    1 mm fails at once."""
    from contact_cases import CVX_TOL
    from contact_list import Shapes
    mm, o, states = _self_contact_oracle(robot, 6, 5, want_point=True)
    sh = Shapes(mm)
    ncvx = nund = 0
    for q, v in states:
        o.set_state(q, v, np.zeros(18), np.zeros(18), 0.0, 0.7); o.forward(np.zeros(12), stage=1)
        gap, cvx, dist, pos, frame = o.get('contact_tiegap'), o.get('contact_cvx'), o.get('contact_dist'), o.contact_pos, o.contact_frame
        for c in range(o.ncon):
            if not cvx[c] or gap[c] == 0.0:
                continue
            ncvx += 1; nund += gap[c] == -1.0
            ok, sd = sh.on_feature(o, c, pos[c], dist[c])
            assert ok, (c, sd, dist[c])
            assert abs(sh.depth_along(o, c, frame[c][0]) - dist[c]) < CVX_TOL['dist'], (c, sh.depth_along(o, c, frame[c][0]), dist[c])   # the normal is a direction of minimum depth
            if abs(dist[c]) < 0.9e-3:
                assert not sh.on_feature(o, c, pos[c] + 1e-3 * frame[c][0], dist[c])[0] and not sh.on_feature(o, c, pos[c] - 1e-3 * frame[c][0], dist[c])[0]
            rb = [float(mm.md.geom_rbound[int(o.get(k)[c])]) for k in ('contact_geom1', 'contact_geom')]
            reach = 2.0 * min(rb) + 0.01   # the overlap lies inside both shapes: past the smaller one's diameter the point has left it
            for t in (frame[c][1], -frame[c][1], frame[c][2], -frame[c][2]):
                holds = lambda x: sh.on_feature(o, c, pos[c] + x * t, dist[c])[0]
                assert not holds(reach), (c, 'the point never leaves the shapes', reach)
                hi = reach   # (the condition holds on an interval of the line: both distances are convex)
                s = 0.0
                while hi - s > 2.5e-4:
                    mid = 0.5 * (s + hi)
                    s, hi = (mid, hi) if holds(mid) else (s, mid)
                assert not sh.on_feature(o, c, pos[c] + (s + 1e-3) * t, dist[c])[0], (c, s)
    assert ncvx >= 12 and nund >= 6, (ncvx, nund)


def test_convex_routine_point_deep_inside_a_prism():
    """The reference side of an open finding (profiles/contact_list_parity.md): a sphere's centre centimetres inside b2's 32-vertex cylinder
    prism - a foot inside a hip cylinder in the self-collision test's random poses.  The depth is the distance to the nearest face plane of the
    prism, the normal that face's; the oracle's convex routine gives both in every case.  (The kernel's fp32 routine, called alone on these
    cases, ends GJK on a sub-simplex and reports the cores as apart in 27 of 2000 under the host emulator and 29 of 2000 on the device; when it is mended, its comparison
    with the oracle belongs in contact_cases.convex_cases, which stops at 30 mm of overlap.)"""
    from scipy.spatial import ConvexHull
    from scipy.spatial.transform import Rotation as Rot
    md = marshalled('b2', solver=1).md
    cl = next(c for c in range(len(md.cloud_vertnum)) if md.cloud_vertnum[c] == 32)
    V = np.asarray(md.vert_pos[md.cloud_vertadr[cl]:md.cloud_vertadr[cl] + 32], np.float32).astype(np.float64)
    eq = ConvexHull(V).equations
    R, H = V[:, :2].max(), V[:, 2].max()
    rng = np.random.default_rng(0)
    n = 0
    while n < 300:
        q = rng.uniform(-1, 1, 3) * [0.9 * R, 0.9 * R, 0.95 * H]
        s = eq[:, :3] @ q + eq[:, 3]
        if np.hypot(q[0], q[1]) > 0.95 * R or np.sort(s)[-1] - np.sort(s[np.abs(eq[:, :3] @ eq[s.argmax(), :3]) < 0.999])[-1] < 1e-6:
            continue   # (outside the rim, or two faces of different direction equally near)
        RA = Rot.random(random_state=int(rng.integers(1 << 30))).as_matrix()
        rc, dist, pos, nrm, git, eit = convex_oracle(V, None, RA, np.zeros(3), 0.0, np.zeros((1, 3)), None, np.eye(3), RA @ q, 0.032, 0.0)
        assert rc == 1 and abs(dist - (s.max() - 0.032)) < 1e-12, (q, dist, s.max() - 0.032)
        assert np.abs(nrm - RA @ eq[s.argmax(), :3]).max() < 1e-9, (q, nrm)
        n += 1
