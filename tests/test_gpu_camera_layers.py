"""gq_camera_layered / Camera.render(ghost_qpos=, markers=) / QuadrupedEnv.render(ghost_qpos=, markers=): bit identity with
gq_camera_shaded where no layer shows, a ghost at alpha 1 against the opaque robot it copies, the fp64 numpy caster, shader and
compositor (test_gpu_camera.Caster, camera_shading.py, camera_layers.py), env locality and unchanged rollouts."""
import numpy as np
import pytest
import torch

from camera_layers import composite, marker_hit
from camera_shading import background, lights_of, make_caster, seg_band, shade, surface, to_bytes, unit
from test_gpu_camera import ZFAR, _env, _oracle_poses, _pixel_dirs, _qmat

pytestmark = pytest.mark.gpu


def _q(env):
    """the envs' qpos, moved in x / y next to env 0 (the envs spawn far apart; every env has the same static scene, so one world camera
    then sees every env's robot at much the same place)"""
    q = env.qpos.clone()
    q[:, 0:2] = q[0:1, 0:2] + torch.linspace(0.0, 0.05, env.num_envs, dtype=torch.float64, device=q.device).unsqueeze(1)
    return q


def _world_cam(env, W, H, f=(0.55, 0.75, -0.36), dist=1.3, q=None, **kw):
    """a world camera (body 0) about dist from the mean base of the envs (of q, default _q(env)), looking along f"""
    from gym_quadruped_amd.mjcf import mat_to_quat
    from gym_quadruped_amd.sensors import Camera
    f = np.asarray(f, np.float64) / np.linalg.norm(f)
    right = np.cross(f, [0, 0, 1.0]); right /= np.linalg.norm(right)
    R = np.stack([right, np.cross(right, f), -f], 1)
    target = (_q(env) if q is None else q)[:, 0:3].double().mean(0).cpu().numpy()
    return Camera(W, H, 30, env.robot_model, env.sim_data, body=0, pos=target - dist * f, quat=mat_to_quat(R), fovy=60.0, zfar=ZFAR, rgb=True, **kw)


def _markers(env, behind=False, q=None):
    """a sphere, a capsule and an arrow about each env's base (of q, default _q(env); world rows [N, 3, 16])"""
    from gym_quadruped_amd.utils.visual import Markers, render_line, render_sphere, render_vector
    b = (_q(env) if q is None else q)[:, 0:3].double()
    m = Markers(env.num_envs, env.device)
    render_sphere(m, b + torch.tensor([0.0, -0.35, 0.15], dtype=torch.float64, device=b.device), 0.16, (0.9, 0.1, 0.1, 0.5))
    render_line(m, b + torch.tensor([-0.4, 0.1, 0.3], dtype=torch.float64, device=b.device), b + torch.tensor([0.3, -0.2, 0.25], dtype=torch.float64,
                device=b.device), 0.03, (0.1, 0.8, 0.2, 0.7))
    render_vector(m, (0.2, -0.9, 0.4), b + torch.tensor([0.0, 0.3, 0.0] if behind else [-0.2, 0.0, 0.2], dtype=torch.float64, device=b.device), 0.6,
                  (0.2, 0.3, 0.9, 0.8))
    m.data[:, 2, 7:10] = torch.tensor([0.03, 0.07, 0.3], device=b.device)   # a fat arrow: many pixels on its head
    return m


@pytest.mark.parametrize('robot,scene', [('aliengo', 'random_boxes'), ('go2', 'flat')])
def test_no_layers_and_zero_alpha_are_bit_identical(robot, scene):
    n = 6
    env = _env(robot, n, scene=scene, seed=3, steps=15)
    cam = _world_cam(env, 48, 40)
    q = _q(env)
    cam.render(qpos=q)
    ref = [t.clone() for t in (cam._depth_plane, cam._seg, cam._xpos, cam._xmat, cam._rgba)]
    ghosts = q.unsqueeze(1).repeat(1, 3, 1)
    ghosts[:, 0, 0] += 0.2
    ghosts[:, 1, 1] -= 0.3
    m = _markers(env)
    m0 = m.data.clone()
    m0[..., 13] = 0.0
    for kw in (dict(ghost_qpos=ghosts, ghost_alpha=0.0, markers=m0), dict(markers=torch.zeros(n, 0, 16, device=env.device)),
               dict(ghost_qpos=ghosts, ghost_alpha=0.7, markers=m)):
        cam.render(qpos=q, **kw)
        out = (cam._depth_plane, cam._seg, cam._xpos, cam._xmat)
        assert all(torch.equal(a, b) for a, b in zip(out, ref[:4])), kw.keys()   # depth, seg and pose never change
        if kw.get('ghost_alpha', 0.0) == 0.0 and 'markers' in kw and kw['markers'] is not m:
            assert torch.equal(cam._rgba, ref[4])
    assert not torch.equal(cam._rgba, ref[4])   # the visible layers do change the image
    # render('rgb_array') without the new arguments is today's frame: that of a separate plain shaded camera with the same pose
    from gym_quadruped_amd.mjcf import mat_to_quat
    from gym_quadruped_amd.sensors import Camera
    frame = env.render('rgb_array', width=40, height=32)
    az, el, dist = np.deg2rad(90.0), np.deg2rad(-45.0), 2.0
    f = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    right = np.cross(f, [0, 0, 1.0]); right /= np.linalg.norm(right)
    plain = Camera(40, 32, 30, env.robot_model, env.sim_data, body='base', pos=-dist * f, quat=mat_to_quat(np.stack([right, np.cross(right, f), -f], 1)),
                   fovy=45.0, rgb=True, track=True)
    assert torch.equal(frame, plain.image)
    frame_t = env.render('rgb_array', True, None, 0.5, width=40, height=32)
    assert not torch.equal(frame, frame_t)
    with_l = env.render('rgb_array', False, env.qpos, 0.5, width=40, height=32, markers=_markers(env, q=env.qpos))
    assert torch.equal(env.render('rgb_array', width=40, height=32), frame) and not torch.equal(with_l, frame)


@pytest.mark.parametrize('robot,scene,n,S', [('aliengo', 'flat', 4, 64), ('aliengo', 'random_boxes', 4, 64), ('go2', 'flat', 4, 48),
                                             ('mini_cheetah', 'flat', 2, 48)])
def test_ghost_at_alpha_one_matches_the_opaque_robot(robot, scene, n, S):
    env = _env(robot, n, scene=scene, seed=5, steps=10)
    cam = _world_cam(env, S, S, dist={'mini_cheetah': 0.7}.get(robot, 1.3))
    q = _q(env)
    cam.render(qpos=q)
    plain, seg = cam._rgba[..., :3].clone(), cam._seg.clone()
    away = q.clone()
    away[:, 0] += 100.0   # the real robot out of view; the camera is a world camera and stays
    ghost = cam.layered_image(away, ghost_qpos=q.unsqueeze(1), ghost_alpha=1.0)
    ng = env.mjModel.ngeom
    assert not bool(((cam._seg >= 0) & (cam._seg < ng)).any())
    robot_px = (seg >= 0) & (seg < ng)
    assert float(robot_px.float().mean()) > 0.03
    # the 1-pixel band around the robot's silhouette: there the ghost's hit may fall on either side of it (the edges between two
    # robot geoms are the same geoms in both images)
    band = torch.as_tensor(np.stack([seg_band(s, S, S).reshape(S, S) for s in robot_px.int().cpu().numpy()]), device=seg.device)
    sel = robot_px & ~band
    d = (ghost.int() - plain.int()).abs().amax(-1)
    assert int(d[sel].max()) <= 1, int(d[sel].max())
    assert float(sel.float().sum()) > 0.35 * float(robot_px.float().sum())   # thin legs lie mostly in the band at these sizes


@pytest.mark.parametrize('robot,scene,kind', [('aliengo', 'random_boxes', 'world'), ('go2', 'flat', 'body'), ('go2', 'flat', 'track'),
                                             ('mini_cheetah', 'flat', 'world')])
def test_ghost_posed_like_the_robot_adds_nothing(robot, scene, kind):
    """t < t0 is strict: a ghost at the robot's own qpos, even at alpha 1, leaves every byte of the plain shaded image (the ghost pose
    pass reproduces the pose pass's geom frames bit for bit, for world, body and tracking cameras)"""
    from test_gpu_camera import _make_cam
    n = 4
    env = _env(robot, n, scene=scene, seed=11, steps=12)
    if kind == 'world':
        q = _q(env)
        cam = _world_cam(env, 48, 48, dist={'mini_cheetah': 0.7}.get(robot, 1.3))
        plain = cam.layered_image(q).clone()
        robot_px = float(((cam._seg >= 0) & (cam._seg < env.mjModel.ngeom)).float().mean())
        same = cam.layered_image(q, ghost_qpos=q.unsqueeze(1), ghost_alpha=1.0)
    elif kind == 'body':   # a camera fixed to the base under the trunk, looking back at the legs
        cam = _make_cam(env, 48, 48, rgb=True)
        plain = cam.image.clone()
        robot_px = float(((cam._seg >= 0) & (cam._seg < env.mjModel.ngeom)).float().mean())
        same = cam.layered_image(ghost_qpos=env.qpos.unsqueeze(1), ghost_alpha=1.0)
    else:
        plain = env.render('rgb_array', width=48, height=40).clone()
        (cam,) = env._render_cams.values()
        robot_px = float(((cam._seg >= 0) & (cam._seg < env.mjModel.ngeom)).float().mean())
        same = env.render('rgb_array', False, env.qpos, 1.0, width=48, height=40)
    assert robot_px > 0.02, robot_px   # the robot is in view
    assert torch.equal(same, plain)


def _oracle_image(caster, app, poses, ghost_poses, alphas, rows, co, Rc, Dw, znear):
    """the fp64 layered image: bytes [P, 3] and the pixels whose layers are ambiguous"""
    lights = lights_of(app, Rc)
    t0, seg = caster.cast(co, Dw, poses, znear, ZFAR)
    C0 = background(app, Dw)
    amb = np.zeros(len(Dw), bool)
    hit = seg >= 0
    if hit.any():
        nn, col, mat, a, hp = surface(caster, app, poses, co, Dw[hit], t0[hit], seg[hit])
        C0[hit] = shade(col, mat, nn, -unit(Dw[hit]), hp, lights)
        amb[hit] = a
    lay_t, lay_S, lay_a = [], [], []
    for gp, al in zip(ghost_poses, alphas):
        tg, sg = caster.cast(co, Dw, gp, znear, ZFAR, flags=1)
        S = np.zeros((len(Dw), 3))
        h = sg >= 0
        if h.any():
            nn, col, mat, a, hp = surface(caster, app, gp, co, Dw[h], tg[h], sg[h])
            S[h] = shade(col, mat, nn, -unit(Dw[h]), hp, lights)
            amb[h] |= a
        amb |= seg_band(sg, *caster.hw)
        lay_t.append(np.where(h, tg, np.nan)); lay_S.append(S); lay_a.append(al)
    for r in rows:
        tm, S = np.full(len(Dw), np.nan), np.zeros((len(Dw), 3))
        for p in range(len(Dw)):
            t, nrm = marker_hit(r, co, Dw[p])
            if t is not None and t >= znear:
                tm[p] = t
                S[p] = shade([r[10:13]], [(0.5, 0.5, 0.0)], [nrm], [-unit(Dw[p])], [co + t * Dw[p]], lights)[0]
        amb |= seg_band(np.where(np.isnan(tm), -1, 0), *caster.hw)
        lay_t.append(tm); lay_S.append(S); lay_a.append(r[13])
    out = np.zeros((len(Dw), 3))
    for p in range(len(Dw)):
        ts = [None if np.isnan(t[p]) else t[p] for t in lay_t]
        for t in ts:   # a layer within 1e-4 m of the opaque hit or of another layer: its order is ambiguous
            if t is not None and (abs(t - t0[p]) < 1e-4 or sum(u is not None and abs(u - t) < 1e-4 for u in ts) > 1):
                amb[p] = True
        out[p] = composite(C0[p], t0[p], [(t, S[p], a) for t, S, a in zip(ts, lay_S, lay_a)], znear)
    return to_bytes(out), seg, amb


@pytest.mark.parametrize('robot,scene', [('aliengo', 'flat'), ('go2', 'random_boxes')])
def test_layers_match_numpy_oracle(robot, scene):
    from test_gpu_camera_rgb import _appearance
    n, S = 2, 48
    env = _env(robot, n, scene=scene, seed=8, steps=12)
    app = _appearance(env.mjModel)
    cam = _world_cam(env, S, S, appearance=app)
    q = _q(env)
    gq = q.unsqueeze(1).repeat(1, 2, 1)
    gq[:, 0, 0] += 0.25; gq[:, 0, 1] -= 0.15; gq[:, 0, 7:] += 0.2
    gq[:, 1, 0] -= 0.3; gq[:, 1, 1] += 0.2; gq[:, 1, 7:] -= 0.15
    alphas = (0.3, 0.6)
    m = _markers(env)
    m.data[1, 2] = _markers(env, behind=True).data[1, 2]   # env 1: the arrow behind the robot
    img = cam.layered_image(q, ghost_qpos=gq, ghost_alpha=list(alphas), markers=m).cpu().numpy().astype(np.int64)
    seg = cam._seg.cpu().numpy()
    poses = _oracle_poses(robot, q.cpu().numpy())
    gposes = [_oracle_poses(robot, gq[:, g].cpu().numpy()) for g in range(2)]
    caster = make_caster(env)
    caster.hw = (S, S)
    Rc = _qmat(cam._quat)
    Dw = _pixel_dirs(S, S, cam.fov, np.arange(S * S)) @ Rc.T
    compared = 0
    for e in range(n):
        ref, ref_seg, amb = _oracle_image(caster, app, poses[e], [gposes[0][e], gposes[1][e]], alphas, m.data[e].double().cpu().numpy(), cam._pos,
                                          Rc, Dw, cam._znear)
        ok = (seg[e].reshape(-1) == ref_seg) & ~amb & ~seg_band(ref_seg, S, S)
        d = np.abs(img[e].reshape(-1, 3) - ref).max(1)
        assert d[ok].max(initial=0) <= 2, (robot, e, np.argwhere((d > 2) & ok)[:5].ravel(), d[ok].max())
        compared += int(ok.sum())
    assert compared >= 0.5 * n * S * S, compared


def test_arrow_head_seen_side_on_matches_oracle():
    """a camera looking across a long arrow: its cone head's silhouette and shading against the fp64 cone.  Layers write no depth, so
    the head's hit depth is seen through its colour only (its silhouette, and through the lighting the normal at the hit point);
    camera_layers.marker_hit itself is pinned to the analytic cone depth in test_camera_layers_host.py."""
    from gym_quadruped_amd.sensors import Appearance
    from gym_quadruped_amd.utils.visual import Markers, render_vector
    n, S = 2, 64
    env = _env('aliengo', n, scene='flat', seed=1, steps=0)
    app = Appearance.default(env.mjModel)
    cam = _world_cam(env, S, S, f=(0.0, 1.0, -0.05), dist=1.0, appearance=app)
    q = _q(env)
    b = q[:, 0:3].double()
    m = Markers(n, env.device)
    render_vector(m, (1.0, 0.0, 0.0), b + torch.tensor([-0.3, -0.4, 0.05], dtype=torch.float64, device=b.device), 0.6, (0.9, 0.6, 0.1, 1.0))
    m.data[:, 0, 7:10] = torch.tensor([0.03, 0.09, 0.4], device=b.device)
    img = cam.layered_image(q, markers=m).cpu().numpy().astype(np.int64)
    caster = make_caster(env)
    caster.hw = (S, S)
    Rc = _qmat(cam._quat)
    Dw = _pixel_dirs(S, S, cam.fov, np.arange(S * S)) @ Rc.T
    poses = _oracle_poses('aliengo', q.cpu().numpy())
    row = m.data[0].double().cpu().numpy()
    ref, ref_seg, amb = _oracle_image(caster, app, poses[0], [], [], row, cam._pos, Rc, Dw, cam._znear)
    head = np.zeros(S * S, bool)
    for p in range(S * S):
        t, _ = marker_hit(row[0], cam._pos, Dw[p])
        if t is not None:
            hp = cam._pos + t * Dw[p] - row[0, 1:4]
            head[p] = hp @ (row[0, 4:7] / np.linalg.norm(row[0, 4:7])) > 0.6 * 0.6 + 1e-3
    ok = (cam._seg[0].cpu().numpy().reshape(-1) == ref_seg) & ~amb & ~seg_band(ref_seg, S, S)
    assert (head & ok).sum() >= 10, (head & ok).sum()
    d = np.abs(img[0].reshape(-1, 3) - ref).max(1)
    assert d[ok].max() <= 2


def test_env_local_and_rollout_unchanged():
    n = 8
    env = _env('aliengo', n, scene='random_boxes', seed=2, steps=10)
    cam = _world_cam(env, 40, 32)
    gq = env.qpos.unsqueeze(1).repeat(1, 2, 1)
    gq[:, 0, 0] += 0.2
    gq[:, 1, 1] += 0.2
    m = _markers(env)
    a = cam.layered_image(ghost_qpos=gq, ghost_alpha=[0.4, 0.7], markers=m).clone()
    k = 5
    gq2, m2 = gq.clone(), m.data.clone()
    gq2[k, 0, 0] -= 0.4
    m2[k, 0, 1:4] += 0.1
    b = cam.layered_image(ghost_qpos=gq2, ghost_alpha=[0.4, 0.7], markers=m2)
    diff = (a != b).flatten(1).any(1).cpu().tolist()
    assert diff == [e == k for e in range(n)]
    env.close()
    runs = []
    for with_cam in (False, True):
        env = _env('go2', 6, scene='flat', seed=4, steps=0)
        cam = _world_cam(env, 32, 32) if with_cam else None
        g = torch.Generator(device='cuda:0').manual_seed(7)
        for _ in range(20):
            env.step(torch.randn(6, 12, generator=g, device='cuda:0') * 5.0)
            if cam is not None:
                cam.render(ghost_qpos=env.qpos.unsqueeze(1), ghost_alpha=0.5, markers=_markers(env))
                env.render('rgb_array', True, env.qpos, 0.3, width=24, height=16)
        torch.cuda.synchronize()
        runs.append((env.qpos.clone(), env.qvel.clone()))
        env.close()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
