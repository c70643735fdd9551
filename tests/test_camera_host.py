"""Host side of the depth / segmentation camera: the MJCF compiler's camera tables, the sensor's image algebra (the reference's
sensors/rgbd_camera.py, restated in numpy) and the hull face planes gq_camera clips against."""
import types

import numpy as np
import pytest
import torch


def _toy_xml(cams):
    legs = ''.join(f'''<body name="L{i}_hip" pos="0.1 0 0"><inertial pos="0 0 0" mass="1" diaginertia="1e-3 1e-3 1e-3"/>
      <joint name="j{i}a" axis="0 1 0"/><body name="L{i}_thigh"><inertial pos="0 0 -0.1" mass="1" diaginertia="1e-3 1e-3 1e-3"/><joint name="j{i}b" axis="0 1 0"/>
      <body name="L{i}_calf" pos="0 0 -0.2"><inertial pos="0 0 -0.1" mass="0.5" diaginertia="1e-3 1e-3 1e-3"/><joint name="j{i}c" axis="1 0 0"/>
      <geom name="{n}" size="0.02" pos="0 0 -0.2"/></body></body></body>''' for i, n in enumerate(['FL', 'FR', 'RL', 'RR']))
    return f'''<mujoco model="toy"><compiler angle="radian"/><default><camera fovy="60"/><default class="wide"><camera fovy="100"/></default></default>
      <worldbody><camera name="world_cam" pos="1 2 3" zaxis="0 0 1"/>
      <body name="base" pos="0 0 0.5"><inertial pos="0 0 0" mass="5" diaginertia="0.1 0.1 0.1"/><freejoint/>{cams}{legs}</body></worldbody>
      <actuator>{''.join(f'<motor name="m{i}{c}" joint="j{i}{c}"/>' for i in range(4) for c in 'abc')}</actuator></mujoco>'''


def test_mjcf_camera_tables(tmp_path):
    from gym_quadruped_amd.mjcf import compile_mjcf, quat_to_mat
    cams = ('<camera name="q" pos="0.3 0 0.1" quat="0 0 0 2"/>'
            '<camera name="xy" pos="0 -1 0.8" xyaxes="1 0 0 0 1 1" mode="trackcom"/>'
            '<camera name="w" class="wide" axisangle="0 0 1 1.5707963267948966"/>'
            '<camera name="e" euler="0 0 1.5707963267948966" fovy="30"/>')
    p = tmp_path / 'toy.xml'
    p.write_text(_toy_xml(cams))
    md = compile_mjcf(p)
    assert md.cam_names == ['world_cam', 'q', 'xy', 'w', 'e']
    np.testing.assert_array_equal(md.cam_bodyid, [0, 1, 1, 1, 1])
    np.testing.assert_allclose(md.cam_pos[1], [0.3, 0, 0.1])
    np.testing.assert_allclose(md.cam_fovy, [60, 60, 60, 100, 30])          # <default><camera fovy=> classes, then the element
    np.testing.assert_array_equal(md.cam_mode, [0, 0, 2, 0, 0])             # trackcom is recorded (the sensor refuses it)
    np.testing.assert_allclose(np.linalg.norm(md.cam_quat, axis=1), 1.0, atol=1e-12)
    np.testing.assert_allclose(quat_to_mat(md.cam_quat[1]), np.diag([-1.0, -1.0, 1.0]), atol=1e-12)   # quat normalised
    y = np.array([0, 1, 1]) / np.sqrt(2)
    np.testing.assert_allclose(quat_to_mat(md.cam_quat[2]), np.stack([[1, 0, 0], y, np.cross([1, 0, 0], y)], 1), atol=1e-12)
    rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    np.testing.assert_allclose(quat_to_mat(md.cam_quat[3]), rz, atol=1e-12)
    np.testing.assert_allclose(quat_to_mat(md.cam_quat[4]), rz, atol=1e-12)
    np.testing.assert_allclose(quat_to_mat(md.cam_quat[0]), np.eye(3), atol=1e-12)   # zaxis = +z


def test_aliengo_robotcam():
    from gym_quadruped_amd.mjcf import load_compiled
    md = load_compiled('aliengo')
    i = md.cam_names.index('robotcam')
    assert md.body_names[md.cam_bodyid[i]] == 'base'
    np.testing.assert_allclose(md.cam_pos[i], [0.31, -0.005, 0.00292751])          # aliengo.xml:51
    np.testing.assert_allclose(md.cam_quat[i], [0.5, 0.5, -0.5, -0.5])             # quat="0.4 0.4 -0.4 -0.4", normalised
    assert md.cam_fovy[i] == 45.0 and md.cam_mode[i] == 0
    assert load_compiled('go1').cam_mode[0] == 2                                    # go1's tracking camera is trackcom


def _cpu_camera(W, H, n=2, fovy=45.0):
    from gym_quadruped_amd.mjcf import load_compiled
    from gym_quadruped_amd.sensors.rgbd_camera import Camera
    env = types.SimpleNamespace(mjModel=load_compiled('aliengo'), num_envs=n, device=torch.device('cpu'), simulation_time=torch.zeros(n))
    return Camera(W, H, 30, env.mjModel, env, body='base', fovy=fovy, save_dir=str('/nonexistent/'))


@pytest.mark.parametrize('W,H', [(64, 64), (40, 24)])
def test_image_algebra_matches_reference(W, H):
    cam = _cpu_camera(W, H)
    rng = np.random.default_rng(0)
    plane = rng.uniform(0.2, 5.0, (2, H, W)).astype(np.float32)
    # rgbd_camera.py intrinsic_mat :120-147
    theta = np.deg2rad(45.0)
    K = np.array([[(W / 2) / np.tan(theta / 2), 0, (W - 1) / 2.0], [0, (H / 2) / np.tan(theta / 2), (H - 1) / 2.0], [0, 0, 1]])
    np.testing.assert_allclose(cam.intrinsic_mat, K)
    # rgbd_camera.py depth_image :196-206
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    rng_img = []
    for e in range(2):
        x = (i - K[0][2]) * plane[e] / K[0][0]
        y = (j - K[1][2]) * plane[e] / K[1][1]
        rng_img.append(np.sqrt(plane[e] ** 2 + x ** 2 + y ** 2))
    got = cam._range(torch.as_tensor(plane)).numpy()
    np.testing.assert_allclose(got, np.stack(rng_img), rtol=1e-6)
    # rgbd_camera.py _depth_to_point_cloud :256-300
    pc = cam._depth_to_point_cloud(torch.as_tensor(got)).numpy()
    for e in range(2):
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        hom = np.vstack((xx.flatten(), yy.flatten(), np.ones(H * W)))
        pts = (np.linalg.inv(K) @ hom * -got[e].flatten()).T
        np.testing.assert_allclose(pc[e], pts, rtol=1e-5, atol=1e-6)
    if W == H:   # square: the reference's range is the Euclidean length of the pixel ray up to the planar depth
        t = np.tan(theta / 2)
        dx, dy = (2 * (j + 0.5) / W - 1) * t, (1 - 2 * (i + 0.5) / H) * t
        np.testing.assert_allclose(got[0], plane[0] * np.sqrt(1 + dx ** 2 + dy ** 2), rtol=1e-5)
    with pytest.raises(NotImplementedError):
        cam.image


def test_camera_refuses_non_fixed_modes():
    from gym_quadruped_amd.mjcf import load_compiled
    from gym_quadruped_amd.sensors import Camera
    env = types.SimpleNamespace(mjModel=load_compiled('go1'), num_envs=1, device=torch.device('cpu'), simulation_time=torch.zeros(1))
    with pytest.raises(ValueError, match='trackcom'):
        Camera(8, 8, 30, env.mjModel, env, cam_name='tracking')


@pytest.mark.parametrize('robot', ['mini_cheetah', 'spot'])
def test_hull_face_planes(robot):
    from gym_quadruped_amd.cabi import hull_planes
    from gym_quadruped_amd.mjcf import load_compiled
    md = load_compiled(robot)
    P, adr = hull_planes(md)
    assert adr[0] == 0 and adr[-1] == len(P) and len(adr) == len(md.cloud_vertnum) + 1
    np.testing.assert_allclose(np.linalg.norm(P[:, :3], axis=1), 1.0, atol=1e-12)
    n_hulls = 0
    for cl in range(len(md.cloud_vertnum)):
        Q = P[adr[cl]:adr[cl + 1]]
        if not len(Q):
            continue
        n_hulls += 1
        a, n = md.cloud_vertadr[cl], md.cloud_vertnum[cl]
        s = md.vert_pos[a:a + n] @ Q[:, :3].T - Q[:, 3]
        assert s.max() <= 1e-9                            # every vertex inside every face plane
        np.testing.assert_allclose(s.max(0), 0.0, atol=1e-9)   # and every plane touches the hull
        assert len({tuple(np.round(q[:3], 6)) for q in Q}) == len(Q)   # coplanar triangles merged: one plane per facet normal
    assert n_hulls > 0
