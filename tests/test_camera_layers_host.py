"""Host side of the layered camera (gq_camera_layered): the GqCamLayers mirror and checks, Camera.render / QuadrupedEnv.render's layer
arguments against the argument table, the utils.visual builders, the tint palette, and known answers of the numpy compositor."""
import ctypes
import types

import numpy as np
import pytest
import torch

from camera_layers import composite, marker_hit


def test_camlayers_mirror_abi_and_export():
    from gym_quadruped_amd import _lib
    # (GqCamLayers' layout and the GQ_CAM_MAX* limits against the header: tests/test_host_and_abi.py, for every struct and constant)
    L = _lib.lib()
    assert L.gq_version() == 660 and 'gq_camera_layered' in _lib.EXPORTS and hasattr(L, 'gq_camera_layered')


def _shade_ok():
    from gym_quadruped_amd.mjcf import load_compiled
    from gym_quadruped_amd.sensors import Appearance
    s = Appearance.default(load_compiled('aliengo')).struct()
    s.geom_mat = 16   # any non-null device address: the calls stop at the null batch
    return s


def _layers(**kw):
    from gym_quadruped_amd.cabi import GqCamLayers
    L = GqCamLayers()
    L.struct_size = ctypes.sizeof(GqCamLayers)
    L.n_ghost, L.ghost_qpos, L.ghost_stride, L.ghost_alpha = 2, 16, 19, 16
    L.n_marker, L.markers = 3, 16
    for k, v in kw.items():
        setattr(L, k, v)
    return L


def _call(L, shade, layers, rgba=16):
    pos, quat = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 4)(1, 0, 0, 0)
    rc = L.gq_camera_layered(None, None, 19, 0, pos, quat, 45.0, 8, 8, 0.01, 10.0, 3, None, None, None, None, None, None,
                             None if shade is None else ctypes.byref(shade), rgba, None if layers is None else ctypes.byref(layers), None)
    return rc, L.gq_last_error().decode()


def test_gq_camera_layered_checks_every_field():
    from gym_quadruped_amd import _lib
    L = _lib.lib()
    rc, err = _call(L, _shade_ok(), _layers())
    assert rc == -1 and 'null argument' in err, err   # every layer and shade field passes: the null batch is refused
    rc, err = _call(L, _shade_ok(), _layers(n_ghost=0, ghost_qpos=None, ghost_alpha=None, n_marker=0, markers=None))
    assert rc == -1 and 'null argument' in err, err

    def bad(layers, what, shade=None, rgba=16):
        rc, err = _call(L, shade if shade is not None else _shade_ok(), layers, rgba)
        assert rc == -1 and what in err, err
    rc, err = _call(L, _shade_ok(), None)
    assert rc == -1 and 'null layers' in err
    bad(_layers(struct_size=ctypes.sizeof(_layers()) - 4), 'struct_size')
    bad(_layers(n_ghost=9), 'n_ghost')
    bad(_layers(n_ghost=-1), 'n_ghost')
    bad(_layers(n_marker=33), 'n_marker')
    bad(_layers(n_marker=-1), 'n_marker')
    bad(_layers(ghost_qpos=None), 'ghost_qpos')
    bad(_layers(ghost_alpha=None), 'ghost_alpha')
    bad(_layers(ghost_stride=18), 'ghost_stride')
    bad(_layers(markers=None), 'markers')
    # what gq_camera_shaded refuses
    s = _shade_ok(); s.struct_size -= 4
    bad(_layers(), 'GqCamShade.struct_size', shade=s)
    s = _shade_ok(); s.geom_mat = None
    bad(_layers(), 'geom_mat', shade=s)
    s = _shade_ok(); s.bg_top[0] = 2.0
    bad(_layers(), 'bg_top', shade=s)
    bad(_layers(), 'null rgba', rgba=None)
    rc, err = _call(L, None, _layers())
    assert rc == -1 and 'null shade' in err


class _RecordingLib:
    def __init__(self, proxy):
        self._proxy, self.args = proxy, {}

    def __getattr__(self, name):
        fn = getattr(self._proxy, name)

        def call(*a):
            self.args[name] = a
            return fn(*a)
        return call

    @property
    def calls(self):
        return self._proxy.calls


def _cpu_env(robot='aliengo', n=3):
    from gym_quadruped_amd.mjcf import load_compiled
    return types.SimpleNamespace(mjModel=load_compiled(robot), robot_model=None, num_envs=n, device=torch.device('cpu'), simulation_time=torch.zeros(n),
                                 qpos=torch.zeros(n, 19, dtype=torch.float64), _hbatch=None)


@pytest.fixture
def rec_lib(monkeypatch):
    from test_host_and_abi import _TypeCheckedLib
    from gym_quadruped_amd import _lib
    rec = _RecordingLib(_TypeCheckedLib(_lib.lib()))
    monkeypatch.setattr(_lib, 'lib', lambda: rec)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda dev=None: types.SimpleNamespace(cuda_stream=None))
    return rec


def test_camera_render_maps_layer_arguments(rec_lib):
    from gym_quadruped_amd.cabi import GqCamLayers
    from gym_quadruped_amd.sensors import Camera
    from gym_quadruped_amd.utils.visual import Markers, render_sphere
    env = _cpu_env()
    N = env.num_envs
    cam = Camera(16, 8, 30, env.mjModel, env, body='base', pos=(0.0, -1.0, 0.5), rgb=True, save_dir='/nonexistent/')
    cam.render()
    assert rec_lib.calls == ['gq_camera_shaded']   # no layers: the shaded call, as before
    q1 = np.arange(19, dtype=np.float64)
    for gq, G in ((q1, 1), (np.stack([q1, q1 + 1]), 2), (torch.as_tensor(np.stack([np.stack([q1 + e, q1 - e]) for e in range(N)])), 2)):
        for ga in (0.3, [0.2, 0.4][:G], np.full((N, G), 0.7)):
            cam.render(ghost_qpos=gq, ghost_alpha=ga)
            a = rec_lib.args['gq_camera_layered']
            L = a[-2]._obj
            assert isinstance(L, GqCamLayers) and L.struct_size == ctypes.sizeof(GqCamLayers)
            assert L.n_ghost == G and L.ghost_stride == 19 and L.n_marker == 0 and not L.markers and not L.ghost_rgb
            q, al = cam._keep_layers[0], cam._keep_layers[1]
            assert q.shape == (N, G, 19) and q.dtype == torch.float64 and q.is_contiguous() and L.ghost_qpos == q.data_ptr()
            assert al.shape == (N, G) and al.dtype == torch.float32 and L.ghost_alpha == al.data_ptr()
            want = torch.as_tensor(np.asarray(gq), dtype=torch.float64).reshape(-1, G, 19).expand(N, G, 19)
            assert torch.equal(q, want)
            assert torch.allclose(al, torch.as_tensor(np.broadcast_to(np.asarray(ga, np.float64), (N, G)).copy(), dtype=torch.float32))
            assert a[-3] == cam._rgba.data_ptr()
    cam.render(ghost_qpos=q1, ghost_rgb=(0.1, 0.2, 0.3))
    assert rec_lib.args['gq_camera_layered'][-2]._obj.ghost_rgb == cam._keep_layers[2].data_ptr()
    m = Markers(N, 'cpu')
    render_sphere(m, (0.0, 0.0, 1.0), 0.2, (1.0, 0.0, 0.0, 0.5))
    for mk in (m, m.data.clone()):
        cam.render(markers=mk)
        L = rec_lib.args['gq_camera_layered'][-2]._obj
        assert L.n_ghost == 0 and L.n_marker == 1 and L.markers == cam._keep_layers[-1].data_ptr()
        assert torch.equal(cam._keep_layers[-1], m.data)
    # refused before any call
    n_calls = len(rec_lib.calls)
    for kw in (dict(ghost_qpos=np.zeros(18)), dict(ghost_qpos=np.zeros((9, 19))), dict(ghost_qpos=np.zeros((N + 1, 2, 19))),
               dict(ghost_qpos=q1, ghost_alpha=1.5), dict(ghost_qpos=q1, ghost_alpha=-0.1), dict(ghost_qpos=q1, ghost_alpha=[0.5, 0.5]),
               dict(ghost_qpos=np.full(19, np.nan)), dict(ghost_qpos=q1, ghost_alpha=float('nan')), dict(ghost_rgb=(1.0, 0.0, 0.0)),
               dict(ghost_qpos=q1, ghost_rgb=(2.0, 0.0, 0.0)), dict(markers=torch.zeros(N, 33, 16)), dict(markers=torch.zeros(N, 2, 15)),
               dict(markers=torch.full((N, 1, 16), float('nan'))), dict(markers=torch.full((N, 1, 16), 5.0))):
        with pytest.raises(ValueError):
            cam.render(**kw)
    with pytest.raises(ValueError, match='rgb=True'):
        Camera(16, 8, 30, env.mjModel, env, body='base').render(ghost_qpos=q1)
    assert len(rec_lib.calls) == n_calls


def test_camera_layered_image_argument_table(rec_lib):
    """Camera.layered_image renders with its layers (gq_camera_layered) and returns the RGB view of that render; image renders again
    without layers (gq_camera_shaded)"""
    from gym_quadruped_amd.sensors import Camera
    from gym_quadruped_amd.utils.visual import Markers, render_vector
    env = _cpu_env('go2', 2)
    N = env.num_envs
    cam = Camera(16, 8, 30, env.mjModel, env, body='base', pos=(0.0, -1.0, 0.5), rgb=True, save_dir='/nonexistent/')
    m = Markers(N, 'cpu')
    render_vector(m, (1.0, 0.0, 0.0), (0.0, 0.0, 0.5), 0.3, (1.0, 0.5, 0.0, 0.7))
    q = torch.zeros(N, 19, dtype=torch.float64)
    q[:, 3] = 1.0
    gq = torch.zeros(N, 2, 19, dtype=torch.float64)
    img = cam.layered_image(q, ghost_qpos=gq, ghost_alpha=[0.25, 0.5], ghost_rgb=(0.2, 0.4, 0.6), markers=m)
    assert rec_lib.calls == ['gq_camera_layered']
    a = rec_lib.args['gq_camera_layered']
    L = a[-2]._obj
    assert a[1] == cam._keep.data_ptr() and torch.equal(cam._keep, q)           # the qpos drawn
    assert a[-3] == cam._rgba.data_ptr() and img.shape == (N, 8, 16, 3) and img.data_ptr() == cam._rgba.data_ptr()
    assert L.n_ghost == 2 and L.ghost_qpos == cam._keep_layers[0].data_ptr() and L.ghost_alpha == cam._keep_layers[1].data_ptr()
    assert L.ghost_rgb == cam._keep_layers[2].data_ptr() and cam._keep_layers[2].shape == (N, 2, 3)
    assert L.n_marker == 1 and L.markers == cam._keep_layers[3].data_ptr() and torch.equal(cam._keep_layers[3], m.data)
    assert torch.equal(cam._keep_layers[1], torch.tensor([[0.25, 0.5]] * N))
    cam.layered_image()                          # no layers: the shaded call
    cam.image
    assert rec_lib.calls == ['gq_camera_layered', 'gq_camera_shaded', 'gq_camera_shaded']
    with pytest.raises(ValueError):
        cam.layered_image(ghost_qpos=gq, ghost_alpha=1.5)
    assert len(rec_lib.calls) == 3
    with pytest.raises(NotImplementedError, match='rgb=True'):
        Camera(16, 8, 30, env.mjModel, env, body='base').layered_image(ghost_qpos=gq)


def test_env_render_accepts_reference_arguments(rec_lib):
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    from gym_quadruped_amd.utils.visual import Markers, render_line
    env = _cpu_env('go2', 2)
    env.robot_model, env.sim_data = env.mjModel, env
    env.render = types.MethodType(QuadrupedEnv.render, env)
    q = np.zeros(19)
    env.render('rgb_array', True, q, 0.3, width=16, height=8)      # the reference's positional order
    L = rec_lib.args['gq_camera_layered'][-2]._obj
    assert L.n_ghost == 1
    (cam_t,) = [c for k, c in env._render_cams.items() if 'tint' in k]
    assert float(cam_t._keep_layers[1][0, 0]) == pytest.approx(0.3)
    from gym_quadruped_amd.utils.visual import tinted_geom_mat
    np.testing.assert_array_equal(cam_t.appearance.geom_mat, tinted_geom_mat(env.mjModel, cam_t.appearance.geom_mat))
    assert not np.array_equal(cam_t.appearance.geom_mat[:, :3], np.asarray(env.mjModel.geom_rgba)[:, :3])
    m = Markers(2, 'cpu')
    render_line(m, (0, 0, 0), (1, 0, 0), 0.01, (0, 1, 0, 1))
    env.render('rgb_array', width=16, height=8, markers=m)
    assert rec_lib.args['gq_camera_layered'][-2]._obj.n_marker == 1
    n = len(rec_lib.calls)
    env.render('rgb_array', width=16, height=8)
    assert rec_lib.calls[n:] == ['gq_camera_shaded']
    with pytest.raises(NotImplementedError):
        env.render('human', True, q, 0.5)
    with pytest.raises(ValueError):
        env.render('rgb_array', False, q, 2.0, width=16, height=8)


# ---- utils.visual builders
def test_visual_builders_rows():
    from gym_quadruped_amd.utils.visual import Markers, render_frame, render_line, render_sphere, render_vector
    N = 3
    m = Markers(N, 'cpu')
    i = render_line(m, (0.0, 1.0, 2.0), np.array([[1.0, 1.0, 2.0], [0.0, 3.0, 2.0], [0.0, 1.0, 5.0]]), 0.05, (0.1, 0.2, 0.3, 0.4))
    assert i == 0 and m.data.shape == (N, 1, 16) and m.data.dtype == torch.float32
    r = m.data[:, 0].double().numpy()
    assert (r[:, 0] == 2).all()
    np.testing.assert_allclose(r[:, 1:4], [[0, 1, 2]] * 3, rtol=1e-7)
    np.testing.assert_allclose(r[:, 4:7], [[1, 0, 0], [0, 2, 0], [0, 0, 3]], rtol=1e-7)
    np.testing.assert_allclose(r[:, 7], 0.05, rtol=1e-7)
    np.testing.assert_allclose(r[:, 10:14], [[0.1, 0.2, 0.3, 0.4]] * 3, rtol=1e-7)
    j = render_vector(m, (0.0, 3.0, 4.0), (1.0, 1.0, 1.0), np.array([1.0, 2.0, 10.0]), (1, 0, 0, 1))
    r = m.data[:, j].double().numpy()
    assert j == 1 and (r[:, 0] == 3).all()
    np.testing.assert_allclose(np.linalg.norm(r[:, 4:7], axis=1), [1.0, 2.0, 10.0], rtol=1e-6)
    np.testing.assert_allclose(r[:, 4:7] / np.linalg.norm(r[:, 4:7], axis=1, keepdims=True), [[0, 0.6, 0.8]] * 3, rtol=1e-6)
    assert 0 < r[0, 9] < 1 and r[0, 8] >= r[0, 7]
    k = render_sphere(m, (0.0, 0.0, 1.0), 0.4, (0, 0, 1, 0.5))
    r = m.data[:, k].double().numpy()
    assert (r[:, 0] == 1).all() and np.allclose(r[:, 7], 0.2)
    # an index passed back overwrites in place
    assert render_sphere(m, (5.0, 0.0, 1.0), 0.2, (0, 0, 1, 0.5), index=k) == k and len(m) == 3
    np.testing.assert_allclose(m.data[:, k, 1:4].numpy(), [[5, 0, 1]] * 3)
    # render_frame: red along column 1, green along column 0, blue along column 2 of the rotation
    ang = 0.3
    qz = (np.cos(ang / 2), 0.0, 0.0, np.sin(ang / 2))
    ids = render_frame(m, (1.0, 2.0, 3.0), qz, 0.5, alpha=0.6)
    Rm = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    for idx, col, rgb in zip(ids, (1, 0, 2), ((1, 0, 0), (0, 1, 0), (0, 0, 1))):
        r = m.data[0, idx].double().numpy()
        assert r[0] == 2
        np.testing.assert_allclose(r[4:7], Rm[:, col] * 0.5, atol=1e-6)
        np.testing.assert_allclose(r[10:14], (*rgb, 0.6), atol=1e-7)
        np.testing.assert_allclose(r[7], 0.01, rtol=1e-6)
    assert render_frame(m, (0.0, 0.0, 0.0), (1, 0, 0, 0), 1.0, index=ids) == ids and len(m) == 6
    with pytest.raises(ValueError):
        render_sphere(m, np.zeros((N + 1, 3)), 0.1, (1, 1, 1, 1))
    for _ in range(32 - len(m)):
        render_sphere(m, (0, 0, 0), 0.1, (1, 1, 1, 1))
    with pytest.raises(ValueError):
        render_sphere(m, (0, 0, 0), 0.1, (1, 1, 1, 1))


def test_velocity_markers_colours_and_offsets():
    from gym_quadruped_amd.utils.visual import velocity_markers
    N = 2
    qpos = torch.zeros(N, 19, dtype=torch.float64)
    qpos[:, 0:3] = torch.tensor([[1.0, 2.0, 0.4], [0.0, 0.0, 0.3]], dtype=torch.float64)
    yaw = np.pi / 2
    qpos[:, 3], qpos[:, 6] = np.cos(yaw / 2), np.sin(yaw / 2)
    qvel = torch.zeros(N, 18, dtype=torch.float64)
    qvel[:, 0:3] = torch.tensor([[0.3, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    cmd = torch.tensor([[0.5, 0.0, 0.0], [0.0, 0.2, 0.0]])
    env = types.SimpleNamespace(num_envs=N, device=torch.device('cpu'), qpos=qpos, qvel=qvel, target_base_vel=lambda: (cmd, torch.zeros(N)),
                                external_disturbances_kwargs=None)
    m = velocity_markers(env)
    assert len(m) == 2
    r = m.data.double().numpy()
    np.testing.assert_allclose(r[:, 0, 10:14], [[1, 0.5, 0, 0.7]] * 2, rtol=1e-6)
    np.testing.assert_allclose(r[:, 1, 10:14], [[0, 1, 1, 0.7]] * 2, rtol=1e-6)
    np.testing.assert_allclose(r[:, 0, 1:4], qpos[:, 0:3].numpy() + [0, 0, 0.10], rtol=1e-6)
    np.testing.assert_allclose(r[:, 1, 1:4], qpos[:, 0:3].numpy() + [0, 0, 0.15], rtol=1e-6)
    np.testing.assert_allclose(r[:, 0, 4:7], [[0, 0.5, 0], [-0.2, 0, 0]], atol=1e-6)   # heading frame -> world (yaw 90 deg)
    np.testing.assert_allclose(r[:, 1, 4:7], [[0.3, 0, 0], [0, 0, 0]], atol=1e-7)      # zero velocity: a zero-length arrow
    env.external_disturbances_kwargs = {'x': [1.0]}
    env._applied = torch.zeros(N, 18)
    env._applied[:, 0] = 5.0
    m = velocity_markers(env)
    assert len(m) == 3
    np.testing.assert_allclose(m.data[:, 2, 4:7].numpy(), [[0.1, 0, 0]] * 2, atol=1e-7)
    np.testing.assert_allclose(m.data[:, 2, 10:14].numpy(), [[1, 0, 0, 0.7]] * 2, atol=1e-7)


# the reference palette's outcome on the registry robots (utils/mujoco/visual.py change_robot_appearance): the trunk body gets teal, the
# FL_ / FR_ / RL_ / RR_ leg bodies orange, grey, yellow and light grey (hyqreal1 has no collision geom on its hip bodies)
PALETTE = {'teal': (0.054, 0.415, 0.505), 'orange': (0.698, 0.376, 0.082), 'grey': (0.260, 0.263, 0.263), 'yellow': (0.800, 0.480, 0.000),
           'lightgrey': (0.710, 0.703, 0.703)}
TRUNK = {'aliengo': 'base', 'b2': 'base', 'go1': 'trunk', 'go2': 'base', 'hyqreal1': 'base', 'hyqreal2': 'base', 'mini_cheetah': 'base',
         'spot': 'body'}


def _tint_table(robot):
    links = ('thigh', 'calf') if robot == 'hyqreal1' else ('hip', 'thigh', 'calf')
    out = {TRUNK[robot]: 'teal'}
    for leg, colour in (('FL', 'orange'), ('FR', 'grey'), ('RL', 'yellow'), ('RR', 'lightgrey')):
        out.update({f'{leg}_{k}': colour for k in links})
    return out


@pytest.mark.parametrize('robot', sorted(TRUNK))
def test_tint_palette_on_registry_robots(robot):
    from gym_quadruped_amd.mjcf import load_compiled
    from gym_quadruped_amd.sensors import Appearance
    from gym_quadruped_amd.utils import visual as V
    assert V.tint_color('left_front') == V.FL_COLOR and V.tint_color('LH_thigh') == V.HL_COLOR and V.tint_color('trunk') == V.ROBOT_COLOR
    md = load_compiled(robot)
    app = Appearance.default(md)
    gm = V.tinted_geom_mat(md, app.geom_mat)
    assert gm is not app.geom_mat and np.array_equal(app.geom_mat, Appearance.default(md).geom_mat)   # the input is not modified
    got = {}
    for g in range(md.ngeom):
        b = int(md.geom_bodyid[g])
        if b == 0:   # the world's geoms keep their material
            np.testing.assert_array_equal(gm[g], app.geom_mat[g])
            continue
        colour = [k for k, v in PALETTE.items() if np.allclose(gm[g, :3], v, rtol=0, atol=1e-12)]
        assert len(colour) == 1 and gm[g, 3] == 1.0, (robot, md.body_names[b], gm[g])
        np.testing.assert_array_equal(gm[g, 4:], app.geom_mat[g, 4:])   # specular, shininess, emission kept
        assert got.setdefault(md.body_names[b], colour[0]) == colour[0]
    assert got == _tint_table(robot)


# ---- known answers of the compositor and the marker shapes
def test_compositor_known_answers():
    C0, t0 = np.array([0.2, 0.4, 0.6]), 5.0
    np.testing.assert_array_equal(composite(C0, t0, []), C0)
    S1 = np.array([1.0, 0.0, 0.0])
    np.testing.assert_allclose(composite(C0, t0, [(2.0, S1, 0.25)]), 0.25 * S1 + 0.75 * C0)
    # two layers: the far one first
    S2 = np.array([0.0, 1.0, 0.0])
    want = 0.5 * S1 + 0.5 * (0.25 * S2 + 0.75 * C0)
    np.testing.assert_allclose(composite(C0, t0, [(1.0, S1, 0.5), (3.0, S2, 0.25)]), want)
    np.testing.assert_allclose(composite(C0, t0, [(3.0, S2, 0.25), (1.0, S1, 0.5)]), want)
    # behind the opaque hit, or at its depth exactly: nothing
    np.testing.assert_array_equal(composite(C0, t0, [(5.0, S1, 1.0), (6.0, S2, 1.0), (None, S1, 1.0)]), C0)
    # a tie: the higher index is farther, so the lower index ends on top
    np.testing.assert_allclose(composite(C0, t0, [(2.0, S1, 1.0), (2.0, S2, 1.0)]), S1)
    np.testing.assert_allclose(composite(C0, t0, [(2.0, S2, 1.0), (2.0, S1, 1.0)]), S2)
    # the cut-off: nine opaque-ish layers, the farthest is dropped
    lay = [(1.0 + k, np.full(3, k / 10.0), 0.5) for k in range(9)]
    C = C0.copy()
    for t, S, a in reversed(lay[:8]):
        C = a * S + (1 - a) * C
    np.testing.assert_allclose(composite(C0, 20.0, lay), C)
    assert not np.allclose(composite(C0, 20.0, lay), composite(C0, 20.0, lay, maxlayer=9))
    # alpha 0 everywhere: C0 exactly
    np.testing.assert_array_equal(composite(C0, t0, [(1.0 + k, np.ones(3), 0.0) for k in range(12)]), C0)


def test_marker_shapes_known_answers():
    co = np.zeros(3)
    # sphere at z = -3 of radius 0.5, looking down -z
    t, n = marker_hit([1, 0, 0, -3, 0, 0, 0, 0.5, 0, 0, 1, 1, 1, 1, 0, 0], co, np.array([0, 0, -1.0]))
    assert t == pytest.approx(2.5) and np.allclose(n, [0, 0, 1])
    # capsule from (-1, 0, -3) to (1, 0, -3), radius 0.1: the side at 2.9, a cap end at x = 1.1
    row = [2, -1, 0, -3, 2, 0, 0, 0.1, 0, 0, 1, 1, 1, 1, 0, 0]
    t, n = marker_hit(row, co, np.array([0.3, 0, -3.0]) / 3)
    assert t == pytest.approx(2.9 * 3 / 3, rel=1e-9) and np.allclose(n, [0, 0, 1])
    t, _ = marker_hit(row, np.array([5.0, 0, -3]), np.array([-1.0, 0, 0]))
    assert t == pytest.approx(5 - 1.1)
    assert marker_hit([2, 0, 0, -3, 0, 0, 0, 0.1, 0, 0, 1, 1, 1, 1, 0, 0], co, np.array([0, 0, -1.0]))[0] is None   # zero length
    # arrow from (0, 0, -4) along +z of length 2 (tip at z = -2), head share 0.25 (base at z = -2.5), head radius 0.2, shaft 0.05:
    # looking down the axis the tip is the first point; from the side at height z, the cone radius is 0.2 (z_tip - z) / 0.5
    row = [3, 0, 0, -4, 0, 0, 2, 0.05, 0.2, 0.25, 1, 0, 0, 1, 0, 0]
    t, n = marker_hit(row, co, np.array([0, 0, -1.0]))
    assert t == pytest.approx(2.0, abs=1e-9)
    z = -2.3
    t, n = marker_hit(row, np.array([3.0, 0, z]), np.array([-1.0, 0, 0]))
    assert t == pytest.approx(3.0 - 0.2 * (-2 - z) / 0.5)
    np.testing.assert_allclose(n, np.array([1.0, 0, 0.4]) / np.linalg.norm([1.0, 0, 0.4]), atol=1e-12)
    t, n = marker_hit(row, np.array([3.0, 0, -3.0]), np.array([-1.0, 0, 0]))   # the shaft
    assert t == pytest.approx(2.95) and np.allclose(n, [1, 0, 0])
    t, n = marker_hit(row, np.array([0.15, 0, -3.0]), np.array([0, 0, 1.0]))   # under the head's rim: its base disc
    assert t == pytest.approx(0.5) and np.allclose(n, [0, 0, -1])
