"""Batched depth / segmentation camera - mirror of the reference's ``gym_quadruped/sensors/rgbd_camera.py`` (``Camera`` :12-334).

The reference renders one ``mujoco.Renderer`` image per call.  Here ``gq_camera`` ray casts the images of every env in two kernel
launches (csrc/gq_camera.h), against the collision geometry the device model holds: the robot's foot spheres and link geoms, the floor,
the world boxes and the height field.  Visual-only geoms (``contype = conaffinity = 0``, group-2 meshes) have no geometry in this
package, so silhouettes follow the collision shapes; each env is its own world (other envs' robots are never drawn).  With ``rgb=True``
the same rays are shaded (``gq_camera_shaded``: per-geom colours, a floor checker, a headlight and up to seven lights, see ``Appearance``)
and ``image`` is the RGB image; without it ``image`` raises.  ``layered_image(ghost_qpos=, ghost_alpha=, ghost_rgb=, markers=)`` is
the RGB image with translucent ghost robots and markers composited over it (``gq_camera_layered``).  DESIGN.md §2 pins the pixel rays,
the depth rules, the segmentation ids, the lighting model and the layers.

The pose is that of the ``qpos`` the images are cast from - the env's current state by default.  MuJoCo's ``update_scene`` after
``mj_step`` shows the kinematics of the step's START (mjData.xpos is not updated by the integrator): a caller who wants that timing
passes a ``qpos`` saved before the step to ``render(qpos=...)``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from datetime import datetime

import numpy as np
import torch

from .. import _lib
from ..cabi import (GQ_CAM_MAXGHOST, GQ_CAM_MAXLIGHT, GQ_CAM_MAXMARKER, GQ_CAM_ROBOT, GQ_CAM_SCENE, GQ_CAM_TRACK, GqCamLayers, GqCamShade,
                    hull_planes)
from ..mjcf import CAMERA_MODES


@dataclasses.dataclass
class Light:
    """One light of ``Appearance`` (include/gq.h GqCamLight).  The field defaults are MuJoCo's ``<light>`` defaults; world axes."""
    pos: tuple = (0.0, 0.0, 0.0)
    dir: tuple = (0.0, 0.0, -1.0)
    ambient: tuple = (0.0, 0.0, 0.0)
    diffuse: tuple = (0.7, 0.7, 0.7)
    specular: tuple = (0.3, 0.3, 0.3)
    attenuation: tuple = (1.0, 0.0, 0.0)
    cutoff: float = 45.0       # degrees, spot lights
    exponent: float = 10.0     # spot lights
    directional: bool = False


@dataclasses.dataclass
class Appearance:
    """What the shaded camera draws with (include/gq.h GqCamShade): ``geom_mat`` [ngeom, 7] (rgba, specular, shininess, emission per
    ModelDesc geom), the world boxes' material, the floor / height-field checker, the background gradient, the headlight and up to
    seven more lights.  Colours and material values lie in [0, 1].  ``Appearance.default(model)`` takes the geoms' colours from the
    model; the scene values are this package's choice, the headlight is MuJoCo's default."""
    geom_mat: np.ndarray
    box_mat: tuple = (0.62, 0.52, 0.40, 1.0, 0.2, 0.3, 0.0)
    floor_rgb1: tuple = (0.42, 0.45, 0.48)
    floor_rgb2: tuple = (0.30, 0.33, 0.36)
    floor_square: float = 0.5
    floor_mark_rgb: tuple = (0.65, 0.67, 0.70)
    floor_mark_w: float = 0.0
    floor_specular: float = 0.1
    floor_shininess: float = 0.2
    floor_emission: float = 0.0
    bg_top: tuple = (0.62, 0.75, 0.90)
    bg_bottom: tuple = (0.20, 0.22, 0.25)
    head_ambient: tuple = (0.1, 0.1, 0.1)
    head_diffuse: tuple = (0.4, 0.4, 0.4)
    head_specular: tuple = (0.5, 0.5, 0.5)
    head_active: bool = True
    lights: list = dataclasses.field(default_factory=lambda: [Light(dir=(0.3, 0.2, -1.0), ambient=(0.1, 0.1, 0.1), diffuse=(0.6, 0.6, 0.6),
                                                                    directional=True)])

    @classmethod
    def default(cls, model) -> 'Appearance':
        """The model's geom colours and materials (``ModelDesc.geom_rgba`` etc.) and this package's scene defaults."""
        return cls(geom_mat=geom_materials(model))

    def struct(self) -> GqCamShade:
        """The ``GqCamShade`` of these values (``geom_mat`` left NULL: the caller sets the device pointer).  Raises ValueError on a value
        gq_camera_shaded would refuse."""
        gm = np.asarray(self.geom_mat, dtype=np.float64)
        if gm.ndim != 2 or gm.shape[1] != 7 or not np.all(np.isfinite(gm)) or gm.min(initial=0.0) < 0 or gm.max(initial=0.0) > 1:
            raise ValueError('Appearance.geom_mat must be [ngeom, 7] with values in [0, 1]')
        if len(self.lights) > GQ_CAM_MAXLIGHT:
            raise ValueError(f'at most {GQ_CAM_MAXLIGHT} lights besides the headlight (got {len(self.lights)})')
        s = GqCamShade()
        s.struct_size = C.sizeof(GqCamShade)
        s.nlight = len(self.lights)
        for k in ('box_mat', 'floor_rgb1', 'floor_rgb2', 'floor_mark_rgb', 'bg_top', 'bg_bottom', 'head_ambient', 'head_diffuse', 'head_specular'):
            v = getattr(self, k)
            getattr(s, k)[:] = [float(x) for x in v]
        for k in ('floor_square', 'floor_mark_w', 'floor_specular', 'floor_shininess', 'floor_emission'):
            setattr(s, k, float(getattr(self, k)))
        s.head_active = int(bool(self.head_active))
        for i, L in enumerate(self.lights):
            o = s.light[i]
            for k in ('pos', 'dir', 'ambient', 'diffuse', 'specular', 'attenuation'):
                getattr(o, k)[:] = [float(x) for x in getattr(L, k)]
            o.cutoff, o.exponent, o.directional = float(L.cutoff), float(L.exponent), int(bool(L.directional))
        return s


def geom_materials(md) -> np.ndarray:
    """[ngeom, 7] float64: rgba, specular, shininess, emission of every ModelDesc geom."""
    return np.concatenate([np.asarray(md.geom_rgba, np.float64).reshape(-1, 4), np.stack([md.geom_specular, md.geom_shininess, md.geom_emission], 1)], 1)


class Camera:
    """``Camera(width, height, fps, mj_model, mj_data, cam_name='', save_dir='data/img/')`` as in the reference, batched over the envs of
    ``mj_data`` (the ``QuadrupedEnv``; ``env.sim_data``).  Extensions: a camera that is not in the MJCF - ``body`` (name or ModelDesc
    index, 0 = world), ``pos``, ``quat`` (wxyz, MuJoCo's camera frame: looks along -z, y up) and ``fovy`` (degrees) - and the depth range
    ``znear`` / ``zfar`` (metres; MuJoCo's defaults scaled by a 1 m extent); ``rgb=True``: also shade an RGB image (``image``) with
    ``appearance`` (default ``Appearance.default(model)``); ``track=True`` (cameras given by ``body=`` only): ``pos`` and ``quat`` are in
    world axes - the camera follows the body's position and keeps its own orientation (MuJoCo's ``mode="track"`` idea)."""

    def __init__(self, width, height, fps, mj_model, mj_data, cam_name: str = '', save_dir='data/img/', *, body=None, pos=None, quat=None,
                 fovy=None, znear: float = 0.01, zfar: float = 50.0, rgb: bool = False, appearance: Appearance | None = None,
                 track: bool = False):
        env = mj_data
        md = env.mjModel
        self._env, self._md = env, md
        self._cam_name = cam_name
        if cam_name:
            if cam_name not in md.cam_names:
                raise ValueError(f'no camera {cam_name!r} in model {md.name} (cameras: {md.cam_names})')
            self._cam_id = md.cam_names.index(cam_name)
            mode = int(md.cam_mode[self._cam_id])
            if mode != CAMERA_MODES['fixed']:
                name = [k for k, v in CAMERA_MODES.items() if v == mode][0]
                raise ValueError(f'camera {cam_name!r} has mode="{name}": only fixed cameras (mode="fixed") are supported')
            body_id, cpos, cquat, cfovy = int(md.cam_bodyid[self._cam_id]), md.cam_pos[self._cam_id], md.cam_quat[self._cam_id], float(md.cam_fovy[self._cam_id])
        elif body is not None:
            self._cam_id = -1
            body_id, cpos, cquat, cfovy = (md.body_names.index(body) if isinstance(body, str) else int(body)), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), 45.0
        else:
            raise ValueError('Camera needs cam_name= (a <camera> of the MJCF) or body= (extension: a camera given by body, pos, quat, fovy)')
        if track and (cam_name or body_id == 0):
            raise ValueError('track=True is for cameras given by body= (a moving body, not the world)')
        self._body = body_id
        self._flags = GQ_CAM_ROBOT | GQ_CAM_SCENE | (GQ_CAM_TRACK if track else 0)
        self._pos = np.asarray(cpos if pos is None else pos, dtype=np.float64).reshape(3)
        self._quat = np.asarray(cquat if quat is None else quat, dtype=np.float64).reshape(4)
        self._quat = self._quat / np.linalg.norm(self._quat)
        self._fovy = float(cfovy if fovy is None else fovy)
        self._znear, self._zfar = float(znear), float(zfar)
        self._width, self._height = int(width), int(height)
        self.interval = float(1 / fps)
        t = env.simulation_time
        self.last_time = float(t.reshape(-1)[0]) if torch.is_tensor(t) else float(t)
        self.save_counter = 0
        timestamp = str(datetime.now()).replace(':', '_').replace(' ', '_')
        self._save_dir = os.path.join(save_dir + self._cam_name + '/', 'data_' + timestamp)
        self.K = self.intrinsic_mat
        # face planes of the hull clouds: built once per camera
        P, adr = hull_planes(md)
        self._planes = torch.as_tensor(P, dtype=torch.float32, device=env.device).contiguous() if len(P) else None
        self._plane_adr = np.ascontiguousarray(adr, dtype=np.int32) if len(P) else None
        N, H, W, dev = env.num_envs, self._height, self._width, env.device
        self._depth_plane = torch.zeros(N, H, W, dtype=torch.float32, device=dev)
        self._seg = torch.full((N, H, W), -1, dtype=torch.int32, device=dev)
        self._xpos = torch.zeros(N, 3, dtype=torch.float64, device=dev)
        self._xmat = torch.zeros(N, 9, dtype=torch.float32, device=dev)
        self._rgb = bool(rgb)
        if self._rgb:
            self.appearance = appearance if appearance is not None else Appearance.default(md)
            if len(self.appearance.geom_mat) != md.ngeom:
                raise ValueError(f'Appearance.geom_mat has {len(self.appearance.geom_mat)} rows, the model {md.ngeom} geoms')
            self._shade = self.appearance.struct()
            self._geom_mat = torch.as_tensor(np.asarray(self.appearance.geom_mat, np.float32), device=dev).contiguous()
            self._shade.geom_mat = self._geom_mat.data_ptr()
            self._rgba = torch.zeros(N, H, W, 4, dtype=torch.uint8, device=dev)

    # ------------------------------------------------------------------ the reference's properties
    @property
    def height(self) -> int:
        return self._height

    @property
    def width(self) -> int:
        return self._width

    @property
    def last_sim_time(self) -> float:
        """The last simulation time, in seconds, from a camera function call (set by the caller, as in the reference)."""
        return self.last_time

    @last_sim_time.setter
    def last_sim_time(self, time) -> None:
        self.last_time = time

    @property
    def save_dir(self) -> str:
        return self._save_dir

    @property
    def name(self) -> str:
        return self._cam_name

    @property
    def id(self) -> int:
        """Index of the camera in ``mj_model.cam_names``; -1 for a camera given by ``body=``."""
        return self._cam_id

    @property
    def fov(self) -> float:
        """Vertical field of view (MuJoCo's ``cam_fovy``), degrees."""
        return self._fovy

    @property
    def intrinsic_mat(self) -> np.ndarray:
        """The reference's pinhole matrix, as written there (rgbd_camera.py :120-147): the vertical fovy sets both focal lengths."""
        theta = np.deg2rad(self.fov)
        f_x = (self._width / 2) / np.tan(theta / 2)
        f_y = (self._height / 2) / np.tan(theta / 2)
        u_0 = (self._width - 1) / 2.0
        v_0 = (self._height - 1) / 2.0
        return np.array([[f_x, 0, u_0], [0, f_y, v_0], [0, 0, 1]])

    @property
    def frame_config(self) -> torch.Tensor:
        """Camera -> world ``[N, 4, 4]`` float64 in MuJoCo's camera frame (x right, y up, looking along -z), as of the last render.
        The reference's version cannot run (``T[:3, :3] = Rotation.from_matrix(...)`` assigns a non-array); this is what it means."""
        T = torch.zeros(self._env.num_envs, 4, 4, dtype=torch.float64, device=self._env.device)
        T[:, :3, :3] = self._xmat.reshape(-1, 3, 3).double()
        T[:, :3, 3] = self._xpos
        T[:, 3, 3] = 1.0
        return T

    @property
    def projection_mat(self) -> torch.Tensor:
        """World -> pixel ``[N, 3, 4]`` float64: ``K @ [R | t]`` in the OpenCV convention (x right, y down, z forward), as of the last
        render.  The reference's ``K (3x3) @ T (4x4)`` is a shape error; this is the matrix its name promises.  For a square image a
        world point projects to the pixel centre (column, row) its ray goes through."""
        Rmj = self._xmat.reshape(-1, 3, 3).double()
        flip = torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=torch.float64, device=Rmj.device))
        Rcv = flip @ Rmj.transpose(1, 2)
        t = -(Rcv @ self._xpos.unsqueeze(-1))
        K = torch.as_tensor(self.K, dtype=torch.float64, device=Rmj.device)
        return K @ torch.cat([Rcv, t], dim=2)

    # ------------------------------------------------------------------ images
    def render(self, qpos=None, *, ghost_qpos=None, ghost_alpha=0.5, ghost_rgb=None, markers=None):
        """Cast depth and segmentation of every env from ``qpos`` ([N, 19] float64, default: the env's current state).

        Layers (``rgb=True`` cameras; ``gq_camera_layered``), drawn translucent over the RGB image and never into depth or
        segmentation: ``ghost_qpos`` ``[19]``, ``[G, 19]`` (the same ghosts in every env) or ``[N, G, 19]``, G <= 8: the robot posed from
        each row, at ``ghost_alpha`` (a float, ``[G]`` or ``[N, G]`` in [0, 1]) and with the camera's colours, or ``ghost_rgb`` (``[3]``,
        ``[G, 3]`` or ``[N, G, 3]`` in [0, 1]); ``markers``: a ``utils.visual.Markers`` or an ``[N, K, 16]`` tensor, K <= 32.  Bad shapes
        and values raise ValueError before anything is launched.  Without layers the call is ``gq_camera_shaded``'s.  ``layered_image``
        renders with layers and returns that frame; ``image``, ``shoot`` and ``save`` render again without layers."""
        env = self._env
        layers = self._layers(ghost_qpos, ghost_alpha, ghost_rgb, markers)
        q = env.qpos if qpos is None else torch.as_tensor(qpos, dtype=torch.float64, device=env.device).reshape(-1, 19).expand(env.num_envs, 19).contiguous()
        if q.stride(1) != 1:
            q = q.contiguous()
        self._keep = q   # alive until the next call: the launch is asynchronous
        stream = torch.cuda.current_stream(env.device).cuda_stream
        pos = (np.ctypeslib.as_ctypes(self._pos))
        quat = (np.ctypeslib.as_ctypes(self._quat))
        args = (env._hbatch, q.data_ptr(), int(q.stride(0)), self._body, pos, quat, self._fovy, self._width, self._height, self._znear, self._zfar,
                self._flags, None if self._planes is None else self._planes.data_ptr(),
                None if self._plane_adr is None else np.ctypeslib.as_ctypes(self._plane_adr),
                self._depth_plane.data_ptr(), self._seg.data_ptr(), self._xpos.data_ptr(), self._xmat.data_ptr())
        if layers is not None:
            _lib.check(_lib.lib().gq_camera_layered(*args, C.byref(self._shade), self._rgba.data_ptr(), C.byref(layers), stream), 'gq_camera_layered')
        elif self._rgb:
            _lib.check(_lib.lib().gq_camera_shaded(*args, C.byref(self._shade), self._rgba.data_ptr(), stream), 'gq_camera_shaded')
        else:
            _lib.check(_lib.lib().gq_camera(*args, stream), 'gq_camera')

    def _layers(self, ghost_qpos, ghost_alpha, ghost_rgb, markers):
        """The GqCamLayers of render()'s layer arguments (None: no layers); its device tensors stay alive until the next call.  The value
        checks are reduced on the device and read back once (one synchronisation per call)."""
        if ghost_qpos is None and markers is None:
            if ghost_rgb is not None:
                raise ValueError('ghost_rgb without ghost_qpos')
            return None
        if not self._rgb:
            raise ValueError('ghosts and markers are drawn into the RGB image: they need Camera(..., rgb=True)')
        N, dev = self._env.num_envs, self._env.device
        checks = []   # (device bool scalar, message): all read back at once below

        def per_env(x, width, what, dtype):   # [.., width] -> [N, G, width]: no env axis, or [N, G, width]
            t = torch.as_tensor(x.detach() if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)).to(device=dev, dtype=torch.float64)
            if t.ndim == 1:
                t = t.reshape(1, 1, -1)
            elif t.ndim == 2:
                t = t.unsqueeze(0)
            if t.ndim != 3 or t.shape[2] != width or t.shape[0] not in (1, N):
                raise ValueError(f'{what}: expected [{width}], [G, {width}] or [{N}, G, {width}], got {tuple(np.shape(x))}')
            checks.append((torch.isfinite(t).all(), f'{what} has values that are not finite'))
            return t.expand(N, t.shape[1], width).to(dtype).contiguous()

        L = GqCamLayers()
        L.struct_size = C.sizeof(GqCamLayers)
        keep = []
        if ghost_qpos is not None:
            q = per_env(ghost_qpos, 19, 'ghost_qpos', torch.float64)
            G = q.shape[1]
            if not 1 <= G <= GQ_CAM_MAXGHOST:
                raise ValueError(f'ghost_qpos: 1 .. {GQ_CAM_MAXGHOST} ghosts per env (got {G})')
            a = torch.as_tensor(ghost_alpha.detach() if torch.is_tensor(ghost_alpha) else np.asarray(ghost_alpha, np.float64)).to(dev, torch.float64)
            if a.ndim == 0 or (a.ndim == 1 and a.shape[0] == G):
                a = a.reshape(1, -1).expand(N, G)
            elif not (a.ndim == 2 and a.shape == (N, G)):
                raise ValueError(f'ghost_alpha: expected a float, [{G}] or [{N}, {G}], got {tuple(a.shape)}')
            checks.append((((a >= 0) & (a <= 1)).all(), 'ghost_alpha must lie in [0, 1]'))
            a = a.expand(N, G).float().contiguous()
            L.n_ghost, L.ghost_qpos, L.ghost_stride, L.ghost_alpha = G, q.data_ptr(), 19, a.data_ptr()
            keep += [q, a]
            if ghost_rgb is not None:
                c = per_env(ghost_rgb, 3, 'ghost_rgb', torch.float32)
                if c.shape[1] == 1 and G > 1:
                    c = c.expand(N, G, 3).contiguous()
                if c.shape[1] != G:
                    raise ValueError(f'ghost_rgb: {c.shape[1]} colours for {G} ghosts')
                checks.append((((c >= 0) & (c <= 1)).all(), 'ghost_rgb must lie in [0, 1]'))
                L.ghost_rgb = c.data_ptr()
                keep.append(c)
        elif ghost_rgb is not None:
            raise ValueError('ghost_rgb without ghost_qpos')
        if markers is not None:
            m = markers.data if hasattr(markers, 'data') and not torch.is_tensor(markers) else markers
            m = torch.as_tensor(m).to(dev, torch.float32)
            if m.ndim != 3 or m.shape[0] != N or m.shape[2] != 16:
                raise ValueError(f'markers: expected [{N}, K, 16], got {tuple(m.shape)}')
            if m.shape[1] > GQ_CAM_MAXMARKER:
                raise ValueError(f'markers: at most {GQ_CAM_MAXMARKER} per env (got {m.shape[1]})')
            typ = m[..., 0]
            checks += [(torch.isfinite(m).all(), 'markers has values that are not finite'),
                       (((typ == 0) | (typ == 1) | (typ == 2) | (typ == 3)).all(), 'marker type must be 0 (none), 1 (sphere), 2 (capsule) or 3 (arrow)'),
                       (((m[..., 10:14] >= 0) & (m[..., 10:14] <= 1)).all(), 'marker rgba must lie in [0, 1]'),
                       ((m[..., 7:9] >= 0).all(), 'marker sizes must be >= 0'),
                       (((m[..., 9] > 0) & (m[..., 9] < 1) | (typ != 3)).all(), 'an arrow marker\'s head share size[2] must lie in (0, 1)')]
            m = m.contiguous()
            L.n_marker, L.markers = m.shape[1], (m.data_ptr() if m.shape[1] else None)
            keep.append(m)
        ok = torch.stack([c for c, _ in checks]).cpu().tolist()
        for good, (_, msg) in zip(ok, checks):
            if not good:
                raise ValueError(msg)
        self._keep_layers = keep
        return L

    @property
    def depth_plane(self) -> torch.Tensor:
        """Planar depth ``[N, H, W]`` (distance along the camera's -z; what the renderer's depth buffer holds), zfar where nothing is hit."""
        self.render()
        return self._depth_plane

    def _range(self, depth_plane):
        # the reference's algebra, verbatim (rgbd_camera.py depth_image): the ROW index pairs with K[0][2] and K[0][0].  For a square
        # image this is the Euclidean range along each pixel's ray; for other shapes it is the reference's quirk, kept.
        K = self.K
        i, j = torch.meshgrid(torch.arange(self.height, device=depth_plane.device), torch.arange(self.width, device=depth_plane.device), indexing='ij')
        x_camera = (i - K[0][2]) * depth_plane / K[0][0]
        y_camera = (j - K[1][2]) * depth_plane / K[1][1]
        return torch.sqrt(depth_plane ** 2 + x_camera ** 2 + y_camera ** 2)

    @property
    def depth_image(self) -> torch.Tensor:
        """``[N, H, W]`` float32: the reference's ``depth_image`` of the planar depth."""
        self.render()
        self._depth_image = self._range(self._depth_plane)
        return self._depth_image

    @property
    def seg_image(self) -> torch.Tensor:
        """``[N, H, W]`` int32 segmentation ids: a robot geom's ModelDesc geom index, ``ngeom`` the floor, ``ngeom + 1 + b`` world box b,
        ``ngeom + 1 + nbox`` the height field, -1 no hit.  MuJoCo numbers the whole scene's geoms, so its ids differ from these."""
        self.render()
        self._seg_image = self._seg
        return self._seg

    @property
    def point_cloud(self) -> torch.Tensor:
        """``[N, H * W, 3]``: the reference's ``_depth_to_point_cloud(depth_image)``."""
        self._point_cloud = self._depth_to_point_cloud(self.depth_image)
        return self._point_cloud

    def _depth_to_point_cloud(self, depth_image: torch.Tensor) -> torch.Tensor:
        # rgbd_camera.py _depth_to_point_cloud, batched: K^-1 [x, y, 1] * (-depth), x = column, y = row
        n, height, width = depth_image.shape
        y, x = torch.meshgrid(torch.arange(height, device=depth_image.device), torch.arange(width, device=depth_image.device), indexing='ij')
        hom = torch.stack([x.flatten(), y.flatten(), torch.ones_like(x.flatten())]).to(torch.float64)
        K_inv = torch.as_tensor(np.linalg.inv(self.intrinsic_mat), dtype=torch.float64, device=depth_image.device)
        pts = (K_inv @ hom).unsqueeze(0) * (-depth_image.reshape(n, 1, -1).double())
        return pts.transpose(1, 2).to(depth_image.dtype)

    @property
    def image(self) -> torch.Tensor:
        """``[N, H, W, 3]`` uint8 RGB (a view of the ``[N, H, W, 4]`` RGBA buffer, overwritten by the next render).  Needs ``rgb=True``."""
        if not self._rgb:
            raise NotImplementedError('Camera.image (RGB) needs Camera(..., rgb=True): this camera casts depth and segmentation only '
                                      '(depth_image, depth_plane, seg_image and point_cloud).')
        self.render()
        return self._rgba[..., :3]

    def layered_image(self, qpos=None, *, ghost_qpos=None, ghost_alpha=0.5, ghost_rgb=None, markers=None) -> torch.Tensor:
        """``[N, H, W, 3]`` uint8 RGB with ghosts and markers composited over it (``render``'s layer arguments; without any it is
        ``image`` of ``qpos``).  A view of the RGBA buffer, overwritten by the next render.  Needs ``rgb=True``."""
        if not self._rgb:
            raise NotImplementedError('Camera.layered_image (RGB) needs Camera(..., rgb=True)')
        self.render(qpos, ghost_qpos=ghost_qpos, ghost_alpha=ghost_alpha, ghost_rgb=ghost_rgb, markers=markers)
        return self._rgba[..., :3]

    def shoot(self, autosave: bool = True, img: bool = False, depth: bool = True, seg: bool = True) -> None:
        """Cast once and keep depth image, point cloud and segmentation, and with ``img=True`` the RGB image (needs ``rgb=True``)."""
        if img and not self._rgb:
            self.image
        self.render()
        self._depth_image = self._range(self._depth_plane)
        self._point_cloud = self._depth_to_point_cloud(self._depth_image)
        self._seg_image = self._seg.clone()
        if img:
            self._image = self._rgba[..., :3].clone()
        if autosave:
            self.save(img=img, depth=depth, seg=seg, fresh=False)

    def save(self, img_name: str = '', img: bool = False, depth: bool = False, seg: bool = False, fresh: bool = True) -> None:
        """Save RGB ``[N, H, W, 3]`` uint8, depth ``[N, H, W]`` and segmentation ``[N, H, W]`` as ``.npy`` (the reference writes PNGs
        through cv2, which is not a dependency here).  ``fresh=False``: save what the last ``shoot`` cast instead of casting again."""
        if img and not self._rgb:
            self.image
        os.makedirs(os.path.join(self._save_dir, 'images'), exist_ok=True)
        if fresh:
            self.render()
            self._depth_image, self._seg_image = self._range(self._depth_plane), self._seg
            if img:
                self._image = self._rgba[..., :3]
        print(f'saving {"image " if img else ""}{"depth image " if depth else ""}{"segmentation image " if seg else ""}to {self.save_dir}')
        stem = f'{img_name}_' if img_name else ''
        suffix = '' if img_name else f'_{self.save_counter}'
        if seg:
            np.save(os.path.join(self._save_dir, f'{stem}seg{suffix}.npy'), self._seg_image.cpu().numpy())
        if depth:
            np.save(os.path.join(self._save_dir, 'images', f'{stem}depth{suffix}.npy'), self._depth_image.cpu().numpy())
        if img:
            np.save(os.path.join(self._save_dir, 'images', f'{stem}image{suffix}.npy'), self._image.cpu().numpy())
        if not img_name:
            self.save_counter += 1
