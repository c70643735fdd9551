"""Batched counterparts of the reference's ``gym_quadruped/utils/mujoco/visual.py`` marker helpers, for ``sensors.Camera.render(markers=)``
and ``QuadrupedEnv.render(markers=)``.

The reference appends decorative geoms to a viewer's scene; here each helper appends one row per env to a ``Markers`` container (a
``[N, K, 16]`` float32 tensor, include/gq.h GqCamLayers), which ``gq_camera_layered`` draws as translucent layers.  Every argument may
carry a leading env axis or none (then it is broadcast to every env).  The returned index stands where the reference returns a
``geom_id``: passing it back as ``index=`` overwrites that marker in place.

Row layout (world axes): ``type, pos[3], axis[3], size[3], rgba[4], pad[2]``; type 1 sphere (radius size[0]), 2 capsule from pos to
pos + axis (radius size[0]), 3 arrow from pos to pos + axis (shaft radius size[0], head base radius size[1], head share size[2]).
"""
from __future__ import annotations

import numpy as np
import torch

from ..cabi import GQ_CAM_MAXMARKER

SPHERE, CAPSULE, ARROW = 1, 2, 3
ARROW_SHAFT = 0.01        # the reference's mjGEOM_ARROW size[0:2]
ARROW_HEAD_RADIUS = 0.02  # this package's choice
ARROW_HEAD_SHARE = 0.25


class Markers:
    """``data``: ``[num_envs, K, 16]`` float32 rows on ``device``, K <= GQ_CAM_MAXMARKER (32)."""

    def __init__(self, num_envs: int, device='cuda:0'):
        self.num_envs, self.device = int(num_envs), torch.device(device)
        self.data = torch.zeros(self.num_envs, 0, 16, dtype=torch.float32, device=self.device)

    def __len__(self) -> int:
        return self.data.shape[1]

    def _put(self, rows: torch.Tensor, index: int | None) -> int:
        if index is None or index < 0:
            if len(self) >= GQ_CAM_MAXMARKER:
                raise ValueError(f'at most {GQ_CAM_MAXMARKER} markers per env')
            self.data = torch.cat([self.data, rows.unsqueeze(1)], 1).contiguous()
            return len(self) - 1
        if index >= len(self):
            raise ValueError(f'marker index {index} out of range (have {len(self)})')
        self.data[:, index] = rows
        return int(index)

    def _env(self, x, width: int) -> torch.Tensor:
        """x as [N, width] float64 (broadcast over the envs when it has no env axis)."""
        t = torch.as_tensor(np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float64), device=self.device)
        t = t.reshape(-1, width) if t.numel() != width else t.reshape(1, width)
        if t.shape[0] not in (1, self.num_envs):
            raise ValueError(f'expected [{width}] or [{self.num_envs}, {width}], got {tuple(t.shape)}')
        return t.expand(self.num_envs, width)

    def row(self, type_, pos, axis, size, rgba, index=None) -> int:
        rows = torch.cat([torch.full((self.num_envs, 1), float(type_), dtype=torch.float64, device=self.device), self._env(pos, 3),
                          self._env(axis, 3), self._env(size, 3), self._env(rgba, 4),
                          torch.zeros(self.num_envs, 2, dtype=torch.float64, device=self.device)], 1)
        return self._put(rows.float(), index)


def render_vector(markers: Markers, vector, pos, scale, color=(1.0, 0.0, 0.0, 1.0), index=None) -> int:
    """An arrow from ``pos`` along ``vector`` of length ``scale`` (the reference's mjGEOM_ARROW of size (0.01, 0.01, scale)).  A zero
    vector gives a zero-length arrow, which is not drawn (the reference points it in a random direction)."""
    v = markers._env(vector, 3)
    n = torch.linalg.norm(v, dim=1, keepdim=True)
    axis = torch.where(n > 1e-12, v / n.clamp_min(1e-300), torch.zeros_like(v)) * markers._env(scale, 1)
    return markers.row(ARROW, pos, axis, (ARROW_SHAFT, ARROW_HEAD_RADIUS, ARROW_HEAD_SHARE), color, index)


def render_sphere(markers: Markers, position, diameter, color, index=None) -> int:
    """A sphere of ``diameter`` at ``position``."""
    size = torch.cat([0.5 * markers._env(diameter, 1), torch.zeros(markers.num_envs, 2, dtype=torch.float64, device=markers.device)], 1)
    return markers.row(SPHERE, position, (0.0, 0.0, 0.0), size, color, index)


def render_line(markers: Markers, initial_point, target_point, width, color, index=None) -> int:
    """A capsule of radius ``width`` from ``initial_point`` to ``target_point`` (zero length: not drawn)."""
    p0 = markers._env(initial_point, 3)
    size = torch.cat([markers._env(width, 1), torch.zeros(markers.num_envs, 2, dtype=torch.float64, device=markers.device)], 1)
    return markers.row(CAPSULE, p0, markers._env(target_point, 3) - p0, size, color, index)


def render_frame(markers: Markers, pos, quat_wxyz, scale, alpha=1.0, index=(None, None, None)) -> tuple[int, int, int]:
    """Three lines from ``pos``, red / green / blue, of length ``scale`` and width ``0.02 scale``.  As in the reference, the red "x" line
    runs along COLUMN 1 of the rotation and the green "y" line along column 0 (its quirk, kept); blue is column 2."""
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError('alpha must be in [0, 1]')
    q = markers._env(quat_wxyz, 4)
    w, x, y, z = (q / torch.linalg.norm(q, dim=1, keepdim=True)).unbind(1)
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                     torch.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                     torch.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)
    s = markers._env(scale, 1)
    p = markers._env(pos, 3)
    ids = []
    for col, rgb, i in zip((1, 0, 2), ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), index):
        ids.append(render_line(markers, p, p + R[:, :, col] * s, 0.02 * s, (*rgb, float(alpha)), i))
    return tuple(ids)


def velocity_markers(env, markers: Markers | None = None) -> Markers:
    """The arrows the reference's ``render()`` draws: the commanded base velocity (world axes) in orange (1, 0.5, 0, 0.7) from base +
    (0, 0, 0.10) m and the actual one in cyan (0, 1, 1, 0.7) from base + (0, 0, 0.15) m, each of length |v|; with external
    disturbances configured, also the applied base force in red (1, 0, 0, 0.7) from base + (0, 0, 0.2) m, length 0.1."""
    m = markers if markers is not None else Markers(env.num_envs, env.device)
    base = env.qpos[:, 0:3].double()
    cmd_h, _ = env.target_base_vel()   # heading frame: rotate by the base yaw into the world
    qw, qx, qy, qz = env.qpos[:, 3:7].double().unbind(1)
    yaw = torch.atan2(2 * (qw * qz + qx * qy), 1 - 2 * (qy * qy + qz * qz))
    c, s = torch.cos(yaw), torch.sin(yaw)
    cmd_h = cmd_h.double()
    ref = torch.stack([c * cmd_h[:, 0] - s * cmd_h[:, 1], s * cmd_h[:, 0] + c * cmd_h[:, 1], cmd_h[:, 2]], 1)
    vel = env.qvel[:, 0:3].double()
    up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=base.device)
    render_vector(m, ref, base + 0.10 * up, torch.linalg.norm(ref, dim=1), (1.0, 0.5, 0.0, 0.7))
    render_vector(m, vel, base + 0.15 * up, torch.linalg.norm(vel, dim=1), (0.0, 1.0, 1.0, 0.7))
    if getattr(env, 'external_disturbances_kwargs', None) is not None:
        render_vector(m, env._applied[:, 0:3].double(), base + 0.2 * up, 0.1, (1.0, 0.0, 0.0, 0.7))
    return m


# ---- the reference's change_robot_appearance palette (visual.py), applied to a geom material table
ROBOT_COLOR = (0.054, 0.415, 0.505)     # teal
FL_COLOR = (0.698, 0.376, 0.082)        # orange
FR_COLOR = (0.260, 0.263, 0.263)        # grey
HL_COLOR = (0.800, 0.480, 0.000)        # yellow
HR_COLOR = (0.710, 0.703, 0.703)        # light grey


def tint_color(body_name: str):
    """The reference's body-name substring rule, verbatim and in its order ('left' matches FL first, 'right' FR first)."""
    n = body_name.lower()
    if any(s in n for s in ['fl_', 'lf_', 'left', '_0']):
        return FL_COLOR
    if any(s in n for s in ['fr_', 'rf_', 'right', '_120']):
        return FR_COLOR
    if any(s in n for s in ['rl_', 'hl_', 'lh_', 'left']):
        return HL_COLOR
    if any(s in n for s in ['rr_', 'hr_', 'rh_', 'right']):
        return HR_COLOR
    return ROBOT_COLOR


def tinted_geom_mat(md, geom_mat) -> np.ndarray:
    """A copy of ``geom_mat`` [ngeom, 7] with the palette on the robot's geoms (body > 0, not transparent), alpha 1."""
    gm = np.array(geom_mat, dtype=np.float64, copy=True)
    for g in range(md.ngeom):
        b = int(md.geom_bodyid[g])
        name = md.body_names[b]
        if b == 0 or name in ('floor', 'plane', 'world', 'ground') or gm[g, 3] == 0.0 or not name:
            continue
        gm[g, :3] = tint_color(name)
        gm[g, 3] = 1.0
    return gm
