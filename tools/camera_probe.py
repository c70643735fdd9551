"""Time gq_camera (sensors.Camera.render: the pose pass and the pixel pass) with HIP events for a batch of envs; with --rgb the shaded
call gq_camera_shaded (Camera(rgb=True), default Appearance) on the same cases; with --ghosts G / --markers K (implies --rgb) the layered
call gq_camera_layered with G ghosts (the env's pose shifted by 0.15 m steps in x and y, alpha 0.5) and K markers (spheres, lines and
arrows about the base).

    python tools/camera_probe.py [--envs 4096] [--frames 50] [--warmup 5] [--rgb] [--ghosts G] [--markers K] [--cases N]

Cases: aliengo robotcam 64 x 64 on flat, random_boxes and perlin; mini_cheetah 64 x 64 with a camera under the trunk looking back at
the legs; aliengo flat 128 x 128.  Prints one JSON line per case: median and spread of the per-frame time (ms)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gym_quadruped_amd.mjcf import mat_to_quat  # noqa: E402
from gym_quadruped_amd.quadruped_env import QuadrupedEnv  # noqa: E402
from gym_quadruped_amd.sensors import Camera  # noqa: E402

CASES = [('aliengo', 'flat', 64), ('aliengo', 'random_boxes', 64), ('aliengo', 'perlin', 64), ('mini_cheetah', 'flat', 64), ('aliengo', 'flat', 128)]


def layers(env, G, K):
    """render() keyword arguments of G ghosts and K markers (empty: the plain call)"""
    kw = {}
    if G:
        q = env.qpos.unsqueeze(1).repeat(1, G, 1)
        q[:, :, 0:2] += 0.15 * torch.arange(1, G + 1, device=q.device, dtype=q.dtype).unsqueeze(1)
        kw.update(ghost_qpos=q, ghost_alpha=0.5)
    if K:
        from gym_quadruped_amd.utils.visual import Markers, render_line, render_sphere, render_vector
        m = Markers(env.num_envs, env.device)
        b = env.qpos[:, 0:3].double()
        for k in range(K):
            off = torch.tensor([0.1 * (k % 4) - 0.15, 0.1 * (k // 4) - 0.2, 0.15], dtype=torch.float64, device=b.device)
            [lambda: render_sphere(m, b + off, 0.08, (1.0, 0.2, 0.2, 0.5)),
             lambda: render_line(m, b + off, b + off + 0.2, 0.02, (0.2, 1.0, 0.2, 0.6)),
             lambda: render_vector(m, (0.3, 0.2, 0.1), b + off, 0.3, (0.2, 0.2, 1.0, 0.7))][k % 3]()
        kw['markers'] = m
    return kw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rgb', action='store_true', help='time the shaded call (depth, segmentation and RGB)')
    ap.add_argument('--ghosts', type=int, default=0, help='ghost robots per env (gq_camera_layered)')
    ap.add_argument('--markers', type=int, default=0, help='markers per env (gq_camera_layered)')
    ap.add_argument('--cases', type=int, default=len(CASES), help='only the first N cases')
    a = ap.parse_args()
    a.rgb = a.rgb or a.ghosts > 0 or a.markers > 0
    for robot, scene, S in CASES[:a.cases]:
        env = QuadrupedEnv(robot, scene=scene, num_envs=a.envs, device='cuda:0', state_obs_names=('qpos',), seed=0)
        env.reset(seed=0)
        g = torch.Generator(device='cuda:0').manual_seed(0)
        for _ in range(30):
            env.step(torch.randn(a.envs, 12, generator=g, device='cuda:0') * 5.0)
        if robot == 'aliengo':
            cam = Camera(S, S, 30, env.robot_model, env.sim_data, cam_name='robotcam', rgb=a.rgb)
        else:
            q = mat_to_quat(np.stack([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], 1))
            cam = Camera(S, S, 30, env.robot_model, env.sim_data, body='base', pos=(0.35, 0.0, -0.12), quat=q, fovy=90.0, rgb=a.rgb)
        kw = layers(env, a.ghosts, a.markers)
        for _ in range(a.warmup):
            cam.render(**kw)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.frames):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); cam.render(**kw); e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        hit = float((cam._depth_plane < cam._zfar).float().mean())
        print(json.dumps(dict(robot=robot, scene=scene, size=S, rgb=a.rgb, ghosts=a.ghosts, markers=a.markers, envs=a.envs, frames=a.frames, median_ms=float(np.median(ms)),
                              p10_ms=float(np.percentile(ms, 10)), p90_ms=float(np.percentile(ms, 90)), hit_fraction=hit)), flush=True)
        env.close()
        del env, cam
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
