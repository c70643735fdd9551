"""A policy that sends JOINT TARGETS at 125 Hz while the physics runs at 500 Hz: what a legged robot's low-level interface takes
(q_des, qd_des, tau_ff, kp, kd per joint) and what most learned controllers output.

    for each policy step:
        q_des = policy(obs)                                     # here: the standing posture + a per-env trot-like sine on the joints
        obs, reward, terminated, truncated, info = env.step_pd(q_des, kp, kd, decimation=4)

``step_pd`` is ONE launch per policy step: the wavefront that steps an env evaluates tau = kp (q_des - q) + kd (qd_des - qd) + tau_ff at
every 2 ms substep from the env's fresh joint state and plays the four substeps back to back.  The loop it replaces - four ``step``
calls with the torch PD expression in between - leaves the same bits (shown below) at four launches and a dozen small torch kernels
per policy step.

    python examples/joint_targets.py [n_envs] [policy steps]
"""
import math
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gym_quadruped_amd.quadruped_env import QuadrupedEnv  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
K = int(sys.argv[2]) if len(sys.argv) > 2 else 250
D = 4
mk = lambda: QuadrupedEnv('mini_cheetah', state_obs_names=('base_lin_vel', 'base_ori_euler_xyz', 'contact_state'), num_envs=n, device='cuda:0',
                          auto_reset='next_step', seed=3)   # (no joint columns in the observation row: the law reads the state)
key = None
phase = torch.rand(n, 1, device='cuda:0') * 2 * math.pi      # every env its own gait phase
amp = torch.tensor([0.0, 0.25, -0.4] * 4, device='cuda:0')   # hip, thigh, calf
kp = torch.tensor([40.0, 40.0, 50.0] * 4)                    # 12 values: one row for the batch (a [N, 12] tensor gives per-env gains)
kd = 1.0


def policy(t):
    return key + amp * torch.sin(2 * math.pi * 2.0 * t + phase)


# 1. one launch per policy step
env = mk()
env.reset(random=True)
key = env._key_qpos[7:19].float()
fallen = torch.zeros(n, dtype=torch.bool, device='cuda:0')
torch.cuda.synchronize(); t0 = time.perf_counter()
for k in range(K):
    obs, reward, terminated, truncated, info = env.step_pd(policy(k * D * 0.002), kp, kd, decimation=D)
    fallen |= terminated                                     # OR over the window: a robot that fell and re-spawned inside it is not missed
torch.cuda.synchronize(); dt = time.perf_counter() - t0
print(f'step_pd, decimation {D}:                      {n * K * D / dt / 1e6:7.2f} M env-steps/s  ({dt / K * 1e6:.1f} us per policy step), '
      f'{int(fallen.sum())} of {n} envs fell at least once')

# 2. the loop it replaces
ref = mk()
ref.reset(random=True)
kpd = kp.to('cuda:0')
torch.cuda.synchronize(); t0 = time.perf_counter()
for k in range(K):
    q_des = policy(k * D * 0.002)
    for _ in range(D):
        tau = kpd * (q_des - ref.qpos[:, 7:].float()) + kd * (0.0 - ref.qvel[:, 6:]) + 0.0
        ref.step(tau)
torch.cuda.synchronize(); dt = time.perf_counter() - t0
print(f'{D} x (torch PD expression, step) per policy step: {n * K * D / dt / 1e6:7.2f} M env-steps/s  ({dt / K * 1e6:.1f} us per policy step)')
print('same state afterwards, bit for bit:', bool(torch.equal(env.qpos, ref.qpos) and torch.equal(env.qvel, ref.qvel)))
