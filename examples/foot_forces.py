"""A batch that STANDS ON COMMANDED FOOT FORCES: what a whole-body / MPC controller sends between two solver updates - per foot a
force and a soft Cartesian impedance - held at a 100 Hz command rate over 500 Hz physics.

    for each command step:
        f_ff = -(ground reaction the controller wants)          # here: every foot carries a quarter of the weight, -m g / 4 along world z,
                                                                  # expressed in the base axes of the env's current orientation
        obs, reward, terminated, truncated, info = env.step_feet(p_des, kp, kd, f_ff=f_ff, frame='base', decimation=5)

``step_feet`` is ONE launch per command step: the wavefront that steps an env rebuilds the leg Jacobians from the env's fresh joint
state at every 2 ms substep and applies tau_leg = J^T (f_ff + kp (p_des - p) + kd (v_des - v)) + tau_ff.  A force command has no
joint-space form - the Jacobian must be fresh at every substep - so the alternative is five times (feet_jacobians, einsums, step) per
command step on an ``accessors=True`` env (tools/closed_loop_probe.py --foot-cmd 5 times both).

    python examples/foot_forces.py [n_envs] [command steps]
"""
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gym_quadruped_amd.quadruped_env import QuadrupedEnv  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
K = int(sys.argv[2]) if len(sys.argv) > 2 else 200
D = 5   # 500 Hz physics, 100 Hz commands
env = QuadrupedEnv('mini_cheetah', state_obs_names=('base_pos', 'base_ori_euler_xyz', 'feet_pos:base'), num_envs=n, device='cuda:0',
                   auto_reset='next_step', seed=3)
footholds = env.reset(random=False)['feet_pos:base'].clone()          # the keyframe footholds relative to the base, [N, 12] in legs_order
env.reset(random=True)
weight = float(env.mjModel.body_mass.sum()) * 9.81
kp, kd = [400.0, 400.0, 1500.0], 15.0                                 # per axis, N/m and N s/m: soft - the forces carry the robot; the PD in the
                                                                      # base frame holds the attitude (4 kp_z y^2 must exceed the toppling m g h)


def stance_forces(quat):
    """the force ON each foot, -m g / 4 along world z, in base axes: [N, 12]"""
    w, x, y, z = quat.float().unbind(1)
    up = torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1)   # world z in base axes
    return (-weight / 4 * up).repeat(1, 4)


fallen = torch.zeros(n, dtype=torch.bool, device='cuda:0')
torch.cuda.synchronize(); t0 = time.perf_counter()
for k in range(K):
    obs, reward, terminated, truncated, info = env.step_feet(footholds, kp, kd, f_ff=stance_forces(env.qpos[:, 3:7]), frame='base', decimation=D)
    fallen |= terminated                                              # OR over the window
torch.cuda.synchronize(); dt = time.perf_counter() - t0
z = obs['base_pos'][:, 2]
print(f'step_feet, decimation {D}: {n * K * D / dt / 1e6:7.2f} M env-steps/s  ({dt / K * 1e6:.1f} us per command step)')
print(f'after {K * D * 0.002:.1f} s: base height {float(z.mean()):.3f} m (min {float(z.min()):.3f}), '
      f'|roll|, |pitch| <= {float(obs["base_ori_euler_xyz"][:, :2].abs().max()):.3f} rad, {int(fallen.sum())} of {n} envs fell at least once')
