"""A neural policy IN the closed-loop rollout: a small MLP between the published observation rows and the action mailboxes, evaluated by
a resident policy kernel on the matrix cores (``QuadrupedEnv.rollout_policy`` -> ``gq_rollout_policy``).  The loop it replaces is

    for p in range(steps // decimation):
        a = net(obs_row)                                               # a handful of small torch launches
        obs, ... = env.step_pd(q_default + action_scale * a, kp, kd, decimation=decimation)

Here the network is random (small weights, tanh output): with ``action_scale = 0.1`` the batch stays near its keyframe, which is all
this example shows - plus that the torch module and the device policy are the same network.

    python examples/mlp_policy.py [n_envs] [steps]
"""
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gym_quadruped_amd.policy import MlpPolicy  # noqa: E402
from gym_quadruped_amd.quadruped_env import QuadrupedEnv  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
K = int(sys.argv[2]) if len(sys.argv) > 2 else 400
D, KP, KD, SCALE = 4, 25.0, 0.8, 0.1
names = ('qpos_js', 'qvel_js', 'base_lin_vel:base', 'base_ang_vel:base', 'gravity_vector:base', 'contact_state')   # the network reads the first 33 columns
env = QuadrupedEnv('mini_cheetah', state_obs_names=names, num_envs=n, device='cuda:0', auto_reset='next_step', seed=3)
env.reset(random=True)

torch.manual_seed(0)
net = torch.nn.Sequential(torch.nn.Linear(33, 64), torch.nn.ELU(), torch.nn.Linear(64, 64), torch.nn.ELU(), torch.nn.Linear(64, 12), torch.nn.Tanh()).to('cuda:0')
policy = MlpPolicy.from_torch(net)

# the device policy is the torch module: the matrix-core form against torch's float32 and against the plain fmaf loop that defines it
rows = env._obs_buf[:, :33].contiguous()
with torch.no_grad():
    want = net(rows)
tile, scalar = env.policy_eval(policy, rows, impl='tile'), env.policy_eval(policy, rows, impl='scalar')
print(f'policy_eval against the torch module: max difference {float((tile - want).abs().max()):.2e}; tile and scalar forms equal bit for bit: {bool(torch.equal(tile, scalar))}')

K = K // D * D
torch.cuda.synchronize(); t0 = time.perf_counter()
out = env.rollout_policy(K, policy, KP, KD, action_scale=SCALE, decimation=D, record_actions=True)
torch.cuda.synchronize(); dt = time.perf_counter() - t0
standing = int((out['obs']['contact_state'].sum(1) >= 3).sum())
drift = float((env.qpos[:, 7:].float() - env._key_qpos[7:19].float()).abs().max())
print(f'rollout_policy: {n * K / dt / 1e6:7.2f} M env-steps/s ({dt / K * 1e6:.1f} us per step, a new action every {D} steps); '
      f'{standing} of {n} envs stand, largest joint offset from the keyframe {drift:.2f} rad, largest |action| {float(out["policy_actions"].abs().max()):.2f}')
env.close()
