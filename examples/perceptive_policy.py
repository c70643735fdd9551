"""A PERCEPTIVE policy in the closed-loop rollout: aliengo on the ``perlin`` terrain, an 11 x 17 height scan around the base in the input row
of a small MLP (``MlpPolicy(..., height_scan=HeightScan(11, 17, ...))`` -> ``gq_rollout_policy_scan``).  The env's
``HeightMap(follow_base=True)`` is the map the STEPPING wavefront writes at every step; the policy seat reads it where it lies, next to the
observation row.  The loop it replaces is

    for p in range(steps // decimation):
        hits = height_map.update_height_map()                                      # (the last step wrote it)
        scan = clamp((obs['base_pos'][:, 2:3] - offset) - hits[..., 2], -clip, clip) * scale
        a = net(cat(obs_row[:, :in_obs], scan, a_prev))
        obs, ... = env.step_pd(q_default + action_scale * a, kp, kd, decimation=decimation)

The rollout records what the network was fed (``record_transitions=True``); this example rebuilds the first policy step's row in torch from
``env.height_scan`` and shows where the scan columns sit.

    python examples/perceptive_policy.py [n_envs] [steps]
"""
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gym_quadruped_amd.policy import HeightScan, MlpPolicy  # noqa: E402
from gym_quadruped_amd.quadruped_env import QuadrupedEnv  # noqa: E402
from gym_quadruped_amd.reward import RewardSpec  # noqa: E402
from gym_quadruped_amd.sensors import HeightMap  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
K = int(sys.argv[2]) if len(sys.argv) > 2 else 400
D, KP, KD, SCALE = 4, 40.0, 1.0, 0.25
# the network reads the first 33 columns; base_pos (the scan's z) stands behind them
names = ('qpos_js', 'qvel_js', 'base_lin_vel:base', 'base_ang_vel:base', 'gravity_vector:base', 'base_pos')
IN_OBS = 33
env = QuadrupedEnv('aliengo', scene='perlin', state_obs_names=names, num_envs=n, device='cuda:0', auto_reset='next_step', seed=3)
height_map = HeightMap(11, 17, 0.1, 0.1, env.mjModel, env, follow_base=True)   # 1.1 m x 1.7 m around the base, in its heading frame
env.reset(random=True)

scan = HeightScan(11, 17, offset=0.35, clip=0.5, scale=2.0)   # 0 where the ground lies 0.35 m under the base; +-1 at half a metre above / below that
torch.manual_seed(0)
net = torch.nn.Sequential(torch.nn.Linear(IN_OBS + scan.cells + 12, 128), torch.nn.ELU(), torch.nn.Linear(128, 64), torch.nn.ELU(), torch.nn.Linear(64, 12),
                          torch.nn.Tanh()).to('cuda:0')
policy = MlpPolicy.from_torch(net, feed_last_action=True, height_scan=scan)
print(f'input row: {policy.in_obs} observation columns | {scan.cells} scan columns | 12 action columns = {policy.in_dim}')

K = K // D * D
first_row, first_scan = env._obs_buf.clone(), env.height_scan(scan)   # what the first policy step will be fed (the map is brought up to date)
torch.cuda.synchronize(); t0 = time.perf_counter()
out = env.rollout_policy(K, policy, KP, KD, action_scale=SCALE, decimation=D, noise_sigma=0.3, record_transitions=True, reward=RewardSpec(alive=1.0, termination=-1.0))
torch.cuda.synchronize(); dt = time.perf_counter() - t0
print(f'rollout_policy(height scan): {n * K / dt / 1e6:7.2f} M env-steps/s ({dt / K * 1e6:.1f} us per step, a new action every {D} steps)')
print('dict keys:', ', '.join(f'{k} {tuple(v.shape)}' for k, v in out.items() if torch.is_tensor(v)))

rows = out['policy_obs']
rebuilt = torch.cat([first_row[:, :IN_OBS], first_scan, torch.zeros(n, 12, device='cuda:0')], dim=1)
print(f'policy_obs[0] rebuilt from the observation row and env.height_scan: identical = {torch.equal(rows[0], rebuilt)}')
fed = rows[:, :, IN_OBS:IN_OBS + scan.cells]
print(f'scan columns over the rollout: min {float(fed.min()):+.3f}, max {float(fed.max()):+.3f}, saturated {float((fed.abs() == scan.clip * scan.scale).float().mean()):.1%}; '
      f'{int(out["dones"].sum())} of {out["dones"].numel()} windows ended an episode')
with torch.no_grad():
    print(f'network in torch on the recorded rows: max |difference| to policy_means {float((net(rows) - out["policy_means"]).abs().max()):.2e}')
# the scan of the state the rollout left (the last step wrote the map): a critic's input, at no ray launch
print(f'env.height_scan after the rollout: {tuple(env.height_scan(scan).shape)}, map current = {env._hm_fresh}')
env.close()
