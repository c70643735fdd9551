"""A RECURRENT policy in the closed-loop rollout: a GRU cell and an MLP head in the policy seat (``QuadrupedEnv.rollout_policy`` with a
``GruPolicy`` -> ``gq_rollout_policy_gru``), the hidden state on the device in ``env.policy_hidden``.  The loop it replaces is

    for p in range(steps // decimation):
        h = cell(obs_row, h);  a = head(h)                             # a handful of small torch launches
        obs, ... = env.step_pd(q_default + action_scale * a, kp, kd, decimation=decimation)
        h = h * (1 - terminated)                                       # ... and the episode bookkeeping, at the policy's rate only

The rollout records what a recurrent learner needs (``record_transitions=True``): the rows the cell was fed, the hidden state FED at every
policy step (after the episode rule), the actions and ``dones``.  This example recomputes the hidden sequence in torch from those records
with the learner's mask ``h <- (1 - done) h`` and prints the difference: the state the device fed is the state backpropagation through
time would start from.

    python examples/gru_policy.py [n_envs] [steps]
"""
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gym_quadruped_amd.policy import GruPolicy  # noqa: E402
from gym_quadruped_amd.quadruped_env import QuadrupedEnv  # noqa: E402
from gym_quadruped_amd.reward import RewardSpec  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
K = int(sys.argv[2]) if len(sys.argv) > 2 else 400
D, KP, KD, SCALE, H = 4, 25.0, 0.8, 0.25, 64
names = ('qpos_js', 'qvel_js', 'base_lin_vel:base', 'base_ang_vel:base', 'gravity_vector:base', 'contact_state')   # the cell reads the first 33 columns
env = QuadrupedEnv('mini_cheetah', state_obs_names=names, num_envs=n, device='cuda:0', auto_reset='next_step', seed=3)
env.reset(random=True)

torch.manual_seed(0)
cell = torch.nn.GRUCell(33, H).to('cuda:0')
head = torch.nn.Sequential(torch.nn.Linear(H, 64), torch.nn.ELU(), torch.nn.Linear(64, 12), torch.nn.Tanh()).to('cuda:0')
policy = GruPolicy.from_torch(cell, head)

K = K // D * D
torch.cuda.synchronize(); t0 = time.perf_counter()
out = env.rollout_policy(K, policy, KP, KD, action_scale=SCALE, decimation=D, noise_sigma=0.5, record_transitions=True, reward=RewardSpec(alive=1.0, termination=-1.0))
torch.cuda.synchronize(); dt = time.perf_counter() - t0
fed, rows, dones = out['policy_hidden'], out['policy_obs'], out['dones']
print(f'rollout_policy(GruPolicy): {n * K / dt / 1e6:7.2f} M env-steps/s ({dt / K * 1e6:.1f} us per step, a new action every {D} steps); '
      f'{int(dones.sum())} of {dones.numel()} windows ended an episode')

# the hidden sequence again, in torch, from the recorded rows and the dones mask
with torch.no_grad():
    h = fed[0]
    worst_h = worst_a = 0.0
    for s in range(K // D):
        worst_h = max(worst_h, float((h - fed[s]).abs().max()))
        h = cell(rows[s], h)
        worst_a = max(worst_a, float((head(h) - out['policy_means'][s]).abs().max()))
        h = h * (~dones[s]).float().unsqueeze(1)
    worst_h = max(worst_h, float((h - env.policy_hidden).abs().max()))
zero_where_done = bool(((fed[1:] == 0).all(dim=2) == dones[:-1]).all())
print(f'hidden sequence recomputed in torch with h <- (1 - done) h: max |difference| {worst_h:.2e} (actions {worst_a:.2e}) over {K // D} policy steps; '
      f'the fed state is zero exactly where the window before was done: {zero_where_done}')
env.close()
