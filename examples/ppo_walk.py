"""The PPO loop of examples/ppo_rollout.py on a WALKING task: forward velocity commands, and the foot terms of the reward - the touchdown
reward on foot air time that makes a gait emerge, with penalties on slipping stance feet, hard landings and low swing feet
(``RewardSpec(..., feet=FootRewardSpec(...))``).  The air times are state the env owns (``env.feet_air_time``): they cross windows and
calls on the device, and are zeroed when an env re-spawns.

A minimal PPO loop around the learning rollout: the actor is a torch module that is packed into the device policy every iteration
(``MlpPolicy.from_torch``), ONE ``rollout_policy(..., reward=spec, record_transitions=True)`` per iteration plays ``K`` physics steps of
every env with the network, the exploration noise, the control law, the reward and the window bookkeeping on the device, and returns -
at the policy's rate - what the update needs:

    policy_obs   [K // D, N, in_dim]   the row the network saw            -> the critic's input, the actor's input in the update
    policy_means [K // D, N, 12]       its output before the noise        -> the old log-probability (with policy_actions and sigma)
    policy_actions                     mean + sigma z, as applied
    rewards      [K // D, N]           the task reward summed per window
    dones        [K // D, N]           the env fell inside the window     -> GAE stops there (the new episode starts at the next window)

The rest is plain torch: a critic, GAE, the clipped surrogate.  It is an example, not a benchmark of learning: a few iterations, printing
the mean window reward, the falls and the mean air time of the feet that are off the ground.

    python examples/ppo_walk.py [n_envs] [iterations]
"""
import math
import sys
from pathlib import Path

import torch
import torch.nn as nn

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gym_quadruped_amd.policy import MlpPolicy  # noqa: E402
from gym_quadruped_amd.quadruped_env import QuadrupedEnv  # noqa: E402
from gym_quadruped_amd.reward import FootRewardSpec, RewardSpec  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K, D, KP, KD, SCALE, SIGMA = 96, 4, 25.0, 0.8, 0.25, 0.2
GAMMA, LAM, CLIP, EPOCHS, BATCHES = 0.99, 0.95, 0.2, 4, 4
# the network reads the first 33 columns; the reward's observables follow them
names = ('qpos_js', 'qvel_js', 'base_lin_vel:base', 'base_ang_vel:base', 'gravity_vector:base', 'base_pos', 'base_lin_vel_err:base', 'base_ang_vel_err:base',
         'contact_state', 'contact_forces', 'feet_vel', 'feet_pos:base')
env = QuadrupedEnv('mini_cheetah', state_obs_names=names, base_vel_command_type='forward', ref_base_lin_vel=(0.3, 0.8), num_envs=n, device='cuda:0',
                   auto_reset='next_step', seed=3)
env.reset(random=True)
spec = RewardSpec(track_lin_vel=1.0, track_ang_vel=0.5, lin_vel_z=-2.0, ang_vel_xy=-0.05, orientation=-1.0, base_height=-20.0, torques=-1e-5, action_rate=-0.01,
                  alive=0.5, termination=-1.0, base_height_target=float(env._key_qpos[2]),
                  feet=FootRewardSpec(air_time=2.0, air_time_target=0.1, min_cmd_speed=0.1, slip=-0.05, impact=-1e-3, impact_limit=60.0,
                                      clearance=-2.0, clearance_target=-0.2))
assert set(spec.required_obs()) <= set(names)

torch.manual_seed(0)
dev = 'cuda:0'
actor = nn.Sequential(nn.Linear(33, 256), nn.ELU(), nn.Linear(256, 128), nn.ELU(), nn.Linear(128, 64), nn.ELU(), nn.Linear(64, 12)).to(dev)
critic = nn.Sequential(nn.Linear(33, 256), nn.ELU(), nn.Linear(256, 128), nn.ELU(), nn.Linear(128, 1)).to(dev)
with torch.no_grad():
    actor[-1].weight.mul_(0.1); actor[-1].bias.zero_()   # start near the keyframe
opt = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()), lr=3e-4)


def log_prob(mean, action):
    return (-0.5 * ((action - mean) / SIGMA) ** 2 - math.log(SIGMA) - 0.5 * math.log(2 * math.pi)).sum(-1)


W = K // D
for it in range(iters):
    out = env.rollout_policy(K, MlpPolicy.from_torch(actor), KP, KD, action_scale=SCALE, decimation=D, noise_sigma=SIGMA, reward=spec, record_transitions=True)
    obs, means, acts, rew, done = out['policy_obs'], out['policy_means'], out['policy_actions'], out['rewards'], out['dones'].float()
    with torch.no_grad():
        old_lp = log_prob(means, acts)
        v = critic(obs).squeeze(-1)                                    # [W, N]
        v_last = critic(env._obs_buf[:, :33]).squeeze(-1)              # the value of the row after the last window
        adv, gae = torch.zeros_like(rew), torch.zeros(n, device=dev)
        for s in reversed(range(W)):
            nxt = v_last if s == W - 1 else v[s + 1]
            delta = rew[s] + GAMMA * nxt * (1 - done[s]) - v[s]
            gae = delta + GAMMA * LAM * (1 - done[s]) * gae
            adv[s] = gae
        ret = adv + v
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    flat = lambda t: t.reshape(W * n, *t.shape[2:])
    f_obs, f_act, f_lp, f_adv, f_ret = flat(obs), flat(acts), flat(old_lp), flat(adv), flat(ret)
    for _ in range(EPOCHS):
        for idx in torch.randperm(W * n, device=dev).chunk(BATCHES):
            ratio = (log_prob(actor(f_obs[idx]), f_act[idx]) - f_lp[idx]).exp()
            surrogate = torch.min(ratio * f_adv[idx], ratio.clamp(1 - CLIP, 1 + CLIP) * f_adv[idx]).mean()
            loss = -surrogate + 0.5 * (critic(f_obs[idx]).squeeze(-1) - f_ret[idx]).pow(2).mean()
            opt.zero_grad(); loss.backward(); opt.step()
    air = env.feet_air_time
    print(f'iteration {it:3d}: mean window reward {float(rew.mean()):+.5f}, windows with a fall {int(done.sum())} of {W * n}, feet in the air '
          f'{int((air > 0).sum())} of {4 * n}, their mean air time {float(air[air > 0].mean()) if bool((air > 0).any()) else 0.0:.3f} s', flush=True)
env.close()
