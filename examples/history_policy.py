"""A feed-forward policy WITH MEMORY in the closed-loop rollout: an MLP that reads the last few proprioceptive frames and the actions that
went with them (``MlpPolicy(..., feed_last_action=True, history=ObsHistory(frames, cols))`` -> ``gq_rollout_policy_hist``), the frames on the
device in ``env.policy_history``.  The torch loop it replaces and the rollout, side by side on twin envs - the same bits:

    hist = where(fell, 0, hist)                                        # the episode rule, at the policy's rate
    x = cat(obs_row[:, :in_obs], a_prev, hist.flatten(1));  a = policy(x)
    hist = cat(cat(obs_row[:, :cols], a_prev)[:, None], hist[:, :-1])  # the current block becomes the newest frame
    for k in range(decimation):                                        # the joint-impedance law on the held action, every step
        env.step(kp * (q_default + action_scale * a - q) - kd * qd)

    python examples/history_policy.py [n_envs] [steps]
"""
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gym_quadruped_amd.policy import MlpPolicy, ObsHistory  # noqa: E402
from gym_quadruped_amd.quadruped_env import QuadrupedEnv  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
K = int(sys.argv[2]) if len(sys.argv) > 2 else 200
D, KP, KD, SCALE, L, COLS, IN_OBS = 4, 25.0, 0.8, 0.25, 3, 24, 33
K = K // D * D
names = ('qpos_js', 'qvel_js', 'base_lin_vel:base', 'base_ang_vel:base', 'gravity_vector:base', 'contact_state')   # the network reads the first 33 columns
mk = lambda: QuadrupedEnv('mini_cheetah', state_obs_names=names, num_envs=n, device='cuda:0', auto_reset='next_step', seed=3)
loop_env, env = mk(), mk()
loop_env.reset(random=True); env.reset(random=True)

torch.manual_seed(0)
F = COLS + 12                                                          # a frame: joint angles and velocities, and the action fed with them
net = torch.nn.Sequential(torch.nn.Linear(IN_OBS + 12 + L * F, 128), torch.nn.ELU(), torch.nn.Linear(128, 64), torch.nn.ELU(), torch.nn.Linear(64, 12)).to('cuda:0')
policy = MlpPolicy.from_torch(net, feed_last_action=True, history=ObsHistory(L, COLS))
q0 = env._key_qpos[7:19].float()


def torch_loop(e, calls):
    """the loop the rollout replaces; the network itself through policy_eval, so that the two sides can be compared bit for bit"""
    hist, fell = torch.zeros(n, L, F, device='cuda:0'), e._terminated.bool()   # (the envs that wait for their re-spawn have fallen too)
    for _ in range(calls):
        a_prev = torch.zeros(n, 12, device='cuda:0')                  # the fed-back action is zero at a call's first policy step
        for s in range(K // D):
            hist = torch.where(fell[:, None, None], torch.zeros_like(hist), hist)
            row = e._obs_buf.clone()
            a = e.policy_eval(policy, torch.cat([row[:, :IN_OBS], a_prev, hist.flatten(1)], dim=1))
            hist = torch.cat([torch.cat([row[:, :COLS], a_prev], dim=1)[:, None], hist[:, :-1]], dim=1)
            fell = torch.zeros(n, dtype=torch.bool, device='cuda:0')
            for k in range(D):
                row = e._obs_buf
                e.step(KP * ((q0 + SCALE * a) - row[:, 0:12]) + KD * (0 - row[:, 12:24]) + 0)
                fell |= e._terminated.bool()
            a_prev = a
    return hist


for name, fn in (('torch loop', lambda: torch_loop(loop_env, 2)),
                 ('rollout_policy', lambda: [env.rollout_policy(K, policy, KP, KD, action_scale=SCALE, decimation=D) for _ in range(2)])):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print(f'{name:15s} {n * 2 * K / dt / 1e6:7.2f} M env-steps/s ({dt / (2 * K) * 1e6:.1f} us per step, a new action every {D} steps, {L} frames of {F} words)')
same = all(torch.equal(getattr(loop_env, f), getattr(env, f)) for f in ('_qpos', '_qvel', '_obs_buf', '_terminated', '_episode'))
print(f'two calls of {K} steps: state, observation rows and episode counts of the two sides are bit-equal: {same}; '
      f'episodes max {int(env._episode.max())}; env.policy_history {tuple(env.policy_history.shape)}')
loop_env.close(); env.close()
