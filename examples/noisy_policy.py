"""SENSOR NOISE on what the in-loop policy observes (``rollout_policy(..., obs_noise=ObsNoise(...))`` -> ``gq_rollout_policy_noise``): the
network is fed joint encoders, gyro and velocity estimate with noise on them, while the drive's own control loop, the physics and the
learner's records of the true state are untouched.  The torch loop it replaces and the rollout, side by side on twin envs - the same bits:

    n_ref = draws(kind, seed, column, step0 + k, env id)                # one Philox block per noised word (csrc/gq_policy_noise.h)
    row_noisy = where(amp > 0, row + amp * n_ref, row);  a = policy(cat(row_noisy, a_prev))
    for k in range(decimation):                                         # the joint-impedance law on the TRUE joint state, every step
        env.step(kp * (q_default + action_scale * a - q) - kd * qd)

The loop's noise is rebuilt in numpy from the Philox reference of the tests (tests/obs_noise_ref.py on tests/philox_ref.py).

    python examples/noisy_policy.py [n_envs] [steps] [uniform|normal]
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))
import obs_noise_ref as R  # noqa: E402
from gym_quadruped_amd.policy import MlpPolicy, ObsNoise  # noqa: E402
from gym_quadruped_amd.quadruped_env import QuadrupedEnv  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
K = int(sys.argv[2]) if len(sys.argv) > 2 else 200
KIND = sys.argv[3] if len(sys.argv) > 3 else 'uniform'
D, KP, KD, SCALE, IN_OBS = 4, 25.0, 0.8, 0.25, 33
K = K // D * D
names = ('qpos_js', 'qvel_js', 'base_lin_vel:base', 'base_ang_vel:base', 'gravity_vector:base', 'contact_state')   # the network reads the first 33 columns
mk = lambda: QuadrupedEnv('mini_cheetah', state_obs_names=names, num_envs=n, device='cuda:0', auto_reset='next_step', seed=3)
loop_env, env = mk(), mk()
loop_env.reset(random=True); env.reset(random=True)

torch.manual_seed(0)
net = torch.nn.Sequential(torch.nn.Linear(IN_OBS + 12, 128), torch.nn.ELU(), torch.nn.Linear(128, 64), torch.nn.ELU(), torch.nn.Linear(64, 12)).to('cuda:0')
policy = MlpPolicy.from_torch(net, feed_last_action=True)
# a sim-to-real recipe's amplitudes, by observation name, in raw units: rad, rad/s, m/s, rad/s, and the unit gravity vector; contact_state has none
noise = ObsNoise.from_names(env, {'qpos_js': 0.01, 'qvel_js': 1.5, 'base_lin_vel:base': 0.1, 'base_ang_vel:base': 0.2, 'gravity_vector:base': 0.05}, kind=KIND)
amp = noise.table(policy)
q0 = env._key_qpos[7:19].float()


def torch_loop(e, calls):
    """the loop the rollout replaces; the network itself through policy_eval, so that the two sides can be compared bit for bit"""
    amp_t, cols, gids, seed = torch.from_numpy(amp).to('cuda:0'), np.flatnonzero(amp > 0), np.arange(n), int(e._seed)
    for _ in range(calls):
        step0 = int(e._launches) & 0x7fffffff                         # the counter the rollout keys its draws with
        a_prev = torch.zeros(n, 12, device='cuda:0')                  # the fed-back action is zero at a call's first policy step
        for s in range(K // D):
            n_ref = np.zeros((n, IN_OBS), dtype=np.float32)
            n_ref[:, cols] = R.draws(KIND, seed, cols, np.full(n, step0 + s * D), gids)
            row = e._obs_buf[:, :IN_OBS].clone()
            row_noisy = torch.where(amp_t > 0, row + amp_t * torch.from_numpy(n_ref).to('cuda:0'), row)
            a = e.policy_eval(policy, torch.cat([row_noisy, a_prev], dim=1))
            for k in range(D):
                true = e._obs_buf                                      # the drive's encoder loop reads the true joint state
                e.step(KP * ((q0 + SCALE * a) - true[:, 0:12]) + KD * (0 - true[:, 12:24]) + 0)
            a_prev = a
    return row_noisy


for name, fn in (('torch loop', lambda: torch_loop(loop_env, 2)),
                 ('rollout_policy', lambda: [env.rollout_policy(K, policy, KP, KD, action_scale=SCALE, decimation=D, obs_noise=noise) for _ in range(2)])):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print(f'{name:15s} {n * 2 * K / dt / 1e6:7.2f} M env-steps/s ({dt / (2 * K) * 1e6:.1f} us per step, a new action every {D} steps, {KIND} noise on {int((amp > 0).sum())} columns)')
same = all(torch.equal(getattr(loop_env, f), getattr(env, f)) for f in ('_qpos', '_qvel', '_obs_buf', '_terminated', '_episode'))
print(f'two calls of {K} steps: state, observation rows and episode counts of the two sides are bit-equal: {same}; episodes max {int(env._episode.max())}')
r = env.rollout_policy(D, policy, KP, KD, action_scale=SCALE, decimation=D, obs_noise=noise, record_transitions=True)
d = (r['policy_obs'] - r['policy_obs_clean'])[0]
print(f'policy_obs - policy_obs_clean, largest |difference| per observation: ' +
      ', '.join(f'{k} {float(d[:, a:b].abs().max()):.3f}' for k, a, b in (('qpos_js', 0, 12), ('qvel_js', 12, 24), ('lin vel', 24, 27), ('ang vel', 27, 30), ('gravity', 30, 33), ('action', 33, 45))))
loop_env.close(); env.close()
