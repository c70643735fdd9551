"""Throughput of the learning rollout with and without the foot terms of the reward, and of what the foot terms replace
(profiles/foot_reward_throughput.txt).
usage: foot_reward_probe.py robot n_envs [K] [--runs R] [--forms learn,feet,replaced] [--tag TEXT]

Workload as tools/closed_loop_probe.py --mlp 256,128,64 --learn: flat, network (256, 128, 64) elu on 33 observation columns, K = 96 physics
steps per call, decimation 4, 128 policy wavefronts, exploration noise 0.1, forward commands; the observation row carries the twelve terms'
observables and the feet's behind the network's columns (82 columns) in EVERY form.  Forms, timed in turn R times over from the same state:

  learn     rollout_policy(reward=<the twelve terms>, record_transitions=True) - no foot term: gq_rollout_policy_learn.  This form runs on
            the parent commit as well (--forms learn), which is how the two commits are compared.
  feet      the same call with feet=FootRewardSpec(all four terms): gq_rollout_policy_learn_feet
  replaced  what `feet` replaces: rollout_policy(record_obs=True, record_actions=True), the twelve terms and the four foot terms as torch
            expressions over obs_seq, the air-time recurrence as a torch loop over the K steps, summed per window; policy_eval for the means
            (no termination bookkeeping: obs_seq does not carry the flags)."""
import sys, time
from pathlib import Path
import torch
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gym_quadruped_amd.policy import MlpPolicy
from gym_quadruped_amd.quadruped_env import QuadrupedEnv
from gym_quadruped_amd.reward import RewardSpec


def _opt(name, default, conv):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    v = conv(sys.argv[i + 1])
    del sys.argv[i:i + 2]
    return v


RUNS = _opt('--runs', 3, int)
FORMS = _opt('--forms', ['learn', 'feet', 'replaced'], lambda t: t.split(','))
TAG = _opt('--tag', '', str)
robot, n = sys.argv[1], int(sys.argv[2])
K = int(sys.argv[3]) if len(sys.argv) > 3 else 96
KP, KD, D, scale, sigma, pw = 25.0, 0.8, 4, 0.25, 0.1, 128
names = ('qpos_js', 'qvel_js', 'base_lin_vel:base', 'base_ang_vel:base', 'gravity_vector:base', 'base_pos', 'base_lin_vel_err:base', 'base_ang_vel_err:base',
         'contact_state', 'contact_forces', 'feet_vel', 'feet_pos:base')
env = QuadrupedEnv(robot, scene='flat', state_obs_names=names, base_vel_command_type='forward', ref_base_lin_vel=(0.0, 1.0), num_envs=n, auto_reset='next_step', seed=1)
env.reset(random=True)
torch.manual_seed(0)
dims = [33, 256, 128, 64, 12]
mods = []
for a, b in zip(dims[:-1], dims[1:]):
    mods += [torch.nn.Linear(a, b), torch.nn.ELU()]
policy = MlpPolicy.from_torch(torch.nn.Sequential(*mods[:-1]).to('cuda'))
W = K // D
env.rollout_policy(300 // D * D, policy, KP, KD, action_scale=scale, decimation=D)   # settle into the policy's regime
wt = dict(track_lin_vel=1.0, track_ang_vel=0.5, lin_vel_z=-2.0, ang_vel_xy=-0.05, orientation=-0.2, base_height=-30.0, torques=-1e-5, joint_vel=-1e-3,
          power=-2e-5, action_rate=-0.01, alive=0.25)
fw = dict(air_time=1.0, slip=-0.1, impact=-0.01, clearance=-5.0)
fp = dict(air_time_target=0.2, min_cmd_speed=0.5, impact_limit=10.0, clearance_target=-0.2)
spec = RewardSpec(base_height_target=0.3, **wt)
with_feet = None
if 'feet' in FORMS or 'replaced' in FORMS:
    from gym_quadruped_amd.reward import FootRewardSpec
    with_feet = RewardSpec(base_height_target=0.3, feet=FootRewardSpec(**fw, **fp), **wt)
sd, launches, row0, dt = env.state_dict(), env._launches, env._obs_buf.clone(), env.simulation_dt
kw = dict(action_scale=scale, decimation=D, noise_sigma=sigma, policy_waves=pw)


def restore():
    env.load_state_dict(sd); env._launches = launches; env._obs_buf.copy_(row0); torch.cuda.synchronize()


def learn():
    return env.rollout_policy(W * D, policy, KP, KD, reward=spec, record_transitions=True, **kw)


def feet():
    return env.rollout_policy(W * D, policy, KP, KD, reward=with_feet, record_transitions=True, **kw)


def replaced():
    first = env._obs_buf[:, :33].clone()
    r = env.rollout_policy(W * D, policy, KP, KD, record_obs=True, record_actions=True, **kw)
    o, u, pol = r['obs_seq'], r['actions'], r['policy_actions']
    qd, vb, wb, gv, z, el, ea = o[..., 12:24], o[..., 24:27], o[..., 27:30], o[..., 30:33], o[..., 35], o[..., 36:39], o[..., 39:42]
    c, fz = o[..., 42:46] != 0, o[..., 46:58].view(W * D, n, 4, 3)[..., 2]
    fv, zb = o[..., 58:70].view(W * D, n, 4, 3), o[..., 70:82].view(W * D, n, 4, 3)[..., 2]
    v2 = (fv[..., :2] ** 2).sum(-1)
    a = pol.repeat_interleave(D, dim=0)
    ap = torch.cat([pol[:1], pol[:-1]]).repeat_interleave(D, dim=0)
    gate = ((el[..., :2] + vb[..., :2]) ** 2).sum(-1) > fp['min_cmd_speed'] ** 2
    t, A = env.feet_air_time.clone(), []
    for k in range(W * D):   # the recurrence: what a stateless expression over rows cannot do
        tn = t + dt
        A.append(torch.where(c[k] & (t > 0), tn - fp['air_time_target'], torch.zeros_like(t)).sum(-1))
        t = torch.where(c[k], torch.zeros_like(t), tn)
    env.feet_air_time = t
    A = torch.stack(A) * gate
    rew = dt * (wt['track_lin_vel'] * torch.exp(-(el[..., :2] ** 2).sum(-1) / 0.25) + wt['track_ang_vel'] * torch.exp(-ea[..., 2] ** 2 / 0.25)
                + wt['lin_vel_z'] * vb[..., 2] ** 2 + wt['ang_vel_xy'] * (wb[..., :2] ** 2).sum(-1) + wt['orientation'] * (gv[..., :2] ** 2).sum(-1)
                + wt['base_height'] * (z - 0.3) ** 2 + wt['torques'] * (u ** 2).sum(-1) + wt['joint_vel'] * (qd ** 2).sum(-1)
                + wt['power'] * (u * qd).abs().sum(-1) + wt['action_rate'] * ((a - ap) ** 2).sum(-1) + wt['alive']
                + fw['air_time'] * A + fw['slip'] * (v2 * c).sum(-1) + fw['impact'] * (fz - fp['impact_limit']).clamp(min=0).sum(-1)
                + fw['clearance'] * ((zb - fp['clearance_target']) ** 2 * v2).sum(-1))
    rewards = rew.view(W, D, n).sum(1)
    rows = torch.cat([first[None], o[D - 1:-1:D, :, :33]])
    means = env.policy_eval(policy, rows.reshape(W * n, 33)).view(W, n, 12)
    return rewards, means


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    s = time.perf_counter() - t0
    return n * W * D / s / 1e6, s / (W * D) * 1e6


forms = [(nm, fn) for nm, fn in (('learn', learn), ('feet', feet), ('replaced', replaced)) if nm in FORMS]
label = dict(learn='learn: reward (12 terms) + record_transitions', feet='feet: the same + the four foot terms', replaced='replaced: record_obs + torch terms + recurrence')
for _, fn in forms:   # warm every path
    restore(); fn()
if 'feet' in FORMS and 'replaced' in FORMS:   # the two forms agree where no env terminated
    restore(); got = feet(); air_got = env.feet_air_time.clone(); restore(); want = replaced()
    quiet = ~got['dones'].any(0)
    print(f'feet vs replaced: |rewards| differ by at most {float((got["rewards"] - want[0])[:, quiet].abs().max()):.2e} over the {int(quiet.sum())} envs without a '
          f'termination (max |reward| {float(want[0].abs().max()):.3f}); air times differ by at most {float((air_got - env.feet_air_time)[quiet].abs().max()):.2e}; '
          f'means equal: {torch.equal(got["policy_means"], want[1])}', flush=True)
tag = f'{TAG}{robot} flat n={n} K={W * D} D={D} waves={pw}'
for r in range(RUNS):
    for nm, fn in forms:
        restore(); m, us = timed(fn)
        print(f'{tag} run {r}: {label[nm]:50s} {m:7.2f} M env-steps/s  {us:6.1f} us/step  status {env.closed_loop_status()}', flush=True)
print(f'{tag}: episodes max {int(env._episode.max())}', flush=True)
