"""Throughput of the closed-loop persistent rollout (gq_rollout_closed) with a PD policy in the loop, next to the step loop and the
open-loop persistent rollout fed with the SAME actions (a standing robot is a different workload from a randomly actuated one).
usage: closed_loop_probe.py [robot] [n_envs] [K] [scene] [--joint-cmd D | --foot-cmd D | --mlp H1,H2,H3 [--decimation D] [--policy-waves W1,W2,..] [--runs R] [--learn]
                             [--history L[,cols] [--scan R,C --side rollout]]
                             | --gru H [--mlp H1,H2] [--decimation D] [--policy-waves W1,..] [--runs R] [--side loop|rollout]]

--joint-cmd D: joint-impedance actions held over a window of D physics steps instead (QuadrupedEnv.step_pd, one launch per window)
against the loop they replace - D x (torch PD expression, env.step) - from the same state with the same per-env commands; K windows
per timing, five timings of each, alternating.  Prints env-steps/s of both, their spreads and the ratio.

--foot-cmd D: foot-space actions held over a window of D physics steps (QuadrupedEnv.step_feet, one launch per window: stance forces
-m g / 4 along world z per foot, a soft Cartesian PD on the keyframe footholds +- 2 cm per env, base frame) against the loop they replace on an
accessors=True env - D x (feet_jacobians, feet_pos, einsums for tau_leg = J_leg^T F, env.step) - with the same commands; timed the same way.

--mlp H1,H2,H3: an MLP policy with these hidden widths (elu, torch's default initialisation, 33 observation columns) in the closed-loop
rollout (QuadrupedEnv.rollout_policy, a new action every D steps: --decimation, default 4) against the loop it replaces on the same
commit - a = torch_module(obs); env.step_pd(q0 + scale * a, kp, kd, decimation=D) - from the same state with the same
network; one timing of the loop, then one of the rollout per entry of --policy-waves (default 64,128,256,512), R times over (--runs,
default 3).  Prints every run of both sides.  --obs-noise none|uniform|normal (with --mlp; use --side rollout: the torch loop stays clean): the
rollout with sensor noise on all 33 columns the network reads (ObsNoise.from_names: joint angles 0.01, joint velocities 1.5, base linear
velocity 0.1, angular velocity 0.2, gravity vector 0.05); none is the call without the switch.

--history L[,cols] (with --mlp): the network also reads the last action and the frames of the last L policy steps (ObsHistory(L, cols), cols
default 33: a 45-word frame; env.policy_history) - against the loop it replaces with the history kept in torch - hist = where(terminated, 0,
hist); cur = cat(obs, a_prev); a = module(cat(cur, hist)); step_pd; hist = cat(cur[:, :cols] | a_prev, hist[:, :-1]) - and against the
history-less rollout_policy of a network with the same hidden widths that reads the observation and the last action (the first entry of
--policy-waves), all three in turn, R times over.  --side rollout: the rollout with the history alone.  --scan R,C (with --side rollout, on
a scene with terrain such as perlin): the row also holds the R x C height scan of a base-following HeightMap (HeightScan(R, C), 0.1 m cells).

--gru H: a recurrent policy - torch.nn.GRUCell(33, H) and a head with the hidden widths of --mlp (default 128,64; elu) - in the closed-loop
rollout (QuadrupedEnv.rollout_policy with a GruPolicy, the hidden state in env.policy_hidden) against the loop it replaces on the same commit -
h = cell(obs, h); a = head(h); h = h * (1 - terminated); env.step_pd(q0 + scale * a, kp, kd, decimation=D) - from the same state with the same
weights; timed as --mlp is.  --side loop / rollout: that side alone, one timing per entry of --policy-waves (a process per timing).

--learn (with --mlp): the learning half instead.  The observation row gets the reward's observables behind the network's 33 columns, and
three forms are timed in turn, R times over, from the same state with the same network and exploration noise: plain rollout_policy; the
same call with reward= (every term on) and record_transitions=True; and what that replaces - rollout_policy(record_obs=True,
record_actions=True), the same reward terms as a torch expression over obs_seq summed per window, and policy_eval on the rows the network
saw for the means (no termination bookkeeping: obs_seq does not carry the flags).  Policy waves: the first entry of --policy-waves."""
import sys, time
from pathlib import Path
import torch
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gym_quadruped_amd.quadruped_env import QuadrupedEnv

JOINT_CMD = 0
if '--joint-cmd' in sys.argv:
    i = sys.argv.index('--joint-cmd')
    JOINT_CMD = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
FOOT_CMD = 0
if '--foot-cmd' in sys.argv:
    i = sys.argv.index('--foot-cmd')
    FOOT_CMD = int(sys.argv[i + 1])
    del sys.argv[i:i + 2]
def _opt(name, default, conv):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    v = conv(sys.argv[i + 1])
    del sys.argv[i:i + 2]
    return v
MLP = _opt('--mlp', None, lambda t: [int(h) for h in t.split(',')])
MLP_D = _opt('--decimation', 4, int)
MLP_WAVES = _opt('--policy-waves', [64, 128, 256, 512], lambda t: [int(w) for w in t.split(',')])
MLP_RUNS = _opt('--runs', 3, int)
HIST = _opt('--history', None, lambda t: [int(v) for v in t.split(',')])
SCAN = _opt('--scan', None, lambda t: [int(v) for v in t.split(',')])
GRU = _opt('--gru', 0, int)
SIDE = _opt('--side', None, str)
OBS_NOISE = _opt('--obs-noise', None, str)   # none | uniform | normal: sensor noise on the --mlp rollout's input row
LEARN = '--learn' in sys.argv
if LEARN:
    sys.argv.remove('--learn')
robot = sys.argv[1] if len(sys.argv) > 1 else 'mini_cheetah'
n = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
K = int(sys.argv[3]) if len(sys.argv) > 3 else 500
scene = sys.argv[4] if len(sys.argv) > 4 else 'flat'
KP, KD = 25.0, 0.8
mk = lambda: QuadrupedEnv(robot, scene=scene, state_obs_names=tuple(QuadrupedEnv.ALL_OBS), num_envs=n, auto_reset='next_step', seed=1)
env = mk()
env.reset(random=True)
g = torch.Generator(device='cuda').manual_seed(0)
pool = [torch.randn(n, 12, generator=g, device='cuda') * 50 for _ in range(16)]
for i in range(300): env.step(pool[i % 16])
torch.cuda.synchronize()

def timed(fn, steps):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return n * steps / dt / 1e6, dt / steps * 1e6

if GRU:
    from gym_quadruped_amd.policy import GruPolicy
    D, scale, head_w = MLP_D, 0.25, MLP or [128, 64]
    names = ('qpos_js', 'qvel_js', 'base_lin_vel:base', 'base_ang_vel:base', 'gravity_vector:base')   # 33 columns
    env = QuadrupedEnv(robot, scene=scene, state_obs_names=names, num_envs=n, auto_reset='next_step', seed=1)
    env.reset(random=True)
    torch.manual_seed(0)
    cell = torch.nn.GRUCell(33, GRU).to('cuda')
    dims = [GRU] + head_w + [12]
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [torch.nn.Linear(a, b), torch.nn.ELU()]
    head = torch.nn.Sequential(*mods[:-1]).to('cuda')
    policy = GruPolicy.from_torch(cell, head)
    q0 = env._key_qpos[7:19].float()
    W = max(1, K // D)
    env.rollout_policy(300 // D * D, policy, KP, KD, action_scale=scale, decimation=D)   # settle into the policy's regime
    sd = env.state_dict(); launches = env._launches
    row0 = env._obs_buf.clone()   # the policy's first action reads the observation row, which is no part of the checkpoint
    def restore():
        env.load_state_dict(sd); env._launches = launches; env._obs_buf.copy_(row0); torch.cuda.synchronize()
    def feature(pw):
        env.rollout_policy(W * D, policy, KP, KD, action_scale=scale, decimation=D, policy_waves=pw)
    def loop():
        with torch.no_grad():
            h = env.policy_hidden.clone()
            for w in range(W):
                h = cell(env._obs_buf, h)
                a = head(h)
                env.step_pd(q0 + scale * a, KP, KD, decimation=D)
                h = h * (1.0 - env._terminated.float()).unsqueeze(1)
    restore(); feature(0); restore(); loop()   # warm both paths
    tag = f'{robot} {scene} n={n} gru={GRU} head={head_w} D={D}'
    for r in range(MLP_RUNS):
        if SIDE in (None, 'loop'):
            restore(); m, us = timed(loop, W * D)
            print(f'{tag} run {r}: loop (torch GRUCell + head + step_pd)   {m:7.2f} M env-steps/s  {us:6.1f} us/step', flush=True)
        if SIDE in (None, 'rollout'):
            for pw in MLP_WAVES:
                restore(); m, us = timed(lambda: feature(pw), W * D)
                print(f'{tag} run {r}: rollout_policy, policy waves {pw:4d}       {m:7.2f} M env-steps/s  {us:6.1f} us/step  status {env.closed_loop_status()}', flush=True)
    print(f'{tag}: episodes max {int(env._episode.max())}', flush=True)
    sys.exit(0)

if MLP:
    from gym_quadruped_amd.policy import MlpPolicy
    D, scale = MLP_D, 0.25
    names = ('qpos_js', 'qvel_js', 'base_lin_vel:base', 'base_ang_vel:base', 'gravity_vector:base')   # 33 columns
    if LEARN:
        names += ('base_pos', 'base_lin_vel_err:base', 'base_ang_vel_err:base')
    if SCAN:
        names += ('base_pos',)   # the scan reads the base's z
    env = QuadrupedEnv(robot, scene=scene, state_obs_names=names, num_envs=n, auto_reset='next_step', seed=1)
    env.reset(random=True)
    torch.manual_seed(0)
    dims = [33] + MLP + [12]
    mods = []
    for a, b in zip(dims[:-1], dims[1:]):
        mods += [torch.nn.Linear(a, b), torch.nn.ELU()]
    module = torch.nn.Sequential(*mods[:-1]).to('cuda')
    policy = MlpPolicy.from_torch(module)
    q0 = env._key_qpos[7:19].float()
    W = max(1, K // D)
    env.rollout_policy(300 // D * D, policy, KP, KD, action_scale=scale, decimation=D)   # settle into the policy's regime
    sd = env.state_dict(); launches = env._launches
    def restore():
        env.load_state_dict(sd); env._launches = launches; torch.cuda.synchronize()
    nkw = {}
    if OBS_NOISE not in (None, 'none'):   # a sim-to-real recipe's amplitudes on every column the network reads (33), raw units
        from gym_quadruped_amd.policy import ObsNoise
        nkw = dict(obs_noise=ObsNoise.from_names(env, {'qpos_js': 0.01, 'qvel_js': 1.5, 'base_lin_vel:base': 0.1, 'base_ang_vel:base': 0.2, 'gravity_vector:base': 0.05},
                                                 kind=OBS_NOISE))
    def feature(pw):
        env.rollout_policy(W * D, policy, KP, KD, action_scale=scale, decimation=D, policy_waves=pw, **nkw)
    def loop():
        with torch.no_grad():
            for w in range(W):
                a = module(env._obs_buf)
                env.step_pd(q0 + scale * a, KP, KD, decimation=D)
    if LEARN:
        from gym_quadruped_amd.reward import RewardSpec
        wt = dict(track_lin_vel=1.0, track_ang_vel=0.5, lin_vel_z=-2.0, ang_vel_xy=-0.05, orientation=-0.2, base_height=-30.0, torques=-1e-5, joint_vel=-1e-3,
                  power=-2e-5, action_rate=-0.01, alive=0.25)
        spec = RewardSpec(base_height_target=0.3, **wt)
        pw, sigma, dt = MLP_WAVES[0], 0.1, env.simulation_dt
        row0 = env._obs_buf.clone()   # the policy's first action reads the observation row, which is no part of the checkpoint
        def restore():
            env.load_state_dict(sd); env._launches = launches; env._obs_buf.copy_(row0); torch.cuda.synchronize()
        kw = dict(action_scale=scale, decimation=D, noise_sigma=sigma, policy_waves=pw)
        def plain():
            env.rollout_policy(W * D, policy, KP, KD, **kw)
        def learn():
            return env.rollout_policy(W * D, policy, KP, KD, reward=spec, record_transitions=True, **kw)
        def replaced():
            first = env._obs_buf[:, :33].clone()
            r = env.rollout_policy(W * D, policy, KP, KD, record_obs=True, record_actions=True, **kw)
            o, u, pol = r['obs_seq'], r['actions'], r['policy_actions']
            qd, vb, wb, gv, z, el, ea = o[..., 12:24], o[..., 24:27], o[..., 27:30], o[..., 30:33], o[..., 35], o[..., 36:39], o[..., 39:42]
            a = pol.repeat_interleave(D, dim=0)
            ap = torch.cat([pol[:1], pol[:-1]]).repeat_interleave(D, dim=0)
            rew = dt * (wt['track_lin_vel'] * torch.exp(-(el[..., :2] ** 2).sum(-1) / 0.25) + wt['track_ang_vel'] * torch.exp(-ea[..., 2] ** 2 / 0.25)
                        + wt['lin_vel_z'] * vb[..., 2] ** 2 + wt['ang_vel_xy'] * (wb[..., :2] ** 2).sum(-1) + wt['orientation'] * (gv[..., :2] ** 2).sum(-1)
                        + wt['base_height'] * (z - 0.3) ** 2 + wt['torques'] * (u ** 2).sum(-1) + wt['joint_vel'] * (qd ** 2).sum(-1)
                        + wt['power'] * (u * qd).abs().sum(-1) + wt['action_rate'] * ((a - ap) ** 2).sum(-1) + wt['alive'])
            rewards = rew.view(W, D, n).sum(1)
            rows = torch.cat([first[None], o[D - 1:-1:D, :, :33]])
            means = env.policy_eval(policy, rows.reshape(W * n, 33)).view(W, n, 12)
            return rewards, means
        forms = (('rollout_policy, plain', plain), ('rollout_policy, reward + record_transitions', learn), ('record_obs + torch reward + policy_eval', replaced))
        for _, fn in forms:   # warm every path
            restore(); fn()
        restore(); got = learn(); restore(); want = replaced()   # the two forms agree where no env terminated inside the window
        quiet = ~got['dones'].any(0)
        print(f'learn vs replaced: |rewards| differ by at most {float((got["rewards"] - want[0])[:, quiet].abs().max()):.2e} over the {int(quiet.sum())} envs without a '
              f'termination (max |reward| {float(want[0].abs().max()):.3f}); means equal: {torch.equal(got["policy_means"], want[1])}', flush=True)
        tag = f'{robot} {scene} n={n} mlp={MLP} D={D} K={W * D} waves={pw}'
        for r in range(MLP_RUNS):
            for name, fn in forms:
                restore(); m, us = timed(fn, W * D)
                print(f'{tag} run {r}: {name:46s} {m:7.2f} M env-steps/s  {us:6.1f} us/step  status {env.closed_loop_status()}', flush=True)
        print(f'{tag}: episodes max {int(env._episode.max())}', flush=True)
        sys.exit(0)
    if HIST:
        from gym_quadruped_amd.policy import HeightScan, ObsHistory
        L, cols = HIST[0], HIST[1] if len(HIST) > 1 else 33
        F = cols + 12
        spec, cells = None, 0
        if SCAN:
            from gym_quadruped_amd.sensors import HeightMap
            assert SIDE == 'rollout', '--scan times the rollout alone: give --side rollout'
            hm = HeightMap(SCAN[0], SCAN[1], 0.1, 0.1, env.mjModel, env, follow_base=True)   # (the env holds a weak reference)
            spec, cells = HeightScan(SCAN[0], SCAN[1], offset=0.3, clip=0.5), SCAN[0] * SCAN[1]
        def net(k):
            dims, mods = [k] + MLP + [12], []
            for a, b in zip(dims[:-1], dims[1:]):
                mods += [torch.nn.Linear(a, b), torch.nn.ELU()]
            return torch.nn.Sequential(*mods[:-1]).to('cuda')
        module, module0 = net(45 + cells + L * F), net(45)
        policy = MlpPolicy.from_torch(module, feed_last_action=True, height_scan=spec, history=ObsHistory(L, cols))
        policy0 = MlpPolicy.from_torch(module0, feed_last_action=True)
        env.rollout_policy(300 // D * D, policy, KP, KD, action_scale=scale, decimation=D)   # fill the history in the policy's regime
        sd = env.state_dict(); launches = env._launches
        row0 = env._obs_buf.clone()   # the policy's first action reads the observation row, which is no part of the checkpoint
        def restore():
            env.load_state_dict(sd); env._launches = launches; env._obs_buf.copy_(row0); torch.cuda.synchronize()
        def with_history(pw):
            env.rollout_policy(W * D, policy, KP, KD, action_scale=scale, decimation=D, policy_waves=pw)
        def without():
            env.rollout_policy(W * D, policy0, KP, KD, action_scale=scale, decimation=D, policy_waves=MLP_WAVES[0])
        def loop():
            with torch.no_grad():
                hist, a_prev = env.policy_history.clone(), torch.zeros(n, 12, device='cuda')
                for w in range(W):
                    hist = torch.where(env._terminated.bool()[:, None, None], 0.0, hist)
                    obs = env._obs_buf
                    a = module(torch.cat([obs, a_prev, hist.flatten(1)], dim=1))
                    hist = torch.cat([torch.cat([obs[:, :cols], a_prev], dim=1)[:, None], hist[:, :-1]], dim=1)
                    env.step_pd(q0 + scale * a, KP, KD, decimation=D)
                    a_prev = a
        restore(); with_history(0)   # warm every path
        if SIDE != 'rollout':
            restore(); without(); restore(); loop()
        tag = f'{robot} {scene} n={n} mlp={MLP} D={D} history L={L} cols={cols}' + (f' scan {SCAN[0]}x{SCAN[1]}' if SCAN else '') + f' (in_dim {policy.in_dim})'
        for r in range(MLP_RUNS):
            if SIDE != 'rollout':
                restore(); m, us = timed(loop, W * D)
                print(f'{tag} run {r}: loop (torch module + history in torch + step_pd)  {m:7.2f} M env-steps/s  {us:6.1f} us/step', flush=True)
                restore(); m, us = timed(without, W * D)
                print(f'{tag} run {r}: rollout_policy WITHOUT history (in_dim 45), waves {MLP_WAVES[0]:4d} {m:7.2f} M env-steps/s  {us:6.1f} us/step', flush=True)
            for pw in MLP_WAVES:
                restore(); m, us = timed(lambda: with_history(pw), W * D)
                print(f'{tag} run {r}: rollout_policy with history, policy waves {pw:4d}       {m:7.2f} M env-steps/s  {us:6.1f} us/step  status {env.closed_loop_status()}', flush=True)
        print(f'{tag}: episodes max {int(env._episode.max())}', flush=True)
        sys.exit(0)
    restore(); feature(0); restore(); loop()   # warm both paths
    tag = f'{robot} {scene} n={n} mlp={MLP} D={D}' + (f' obs-noise={OBS_NOISE}' if OBS_NOISE else '')
    for r in range(MLP_RUNS):
        if SIDE in (None, 'loop'):
            restore(); m, us = timed(loop, W * D)
            print(f'{tag} run {r}: loop (torch module + step_pd)          {m:7.2f} M env-steps/s  {us:6.1f} us/step', flush=True)
        for pw in MLP_WAVES if SIDE in (None, 'rollout') else ():
            restore(); m, us = timed(lambda: feature(pw), W * D)
            print(f'{tag} run {r}: rollout_policy, policy waves {pw:4d}       {m:7.2f} M env-steps/s  {us:6.1f} us/step  status {env.closed_loop_status()}', flush=True)
    print(f'{tag}: episodes max {int(env._episode.max())}', flush=True)
    sys.exit(0)

if JOINT_CMD:
    D = JOINT_CMD
    W = max(1, K // D)   # windows per timing: about K physics steps
    key = env._key_qpos[7:19].float()
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, 12, generator=g, device='cuda')
    cmds = [(key + u(-0.6, 0.6), u(-1.0, 1.0), u(-5.0, 5.0)) for _ in range(16)]   # a policy's targets: keyframe +- 0.6 rad, per env
    kp, kd = u(20.0, 60.0), u(0.5, 2.0)
    for i in range(300 // D + 1): env.step_pd(cmds[i % 16][0], kp, kd, decimation=D)   # settle into the tracking regime
    sd = env.state_dict(); launches = env._launches
    def restore():
        env.load_state_dict(sd); env._launches = launches; torch.cuda.synchronize()
    def windows_pd():
        for w in range(W):
            q, qd, ff = cmds[w % 16]
            env.step_pd(q, kp, kd, qd_des=qd, tau_ff=ff, decimation=D)
    def windows_loop():
        for w in range(W):
            q, qd, ff = cmds[w % 16]
            for _ in range(D):
                env.step(kp * (q - env.qpos[:, 7:].float()) + kd * (qd - env.qvel[:, 6:]) + ff)
    restore(); windows_pd(); restore(); windows_loop()   # warm both paths
    res = {'step_pd': [], 'loop': []}
    for r in range(5):
        for name, fn in (('loop', windows_loop), ('step_pd', windows_pd)):
            restore(); res[name].append(timed(fn, W * D)[0])
    for name in ('loop', 'step_pd'):
        v = sorted(res[name])
        print(f'{robot} {scene} n={n} D={D}: {name:8s} median {v[2]:7.2f} M env-steps/s  min {v[0]:7.2f} max {v[-1]:7.2f}  ({W} windows x 5 runs)', flush=True)
    print(f'{robot} {scene} n={n} D={D}: step_pd / loop = {sorted(res["step_pd"])[2] / sorted(res["loop"])[2]:.3f} (medians); episodes max {int(env._episode.max())}', flush=True)
    sys.exit(0)

if FOOT_CMD:
    D = FOOT_CMD
    W = max(1, K // D)   # windows per timing: about K physics steps
    acc = QuadrupedEnv(robot, scene=scene, state_obs_names=tuple(QuadrupedEnv.ALL_OBS), num_envs=n, auto_reset='next_step', seed=1, accessors=True)
    mg4 = float(env.mjModel.body_mass.sum()) * 9.81 / 4
    kp = torch.tensor([400.0, 400.0, 1500.0] * 4, device='cuda')
    kd = torch.tensor([15.0] * 12, device='cuda')
    key = env.reset(random=False)['feet_pos:base'][0].clone()   # the keyframe footholds, base frame, legs_order
    cmds = [key + 0.02 * (2 * torch.rand(n, 12, generator=g, device='cuda') - 1) for _ in range(16)]
    legs = list(env.legs_order)
    cols = {leg: torch.as_tensor(acc.legs_qvel_idx[leg], device='cuda') for leg in legs}

    def stance_force(e):
        """the controller's part, once per window: -m g / 4 along world z per foot, in the base axes of the env's current orientation"""
        w, x, y, z = e.qpos[:, 3:7].float().unbind(1)
        up = torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1)   # world z in base axes
        return (-mg4 * up).repeat(1, 4)

    def torch_law(e, p_des, f_ff):
        """tau_leg = J_leg^T (f_ff + kp (p_des - p) - kd J_leg qd_leg) from the env's getters: what a controller writes today"""
        J, P = e.feet_jacobians(frame='base'), e.feet_pos(frame='base')
        tau = torch.zeros(n, 12, device='cuda')
        for i, leg in enumerate(legs):
            c = cols[leg]
            Jl = J[leg][:, :, c]
            v = torch.einsum('nij,nj->ni', Jl, e.qvel[:, c])
            F = f_ff[:, 3 * i:3 * i + 3] + kp[3 * i:3 * i + 3] * (p_des[:, 3 * i:3 * i + 3] - P[leg]) - kd[3 * i:3 * i + 3] * v
            tau[:, c - 6] = torch.einsum('nij,ni->nj', Jl, F)
        return tau

    def window_feet(w):
        env.step_feet(cmds[w % 16], kp, kd, f_ff=stance_force(env), frame='base', decimation=D)

    def window_loop(w):
        f_ff = stance_force(acc)
        for _ in range(D):
            acc.step(torch_law(acc, cmds[w % 16], f_ff))
    for e in (env, acc):
        e.reset(random=True)
    for i in range(600 // D + 1): window_feet(i)   # settle into the standing regime
    for i in range(600 // D + 1): window_loop(i)
    sd = {id(e): (e.state_dict(), e._launches) for e in (env, acc)}
    def restore(e):
        e.load_state_dict(sd[id(e)][0]); e._launches = sd[id(e)][1]; torch.cuda.synchronize()
    def windows_feet():
        for w in range(W): window_feet(w)
    def windows_loop():
        for w in range(W): window_loop(w)
    windows_feet(); windows_loop()   # warm both paths
    res = {'step_feet': [], 'loop': []}
    for r in range(5):
        for name, fn, e in (('loop', windows_loop, acc), ('step_feet', windows_feet, env)):
            restore(e); res[name].append(timed(fn, W * D)[0])
    for name in ('loop', 'step_feet'):
        v = sorted(res[name])
        print(f'{robot} {scene} n={n} D={D}: {name:9s} median {v[2]:7.2f} M env-steps/s  min {v[0]:7.2f} max {v[-1]:7.2f}  ({W} windows x 5 runs)', flush=True)
    print(f'{robot} {scene} n={n} D={D}: step_feet / loop = {sorted(res["step_feet"])[2] / sorted(res["loop"])[2]:.3f} (medians); '
          f'episodes max {int(env._episode.max())} (step_feet) {int(acc._episode.max())} (loop)', flush=True)
    sys.exit(0)

m, us = timed(lambda: [env.step(pool[i % 16]) for i in range(K)], K)
print(f'{robot} {scene} n={n}: step loop, random actions             {m:7.2f} M env-steps/s  {us:6.1f} us/step', flush=True)
acts = torch.stack([pool[i % 16] for i in range(K)])
m, us = timed(lambda: env.rollout(acts, shards=0), K)
print(f'{robot} {scene} n={n}: persistent open loop, random actions  {m:7.2f} M env-steps/s  {us:6.1f} us/step', flush=True)
# settle into the closed-loop regime, checkpoint, record the policy's actions from there
env.rollout_closed_loop(300, KP, KD, mode='inline')
sd = env.state_dict()
rec = env.rollout_closed_loop(K, KP, KD, mode='inline', record_actions=True)['actions']
def restore():
    env.load_state_dict(sd); torch.cuda.synchronize()
restore(); m, us = timed(lambda: [env.step(rec[i]) for i in range(K)], K)
print(f'{robot} {scene} n={n}: step loop, the PD policy\'s actions    {m:7.2f} M env-steps/s  {us:6.1f} us/step', flush=True)
restore(); m, us = timed(lambda: env.rollout(rec, shards=0), K)
print(f'{robot} {scene} n={n}: persistent open loop, same actions    {m:7.2f} M env-steps/s  {us:6.1f} us/step', flush=True)
restore(); m, us = timed(lambda: env.rollout_closed_loop(K, KP, KD, mode='inline'), K)
print(f'{robot} {scene} n={n}: CLOSED loop, inline PD policy         {m:7.2f} M env-steps/s  {us:6.1f} us/step', flush=True)
for pw, sw in ((64, 0), (256, 0), (64, n - 256 if n > 512 else 0), (16, 0)):
    try:
        restore(); m, us = timed(lambda: env.rollout_closed_loop(K, KP, KD, mode='mailbox', policy_waves=pw, step_waves=sw), K)
        print(f'{robot} {scene} n={n}: CLOSED loop, mailbox, policy waves {pw:3d} step waves {sw or n:5d}: {m:7.2f} M env-steps/s  {us:6.1f} us/step  status {env.closed_loop_status()}', flush=True)
    except Exception as ex:
        print('closed loop failed:', pw, sw, ex, flush=True)
        break
# an exploring policy: the same PD law + Gaussian torque noise of the benchmark's amplitude (robots fall and re-spawn like under random actions)
SIG = 50.0
env.rollout_closed_loop(300, KP, KD, mode='inline', noise_sigma=SIG)
sd = env.state_dict(); launches = env._launches
rec = env.rollout_closed_loop(K, KP, KD, mode='inline', noise_sigma=SIG, record_actions=True)['actions']
def restore():
    env.load_state_dict(sd); env._launches = launches; torch.cuda.synchronize()
restore(); m, us = timed(lambda: [env.step(rec[i]) for i in range(K)], K)
print(f'{robot} {scene} n={n}: step loop, the noisy policy\'s actions {m:7.2f} M env-steps/s  {us:6.1f} us/step', flush=True)
restore(); m, us = timed(lambda: env.rollout(rec, shards=0), K)
print(f'{robot} {scene} n={n}: persistent open loop, same actions    {m:7.2f} M env-steps/s  {us:6.1f} us/step', flush=True)
restore(); m, us = timed(lambda: env.rollout_closed_loop(K, KP, KD, mode='inline', noise_sigma=SIG), K)
print(f'{robot} {scene} n={n}: CLOSED loop, inline PD + noise        {m:7.2f} M env-steps/s  {us:6.1f} us/step', flush=True)
restore(); m, us = timed(lambda: env.rollout_closed_loop(K, KP, KD, mode='mailbox', noise_sigma=SIG), K)
print(f'{robot} {scene} n={n}: CLOSED loop, mailbox PD + noise       {m:7.2f} M env-steps/s  {us:6.1f} us/step  status {env.closed_loop_status()}', flush=True)
print(f'contacts per env (mean of contact_state sum) {float(env._obs_views["contact_state"].sum(1).mean()):.2f}, episodes max {int(env._episode.max())}')
