"""The step kernel's epilogue (csrc/gq_step_body.h S10 - S11: integration, the observation row, the contact rows) is the tail of every launch
and gets rescheduled for speed - lane indices made again instead of reloaded, work moved between lanes.  Rescheduling must not move a bit.
A handful of small batches that reach the branches of the stage the whole-step digests (tests/test_gpu_scene_split.py,
tests/test_gpu_convex_bits.py) do not - the gimbal pole of the Euler angles, feet whose body has several contacts, contacts on tilted world
boxes, the elliptic decode over a long contact list, the PGS arm, layouts that skip blocks, an env over the row budget - are stepped a few
times and hashed: the observation row, reward, flags, the contact rows, qpos, qvel and qacc of every step.  The digests in
tests/golden/obs_lanes_digests.json were recorded by the build BEFORE the epilogue was touched.  Each case also counts what proves that it
reached its branch; the count must equal the recorded one and be positive, so that a digest can never agree merely because the branch was
not taken.  (What these digests catch: the compiler picks the order in which a sum of products is fused per call site, so moving
`R v` behind a per-lane select changes the last bit of base_ang_vel on a third of the envs - profiles/obs_lanes_ab.md.)

A change that is MEANT to move results records new digests with `python tests/test_gpu_obs_lanes.py tests/golden/obs_lanes_digests.json`
and says why."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import obs_lane_cases as oc   # noqa: E402

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'obs_lanes_digests.json'
STEPS = 4
LEGS = ('RR', 'FL', 'RL', 'FR')
IMU_KW = dict(accel_name='imu_acc', gyro_name='imu_gyro', imu_site_name='imu', accel_noise=0.01, gyro_noise=0.02, accel_bias_rate=0.03, gyro_bias_rate=0.04, seed=5)
CASES = ('gimbal_pole', 'folded_all_obs', 'world_boxes', 'elliptic_crouch', 'folded_pgs', 'layout_default_legs', 'layout_all_imu', 'row_budget')


def _env(robot, n, all_obs=True, accessors=True, **kw):
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    kw.setdefault('solver', 'newton')
    if kw['solver'] == 'pgs':
        kw.update(solver_iterations=50, solver_tolerance=0.0)
    else:
        kw.update(solver_iterations=100, solver_tolerance=1e-8)
    if all_obs:
        kw['state_obs_names'] = tuple(QuadrupedEnv.ALL_OBS) + tuple(kw.pop('more_obs', ()))
    return QuadrupedEnv(robot, num_envs=n, device='cuda:0', seed=3, auto_reset=False, accessors=accessors, **kw)


def _load(env, q, v, warm=None, friction=None):
    import torch
    env.reset(random=False)
    env._qpos.copy_(torch.as_tensor(q)); env._qvel.copy_(torch.as_tensor(np.asarray(v, np.float32))); env._warm.zero_()
    if warm is not None:
        env._warm.copy_(torch.as_tensor(warm))
    if friction is not None:
        env._friction.copy_(torch.as_tensor(friction))
    env._cmd.copy_(torch.as_tensor(np.tile(np.asarray(oc.CMD, np.float32), (env.num_envs, 1))))


def _digest_steps(env, acts, count):
    """STEPS steps with the given controls; sha256 over every step's outputs, and the sum (or, count.max: the maximum) of count(env, obs) over the steps"""
    import torch
    h = hashlib.sha256()
    seen = []
    for k in range(STEPS):
        obs = env.step(torch.as_tensor(acts[k]).cuda())[0]
        torch.cuda.synchronize()
        parts = [env._obs_buf, env._reward, env._terminated_b, env._truncated_b, env._invalid_b, env._contacts_dropped, env.qpos, env.qvel, env._qacc]
        if getattr(env, '_contacts', None) is not None:
            parts.append(env._contacts)
        for t in parts:
            h.update(t.detach().contiguous().cpu().numpy().tobytes())
        seen.append(int(count(env, obs)))
    env.close()
    return h.hexdigest(), (max(seen) if getattr(count, 'max', False) else sum(seen))


def _world_contacts(env):
    """(in-list mask [N, 12] of the contacts with a world geom, body of the robot's geom)"""
    import torch
    c = env.contacts()
    slot = torch.arange(c['geom1'].shape[1], device=c['geom1'].device)[None, :]
    world = (slot < c['ncon'][:, None]) & (c['geom1'] < 0)
    body = torch.as_tensor(np.asarray(env.mjModel.geom_bodyid), device=c['geom2'].device)[c['geom2'].long().clamp(min=0)]
    return c, world, body


def _count_calf_pairs(env, obs):
    """envs with at least two world contacts on one calf body"""
    _, world, body = _world_contacts(env)
    hit = None
    for leg in ('FL', 'FR', 'RL', 'RR'):
        two = (world & (body == env._feet_body_id[leg])).sum(dim=1) >= 2
        hit = two if hit is None else hit | two
    return hit.sum()


def _count_pole(env, obs):
    e = obs['base_ori_euler_xyz']
    return ((e[:, 0] == 0.0) & ((e[:, 1].abs() - np.pi / 2).abs() < 1e-3)).sum()


def _count_tilted(env, obs):
    c, world, _ = _world_contacts(env)
    return (world & (c['frame'][:, :, 0, 2] != 1.0)).sum()


def _count_ncon(env, obs):
    return env.contacts()['ncon'].max()


_count_ncon.max = True


def _count_width(env, obs):
    return env._obs_dim


_count_width.max = True


def _count_dropped(env, obs):
    return env._contacts_dropped.sum()


def run_case(name):
    """-> (sha256 over the outputs of the case's STEPS steps, the count that proves the case reached its branch)"""
    import torch
    if name == 'gimbal_pole':
        n = 8
        env = _env('mini_cheetah', n)
        _load(env, *oc.gimbal_states(n))
        return _digest_steps(env, np.zeros((STEPS, n, 12), np.float32), _count_pole)
    if name in ('folded_all_obs', 'folded_pgs'):
        n = 16
        env = _env('mini_cheetah', n, solver='pgs' if name == 'folded_pgs' else 'newton')
        _load(env, *oc.folded_states(n))
        return _digest_steps(env, oc.controls(n, STEPS, sigma=5.0), _count_calf_pairs)
    if name == 'world_boxes':
        n = 32
        env = _env('mini_cheetah', n, scene='random_boxes')
        env.reset(random=True)
        g = torch.Generator(device='cuda:0').manual_seed(2)
        for _ in range(80):   # build-up: the robots drop onto the tilted boxes and fold up
            env.step(torch.randn(n, 12, generator=g, device='cuda:0') * 15)
        return _digest_steps(env, oc.controls(n, STEPS), _count_tilted)
    if name == 'elliptic_crouch':
        n = 16
        env = _env('go2', n)
        assert env._mm.md.cone == 1
        q, v, _ = oc.crouch_states('go2', n)
        _load(env, q, v)
        return _digest_steps(env, oc.controls(n, STEPS), _count_ncon)
    if name == 'layout_default_legs':
        n = 16
        env = _env('mini_cheetah', n, all_obs=False, accessors=False, legs_order=LEGS)
        _load(env, *oc.floor_states('mini_cheetah', n))
        return _digest_steps(env, oc.controls(n, STEPS), _count_width)
    if name == 'layout_all_imu':
        from gym_quadruped_amd.sensors import IMU
        n = 16
        env = _env('aliengo', n, accessors=False, more_obs=IMU.ALL_OBS, sensors=(IMU,), sensors_kwargs=(IMU_KW,))
        _load(env, *oc.floor_states('aliengo', n))
        return _digest_steps(env, oc.controls(n, STEPS), _count_width)
    if name == 'row_budget':
        from row_edge_cases import limit_case
        n = 16
        case = limit_case('go2', n, seed=7)   # its envs with every limit row are drawn until the constraint set does NOT fit the budget: three at this seed
        env = _env('go2', n, self_collision=False)
        _load(env, case['qpos'], case['qvel'], warm=case['warm'], friction=case['friction'])
        return _digest_steps(env, np.tile(case['ctrl'], (STEPS, 1, 1)), _count_dropped)
    raise KeyError(name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_outputs_of_the_observation_stage_are_unchanged(name):
    want = json.loads(GOLDEN.read_text())
    assert want['steps'] == STEPS
    sha, count = run_case(name)
    print(f'{name}: sha256 {sha}, count {count} (recorded {want["cases"][name]["count"]})')
    assert want['cases'][name]['count'] > 0
    assert count == want['cases'][name]['count']
    assert sha == want['cases'][name]['sha256']


if __name__ == '__main__':
    # record (or print) the digests: python tests/test_gpu_obs_lanes.py [out.json]
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    cases = {}
    for name in CASES:
        sha, count = run_case(name)
        cases[name] = {'sha256': sha, 'count': count}
        print(name, json.dumps(cases[name]), flush=True)
        assert count > 0, f'{name}: the case did not reach its branch'
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(json.dumps({'steps': STEPS, 'cases': cases}, indent=1) + '\n')
