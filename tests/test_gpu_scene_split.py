"""The flat self-collision scene is built three times - with both pair routines, without the exact box routines (SCENE_FLAT_SELF_HULL),
without the convex block and its pair exchange (SCENE_FLAT_SELF_PRIM) - and gq_step_call.h model_scene gives each model the build its own
pair table needs.  Leaving a routine out of a kernel must not move a bit: the state of a small batch after a few hundred steps, hashed, must
equal the digest recorded by the build BEFORE the split (one kernel with everything, for every robot), in tests/golden/scene_split_digests.json.
Each case also counts the env-steps that had a robot-robot contact, read from the library's contact rows: the count must equal the recorded
one and be positive, so that a digest can never agree merely because the self-collision stage found nothing.

A change that is MEANT to move results records new digests with `python tests/test_gpu_scene_split.py tests/golden/scene_split_digests.json`
and says why."""
import hashlib
import json
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'scene_split_digests.json'
N, STEPS = 256, 300
# name -> (robot, QuadrupedEnv keywords, friction cone of the robot's model, the scene model_scene picks)
CASES = {
    'hyqreal1': ('hyqreal1', {}, 'elliptic', 'hull'),
    'go2': ('go2', {}, 'elliptic', 'prim'),
    'aliengo': ('aliengo', {}, 'pyramidal', 'prim'),
    'b2': ('b2', {}, None, 'both routines (control: its kernel is the one from before the split)'),
    'mini_cheetah_capsule': ('mini_cheetah', {'self_collision': 'capsule'}, 'pyramidal', 'prim'),
    'mini_cheetah_next_step_reset': ('mini_cheetah', {'auto_reset': 'next_step'}, 'pyramidal', 'hull'),
}


def run_case(name):
    """N envs on the flat floor, ALL_OBS, Newton 100 / 1e-8, random torques (sigma 40; robots fall and fold up), STEPS steps.
    Returns (sha256 over qpos, qvel, the dropped-contact counts and the last observations; env-steps with a robot-robot contact)."""
    import torch
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    robot, kw, cone, _ = CASES[name]
    env = QuadrupedEnv(robot, state_obs_names=tuple(QuadrupedEnv.ALL_OBS), num_envs=N, device='cuda:0', solver='newton',
                       solver_iterations=100, solver_tolerance=1e-8, seed=3, accessors=True, **{'auto_reset': False, **kw})
    if cone is not None:
        assert env._mm.md.cone == (cone == 'elliptic')
    env.reset(random=True)
    g = torch.Generator(device='cuda:0').manual_seed(11)
    slot = torch.arange(12, device='cuda:0')[None, :]
    touching = torch.zeros((), dtype=torch.int64, device='cuda:0')
    obs = None
    for _ in range(STEPS):
        obs = env.step(torch.randn(N, 12, generator=g, device='cuda:0') * 40)[0]
        c = env.contacts()
        touching += ((c['geom1'] >= 0) & (slot < c['ncon'][:, None])).any(dim=1).sum()   # geom1 = -1: a world geom
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (env.qpos, env.qvel, env._contacts_dropped, *(obs[k] for k in sorted(obs))):
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    n_touch = int(touching)
    env.close()
    return h.hexdigest(), n_touch


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_state_digest_and_self_contacts_are_unchanged(name):
    want = json.loads(GOLDEN.read_text())
    assert want['envs'] == N and want['steps'] == STEPS
    sha, n_touch = run_case(name)
    print(f'{name}: sha256 {sha}, env-steps with a robot-robot contact {n_touch} (recorded {want["cases"][name]["self_contact_env_steps"]})')
    assert want['cases'][name]['self_contact_env_steps'] > 0
    assert n_touch == want['cases'][name]['self_contact_env_steps']
    assert sha == want['cases'][name]['sha256']


if __name__ == '__main__':
    # record (or print) the digests: python tests/test_gpu_scene_split.py [out.json]
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    cases = {}
    for name in CASES:
        sha, n_touch = run_case(name)
        cases[name] = {'sha256': sha, 'self_contact_env_steps': n_touch}
        print(name, json.dumps(cases[name]), flush=True)
        assert n_touch > 0, f'{name}: no robot-robot contact in {STEPS} steps - lengthen the case'
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(json.dumps({'envs': N, 'steps': STEPS, 'cases': cases}, indent=1) + '\n')
