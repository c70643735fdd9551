"""Bit-identity of the convex narrow phase (csrc/gq_convex.h) across kernel revisions that only reschedule it: the headline workload's
state after a few hundred steps, hashed, must equal the digest recorded in tests/golden/convex_chain_digest.json - with the pair
exchange (csrc/gq_exchange.h) on and off.  The digest was recorded on MI355X by the build before the EPA fan's neighbours were found
lane-parallel; a change that moves any bit of the narrow phase's answers (the support vertex's tie-break, the rim order of the fan's
neighbours) changes it.  A change that is MEANT to move results records a new digest with
`python tests/test_gpu_convex_bits.py tests/golden/convex_chain_digest.json` and says why."""
import hashlib
import json
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'convex_chain_digest.json'
N, STEPS = 4096, 300


def digest(pair_exchange: bool) -> str:
    """4096 mini_cheetah envs on the flat floor, ALL_OBS, Newton 100 / 1e-8, convex self-collision, random torques without auto-reset
    (robots fall and fold up: the most convex pairs), STEPS steps; sha256 over qpos, qvel, the dropped-contact counts and the last
    observations"""
    import torch
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    env = QuadrupedEnv('mini_cheetah', state_obs_names=tuple(QuadrupedEnv.ALL_OBS), num_envs=N, device='cuda:0', solver='newton',
                       solver_iterations=100, solver_tolerance=1e-8, seed=3, auto_reset=False, pair_exchange=pair_exchange)
    assert env._mm.self_collision == 'convex'
    env.reset(random=True)
    g = torch.Generator(device='cuda:0').manual_seed(11)
    obs = None
    for _ in range(STEPS):
        obs = env.step(torch.randn(N, 12, generator=g, device='cuda:0') * 40)[0]
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (env.qpos, env.qvel, env._contacts_dropped, *(obs[k] for k in sorted(obs))):
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    env.close()
    return h.hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize('pair_exchange', [True, False])
def test_headline_state_digest_is_unchanged(pair_exchange):
    want = json.loads(GOLDEN.read_text())
    assert want['envs'] == N and want['steps'] == STEPS
    assert digest(pair_exchange) == want['sha256']


if __name__ == '__main__':
    # record (or check) the digest: python tests/test_gpu_convex_bits.py [out.json]
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    d = {str(on): digest(on) for on in (True, False)}
    print(json.dumps(d))
    assert d['True'] == d['False'], 'the pair exchange changed the results'
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(json.dumps({'envs': N, 'steps': STEPS, 'sha256': d['True']}, indent=1) + '\n')
