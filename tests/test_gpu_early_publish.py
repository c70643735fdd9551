"""The early publication of convex self pairs on the device (csrc/gq_exchange.h "published early"): a pair that touched a step ago goes
into the pair exchange between the smooth stages and the floor pass, and pass B takes it up as published.  64 mini_cheetah envs, a quarter of
them folded onto themselves (helpers.self_contact_states, the generator of the self-collision parity tests), the rest standing - helpers
with time on their hands, in both windows of the batch's table: every step with the exchange on is the step with it off, bit for bit."""
import numpy as np
import pytest
import torch

from helpers import marshalled, self_contact_states

pytestmark = pytest.mark.gpu

N, STEPS, FOLDED = 64, 12, 16
RESPAWN_AT, APART_AT = 5, 7      # before these steps: env 0 (tangled) is re-spawned, env 1's touching pair is pulled apart by setting its state


@pytest.fixture(scope='module')
def start():
    """start states (folded envs first) and the fixed action sequence"""
    from oracle.oracle import Oracle
    mm = marshalled('mini_cheetah', solver=1, iterations=100, tolerance=1e-8)
    o = Oracle(mm)
    rng = np.random.default_rng(17)
    hip = float(mm.desc.key_qpos[2])
    qf, vf = self_contact_states(mm.md, FOLDED, rng, o, z=(0.7 * hip, 1.3 * hip))
    q = np.tile(mm.md.key_qpos[0], (N, 1)); v = np.zeros((N, 18))
    q[:, 2] = 1.05 * hip
    q[:FOLDED], v[:FOLDED] = qf, 0.2 * vf
    g = torch.Generator().manual_seed(3)
    acts = (torch.randn(STEPS, N, 12, generator=g) * 5).cuda()
    return q, v.astype(np.float32), acts, mm.md.key_qpos[0].copy()


def _env(on):
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    env = QuadrupedEnv('mini_cheetah', state_obs_names=tuple(QuadrupedEnv.ALL_OBS), num_envs=N, device='cuda:0', solver='newton', solver_iterations=100, solver_tolerance=1e-8,
                       seed=0, auto_reset=False, accessors=True, pair_exchange=on)
    assert env._mm.self_collision == 'convex'
    return env


def _load(env, start):
    q, v, _, _ = start
    env.reset(random=False)
    env._qpos.copy_(torch.as_tensor(q)); env._qvel.copy_(torch.as_tensor(v)); env._warm.zero_()


def _snapshot(env):
    c = env.contacts()
    return dict(qpos=env.qpos.clone(), qvel=env.qvel.clone(), obs=env._obs_buf.clone(), reward=env._reward.clone(),
                terminated=env._terminated_b.clone(), truncated=env._truncated_b.clone(), dropped=env._contacts_dropped.clone(),
                **{'contact_' + k: t.clone() for k, t in c.items()})


def _step_loop(on, start, debug):
    """12 steps; the snapshots of every step and, with debug, the pairs each step published early (instrumented variant)"""
    _, _, acts, key = start
    env = _env(on)
    _load(env, start)
    if debug:
        env.enable_debug(N)
    snaps, early = [], []
    for k in range(STEPS):
        if k == RESPAWN_AT:      # a tangled env starts over: its prediction words are stale
            env.reset(env_ids=[0], random=True)
        if k == APART_AT:        # a touching pair pulled apart between two steps: predicted, and culled by the bounding spheres this step
            env._qpos[1, 7:] = torch.as_tensor(key[7:], dtype=torch.float64, device='cuda:0'); env._qvel[1].zero_()
        env.step(acts[k])
        snaps.append(_snapshot(env))
        if debug:
            torch.cuda.synchronize()
            early.append([float(d['xq'][10]) for d in env.debug_internals(N, ['xq'])])
    torch.cuda.synchronize()
    env.close()
    return snaps, early


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.fixture(scope='module')
def reference(start):
    """the step loop with the exchange off: every env keeps its pairs"""
    return _step_loop(False, start, False)[0]


def test_step_loop_is_bit_identical_and_pairs_go_out_early(start, reference):
    snaps, _ = _step_loop(True, start, False)
    for k in range(STEPS):
        _same(snaps[k], reference[k], f'step {k}')
    assert float(reference[0]['contact_ncon'][:FOLDED].sum()) > 0
    # the instrumented variant (held to itself with the exchange off): the same comparison, and its record of the early block
    snaps, early = _step_loop(True, start, True)
    off, _ = _step_loop(False, start, True)
    print('pairs published early, per step:', [sum(x) for x in early])
    for k in range(STEPS):
        _same(snaps[k], off[k], f'instrumented step {k}')
        for name in ('qpos', 'qvel', 'contact_ncon', 'contact_geom1', 'contact_geom2', 'contact_dist'):
            assert torch.equal(snaps[k][name], reference[k][name]), (k, name)
    assert all(sum(x) >= 1 for x in early[1:]), early     # (the first step has no helper word yet; from the second on pairs go out early)

    def self_contacts(k, e):
        n = int(reference[k]['contact_ncon'][e])
        return int((reference[k]['contact_geom1'][e, :n] >= 0).sum())
    # the two staged cases do occur.  Env 0 touched itself before its re-spawn, so its first step afterwards publishes on stale words - for
    # nothing, the new pose has no robot-robot contact - and the step after that has none left.  Env 1 touched itself before its joints were set
    # back to the key posture: the pairs go out early once more and come back apart.
    print('env 0 around its re-spawn:', [(early[k][0], self_contacts(k, 0)) for k in range(RESPAWN_AT - 1, RESPAWN_AT + 2)],
          'env 1 around the pull:', [(early[k][1], self_contacts(k, 1)) for k in range(APART_AT - 1, APART_AT + 2)])
    assert self_contacts(RESPAWN_AT - 1, 0) >= 1 and early[RESPAWN_AT][0] >= 1 and self_contacts(RESPAWN_AT, 0) == 0 and early[RESPAWN_AT + 1][0] == 0
    assert self_contacts(APART_AT - 1, 1) >= 1 and early[APART_AT][1] >= 1 and self_contacts(APART_AT, 1) == 0 and early[APART_AT + 1][1] == 0


@pytest.mark.parametrize('shards', [0, 2])
def test_rollout_is_bit_identical(start, reference, shards):
    """one persistent launch / two shards' launches overlapping on two streams: slots are reused step after step"""
    _, _, acts, key = start
    env = _env(True)
    _load(env, start)
    rows = torch.empty(STEPS, N, env._obs_dim, dtype=torch.float32, device='cuda:0')
    for a, b in ((0, RESPAWN_AT), (RESPAWN_AT, APART_AT), (APART_AT, STEPS)):      # (a rollout takes no state edits: one in front of each, as in the step loop)
        if a == RESPAWN_AT:
            env.reset(env_ids=[0], random=True)
        if a == APART_AT:
            env._qpos[1, 7:] = torch.as_tensor(key[7:], dtype=torch.float64, device='cuda:0'); env._qvel[1].zero_()
        env.rollout(acts[a:b], shards=shards, obs_out=rows[a:b])
        torch.cuda.synchronize()
        _same(_snapshot(env), reference[b - 1], f'rollout shards={shards}, step {b - 1}')
    env.close()
    for k in range(STEPS):
        assert torch.equal(rows[k], reference[k]['obs']), k


def test_stage_cut_between_the_early_block_and_pass_b_leaks_no_slot(start):
    """A stage cut (gq_debug_stop_stage, tools/stage_cuts.py) at marker 14 ends the step behind the early block and in front of pass B, which
    alone gives slots back: under a cut nothing is published early.  40 such launches on the folded envs - had each published its 40 pairs, the
    256-slot table would be full after seven - and the next full steps still publish early, and are the steps of a batch without the exchange."""
    from gym_quadruped_amd import _lib
    _, _, acts, _ = start
    out = []
    for on in (True, False):
        env = _env(on)
        _load(env, start)
        for k in range(2):
            env.step(acts[k])
        _lib.check(env._L.gq_debug_stop_stage(env._hbatch, 14), 'gq_debug_stop_stage')
        q0 = env.qpos.clone()
        for _ in range(40):
            env.step(acts[2])
        torch.cuda.synchronize()
        assert torch.equal(env.qpos, q0)
        _lib.check(env._L.gq_debug_stop_stage(env._hbatch, 0), 'gq_debug_stop_stage')
        env.enable_debug(N)
        early = []
        for k in range(2, 4):
            env.step(acts[k])
            torch.cuda.synchronize()
            early.append(sum(float(d['xq'][10]) for d in env.debug_internals(N, ['xq'])))
        out.append((_snapshot(env), early))
        env.close()
    print('pairs published early in the two steps behind the cuts:', out[0][1])
    assert all(n >= 30 for n in out[0][1]), out[0][1]      # (the step loop above: 41 pairs at these steps)
    _same(out[0][0], out[1][0], 'steps behind 40 stage cuts')
