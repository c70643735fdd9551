"""What the tests of the learning rollout's windows share (tests/test_gpu_learn_rollout.py, tests/test_gpu_foot_reward.py,
tests/test_foot_reward_host.py): bit comparison, the replay of a recorded rollout on the twin, and THE reference loop over recorded steps -
the loop of ``QuadrupedEnv.rollout_policy``'s docstring, in torch or numpy, whichever the flags are.  The definition it is compared with is
``csrc/gq_learn.h``."""
import numpy as np


def _torch(x):
    return type(x).__module__.startswith('torch')


def _bits(x):
    if _torch(x):
        import torch
        return x.contiguous().view(torch.int32)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _replay_flags(a, b, r, K, state):
    """the recorded torques through the step loop on the twin: the rows and `terminated` after every step; the states (the fields
    `state`) end bit-equal"""
    import torch
    rows, term = [], []
    for k in range(K):
        a.step(r['actions'][k])
        rows.append(a._obs_buf.clone())
        term.append(a._terminated.clone())
    torch.cuda.synchronize()
    for f in state:
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    rows = torch.stack(rows)
    if r['obs_seq'] is not None:
        assert torch.equal(rows, r['obs_seq'])
    return rows, torch.stack(term).bool()


def reference_windows(step_reward, term, pending, D, air=None, contact=None, over_limit=None):
    """Every env at once, float32 adds in k order.  term [K, n] bool: `terminated` after every step; pending [n] bool: the envs that wait
    for their re-spawn before the call.  step_reward(k, s, air) -> the reward [n] of step k (policy step s) evaluated for EVERY env, and
    with ``air`` ([n, 4], the air times before the step; None: no foot state) -> (reward, air after the step).  The air times are zeroed
    at a re-spawn step and advanced by the law at every other step, whether or not the window is dead.
    Returns rewards [K // D, n], dones [K // D, n], the final air times (or None) and what the input contained: landings per foot (contact
    [K, n, 4] with t > 0) and those of them inside a dead tail, re-spawns inside a window, dead-tail steps that are not the re-spawn, feet
    over the impact limit (over_limit [K, n, 4]), earning terminations per substep of the window, envs whose last step earns."""
    xp = np
    if _torch(term):
        import torch as xp
    K = term.shape[0]
    rewards, dones = [], []
    seen = dict(landings=0, dead_tail_landings=0, respawn_inside=0, dead_tail_steps=0, impacts=0, done_at=[0] * D, last_step_earns=0)
    for s in range(K // D):
        acc, done, dead = None, term[0] & ~term[0], term[0] & ~term[0]
        for k in range(D * s, D * s + D):
            respawn = term[k - 1] if k > 0 else pending
            r_k = step_reward(k, s, air)
            if air is not None:
                r_k, air_next = r_k
                if contact is not None:
                    landed = contact[k] & (air > 0) & ~respawn[:, None]
                    seen['landings'] = seen['landings'] + landed.sum(0)
                    seen['dead_tail_landings'] += int((landed & dead[:, None]).sum())
                air = xp.where(respawn[:, None], xp.zeros_like(air), air_next)
            seen['respawn_inside'] += int((respawn & (k % D != 0)).sum())
            seen['dead_tail_steps'] += int((dead & ~respawn).sum())
            if over_limit is not None:
                seen['impacts'] += int((over_limit[k] & ~respawn[:, None]).sum())
            acc = xp.zeros_like(r_k) if acc is None else acc
            earn = ~dead & ~respawn
            acc = xp.where(earn, acc + r_k, acc)
            seen['done_at'][k % D] += int((earn & term[k]).sum())
            seen['last_step_earns'] += int(earn.sum()) if k == K - 1 else 0
            done = done | (earn & term[k])
            dead = dead | (earn & term[k])
        rewards.append(acc)
        dones.append(done)
    return xp.stack(rewards), xp.stack(dones), air, seen
