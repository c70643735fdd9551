"""The task reward of the learning rollout (``QuadrupedEnv.rollout_policy(reward=...)``, ``QuadrupedEnv.reward_eval``): a weighted sum
of the usual locomotion terms, evaluated per physics step in the policy seat of the closed-loop rollout.

The law is defined in ``csrc/gq_reward.h`` (float32, a fixed order of IEEE operations and ``fmaf``); this module holds the weights
(no GPU needed), says which observables they need, and restates the law in float64 for tests."""
from __future__ import annotations

import math

import numpy as np

# the terms, in the order of the law's sum (csrc/gq_reward.h, include/gq.h GqLearn)
TERMS = ('track_lin_vel', 'track_ang_vel', 'lin_vel_z', 'ang_vel_xy', 'orientation', 'base_height', 'torques', 'joint_vel', 'power',
         'action_rate', 'alive', 'termination')
# term -> (observable, components read)
_TERM_OBS = {
    'track_lin_vel': ('base_lin_vel_err:base', (0, 1)), 'track_ang_vel': ('base_ang_vel_err:base', (2,)), 'lin_vel_z': ('base_lin_vel:base', (2,)),
    'ang_vel_xy': ('base_ang_vel:base', (0, 1)), 'orientation': ('gravity_vector:base', (0, 1)), 'base_height': ('base_pos', (2,)),
    'joint_vel': ('qvel_js', tuple(range(12))), 'power': ('qvel_js', tuple(range(12))),
}
EXP_CLAMP = 87.0   # exp(-x) is evaluated at min(x, 87)


class RewardSpec:
    """Weights of the reward terms; a term with weight 0 is off and its observable is not required.  Per physics step ::

        r = dt * sum_i w_i * term_i + termination * terminated        (dt: the simulation time step)

        track_lin_vel  exp(-(ex^2 + ey^2) / sigma_lin)   base_lin_vel_err:base[0:2]
        track_ang_vel  exp(-ez^2 / sigma_ang)            base_ang_vel_err:base[2]
        lin_vel_z      vz^2                              base_lin_vel:base[2]
        ang_vel_xy     wx^2 + wy^2                       base_ang_vel:base[0:2]
        orientation    gx^2 + gy^2                       gravity_vector:base[0:2]
        base_height    (z - base_height_target)^2        base_pos[2]
        torques        sum u_j^2                         the torques applied in the step
        joint_vel      sum qd_j^2                        qvel_js (or qvel[6:])
        power          sum |u_j qd_j|
        action_rate    sum (a_j - a_prev_j)^2            the policy's held action and the one before it
        alive          1
        termination    the terminated flag (not multiplied by dt)

    read from the observation row AFTER the step.  Penalties take negative weights."""

    def __init__(self, *, sigma_lin=0.25, sigma_ang=0.25, base_height_target=0.0, **weights):
        unknown = [k for k in weights if k not in TERMS]
        if unknown:
            raise ValueError(f'unknown reward term(s) {unknown}: the terms are {list(TERMS)}')
        self.weights = {t: float(weights.get(t, 0.0)) for t in TERMS}
        for t, w in self.weights.items():
            if not math.isfinite(w):
                raise ValueError(f'the weight of {t} is not finite: {w}')
        self.sigma_lin, self.sigma_ang, self.base_height_target = float(sigma_lin), float(sigma_ang), float(base_height_target)
        if self.weights['track_lin_vel'] != 0.0 and not (self.sigma_lin > 0.0 and math.isfinite(self.sigma_lin)):
            raise ValueError(f'sigma_lin must be positive with track_lin_vel on, got {sigma_lin}')
        if self.weights['track_ang_vel'] != 0.0 and not (self.sigma_ang > 0.0 and math.isfinite(self.sigma_ang)):
            raise ValueError(f'sigma_ang must be positive with track_ang_vel on, got {sigma_ang}')
        if not math.isfinite(self.base_height_target):
            raise ValueError(f'base_height_target is not finite: {base_height_target}')

    def __getattr__(self, name):
        if name in TERMS:
            return self.weights[name]
        raise AttributeError(name)

    def __repr__(self):
        on = ', '.join(f'{t}={w:g}' for t, w in self.weights.items() if w != 0.0)
        return f'RewardSpec({on}, sigma_lin={self.sigma_lin:g}, sigma_ang={self.sigma_ang:g}, base_height_target={self.base_height_target:g})'

    def required_obs(self):
        """the observable names the non-zero terms read (``qvel_js`` may be replaced by ``qvel``), in the terms' order, each once"""
        names = []
        for t in TERMS:
            if self.weights[t] != 0.0 and t in _TERM_OBS and _TERM_OBS[t][0] not in names:
                names.append(_TERM_OBS[t][0])
        return tuple(names)

    def columns(self, state_obs_names):
        """term -> the columns it reads in the observation row that ``state_obs_names`` lays out, for the terms that are on (what the
        library resolves from the batch's layout); ``ValueError`` names a missing observable"""
        from .cabi import OBS_DIMS, OBS_NAMES
        start, at = {}, 0
        for n in state_obs_names:
            start.setdefault(n, at)
            at += OBS_DIMS[OBS_NAMES.index(n)]
        cols = {}
        for t in TERMS:
            if self.weights[t] == 0.0 or t not in _TERM_OBS:
                continue
            name, comps = _TERM_OBS[t]
            if name in start:
                cols[t] = tuple(start[name] + c for c in comps)
            elif name == 'qvel_js' and 'qvel' in start:
                cols[t] = tuple(start['qvel'] + 6 + c for c in comps)
            else:
                raise ValueError(f'the reward term {t} reads {name}: not in state_obs_names {tuple(state_obs_names)}')
        return cols

    def terms64(self, rows64, torques, a, a_prev, terminated, columns):
        """float64 values of the terms that are on, ``{term: [n]}`` (termination: the flag as 0 / 1)"""
        x = np.asarray(rows64, dtype=np.float64)
        n = x.shape[0]
        u = None if torques is None else np.asarray(torques, dtype=np.float64).reshape(n, 12)
        col = lambda t: x[:, list(columns[t])]
        out = {}
        for t in TERMS:
            if self.weights[t] == 0.0:
                continue
            if t == 'track_lin_vel':
                out[t] = np.exp(-np.minimum((col(t) ** 2).sum(1) / np.float64(np.float32(self.sigma_lin)), EXP_CLAMP))
            elif t == 'track_ang_vel':
                out[t] = np.exp(-np.minimum((col(t) ** 2).sum(1) / np.float64(np.float32(self.sigma_ang)), EXP_CLAMP))
            elif t in ('lin_vel_z', 'ang_vel_xy', 'orientation', 'joint_vel'):
                out[t] = (col(t) ** 2).sum(1)
            elif t == 'base_height':
                out[t] = (col(t)[:, 0] - np.float64(np.float32(self.base_height_target))) ** 2
            elif t == 'torques':
                out[t] = (u ** 2).sum(1)
            elif t == 'power':
                out[t] = np.abs(u * col(t)).sum(1)
            elif t == 'action_rate':
                out[t] = ((np.asarray(a, dtype=np.float64).reshape(n, 12) - np.asarray(a_prev, dtype=np.float64).reshape(n, 12)) ** 2).sum(1)
            elif t == 'alive':
                out[t] = np.ones(n)
            else:
                out[t] = np.zeros(n) if terminated is None else np.asarray(terminated).reshape(n).astype(np.float64)
        return out

    def reference(self, rows64, torques, a, a_prev, terminated, columns, dt):
        """float64 evaluation of the law over ``n`` steps: rows ``[n, obs_dim]``, torques / a / a_prev ``[n, 12]`` (None where no weighted
        term reads them), terminated ``[n]`` or None; columns: ``self.columns(state_obs_names)``; dt: the simulation time step (the
        float32 weights, sigmas, target and dt the library holds, widened).  Returns the reward ``[n]``."""
        return self._sum64(rows64, torques, a, a_prev, terminated, columns, dt)[0]

    def magnitude(self, rows64, torques, a, a_prev, terminated, columns, dt):
        """``dt * sum_i |w_i * term_i| + |w_termination|`` per step, arguments as ``reference``: the scale a float32 error bound of the
        law is stated in"""
        return self._sum64(rows64, torques, a, a_prev, terminated, columns, dt)[1]

    def _sum64(self, rows64, torques, a, a_prev, terminated, columns, dt):
        terms = self.terms64(rows64, torques, a, a_prev, terminated, columns)
        dt = np.float64(np.float32(dt))
        n = np.asarray(rows64).shape[0]
        s, mag = np.zeros(n), np.zeros(n)
        for t in TERMS[:-1]:
            if t in terms:
                w = np.float64(np.float32(self.weights[t]))
                s += w * terms[t]
                mag += np.abs(w * terms[t])
        wt = np.float64(np.float32(self.weights['termination']))
        r = dt * s + (wt * terms['termination'] if 'termination' in terms else 0.0)
        return r, dt * mag + abs(wt)

    # -- the C block
    def _struct(self):
        import ctypes as C

        from .cabi import GqLearn
        g = GqLearn(struct_size=C.sizeof(GqLearn), sigma_lin=self.sigma_lin, sigma_ang=self.sigma_ang, base_height_target=self.base_height_target)
        for t in TERMS:
            setattr(g, 'w_' + t, self.weights[t])
        return g
