"""The task reward of the learning rollout (``QuadrupedEnv.rollout_policy(reward=...)``, ``QuadrupedEnv.reward_eval``): a weighted sum
of the usual locomotion terms, evaluated per physics step in the policy seat of the closed-loop rollout.

The law is defined in ``csrc/gq_reward.h`` (float32, a fixed order of IEEE operations and ``fmaf``); this module holds the weights
(no GPU needed), says which observables they need, and restates the law in float64 for tests.

``FootRewardSpec`` (``RewardSpec(..., feet=...)``) adds the foot terms - air time, slip, impact, clearance - defined in
``csrc/gq_reward_feet.h``; the air-time term carries state (``QuadrupedEnv.feet_air_time``), which its float64 restatement carries over a
sequence of steps."""
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
# the foot terms, in the order they continue the sum (csrc/gq_reward_feet.h, include/gq.h GqFootReward)
FOOT_TERMS = ('air_time', 'slip', 'impact', 'clearance')
LEG_NAMES = ('FL', 'FR', 'RL', 'RR')   # the law's foot order, whatever the env's legs_order


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

    def __init__(self, *, sigma_lin=0.25, sigma_ang=0.25, base_height_target=0.0, feet=None, **weights):
        if feet is not None and not isinstance(feet, FootRewardSpec):
            raise ValueError(f'feet must be a FootRewardSpec, got {type(feet).__name__}')
        self.feet = feet
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
        feet = f', feet={self.feet!r}' if self.feet is not None else ''
        return f'RewardSpec({on}, sigma_lin={self.sigma_lin:g}, sigma_ang={self.sigma_ang:g}, base_height_target={self.base_height_target:g}{feet})'

    @property
    def feet_on(self):
        """a foot term (``feet=FootRewardSpec(...)``) has a non-zero weight: the call goes through the ``*_feet`` entry points"""
        return self.feet is not None and self.feet.on

    def required_obs(self):
        """the observable names the non-zero terms read (``qvel_js`` may be replaced by ``qvel``), in the terms' order, each once"""
        names = []
        for t in TERMS:
            if self.weights[t] != 0.0 and t in _TERM_OBS and _TERM_OBS[t][0] not in names:
                names.append(_TERM_OBS[t][0])
        if self.feet is not None:
            names += [n for n in self.feet.required_obs() if n not in names]
        return tuple(names)

    def columns(self, state_obs_names, legs_order=LEG_NAMES):
        """term -> the columns it reads in the observation row that ``state_obs_names`` lays out, for the terms that are on (what the
        library resolves from the batch's layout); ``ValueError`` names a missing observable.  With ``feet``, the foot terms' entries
        (``FootRewardSpec.columns``, which ``legs_order`` bears on) follow the existing ones."""
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
        if self.feet is not None:
            cols.update(self.feet.columns(state_obs_names, legs_order))
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


def _obs_starts(state_obs_names):
    from .cabi import OBS_DIMS, OBS_NAMES
    start, at = {}, 0
    for n in state_obs_names:
        start.setdefault(n, at)
        at += OBS_DIMS[OBS_NAMES.index(n)]
    return start


class FootRewardSpec:
    """Weights and parameters of the foot terms of the reward (``RewardSpec(feet=FootRewardSpec(...))``).  They continue the sum of the
    twelve terms after ``alive``, in this order, each off at weight 0 (its observables are then not required).  Feet are in the order FL,
    FR, RL, RR whatever the env's ``legs_order``; per physics step, from the observation row after it, for foot ``i``:
    ``c_i = contact_state[i] != 0``, ``vx_i, vy_i = feet_vel[i][0:2]``, ``fz_i = contact_forces[i][2]``, ``zb_i = feet_pos:base[i][2]`` ::

        air_time    sum over the feet that LAND in this step (c_i and t_i > 0) of (t_i + dt - air_time_target), t_i the foot's air time so far
                    (then t_i <- 0 if c_i else t_i + dt); 0 while the commanded planar speed |base_lin_vel_err:base + base_lin_vel:base|[0:2] is
                    not above min_cmd_speed (min_cmd_speed = 0: no gate) - the state advances all the same
        slip        sum over the feet in contact of vx_i^2 + vy_i^2
        impact      sum of max(fz_i - impact_limit, 0)
        clearance   sum of (zb_i - clearance_target)^2 (vx_i^2 + vy_i^2)

    The air times are state: ``env.feet_air_time`` ``[N, 4]``, zeroed when an env is reset or re-spawns, so the first contact of an episode
    earns nothing.  The law is ``csrc/gq_reward_feet.h``."""

    def __init__(self, *, air_time=0.0, slip=0.0, impact=0.0, clearance=0.0, air_time_target=0.5, min_cmd_speed=0.1, impact_limit=None,
                 clearance_target=None):
        self.weights = dict(air_time=float(air_time), slip=float(slip), impact=float(impact), clearance=float(clearance))
        for t, w in self.weights.items():
            if not math.isfinite(w):
                raise ValueError(f'the weight of {t} is not finite: {w}')
        self.air_time_target, self.min_cmd_speed = float(air_time_target), float(min_cmd_speed)
        self.impact_limit = None if impact_limit is None else float(impact_limit)
        self.clearance_target = None if clearance_target is None else float(clearance_target)
        if self.weights['air_time'] != 0.0 and not math.isfinite(self.air_time_target):
            raise ValueError(f'air_time_target is not finite with air_time on: {air_time_target}')
        if not (self.min_cmd_speed >= 0.0 and math.isfinite(self.min_cmd_speed)):
            raise ValueError(f'min_cmd_speed must be finite and >= 0, got {min_cmd_speed}')
        if self.weights['impact'] != 0.0 and not (self.impact_limit is not None and self.impact_limit > 0.0 and math.isfinite(self.impact_limit)):
            raise ValueError(f'impact_limit must be positive and finite with impact on, got {impact_limit}')
        if self.weights['clearance'] != 0.0 and not (self.clearance_target is not None and math.isfinite(self.clearance_target)):
            raise ValueError(f'clearance_target must be finite with clearance on, got {clearance_target}')

    def __getattr__(self, name):
        if name in FOOT_TERMS:
            return self.weights[name]
        raise AttributeError(name)

    def __repr__(self):
        on = ', '.join(f'{t}={w:g}' for t, w in self.weights.items() if w != 0.0)
        return (f'FootRewardSpec({on}, air_time_target={self.air_time_target:g}, min_cmd_speed={self.min_cmd_speed:g}, impact_limit={self.impact_limit}, '
                f'clearance_target={self.clearance_target})')

    @property
    def on(self):
        return any(w != 0.0 for w in self.weights.values())

    @property
    def gated(self):
        """the command gate of air_time is evaluated"""
        return self.weights['air_time'] != 0.0 and self.min_cmd_speed > 0.0

    def _term_obs(self):
        """term -> ((observable, per-foot components or None for contact_state / the base columns), ...) for the terms that are on"""
        out = {}
        if self.weights['air_time'] != 0.0:
            out['air_time'] = ('contact_state',) + (('base_lin_vel_err:base', 'base_lin_vel:base') if self.gated else ())
        if self.weights['slip'] != 0.0:
            out['slip'] = ('contact_state', 'feet_vel')
        if self.weights['impact'] != 0.0:
            out['impact'] = ('contact_forces',)
        if self.weights['clearance'] != 0.0:
            out['clearance'] = ('feet_pos:base', 'feet_vel')
        return out

    def required_obs(self):
        """the observable names the non-zero foot terms read, in the terms' order, each once"""
        names = []
        for obs in self._term_obs().values():
            names += [n for n in obs if n not in names]
        return tuple(names)

    def columns(self, state_obs_names, legs_order=LEG_NAMES):
        """what the library resolves from the batch's layout, for the foot terms that are on: 'feet:contact' (4 columns, FL FR RL RR),
        'feet:vx', 'feet:vy', 'feet:fz', 'feet:zb' (4 each, the same physical feet whatever ``legs_order``: contact_state is canonical in
        the row, the others follow ``legs_order``), 'feet:cmd_err', 'feet:cmd_vel' (2 each, with the gate).  ``ValueError`` names a
        missing observable."""
        start = _obs_starts(state_obs_names)
        slot = [tuple(legs_order).index(leg) for leg in LEG_NAMES]   # canonical foot i sits at place slot[i] of a leg-ordered observable
        need = self._term_obs()
        for t, obs in need.items():
            for n in obs:
                if n not in start:
                    raise ValueError(f'the reward term {t} reads {n}: not in state_obs_names {tuple(state_obs_names)}')
        have = {n for obs in need.values() for n in obs}
        cols = {}
        if 'contact_state' in have:
            cols['feet:contact'] = tuple(start['contact_state'] + i for i in range(4))
        if 'feet_vel' in have:
            cols['feet:vx'] = tuple(start['feet_vel'] + 3 * slot[i] for i in range(4))
            cols['feet:vy'] = tuple(start['feet_vel'] + 3 * slot[i] + 1 for i in range(4))
        if 'contact_forces' in have:
            cols['feet:fz'] = tuple(start['contact_forces'] + 3 * slot[i] + 2 for i in range(4))
        if 'feet_pos:base' in have:
            cols['feet:zb'] = tuple(start['feet_pos:base'] + 3 * slot[i] + 2 for i in range(4))
        if self.gated:
            cols['feet:cmd_err'] = (start['base_lin_vel_err:base'], start['base_lin_vel_err:base'] + 1)
            cols['feet:cmd_vel'] = (start['base_lin_vel:base'], start['base_lin_vel:base'] + 1)
        return cols

    def sequence64(self, rows64, columns, dt, air=None, decisions=None):
        """float64 restatement over a SEQUENCE with the state carried through: rows ``[T, n, obs_dim]`` (step after step of ``n``
        independent envs), columns: ``self.columns(...)``, dt: the simulation time step, air: ``[n, 4]`` air times before the first step
        (None: zeros).  The law has thresholds; ``decisions`` (optional) supplies the float32 evaluation's choices so that both sides take
        the same branch: 'gate' ``[T, n]`` bool (the commanded speed is above min_cmd_speed), 'impact' ``[T, n, 4]`` bool (fz above the
        limit).  Returns a dict: 'sum' ``[T, n]`` - the foot terms' share of S, sum w_i term_i; 'magnitude' ``[T, n]`` - sum |w_i term_i|;
        'roundings' ``[T, n]`` - a first-order count, in units of 2^-24, of the float32 law's rounding error in 'sum' (the air-time chain
        grows by one rounding per step in the air); 'air' ``[n, 4]`` - the state after the last step."""
        x = np.asarray(rows64, dtype=np.float64)
        T, n = x.shape[0], x.shape[1]
        f32 = lambda v: np.float64(np.float32(v))
        dt = f32(dt)
        t = np.zeros((n, 4)) if air is None else np.array(air, dtype=np.float64).reshape(n, 4)
        flights = np.where(t > 0, np.round(t / dt), 0.0)   # additions behind each air time (a state handed in counts as dt-steps)
        w = {k: f32(v) for k, v in self.weights.items()}
        col = lambda k, name: x[k][:, list(columns[name])]
        S, M, E = np.zeros((T, n)), np.zeros((T, n)), np.zeros((T, n))
        for k in range(T):
            if w['air_time'] != 0.0:
                c = col(k, 'feet:contact') != 0.0
                tn = t + dt
                land = c & (t > 0)
                d = np.where(land, tn - f32(self.air_time_target), 0.0)
                A = d.sum(1)
                # tn carries flights + 1 roundings of at most 2^-24 tn each; the difference one; the sum of up to four, three
                e = np.where(land, (flights + 1) * np.abs(tn), 0.0).sum(1) + 4.0 * np.abs(d).sum(1)
                flights = np.where(c, 0.0, flights + 1)
                t = np.where(c, 0.0, tn)
                if self.gated:
                    if decisions is not None and 'gate' in decisions:
                        gate = np.asarray(decisions['gate'][k], dtype=bool)
                    else:
                        cmd = col(k, 'feet:cmd_err') + col(k, 'feet:cmd_vel')
                        gate = (cmd ** 2).sum(1) > f32(f32(self.min_cmd_speed) * f32(self.min_cmd_speed))
                    A, e = np.where(gate, A, 0.0), np.where(gate, e, 0.0)
                    d = np.where(gate[:, None], d, 0.0)
                S[k] += w['air_time'] * A; M[k] += abs(w['air_time']) * np.abs(d).sum(1); E[k] += abs(w['air_time']) * e
            if w['slip'] != 0.0:
                c = col(k, 'feet:contact') != 0.0
                Tm = np.where(c, col(k, 'feet:vx') ** 2 + col(k, 'feet:vy') ** 2, 0.0).sum(1)
                S[k] += w['slip'] * Tm; M[k] += abs(w['slip']) * Tm; E[k] += abs(w['slip']) * 8.0 * Tm          # a chain of 8 fmaf over non-negative products
            if w['impact'] != 0.0:
                d = col(k, 'feet:fz') - f32(self.impact_limit)
                pos = np.asarray(decisions['impact'][k], dtype=bool) if decisions is not None and 'impact' in decisions else d > 0
                Tm = np.where(pos, d, 0.0).sum(1)
                Ta = np.where(pos, np.abs(d), 0.0).sum(1)
                S[k] += w['impact'] * Tm; M[k] += abs(w['impact']) * Ta; E[k] += abs(w['impact']) * 4.0 * Ta   # the difference, then up to 3 adds
            if w['clearance'] != 0.0:
                d = col(k, 'feet:zb') - f32(self.clearance_target)
                Tm = (d * d * (col(k, 'feet:vx') ** 2 + col(k, 'feet:vy') ** 2)).sum(1)
                S[k] += w['clearance'] * Tm; M[k] += abs(w['clearance']) * Tm; E[k] += abs(w['clearance']) * 9.0 * Tm   # d, d d (3), the speed (2), 4 fmaf
        return dict(sum=S, magnitude=M, roundings=E, air=t)

    # -- the C block
    def _struct(self, air_time_ptr=None):
        import ctypes as C

        from .cabi import GqFootReward
        g = GqFootReward(struct_size=C.sizeof(GqFootReward), air_time_target=self.air_time_target, min_cmd_speed=self.min_cmd_speed,
                         impact_limit=0.0 if self.impact_limit is None else self.impact_limit,
                         clearance_target=0.0 if self.clearance_target is None else self.clearance_target)
        for t in FOOT_TERMS:
            setattr(g, 'w_' + t, self.weights[t])
        g.air_time = air_time_ptr
        return g
