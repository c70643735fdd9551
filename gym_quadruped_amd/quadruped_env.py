"""Batched ``QuadrupedEnv`` - MI355X-native drop-in for the reference's ``gym_quadruped.quadruped_env.QuadrupedEnv``.

Same constructor arguments, method names, observable names (``ALL_OBS``) and return structure as the reference
(``gym_quadruped/quadruped_env.py:71-406``); every array gains a leading env axis ``N = num_envs`` and lives on the
GPU as a ``torch`` tensor.  Where the reference advances ONE MuJoCo env with ``mujoco.mj_step`` (:271) and assembles
observations in Python (:277-285), this class makes ONE call into ``libgq.so`` (``gq_step``, include/gq.h) that
advances all ``N`` envs, one env per wavefront, and writes observations / termination flags on the device.

PyTorch is plumbing here: it owns the device memory and the stream; all physics, observation, termination and
reset-randomisation arithmetic runs in the hand-written HIP kernels.  There is no CPU fallback.
"""
from __future__ import annotations

import copy
import ctypes as C
import logging
import math
from pathlib import Path
from typing import Any

import numpy as np
import torch

from . import _lib
from .accessors import AccessorsMixin
from .cabi import ALL_OBS as _ALL_OBS
from .cabi import LEG_NAMES, OBS_DIMS, GqObsOut, GqResampleCfg, GqResetCfg, GqState, MarshalledModel, obs_ids_from_names
from .mjcf import ModelDesc, compile_mjcf, load_compiled
from .robot_cfgs import RobotConfig, get_robot_config
from .terrain import generate_terrain
from .utils.math_utils import _process_range
from .utils.quadruped_utils import LegsAttr, configure_observation_space, extract_mj_joint_info, spaces

log = logging.getLogger(__name__)

BASE_OBS = _ALL_OBS[0:10]
BASE_OBS_BASE_FRAME = _ALL_OBS[10:15]
GEN_COORDS_OBS = _ALL_OBS[15:22]
FEET_OBS = _ALL_OBS[22:31]

# Lowest ground friction the pyramidal-cone Newton kernel is held to the fp64 oracle at (tests/row_edge_cases.py, DESIGN.md "Known
# deviations"): R of a pyramid edge row goes with mu^2, and below this the primal Hessian M + J^T D J is out of fp32's reach
PYRAMIDAL_NEWTON_MIN_FRICTION = 0.05


def check_ground_friction(cone: int, solver: str, lowest: float, robot: str = ''):
    """Refuse a ground friction the solver gives a silently wrong answer at: ``ValueError`` for a pyramidal-cone model (``cone`` 0) under
    ``solver='newton'`` when ``lowest`` - the lower end of ``ground_friction_coeff``, or a friction set later - is below the floor."""
    if int(cone) == 0 and solver == 'newton' and float(lowest) < PYRAMIDAL_NEWTON_MIN_FRICTION:
        raise ValueError(
            f"ground friction {float(lowest):g} is below the floor {PYRAMIDAL_NEWTON_MIN_FRICTION:g} of solver='newton' on a pyramidal-cone model"
            f"{' (' + robot + ')' if robot else ''}: the regularisation of a pyramid edge row goes with the square of the friction coefficient, so the "
            "fp32 Newton Hessian loses the contact and the step returns a wrong acceleration without a flag.  solver='pgs' and the "
            'elliptic-cone robots have no such floor.')


def _make_info(env):
    """``info`` dict of ``step``: 'time', 'step_num' (value before this step's increment, as the reference reports
    it, quadruped_env.py:288-290) and 'invalid_contacts' (bool mask instead of a dict of MjContact objects).  A plain
    dict of persistent tensors: 'step_num' is refreshed in place by every step / reset, so ``get``, ``items``, ``**info``
    and copies all see it.  'contacts_dropped' has no reference counterpart: the number of contacts the narrow phase found in the
    step that did not enter the constraint set because the env was at the kernel's capacity (12 contacts / 63 rows; MuJoCo's
    mj_step has no such cap) - 0 on every env means the batch saw all its contacts."""
    return {'time': env._time, 'step_num': env._step_num_prev, 'invalid_contacts': env._invalid_b, 'contacts_dropped': env._contacts_dropped}


class QuadrupedEnv(AccessorsMixin):
    """Batched quadruped environment (see module docstring).  Single-env semantics follow the reference class of the
    same name; ``num_envs`` / ``device`` / ``auto_reset`` / solver knobs are the only additions."""

    _DEFAULT_OBS = ('qpos', 'qvel', 'tau_ctrl_setpoint', 'feet_pos:base', 'feet_vel:base')
    ALL_OBS = list(_ALL_OBS)
    metadata = {'render.modes': ['rgb_array'], 'version': 0}

    def __init__(
        self,
        robot: str,
        state_obs_names: tuple[str, ...] = _DEFAULT_OBS,
        scene: str = 'flat',
        sim_dt: float = 0.002,
        base_vel_command_type: str = 'forward',
        ref_base_lin_vel: tuple[float, float] | float = 0.5,
        ref_base_ang_vel: tuple[float, float] | float = 0.0,
        ground_friction_coeff: tuple[float, float] | float = 1.0,
        legs_order: tuple[str, str, str, str] = ('FL', 'FR', 'RL', 'RR'),
        sensors: tuple = None,
        sensors_kwargs: tuple[dict[str, Any]] = None,
        external_disturbances_kwargs: dict[str, Any] = None,
        *,
        num_envs: int = 1,
        device: str | torch.device = 'cuda:0',
        auto_reset: bool | str = False,
        solver: str = 'newton',
        solver_iterations: int = 100,
        solver_tolerance: float = 1e-8,
        solver_noise_floor: float = 1e-5,
        seed: int | None = None,
        mjcf_path: str | None = None,
        env_id_offset: int = 0,
        accessors: bool = False,
        self_collision: bool | str | None = None,   # None / True / "convex": MuJoCo's behaviour, mesh pairs through the convex routine; "capsule": capsule proxies for mesh / cylinder pairs (faster, approximate); False: off
        pair_exchange: bool = True,   # convex self pairs of an entangled env are shared with idle wavefronts of the launch (csrc/gq_exchange.h): same results, shorter launches; False: every env keeps its pairs
    ):
        self._save_hyperparameters(constructor_params=locals().copy())
        log.info(f'Initializing {robot} environment with scene {scene}.')
        self.robot_name = robot
        self.robot_cfg: RobotConfig = get_robot_config(robot_name=robot)
        self.base_vel_command_type = base_vel_command_type
        self.base_lin_vel_range = _process_range(ref_base_lin_vel)
        self.base_ang_vel_range = _process_range(ref_base_ang_vel)
        self._ground_friction_coeff_range = _process_range(ground_friction_coeff)   # (checked against the solver's floor once the model is known)
        self.legs_order = tuple(legs_order)
        self.num_envs = int(num_envs)
        # False | True / 'same_step' (terminated envs are re-spawned inside the same step call; obs = first of the new
        # episode) | 'next_step' (gymnasium's NEXT_STEP: the terminal obs is returned and the env spends its next step
        # call on reset(), ignoring that action) - see gq_step in include/gq.h
        if auto_reset not in (False, True, 'same_step', 'next_step'):
            raise ValueError(f"auto_reset must be False, True, 'same_step' or 'next_step', got {auto_reset!r}")
        self.auto_reset = bool(auto_reset)
        self.auto_reset_mode = None if not auto_reset else ('next_step' if auto_reset == 'next_step' else 'same_step')
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.GqError('QuadrupedEnv runs on a ROCm GPU only (device must be cuda:N); there is no CPU path')

        # scene + model (reference :150-183)
        self.scene_desc, self.terrain_limits = generate_terrain(scene, self.robot_cfg.hip_height, seed=10)
        self.mjModel: ModelDesc = (compile_mjcf(mjcf_path) if mjcf_path
                                   else load_compiled(Path(self.robot_cfg.mjcf_filename).stem))
        qpos0 = self.mjModel.qpos0.copy()
        if self.robot_cfg.qpos0_js is not None:
            qpos0[7:] = np.asarray(self.robot_cfg.qpos0_js, dtype=np.float64)
        self.mjModel.qpos0 = qpos0
        self._mm = MarshalledModel(self.mjModel, qpos0=qpos0, feet_geom_names=self.robot_cfg.feet_geom_names,
                                   terrain_limits=self.terrain_limits, timestep=sim_dt, solver={'pgs': 0, 'newton': 1}[solver],
                                   iterations=solver_iterations, tolerance=solver_tolerance, noise_floor=solver_noise_floor,
                                   floor=self.scene_desc.get('floor'), boxes=self.scene_desc.get('boxes'),
                                   hfield=self.scene_desc.get('hfield'), self_collision=self_collision)
        self._sim_dt = float(sim_dt)
        self._solver = solver
        check_ground_friction(self.mjModel.cone, solver, self.ground_friction_coeff_range[0], robot)

        # leg index maps (reference :189-212)
        self.joint_info = extract_mj_joint_info(self.mjModel)
        self.legs_qpos_idx = LegsAttr(None, None, None, None)
        self.legs_qvel_idx = LegsAttr(None, None, None, None)
        self.legs_tau_idx = LegsAttr(None, None, None, None)
        for leg in ['FR', 'FL', 'RR', 'RL']:
            qi, vi, ti = [], [], []
            for jn in self.robot_cfg.leg_joints[leg]:
                assert jn in self.joint_info, f'Joint {jn} not found in {list(self.joint_info.keys())}'
                qi.extend(self.joint_info[jn].qpos_idx); vi.extend(self.joint_info[jn].qvel_idx); ti.extend(self.joint_info[jn].tau_idx)
            self.legs_qpos_idx[leg], self.legs_qvel_idx[leg], self.legs_tau_idx[leg] = qi, vi, ti
        self._feet_geom_id = LegsAttr(None, None, None, None)
        self._feet_body_id = LegsAttr(None, None, None, None)
        for leg in ['FR', 'FL', 'RR', 'RL']:
            g = self.mjModel.geom_names.index(self.robot_cfg.feet_geom_names[leg])
            self._feet_geom_id[leg] = g
            self._feet_body_id[leg] = int(self.mjModel.geom_bodyid[g])

        # spaces (reference :215-230; the action Box is unbounded there because of the truthiness slip, quirk B2)
        nu = self.mjModel.nu
        self.action_space = spaces.Box(shape=(nu,), low=np.full(nu, -np.inf), high=np.full(nu, np.inf), dtype=np.float32)
        self.state_obs_names = tuple(state_obs_names)
        self.observation_space = configure_observation_space(mj_model=self.mjModel, obs_names=self.state_obs_names)
        self._obs_ids = obs_ids_from_names(self.state_obs_names)
        # accessors=True: the kernel also writes every ALL_OBS observable the user did not ask for, behind the user's
        # columns, so that the reference's getters (base_lin_vel(frame), feet_pos(frame), ...) are views (accessors.py)
        self._extra_names = tuple(n for n in _ALL_OBS if n not in self.state_obs_names) if accessors else ()
        self._all_ids = list(self._obs_ids) + obs_ids_from_names(self._extra_names)
        self._launches = 0
        self._hm_fresh = False   # a HeightMap(follow_base=True) holds the rays of the CURRENT state (written by the last step's kernel)
        self._hm_follow = None   # weakref to THE HeightMap(follow_base=True) registered with the step kernel (one output slot per batch)
        self._hm_version = -1

        # device state: one tensor per field, env-major rows
        N, dev = self.num_envs, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        self._qpos = torch.zeros(N, 19, dtype=torch.float64, device=dev)
        self._qvel = torch.zeros(N, 18, **f32)
        self._qacc = torch.zeros(N, 18, **f32)
        self._warm = torch.zeros(N, 18, **f32)
        self._applied = torch.zeros(N, 18, **f32)
        self._time = torch.zeros(N, **f32)
        self._friction = torch.full((N,), -1.0, **f32)   # < 0: XML frictions until the first reset sets it
        self._cmd = torch.zeros(N, 4, **f32)
        self._ctrl = torch.zeros(N, nu, **f32)
        self._last_action = self._ctrl
        self._obs_dim = int(sum(OBS_DIMS[i] for i in self._all_ids))   # row width the kernel writes
        self._obs_buf = torch.zeros(N, self._obs_dim, **f32)
        self._reward = torch.zeros(N, **f32)
        self._feet_air = torch.zeros(N, 4, **f32)   # the foot reward terms' state (feet_air_time)
        self._policy_hidden = None                  # a GruPolicy's hidden state [N, H] (policy_hidden): allocated on first use
        self._policy_hist = None                    # an ObsHistory's store (policy_history): (state [N, 2, L, F], ctl [N] int32), on first use
        self._terminated = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._truncated = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._invalid = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._terminated_b = self._terminated.view(torch.bool)
        self._truncated_b = self._truncated.view(torch.bool)
        self._invalid_b = self._invalid.view(torch.bool)
        self._step_num = torch.zeros(N, dtype=torch.int32, device=dev)
        self._step_num_prev = torch.zeros(N, dtype=torch.int32, device=dev)   # info['step_num'], written by the kernel
        self._contacts_dropped = torch.zeros(N, dtype=torch.int32, device=dev)  # info['contacts_dropped'], written by the kernel
        self._lift_failed = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._mask_all = torch.ones(N, dtype=torch.uint8, device=dev)
        # in-episode resampling state (reference :292-305), advanced by the step kernel's epilogue:
        # columns {after_vel, before_vel, n_vel, after_dist, before_dist, n_dist} (gq_batch_set_resampling)
        self._h9 = torch.zeros(N, 6, dtype=torch.int32, device=dev)
        self._h9[:, 1] = 1 << 30
        self._h9[:, 4] = 1 << 30
        self._ext_dist = torch.zeros(N, 6, **f32)
        self._has_cmd = False
        self._obs_views, self._extra_views, k = {}, {}, 0
        for name, i in zip(self.state_obs_names + self._extra_names, self._all_ids):
            (self._obs_views if name in self.state_obs_names else self._extra_views)[name] = self._obs_buf[:, k:k + OBS_DIMS[i]]
            k += OBS_DIMS[i]
        self._key_qpos = torch.as_tensor(self.mjModel.key_qpos[0] if len(self.mjModel.key_qpos) else qpos0, dtype=torch.float64, device=dev)
        self._gen = torch.Generator(device=dev)
        self._gen.manual_seed(0 if seed is None else int(seed))

        # C-ABI handles
        L = _lib.lib()
        self._L = L
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._hmodel = C.c_void_p()
        _lib.check(L.gq_model_create(C.byref(self._mm.desc), int(dev_index), C.byref(self._hmodel)), 'gq_model_create')
        ids = np.asarray(self._all_ids, dtype=np.int32)
        lo = np.asarray([LEG_NAMES.index(l) for l in self.legs_order], dtype=np.int32)
        self._hbatch = C.c_void_p()
        _lib.check(L.gq_batch_create(self._hmodel, N, ids.ctypes.data, len(ids), lo.ctypes.data, C.byref(self._hbatch)), 'gq_batch_create')
        assert L.gq_batch_obs_dim(self._hbatch) == self._obs_dim
        if not pair_exchange and self._mm.self_collision == 'convex':
            L.gq_batch_set_pair_exchange(self._hbatch, 0)   # (a model without convex self pairs has no exchange to switch off)
        self._st = GqState(self._qpos.data_ptr(), self._qvel.data_ptr(), self._qacc.data_ptr(), self._warm.data_ptr(),
                           self._applied.data_ptr(), self._time.data_ptr(), self._friction.data_ptr(), self._cmd.data_ptr())
        self._out = GqObsOut(self._obs_buf.data_ptr(), self._reward.data_ptr(), self._terminated.data_ptr(),
                             self._truncated.data_ptr(), self._invalid.data_ptr(), self._step_num.data_ptr(),
                             self._step_num_prev.data_ptr(), self._contacts_dropped.data_ptr())
        # accessors=True: the production kernel also writes the dynamics row (mj_fullM, qfrc_bias, body poses, foot points) and
        # the contact row (mjData.contact + mj_contactForce) of every step - what the reference's model-based-control getters
        # read from mjData (accessors.py); no instrumented kernel variant involved
        self._dyn = self._contacts = None
        if accessors:
            from .cabi import GQ_CON_STRIDE, GQ_DYN
            self._dyn = torch.zeros(N, GQ_DYN['STRIDE'], **f32)
            self._contacts = torch.zeros(N, GQ_CON_STRIDE, **f32)
            _lib.check(L.gq_batch_set_outputs(self._hbatch, self._dyn.data_ptr(), self._contacts.data_ptr()), 'gq_batch_set_outputs')
        self._info = _make_info(self)
        self._episode = torch.zeros(N, dtype=torch.int32, device=dev)
        t = self.base_vel_command_type
        if not any(k in t for k in ('forward', 'random', 'human')):
            raise ValueError(f'Invalid base linear velocity command type: {t}')
        self._seed = 0 if seed is None else int(seed)
        self._reset_cfg = GqResetCfg(
            seed=self._seed, random=1, q_pos_amp=20 * math.pi / 180, q_vel_amp=0.5, roll_sweep=10 * math.pi / 180,
            pitch_sweep=10 * math.pi / 180, hip_height=float(self.robot_cfg.hip_height),
            lin_vel_range=(C.c_float * 2)(*map(float, self.base_lin_vel_range)),
            ang_vel_range=(C.c_float * 2)(*map(float, self.base_ang_vel_range)),
            friction_range=(C.c_float * 2)(*map(float, self.ground_friction_coeff_range)),
            cmd_forward=int('forward' in t), cmd_random=int('forward' not in t and 'random' in t),
            cmd_rotate=int('rotate' in t), cmd_human=int('human' in t), env_id_offset=int(env_id_offset))
        # auto-reset happens inside the step kernel (terminated envs take a second pass); None = off
        self._auto_cfg_struct = GqResetCfg.from_buffer_copy(self._reset_cfg)  # user reset() options never leak into it
        self._auto_cfg_struct.autoreset_next_step = int(self.auto_reset_mode == 'next_step')
        self._auto_cfg = C.pointer(self._auto_cfg_struct) if self.auto_reset else None

        self.external_disturbances_kwargs = external_disturbances_kwargs
        if self.external_disturbances_kwargs is not None:
            self._sample_external_disturbances(self._mask_all.view(torch.bool))   # reference :240-242 (constructor draw)
        dist_reset = external_disturbances_kwargs is not None and external_disturbances_kwargs.get('type') == 'reset'
        if 'reset' in t or dist_reset:
            rs = GqResampleCfg(seed=self._seed, cmd_reset=int('reset' in t), dist_reset=int(dist_reset), env_id_offset=int(env_id_offset))
            for k, key in enumerate(('x', 'y', 'z', 'roll', 'pitch', 'yaw')):
                r = (external_disturbances_kwargs or {}).get(key)
                kind = 0 if (r is None or len(r) == 0) else min(len(r), 2)
                rs.dist_kind[k] = kind
                rs.dist_range[k][0] = float(r[0]) if kind >= 1 else 0.0
                rs.dist_range[k][1] = float(r[1]) if kind == 2 else 0.0
            self._resample_cfg = rs
            _lib.check(L.gq_batch_set_resampling(self._hbatch, C.byref(rs), C.byref(self._reset_cfg), self._h9.data_ptr(),
                                                 self._ext_dist.data_ptr()), 'gq_batch_set_resampling')
        self.viewer = None
        # sensors (reference :232-236): sensor_cls(mj_model=..., mj_data=..., **kwargs); mj_data is this env
        self.sensors = []
        if sensors is not None:
            for sensor_cls, kw in zip(sensors, sensors_kwargs or [{}] * len(sensors)):
                self.sensors.append(sensor_cls(mj_model=self.mjModel, mj_data=self, **kw))
        from .sensors.imu import IMU
        for sn in self.sensors:
            if isinstance(sn, IMU):
                sn.cfg.seed = int(sn.cfg.seed) + int(env_id_offset)
                _lib.check(L.gq_batch_set_imu(self._hbatch, C.byref(sn.cfg), sn.bias_state.data_ptr()), 'gq_batch_set_imu')
        sensor_obs = [o for sn in self.sensors for o in sn.available_observations()]
        for name in self.state_obs_names:
            if name.startswith('imu') and name not in sensor_obs:
                raise ValueError(f'Invalid observation name: {name}: no sensor provides it (pass sensors=(IMU,), sensors_kwargs=...)')
        self._profile_events = None  # optional (start, end) torch.cuda.Event pair recorded around the gq_step launch

    # ------------------------------------------------------------------ core API
    def step(self, action):
        """Advance every env by one ``sim_dt`` (reference ``step`` :251-307).

        action: ``[N, nu]`` joint torques (tensor / array; ``[nu]`` is broadcast when N == 1).
        Returns ``(obs, reward, terminated, truncated, info)`` with obs a dict ``name -> [N, dim]`` float32 tensor
        (views of one persistent buffer, overwritten by the next call), reward ``[N]``, terminated/truncated ``[N]``
        bool and info {'time' [N], 'step_num' [N], 'invalid_contacts' [N] bool}.
        """
        if (torch.is_tensor(action) and action.dtype == torch.float32 and action.device == self.device
                and action.shape == self._ctrl.shape and action.is_contiguous()):
            self._last_action = action      # zero-copy: the kernel reads the caller's tensor
        else:
            a = torch.as_tensor(action, dtype=torch.float32, device=self.device)
            if a.dim() == 1:
                a = a.unsqueeze(0).expand(self.num_envs, -1)
            if a.shape != self._ctrl.shape:
                raise ValueError(f'action must have shape {tuple(self._ctrl.shape)}, got {tuple(a.shape)}')
            self._ctrl.copy_(a)
            self._last_action = self._ctrl
        stream = torch.cuda.current_stream(self.device).cuda_stream
        ev = self._profile_events
        if ev is not None:
            ev[0].record()
        _lib.check(self._L.gq_step(self._hbatch, self._last_action.data_ptr(), None, self._st, self._out, self._auto_cfg,
                                   self._episode.data_ptr(), self._lift_failed.data_ptr(), stream), 'gq_step')
        if ev is not None:
            ev[1].record()
        self._launches += 1
        # a HeightMap(follow_base=True) registered with this env now holds the rays of the NEW state; the flag is tied to the version counter of the
        # state tensor, so that an in-place write (env.qpos[...] = x) makes it stale again
        self._hm_fresh = self._hm_follow is not None and self._hm_follow() is not None
        self._hm_version = self._qpos._version
        self._note_step()
        for sensor in self.sensors:  # reference :273-274 (kernel-side sensors: no-op)
            sensor.step()

        # command / disturbance resampling (reference :292-305) ran in the kernel's epilogue (gq_batch_set_resampling)
        return self._obs_views, self._reward, self._terminated_b, self._truncated_b, self._info

    def rollout(self, actions, shards: int = 2, obs_out=None):
        """Open-loop rollout: ``K = len(actions)`` steps of every env with the given action sequence (``[K, N, nu]`` float32 on
        the device), equivalent to ``for a in actions: env.step(a)`` - same kernels, same state afterwards, bit for bit -
        but pipelined: the batch is cut into ``shards`` contiguous groups of envs, each group's K launches are chained on a HIP
        stream of its own, and since envs are independent no launch waits for another group's stragglers or for the gap
        between two dependent launches (``gq_step_range``).  With a policy in the loop this is not available - the next
        action needs every env's observation - which is what ``step`` is for; random-action rollouts, dataset recording
        (the reference's examples/aliengo_dataset.py) and replaying planned torque sequences are.  Measured gain on MI355X at
        4096 envs: +6 % with 2 shards; more shards lose (overlapping launches share the SIMDs).

        ``obs_out``: optional ``[K, N, obs_dim]`` float32 tensor that receives the observation rows of every step.
        Host-side sensors get their K ``step()`` calls after the launches (they see the final state only); the per-step
        profiling events of ``step`` are not recorded.
        Returns the observation dict of the last step (views, like ``step``)."""
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.device)
        if a.dim() != 3 or tuple(a.shape[1:]) != tuple(self._ctrl.shape):
            raise ValueError(f'actions must have shape (K, {self.num_envs}, {self.mjModel.nu}), got {tuple(a.shape)}')
        a = a.contiguous()
        K = int(a.shape[0])
        if K == 0:
            raise ValueError('rollout needs at least one step (actions has K == 0)')
        if obs_out is not None and (tuple(obs_out.shape) != (K, self.num_envs, self._obs_dim) or obs_out.dtype != torch.float32 or not obs_out.is_contiguous()):
            raise ValueError(f'obs_out must be a contiguous float32 tensor of shape {(K, self.num_envs, self._obs_dim)}')
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._hm_fresh = False
        _lib.check(self._L.gq_rollout(self._hbatch, a.data_ptr(), K, int(shards), self._st, self._out, self._auto_cfg, self._episode.data_ptr(),
                                      self._lift_failed.data_ptr(), None if obs_out is None else obs_out.data_ptr(), stream), 'gq_rollout')
        self._last_action = a[K - 1]
        self._launches += K
        self._note_step()
        for sensor in self.sensors:  # host-side sensors advance once per env step, as in the step loop (kernel-side ones: no-op)
            for _ in range(K):
                sensor.step()
        return self._obs_views

    def rollout_closed_loop(self, n_steps: int, kp, kd, q_des=None, *, mode: str = 'inline', record_obs: bool = False, record_actions: bool = False,
                            noise_sigma: float = 0.0, policy_waves: int = 0, step_waves: int = 0, timeout_s: float = 5.0, check: bool = True):
        """``n_steps`` steps of every env with a joint-space PD policy IN the loop and no launch boundary (``gq_rollout_closed``):
        the device-side form of ``for k: a = kp * (q_des - obs['qpos_js']) - kd * obs['qvel_js']; obs, ... = env.step(a)``
        (the reference's control loop, README.md:31-33, around quadruped_env.py:251-307).  Env-steps are tasks: a policy kernel on
        a second stream turns each published observation row into the env's next action and queues the env; the wavefronts of
        one persistent step launch pop ready envs, step them (next-step auto-reset included) and publish the result.  An env
        waits for ITS action only - never for the slowest env of a step - so the throughput is that of the open-loop
        persistent rollout, with the loop closed.  State, flags and observations afterwards equal the step loop's with the same
        actions, bit for bit.

        mode 'mailbox': the policy is a kernel of its own on a second stream, actions and observations travel through per-env
        mailboxes and per-XCD ready queues - the general mechanism (any resident policy kernel can take that seat); 'inline': the
        wavefront that steps an env evaluates the PD law itself - no turn-around latency, the faster form when there are no more
        envs than wavefront slots (4096 on an MI355X).  Both leave the same bits.

        kp, kd: scalars or 12 values (hinge order of ``qpos[7:]``); q_des: 12 joint angles (default: keyframe 0); noise_sigma:
        Gaussian exploration noise added to every torque (counter-based draws keyed by the env's seed, the step and the joint).
        Returns a dict with the last observation views under 'obs' and, when asked, 'obs_seq' ``[K, N, obs_dim]`` /
        'actions' ``[K, N, 12]``.  ``check``: wait for the rollout and raise ``GqError`` if a participant gave up waiting
        (deadline ``timeout_s`` per wait) instead of leaving that to the caller."""
        from .cabi import GqPolicyPd
        K = int(n_steps)
        if K < 0:
            raise ValueError('n_steps must be >= 0')
        qd = self._key_qpos[7:19].float().cpu().numpy() if q_des is None else np.asarray(q_des, dtype=np.float32).reshape(12)
        pd = GqPolicyPd()
        pd.kp = (C.c_float * 12)(*np.broadcast_to(np.asarray(kp, dtype=np.float32), (12,)))
        pd.kd = (C.c_float * 12)(*np.broadcast_to(np.asarray(kd, dtype=np.float32), (12,)))
        pd.q_des = (C.c_float * 12)(*[float(v) for v in qd])
        pd.noise_sigma, pd.noise_seed, pd.noise_step0 = float(noise_sigma), int(self._seed or 0) & (2 ** 64 - 1), int(self._launches) & 0x7fffffff
        f32 = dict(dtype=torch.float32, device=self.device)
        obs_seq = torch.empty(K, self.num_envs, self._obs_dim, **f32) if record_obs else None
        act_seq = torch.empty(K, self.num_envs, self.mjModel.nu, **f32) if record_actions else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if mode not in ('inline', 'mailbox'):
            raise ValueError("mode must be 'inline' or 'mailbox'")
        self._hm_fresh = False
        _lib.check(self._L.gq_rollout_closed(self._hbatch, K, int(mode == 'inline'), C.byref(pd), int(policy_waves), int(step_waves), float(timeout_s), self._st, self._out,
                                             self._auto_cfg, self._episode.data_ptr(), self._lift_failed.data_ptr(),
                                             None if obs_seq is None else obs_seq.data_ptr(), None if act_seq is None else act_seq.data_ptr(), stream),
                   'gq_rollout_closed')
        self._launches += K
        if check:
            self.closed_loop_status()
        for sensor in self.sensors:
            for _ in range(K):
                sensor.step()
        return {'obs': self._obs_views, 'obs_seq': obs_seq, 'actions': act_seq}

    def _policy_struct(self, policy, rollout=True):
        """``policy``'s C block for this batch; rollout: after the check only this side can make - the network reads the user's own columns"""
        from .policy import GruPolicy, MlpPolicy
        if not isinstance(policy, (MlpPolicy, GruPolicy)):
            raise ValueError(f'policy must be an MlpPolicy or a GruPolicy, got {type(policy).__name__}')
        width = sum(int(v.shape[1]) for v in self._obs_views.values())
        if rollout and policy.in_obs > width:
            raise ValueError(f"the policy reads {policy.in_obs} observation columns, state_obs_names gives {width} (the accessors' extra columns are not fed to a policy)")
        return policy._struct(self.device, rows_given=not rollout)   # (policy_eval: the rows are the full input rows, a scan's columns among them)

    def _hidden_for(self, policy):
        """``policy_hidden`` for a ``GruPolicy``: zeros on first use, refused when it was sized for another ``H``"""
        H = policy.hidden
        if self._policy_hidden is None:
            self._policy_hidden = torch.zeros(self.num_envs, H, dtype=torch.float32, device=self.device)
        if self._policy_hidden.shape[1] != H:
            raise ValueError(f'env.policy_hidden holds {self._policy_hidden.shape[1]} hidden units per env, the policy has {H}: assign env.policy_hidden '
                             f'a [{self.num_envs}, {H}] tensor first')
        return self._policy_hidden

    def _history_for(self, policy):
        """the store behind ``policy_history`` for an ``MlpPolicy`` with an ``ObsHistory``: empty on first use, refused when it was sized for
        another ``(L, F)``"""
        L, F = policy.history.frames, policy.hist_words
        if self._policy_hist is None:
            self._policy_hist = (torch.zeros(self.num_envs, 2, L, F, dtype=torch.float32, device=self.device),
                                 torch.zeros(self.num_envs, dtype=torch.int32, device=self.device))
        have = tuple(self._policy_hist[0].shape[2:])
        if have != (L, F):
            raise ValueError(f'env.policy_history holds {have[0]} frames of {have[1]} words per env, the policy has {L} of {F}: assign env.policy_history '
                             f'a [{self.num_envs}, {L}, {F}] tensor first')
        return self._policy_hist

    def rollout_policy(self, n_steps: int, policy, kp, kd, q_default=None, action_scale=0.25, action_clip=None, decimation: int = 4, noise_sigma=0.0,
                       record_obs: bool = False, record_actions: bool = False, policy_waves: int = 0, step_waves: int = 0, timeout_s: float = 5.0,
                       check: bool = True, reward=None, record_transitions: bool = False, obs_noise=None):
        """``n_steps`` steps of every env with an MLP policy IN the loop and no launch boundary (``gq_rollout_policy``): the device-side
        form of ::

            for p in range(n_steps // decimation):
                a = policy(cat(obs_row[:, :in_obs], a_prev)) + noise_sigma * z;  a = clip(a, -action_clip, action_clip)
                obs, ... = env.step_pd(q_default + action_scale * a, kp, kd, decimation=decimation)

        on the machinery of ``rollout_closed_loop(mode='mailbox')``: a resident policy kernel takes the ready envs through the network 16
        at a time on the matrix cores (``policy``: an ``MlpPolicy``), holds each env's action for ``decimation`` steps and turns it into
        torques at EVERY step with the joint-impedance law of ``step_pd`` on the ``qpos_js`` / ``qvel_js`` (or ``qpos`` / ``qvel``)
        columns of the observation row; the step side is that of ``rollout_closed_loop``.  State, flags and observations afterwards equal
        the step loop's with the recorded torques, bit for bit.

        The network reads the first ``policy.in_obs`` columns of the observation row - ``state_obs_names``' columns, never the extras of
        ``accessors=True`` - and, with ``feed_last_action``, the env's previous policy action (zeros at the first policy step of a
        call).  ``n_steps`` must be a multiple of ``decimation``: no held action crosses calls.  An env that re-spawns ignores that
        step's torque (next-step auto-reset) and KEEPS its held and its last action: neither is reset with the env.

        kp, kd, action_scale, noise_sigma: a scalar or 12 values (hinge order of ``qpos[7:]``); q_default: 12 joint angles (default:
        keyframe 0); action_clip: None or a bound on ``|a|``; noise_sigma: Gaussian exploration noise on the action (counter-based draws
        keyed by the env's seed, the step and the joint).  Returns a dict: 'obs' (the last observation views), 'obs_seq'
        ``[K, N, obs_dim]`` / 'actions' ``[K, N, 12]`` (the torques) when asked for, else None, and 'policy_actions'
        ``[K // decimation, N, 12]`` (the network's actions, when ``record_actions``).  ``check``: as in ``rollout_closed_loop``.

        THE LEARNING HALF (``gq_rollout_policy_learn``; with ``reward=None`` and ``record_transitions=False`` the call and the dict's keys
        are the ones above).  ``reward``: a ``RewardSpec`` - the policy seat evaluates the reward of every physics step from the
        observation row after it, the torques applied in it, the held action and the one before it and the ``terminated`` flag
        (``csrc/gq_reward.h``), and sums it per decimation window ``s`` (the window law: ``csrc/gq_learn.h`` is its definition), the form of ::

            acc, done, dead = float32(0), 0, False
            for k in range(D * s, D * s + D):
                respawn = (k > 0 and terminated_after[k - 1]) or (k == 0 and the env was waiting for its re-spawn before the call)
                if not dead and not respawn:
                    acc += r_k;  if terminated_after[k]: done, dead = 1, True

        a re-spawn step earns nothing, and after a termination the rest of the window earns nothing (the new episode starts at window
        ``s + 1``); ``action_rate`` is 0 in the first window of a call.  The dict gains 'rewards' ``[K // D, N]`` float32 and 'dones'
        ``[K // D, N]`` bool.  ``record_transitions``: the dict gains 'policy_obs' ``[K // D, N, policy.in_dim]`` - the row the network
        was fed at each policy step, before shift / scale: the observation columns, then the fed-back action - 'policy_means'
        ``[K // D, N, 12]`` - the network's output before noise and clip - and 'policy_actions' (as under ``record_actions``): what the old
        log-probability of a policy-gradient step needs, at the policy's rate.

        THE FOOT TERMS (``gq_rollout_policy_learn_feet``; a ``reward`` without ``feet``, or with every foot weight 0, is the call above):
        ``RewardSpec(..., feet=FootRewardSpec(...))`` continues every step's sum with air time, slip, impact and clearance
        (``csrc/gq_reward_feet.h``).  The air times are ``env.feet_air_time``: they persist across calls, advance at every step but an env's
        re-spawn step, which zeroes them - also in the tail of a window after a fall, which earns nothing.

        A RECURRENT POLICY (``policy``: a ``GruPolicy``, every mode above; ``gq_rollout_policy_gru``): a GRU cell on the same input row, a
        head on its hidden state.  The hidden state is ``env.policy_hidden`` ``[N, H]``: it persists across calls and follows the episode
        rule of ``csrc/gq_policy_gru.h`` - the policy seat zeroes an env's row at the visit that sees its termination (at the first step of
        a call: that the env waits for its re-spawn), before any cell evaluation, so the state fed at policy step ``s + 1`` is zero exactly
        where ``dones[s]`` is set, the mask ``h <- (1 - done) h`` of a recurrent learner.  With ``record_transitions`` the dict gains
        'policy_hidden' ``[K // D, N, H]``: the state FED at each policy step, after the rule.  ``policy_waves=0``: the policy's default.

        A HEIGHT SCAN (a policy built with ``height_scan=HeightScan(rows, cols, ...)``, every mode above; ``gq_rollout_policy_scan``): the env
        must hold a ``HeightMap(rows, cols, ..., follow_base=True)``; its cells, through the scan law of ``csrc/gq_policy_scan.h``, are the
        columns between the observation columns and the fed-back action.  The stepping wavefront casts the map's rays at every step, so the
        scan fed at a policy step is that of the state the observation row fed with it describes - across a re-spawn too.  Before the launch
        the map is brought up to date (``update_height_map()``: nothing when the last step left it, one ray launch after a reset or a state
        write).  'policy_obs' records the scan words as fed; ``env.height_scan`` evaluates the same law on any hits.

        AN OBSERVATION HISTORY (an ``MlpPolicy`` built with ``history=ObsHistory(frames, cols)``, every mode of the MLP above, with or without
        a scan; ``gq_rollout_policy_hist``): the frames of the env's last ``frames`` policy steps - what the network was fed as its current
        block, raw: the first ``cols`` observation words and the fed-back action - follow the fed-back action in the input row, newest first;
        the device-side form of ``hist = where(done, 0, hist); x = cat(row, a_prev, hist); hist = roll(hist) with the current block first``.
        The frames are ``env.policy_history`` ``[N, frames, F]``: they persist across calls and follow the GRU's episode rule
        (``csrc/gq_policy_hist.h``) - all frames of an env become zero at the visit that sees its termination (at the first step of a call:
        that the env waits for its re-spawn), so the history fed at policy step ``s + 1`` is all zero exactly where ``dones[s]`` is set; in
        the plain mode a fall in the call's last step is left to the next call's first step.  The fed-back last action itself keeps its rule
        - zeros at the first policy step of a call, kept across a re-spawn, NOT reset with the env - and a frame holds it as it was fed.
        'policy_obs' records the history words raw, as fed.

        SENSOR NOISE (``obs_noise=ObsNoise(amp, kind, scan_amp)``, every mode above; ``gq_rollout_policy_noise``; with ``None`` the call, the
        entry point and the dict's keys are the ones above): the observation and scan columns the network is FED carry counter-based noise
        in raw units, before shift / scale (``csrc/gq_policy_noise.h``), keyed by the env's seed, the column, the step counter and the
        global env id.  The fed-back action and a history's frames are never noised - a frame, and ``env.policy_history``, hold the noisy
        word the current block was fed.  Only the network's input is noised: the joint-impedance law, the reward, the foot terms and the
        episode rules read the true row, so state, flags and observations afterwards still equal the step loop's with the recorded
        torques.  With ``record_transitions`` 'policy_obs' is the row AS FED, noisy - what an actor's old log-probability needs - and the
        dict gains 'policy_obs_clean' ``[K // D, N, policy.in_dim]``, the same row with the true words in the noised columns - what an
        asymmetric critic needs.  ``obs_noise_eval`` evaluates the same law on given rows."""
        from .policy import GruPolicy
        recurrent = isinstance(policy, GruPolicy)
        K, D = int(n_steps), int(decimation)
        if K < 0:
            raise ValueError('n_steps must be >= 0')
        if D < 1:
            raise ValueError(f'decimation must be >= 1, got {decimation}')
        if K % D:
            raise ValueError(f'n_steps = {K} must be a multiple of decimation = {D}: no held action crosses calls')
        m = self._policy_struct(policy)
        if recurrent:
            m, gr = m
            gr.hidden_state = self._hidden_for(policy).data_ptr()
            policy_waves = int(policy_waves) or policy.default_policy_waves
        scan = getattr(policy, 'height_scan', None)
        if scan is not None:
            sc = scan._struct()
            self._scan_map(scan).update_height_map()   # the hits at policy step 0 belong to the state the env now holds
            if not recurrent:   # (a GruPolicy keeps its own default)
                policy_waves = int(policy_waves) or scan.default_policy_waves
        hist = getattr(policy, 'history', None)
        if hist is not None:
            hs = policy._hist_struct(*self._history_for(policy))
            if scan is None:
                policy_waves = int(policy_waves) or hist.default_policy_waves
        row12 = lambda v: (C.c_float * 12)(*np.broadcast_to(np.asarray(v, dtype=np.float32), (12,)))
        m.kp, m.kd, m.action_scale, m.noise_sigma = row12(kp), row12(kd), row12(action_scale), row12(noise_sigma)
        m.q_default = row12(self._key_qpos[7:19].float().cpu().numpy() if q_default is None else np.asarray(q_default, dtype=np.float32).reshape(12))
        m.action_clip = 0.0 if action_clip is None else float(action_clip)
        if action_clip is not None and not m.action_clip > 0.0:
            raise ValueError(f'action_clip must be positive or None, got {action_clip}')
        m.decimation, m.noise_seed, m.noise_step0 = D, int(self._seed or 0) & (2 ** 64 - 1), int(self._launches) & 0x7fffffff
        obs_seq, act_seq = self._window_records(K, record_obs, record_actions)
        learning = reward is not None or record_transitions
        f32 = dict(dtype=torch.float32, device=self.device)
        pol_seq = torch.empty(K // D, self.num_envs, 12, **f32) if record_actions or record_transitions else None
        m.policy_actions = None if pol_seq is None else pol_seq.data_ptr()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()
        extra = {}
        if learning:
            from .reward import RewardSpec
            if reward is not None and not isinstance(reward, RewardSpec):
                raise ValueError(f'reward must be a RewardSpec, got {type(reward).__name__}')
            g = (reward if reward is not None else RewardSpec())._struct()
            if reward is not None:
                extra['rewards'] = torch.zeros(K // D, self.num_envs, **f32)
                extra['dones'] = torch.zeros(K // D, self.num_envs, dtype=torch.bool, device=self.device)
            if record_transitions:
                extra['policy_obs'] = torch.zeros(K // D, self.num_envs, policy.in_dim, **f32)
                extra['policy_means'] = torch.zeros(K // D, self.num_envs, 12, **f32)
            g.rewards, g.dones = ptr(extra.get('rewards')), ptr(extra.get('dones'))
            g.policy_obs, g.policy_means = ptr(extra.get('policy_obs')), ptr(extra.get('policy_means'))
        if recurrent and record_transitions:
            extra['policy_hidden'] = torch.zeros(K // D, self.num_envs, policy.hidden, **f32)
            gr.hidden_seq = extra['policy_hidden'].data_ptr()
        if obs_noise is not None:
            from .policy import ObsNoise
            if not isinstance(obs_noise, ObsNoise):
                raise ValueError(f'obs_noise must be an ObsNoise, got {type(obs_noise).__name__}')
            if record_transitions:
                extra['policy_obs_clean'] = torch.zeros(K // D, self.num_envs, policy.in_dim, **f32)
            nz = obs_noise._struct(policy, self.device, extra.get('policy_obs_clean'))
        self._hm_fresh = False
        args = (self._hbatch, K, C.byref(m), int(policy_waves), int(step_waves), float(timeout_s), self._st, self._out, self._auto_cfg, self._episode.data_ptr(),
                self._lift_failed.data_ptr(), ptr(obs_seq), ptr(act_seq))
        if obs_noise is not None:   # one entry point: the network, the modes, the scan and the history selected by the blocks given
            gf = reward.feet._struct(self._feet_air.data_ptr()) if learning and reward is not None and reward.feet_on else None
            _lib.check(self._L.gq_rollout_policy_noise(*args[:3], C.byref(gr) if recurrent else None, None if scan is None else C.byref(sc),
                                                       None if hist is None else C.byref(hs), C.byref(nz), *args[3:], C.byref(g) if learning else None,
                                                       None if gf is None else C.byref(gf), stream), 'gq_rollout_policy_noise')
        elif hist is not None:   # one entry point: the modes and the scan selected by the blocks given
            gf = reward.feet._struct(self._feet_air.data_ptr()) if learning and reward is not None and reward.feet_on else None
            _lib.check(self._L.gq_rollout_policy_hist(*args[:3], None if scan is None else C.byref(sc), C.byref(hs), *args[3:], C.byref(g) if learning else None,
                                                      None if gf is None else C.byref(gf), stream), 'gq_rollout_policy_hist')
        elif scan is not None:   # one entry point: the network, the modes and the scan selected by the blocks given
            gf = reward.feet._struct(self._feet_air.data_ptr()) if learning and reward is not None and reward.feet_on else None
            _lib.check(self._L.gq_rollout_policy_scan(*args[:3], C.byref(gr) if recurrent else None, C.byref(sc), *args[3:], C.byref(g) if learning else None,
                                                      None if gf is None else C.byref(gf), stream), 'gq_rollout_policy_scan')
        elif recurrent:   # one entry point, the modes selected by the blocks given
            gf = reward.feet._struct(self._feet_air.data_ptr()) if learning and reward is not None and reward.feet_on else None
            _lib.check(self._L.gq_rollout_policy_gru(*args[:3], C.byref(gr), *args[3:], C.byref(g) if learning else None, None if gf is None else C.byref(gf), stream),
                       'gq_rollout_policy_gru')
        elif learning and reward is not None and reward.feet_on:
            gf = reward.feet._struct(self._feet_air.data_ptr())
            _lib.check(self._L.gq_rollout_policy_learn_feet(*args, C.byref(g), C.byref(gf), stream), 'gq_rollout_policy_learn_feet')
        elif learning:
            _lib.check(self._L.gq_rollout_policy_learn(*args, C.byref(g), stream), 'gq_rollout_policy_learn')
        else:
            _lib.check(self._L.gq_rollout_policy(*args, stream), 'gq_rollout_policy')
        if scan is not None and K > 0:   # every env's last step cast its rays: the map holds those of the state the call leaves, as after step()
            self._hm_fresh, self._hm_version = True, self._qpos._version
        self._launches += K
        if check:
            self.closed_loop_status()
        for sensor in self.sensors:
            for _ in range(K):
                sensor.step()
        return {'obs': self._obs_views, 'obs_seq': obs_seq, 'actions': act_seq, 'policy_actions': pol_seq, **extra}

    def reward_eval(self, spec, rows, torques=None, actions=None, prev_actions=None, terminated=None, feet_air=None):
        """The reward law of ``spec`` (a ``RewardSpec``) alone over ``n`` given steps (``gq_reward_eval``): rows ``[n, obs_dim]`` in this env's
        observation layout (e.g. ``env._obs_buf`` after a step), torques / actions / prev_actions ``[n, 12]`` (None where no weighted
        term reads them), terminated ``[n]`` bool or uint8 (None: all False); float32 tensors on the env's device -> ``[n]`` float32.
        The same routine, hence the same bits, as inside ``rollout_policy(reward=spec)``.

        ``feet_air``: ``[n, 4]`` float32, the feet's air times BEFORE each row's step (``gq_reward_eval_feet``); when given, the result is
        ``(reward, feet_air_next)``.  A spec whose ``air_time`` term is on needs it; a spec without foot terms ignores the state (it is
        returned unchanged)."""
        from .reward import RewardSpec
        if not isinstance(spec, RewardSpec):
            raise ValueError(f'spec must be a RewardSpec, got {type(spec).__name__}')
        if not torch.is_tensor(rows) or rows.dtype != torch.float32 or rows.device != self.device or rows.dim() != 2 or rows.shape[1] != self._obs_dim:
            raise ValueError(f'rows must be a float32 tensor of shape (n, {self._obs_dim}) on {self.device}')
        n = int(rows.shape[0])
        rows = rows.contiguous()

        def arg(t, name, dtype, shape):
            if t is None:
                return None
            if not torch.is_tensor(t) or t.device != self.device or tuple(t.shape) != shape:
                raise ValueError(f'{name} must be a tensor of shape {shape} on {self.device}')
            if dtype is torch.uint8 and t.dtype == torch.bool:
                t = t.to(torch.uint8)
            if t.dtype != dtype:
                raise ValueError(f'{name} must be {dtype}, got {t.dtype}')
            return t.contiguous()
        u, a, ap = (arg(t, nm, torch.float32, (n, 12)) for t, nm in ((torques, 'torques'), (actions, 'actions'), (prev_actions, 'prev_actions')))
        term = arg(terminated, 'terminated', torch.uint8, (n,))
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        ptr = lambda t: None if t is None else t.data_ptr()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        g = spec._struct()
        air = arg(feet_air, 'feet_air', torch.float32, (n, 4))
        if spec.feet_on:
            if spec.feet.air_time != 0.0 and air is None:
                raise ValueError('the air_time term is on: feet_air ([n, 4], the air times before each step) is needed')
            air_next = None if air is None else air.clone()   # (with air_time off the state passes through)
            gf = spec.feet._struct()
            _lib.check(self._L.gq_reward_eval_feet(self._hbatch, C.byref(g), C.byref(gf), rows.data_ptr(), ptr(u), ptr(a), ptr(ap), ptr(term), ptr(air), n,
                                                   out.data_ptr(), ptr(air_next), stream), 'gq_reward_eval_feet')
            return out if air is None else (out, air_next)
        _lib.check(self._L.gq_reward_eval(self._hbatch, C.byref(g), rows.data_ptr(), ptr(u), ptr(a), ptr(ap), ptr(term), n, out.data_ptr(), stream), 'gq_reward_eval')
        return out if air is None else (out, air.clone())

    def _scan_map(self, scan):
        """the env's ``HeightMap(follow_base=True)`` for ``scan`` (a ``policy.HeightScan``): there, and of the scan's grid"""
        hm = self._hm_follow() if self._hm_follow is not None else None
        if hm is None:
            raise ValueError('a height scan reads the env\'s base-following height map: build HeightMap(rows, cols, dist_x, dist_y, env.mjModel, env, '
                             'follow_base=True) first (scenes with world boxes or a height field)')
        if (hm.num_rows, hm.num_cols) != (scan.rows, scan.cols):
            raise ValueError(f'the height scan is {scan.rows} x {scan.cols}, the env\'s base-following height map {hm.num_rows} x {hm.num_cols}')
        return hm

    def height_scan(self, spec, hits=None, z=None):
        """The scan law of ``spec`` (a ``policy.HeightScan``) alone (``gq_height_scan_eval``; the same routine, hence the same bits, as inside
        ``rollout_policy``): hits ``[n, rows, cols, 1, 3]`` or ``[n, rows * cols, 3]`` float32 hit points, z ``[n]`` float32, the base's z of
        each row -> ``[n, rows * cols]`` float32.  Defaults: the env's ``HeightMap(follow_base=True)``, brought up to date, and the base's z
        of the current observation row (``base_pos`` or ``qpos`` must be observed) - what a rollout started now feeds at its first policy
        step.  For a critic's input, or a torch-side loop."""
        from .policy import HeightScan
        if not isinstance(spec, HeightScan):
            raise ValueError(f'spec must be a HeightScan, got {type(spec).__name__}')
        if hits is None:
            hits = self._scan_map(spec).update_height_map()
        if not torch.is_tensor(hits) or hits.dtype != torch.float32 or hits.device != self.device or hits.dim() < 2 or hits.shape[-1] != 3 or \
                hits.numel() != hits.shape[0] * spec.cells * 3:
            raise ValueError(f'hits must be a float32 tensor of shape (n, {spec.rows}, {spec.cols}, 1, 3) or (n, {spec.cells}, 3) on {self.device}')
        n = int(hits.shape[0])
        if z is None:
            if n != self.num_envs:
                raise ValueError(f'z defaults to the env\'s own rows: hits must have {self.num_envs} rows, got {n}')
            views = {**self._extra_views, **self._obs_views}   # the library looks through the whole row: base_pos first, then qpos
            view = views.get('base_pos', views.get('qpos'))
            if view is None:
                raise ValueError('the height scan reads the base\'s z from base_pos (or qpos): not in the env\'s observation row')
            z = view[:, 2]
        if not torch.is_tensor(z) or z.dtype != torch.float32 or z.device != self.device or tuple(z.shape) != (n,):
            raise ValueError(f'z must be a float32 tensor of shape ({n},) on {self.device}')
        hits, z = hits.contiguous(), z.contiguous()
        out = torch.empty(n, spec.cells, dtype=torch.float32, device=self.device)
        sc = spec._struct()
        _lib.check(self._L.gq_height_scan_eval(self._hbatch, C.byref(sc), hits.data_ptr(), z.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream),
                   'gq_height_scan_eval')
        return out

    def obs_noise_eval(self, policy, obs_noise, rows, steps, env_ids):
        """The sensor noise's law alone (``gq_obs_noise_eval``; the same routine, hence the same bits, as inside
        ``rollout_policy(obs_noise=)``): rows ``[n, policy.in_dim]`` float32 raw input rows in 'policy_obs' layout, steps ``[n]`` int - each
        row's absolute step counter, the env's launch counter at the call plus the step ``k`` of the policy step - env_ids ``[n]`` int,
        global env ids -> the rows with the noise added where the law adds it, under this env's seed.  For a torch-side loop, or to rebuild
        'policy_obs' from 'policy_obs_clean'."""
        from .policy import GruPolicy, MlpPolicy, ObsNoise
        if not isinstance(policy, (MlpPolicy, GruPolicy)):
            raise ValueError(f'policy must be an MlpPolicy or a GruPolicy, got {type(policy).__name__}')
        if not isinstance(obs_noise, ObsNoise):
            raise ValueError(f'obs_noise must be an ObsNoise, got {type(obs_noise).__name__}')
        if not torch.is_tensor(rows) or rows.dtype != torch.float32 or rows.device != self.device or rows.dim() != 2 or rows.shape[1] != policy.in_dim:
            raise ValueError(f'rows must be a float32 tensor of shape (n, {policy.in_dim}) on {self.device}')
        n = int(rows.shape[0])
        key = lambda v, name: torch.as_tensor(v, device=self.device).to(torch.int32).reshape(-1).contiguous()
        steps, env_ids = key(steps, 'steps'), key(env_ids, 'env_ids')
        if steps.numel() != n or env_ids.numel() != n:
            raise ValueError(f'steps and env_ids must have one entry per row ({n}), got {steps.numel()} and {env_ids.numel()}')
        rows = rows.contiguous()
        out = torch.empty_like(rows)
        nz = obs_noise._struct(policy, self.device)
        scan = getattr(policy, 'height_scan', None)
        _lib.check(self._L.gq_obs_noise_eval(self._hbatch, C.byref(nz), int(policy.in_obs), 0 if scan is None else scan.cells, int(policy.in_dim),
                                             int(self._seed or 0) & (2 ** 64 - 1), rows.data_ptr(), steps.data_ptr(), env_ids.data_ptr(), n, out.data_ptr(),
                                             torch.cuda.current_stream(self.device).cuda_stream), 'gq_obs_noise_eval')
        return out

    def policy_eval(self, policy, rows, impl: str = 'tile', hidden=None):
        """The network of ``policy`` alone over ``rows`` (``[n, policy.in_dim]`` float32 on the env's device; shift / scale applied to
        the first ``in_obs`` columns; no noise, no clip, no control law) -> ``[n, 12]``.  impl 'tile': the matrix-core form the rollout
        runs, a wavefront per 16 rows; 'scalar': the plain ``fmaf`` loop that defines the law, a thread per row.  Both give the same
        bits (``gq_policy_mlp_eval``).

        A ``GruPolicy`` needs ``hidden`` (``[n, H]`` float32, the states the rows are evaluated from) and returns ``(actions, hidden_next)``
        (``gq_policy_gru_eval``); ``env.policy_hidden`` is neither read nor written."""
        from .policy import GruPolicy
        if impl not in ('tile', 'scalar'):
            raise ValueError("impl must be 'tile' or 'scalar'")
        m = self._policy_struct(policy, rollout=False)
        if not torch.is_tensor(rows) or rows.dtype != torch.float32 or rows.device != self.device or rows.dim() != 2 or rows.shape[1] != policy.in_dim:
            raise ValueError(f'rows must be a float32 tensor of shape (n, {policy.in_dim}) on {self.device}')
        rows = rows.contiguous()
        out = torch.empty(rows.shape[0], 12, dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if isinstance(policy, GruPolicy):
            n, H = int(rows.shape[0]), policy.hidden
            if not torch.is_tensor(hidden) or hidden.dtype != torch.float32 or hidden.device != self.device or tuple(hidden.shape) != (n, H):
                raise ValueError(f'hidden must be a float32 tensor of shape ({n}, {H}) on {self.device}')
            hidden = hidden.contiguous()
            h_next = torch.empty(n, H, dtype=torch.float32, device=self.device)
            m, gr = m
            _lib.check(self._L.gq_policy_gru_eval(self._hbatch, C.byref(m), C.byref(gr), rows.data_ptr(), hidden.data_ptr(), n, int(impl == 'tile'), out.data_ptr(),
                                                  h_next.data_ptr(), stream), 'gq_policy_gru_eval')
            return out, h_next
        if hidden is not None:
            raise ValueError('hidden is the state of a GruPolicy: an MlpPolicy has none')
        _lib.check(self._L.gq_policy_mlp_eval(self._hbatch, C.byref(m), rows.data_ptr(), int(rows.shape[0]), int(impl == 'tile'), out.data_ptr(), stream),
                   'gq_policy_mlp_eval')
        return out

    def step_pd(self, q_des, kp, kd, qd_des=None, tau_ff=None, decimation: int = 4, record_obs: bool = False, record_actions: bool = False):
        """Joint-impedance action held over a decimation window, in one launch (``gq_step_joint_cmd``): ``decimation`` physics steps
        of every env under ``tau = kp * (q_des - q) + kd * (qd_des - qd) + tau_ff``, the law evaluated at every substep from the
        env's fresh joint state with the same command (zero-order hold) - what a robot's low-level interface does with a policy's
        50-100 Hz joint targets.  Equivalent, bit for bit, to ::

            for _ in range(decimation):
                tau = kp * (q_des - env.qpos[:, 7:].float()) + kd * (qd_des - env.qvel[:, 6:]) + tau_ff
                obs, reward, term, trunc, info = env.step(tau)

        without the launch boundaries and the torch kernels in between; every env follows its own command row, and the law reads the
        state, not the observation row (any ``state_obs_names`` works).

        q_des, qd_des, tau_ff: ``[N, 12]`` float32 tensors on the env's device (hinge order of ``qpos[7:]``); the optional two default
        to zero.  kp, kd: a scalar, 12 values, or ``[N, 12]`` (host values are uploaded when they change; a tensor on the env's device is
        used there, without a synchronisation).  Returns ``(obs, reward, terminated, truncated, info)`` like ``step``,
        with ``terminated`` the OR over the window (a buffer of its own: an env that fell and re-spawned inside the window is not
        missed; ``env._terminated`` keeps the last substep's flag); ``truncated``, ``reward`` and the observation are the last
        substep's.  ``info`` also carries 'obs_seq' ``[decimation, N, obs_dim]`` / 'actions' ``[decimation, N, 12]`` when asked for.
        ``torque_ctrl_setpoint`` is the last substep's torque.  Needs the Newton solver and ``auto_reset='next_step'`` (or none)."""
        from .cabi import GqJointCmd
        N, nu = self.num_envs, 12
        D = self._window_checks('step_pd', decimation)
        q = self._cmd_rows(q_des, 'q_des')
        if q is None:
            raise ValueError('q_des must be given')
        qd, ff = self._cmd_rows(qd_des, 'qd_des'), self._cmd_rows(tau_ff, 'tau_ff')
        p, d, sp = self._cmd_gains(self._cmd_gain(kp, 'kp', 0), self._cmd_gain(kd, 'kd', 1))
        obs_seq, act_seq = self._window_records(D, record_obs, record_actions)
        cmd = GqJointCmd(struct_size=C.sizeof(GqJointCmd), gain_stride=sp, q_des=q.data_ptr(), qd_des=None if qd is None else qd.data_ptr(),
                         tau_ff=None if ff is None else ff.data_ptr(), kp=p.data_ptr(), kd=d.data_ptr(), tau_out=self._pd_tau.data_ptr(),
                         terminated_any=self._pd_term_any.data_ptr())
        self._pd_cmd_refs = (q, qd, ff, p, d)   # the launch reads them asynchronously
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._hm_fresh = False
        _lib.check(self._L.gq_step_joint_cmd(self._hbatch, C.byref(cmd), D, self._st, self._out, self._auto_cfg, self._episode.data_ptr(),
                                             self._lift_failed.data_ptr(), None if obs_seq is None else obs_seq.data_ptr(),
                                             None if act_seq is None else act_seq.data_ptr(), stream), 'gq_step_joint_cmd')
        return self._window_done(D, obs_seq, act_seq)

    # -- what step_pd and step_feet share: the checks in front of a command window, its command rows and gains, its results
    def _window_checks(self, who, decimation):
        D = int(decimation)
        if D < 1:
            raise ValueError(f'decimation must be >= 1, got {decimation}')
        if self._mm.desc.solver != 1:
            raise ValueError(f"{who} needs the Newton solver (solver='newton')")
        if self.auto_reset and self.auto_reset_mode != 'next_step':
            raise ValueError(f"{who} needs auto_reset='next_step' (or no auto-reset): a same-step re-spawn does not fit the persistent kernel")
        if getattr(self, '_pd_tau', None) is None:
            N, nu = self.num_envs, 12
            self._pd_gain = torch.zeros(4, nu, dtype=torch.float32, device=self.device)   # rows 0, 1: step_pd's kp, kd; 2, 3: step_feet's
            self._pd_gain_host = [None] * 4
            self._pd_tau = torch.zeros(N, nu, dtype=torch.float32, device=self.device)
            self._pd_term_any = torch.zeros(N, dtype=torch.uint8, device=self.device)
            self._pd_term_any_b = self._pd_term_any.view(torch.bool)
        return D

    def _cmd_rows(self, x, name):
        N, nu = self.num_envs, 12
        if x is None:
            return None
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.device != self.device or tuple(x.shape) != (N, nu):
            raise ValueError(f'{name} must be a float32 tensor of shape ({N}, {nu}) on {self.device}, got '
                             + (f'{x.dtype} {tuple(x.shape)} on {x.device}' if torch.is_tensor(x) else type(x).__name__))
        return x.contiguous()

    def _cmd_gain(self, x, name, k, sizes=(1, 12), spread=None):
        """a gain as (tensor, stride): an ``[N, 12]`` tensor as it is (stride 12), anything smaller as the shared row k of
        ``_pd_gain`` (stride 0).  sizes: the accepted lengths of a shared gain; spread(v): a vector of such a length -> 12 values"""
        if torch.is_tensor(x) and x.dim() == 2:   # (the per-env form first: nothing else is done for it)
            return self._cmd_rows(x, name), 12
        N, nu = self.num_envs, 12

        def bad(shape):
            what = ', '.join(['a scalar'] + [f'{n} values' for n in sizes[1:]])
            return ValueError(f'{name} must be {what} or a ({N}, {nu}) tensor, got shape {tuple(shape)}')
        if torch.is_tensor(x) and x.device == self.device:   # a device tensor stays there: a copy on the stream, no host round trip
            if x.dim() > 1 or x.numel() not in sizes:
                raise bad(x.shape)
            v = x.detach().to(torch.float32).reshape(-1)
            self._pd_gain[k].copy_(spread(v) if spread else v.expand(nu))
            self._pd_gain_host[k] = None
            return self._pd_gain[k], 0
        v = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.float32)
        if v.ndim > 1 or v.size not in sizes:
            raise bad(v.shape)
        v = v.reshape(-1)
        v = np.ascontiguousarray(spread(v) if spread else np.broadcast_to(v, (nu,)), dtype=np.float32).copy()
        if self._pd_gain_host[k] is None or not np.array_equal(self._pd_gain_host[k], v):   # the shared row is uploaded when it changes
            self._pd_gain[k].copy_(torch.from_numpy(v))
            self._pd_gain_host[k] = v
        return self._pd_gain[k], 0

    def _cmd_gains(self, kp, kd):
        (p, sp), (d, sd) = kp, kd
        if sp != sd:   # one stride serves both rows: the shared one is spread
            N, nu = self.num_envs, 12
            p = p if sp == 12 else p.expand(N, nu).contiguous()
            d = d if sd == 12 else d.expand(N, nu).contiguous()
            sp = 12
        return p, d, sp

    def _window_records(self, D, record_obs, record_actions):
        f32 = dict(dtype=torch.float32, device=self.device)
        return (torch.empty(D, self.num_envs, self._obs_dim, **f32) if record_obs else None,
                torch.empty(D, self.num_envs, 12, **f32) if record_actions else None)

    def _window_done(self, D, obs_seq, act_seq):
        self._last_action = self._pd_tau
        self._launches += D
        self._note_step()
        for sensor in self.sensors:
            for _ in range(D):
                sensor.step()
        info = dict(self._info)
        if obs_seq is not None:
            info['obs_seq'] = obs_seq
        if act_seq is not None:
            info['actions'] = act_seq
        return self._obs_views, self._reward, self._pd_term_any_b, self._truncated_b, info

    def step_feet(self, p_des, kp, kd, v_des=None, f_ff=None, tau_ff=None, frame: str = 'base', decimation: int = 4, record_obs: bool = False,
                  record_actions: bool = False):
        """Foot-space action held over a decimation window, in one launch (``gq_step_foot_cmd``): ``decimation`` physics steps of
        every env under, per foot, ::

            F = f_ff + kp * (p_des - p) + kd * (v_des - v)          # virtual force on the foot, 3-vector
            tau_leg = J^T F + tau_ff

        with ``p`` the foot's position relative to the base origin, ``J`` the 3x3 Jacobian of that position in the leg's three joint
        angles and ``v = J qd_leg`` (the foot's velocity relative to the base), all evaluated at every substep from the env's fresh
        state with the same command - the inner loop of a force / whole-body controller between two solver updates, for which ``D`` x
        (``feet_jacobians``, einsum, ``step``) is the alternative.  frame: 'base' (base axes) or 'world' (world AXES; the origin stays
        at the base).  A stance leg that should receive ground reaction ``g`` is commanded ``f_ff = -g`` with zero gains; a swing leg
        gets gains and ``p_des`` / ``v_des``.  Only ``J^T`` is used: no pose is singular.

        p_des, v_des, f_ff: ``[N, 12]`` float32 tensors on the env's device, the feet concatenated in the env's ``legs_order`` (like the
        ``feet_pos`` observable), or a ``LegsAttr`` of ``[N, 3]`` tensors; the optional ones default to zero.  tau_ff: ``[N, 12]`` in hinge
        order (``qpos[7:]``).  kp, kd: a scalar, 3 values (per axis), 12 values (per foot and axis, ``legs_order``) or ``[N, 12]``.
        Everything else - the return value with ``terminated`` the OR over the window, ``info['obs_seq']`` / ``info['actions']`` (the
        torques of every substep), ``torque_ctrl_setpoint``, the requirements - is ``step_pd``'s.  The law reads the state, not the
        observation row: any ``state_obs_names`` works, ``accessors=True`` is not needed."""
        from .cabi import LEG_NAMES, GqFootCmd
        N = self.num_envs
        D = self._window_checks('step_feet', decimation)
        if frame not in ('base', 'world'):
            raise ValueError(f"frame must be 'base' or 'world', got {frame!r}")
        inv = [self.legs_order.index(leg) for leg in LEG_NAMES]   # canonical foot k sits at place inv[k] of the caller's rows
        permuted = inv != [0, 1, 2, 3]

        def feet(x, name):
            if isinstance(x, LegsAttr):
                legs = x.to_list(order=LEG_NAMES)
                if not all(torch.is_tensor(t) and t.dtype == torch.float32 and t.device == self.device and tuple(t.shape) == (N, 3) for t in legs):
                    raise ValueError(f'{name}: every leg of a LegsAttr must be a float32 tensor of shape ({N}, 3) on {self.device}')
                return torch.cat(legs, dim=1)
            x = self._cmd_rows(x, name)
            return x.view(N, 4, 3)[:, inv].reshape(N, 12) if permuted and x is not None else x

        def spread(v):   # a shared gain: 1, 3 (per axis) or 12 (per foot and axis, legs_order) values -> 12 in canonical order
            rep = (lambda t, n: t.repeat(n)) if torch.is_tensor(v) else (lambda t, n: np.tile(t, n))
            v = rep(v, 12 // len(v))
            return v.reshape(4, 3)[inv].reshape(12) if permuted else v

        def gain(x, name, k):
            g, stride = self._cmd_gain(x, name, k, sizes=(1, 3, 12), spread=spread)
            return (g.view(N, 4, 3)[:, inv].reshape(N, 12) if permuted and stride == 12 else g), stride

        p = feet(p_des, 'p_des')
        if p is None:
            raise ValueError('p_des must be given')
        v, f, ff = feet(v_des, 'v_des'), feet(f_ff, 'f_ff'), self._cmd_rows(tau_ff, 'tau_ff')
        gp, gd, stride = self._cmd_gains(gain(kp, 'kp', 2), gain(kd, 'kd', 3))
        obs_seq, act_seq = self._window_records(D, record_obs, record_actions)
        ptr = lambda t: None if t is None else t.data_ptr()
        cmd = GqFootCmd(struct_size=C.sizeof(GqFootCmd), gain_stride=stride, frame=int(frame == 'world'), p_des=p.data_ptr(), v_des=ptr(v), f_ff=ptr(f),
                        tau_ff=ptr(ff), kp=gp.data_ptr(), kd=gd.data_ptr(), tau_out=self._pd_tau.data_ptr(), terminated_any=self._pd_term_any.data_ptr())
        self._pd_cmd_refs = (p, v, f, ff, gp, gd)   # the launch reads them asynchronously
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._hm_fresh = False
        _lib.check(self._L.gq_step_foot_cmd(self._hbatch, C.byref(cmd), D, self._st, self._out, self._auto_cfg, self._episode.data_ptr(),
                                            self._lift_failed.data_ptr(), ptr(obs_seq), ptr(act_seq), stream), 'gq_step_foot_cmd')
        return self._window_done(D, obs_seq, act_seq)

    def closed_loop_status(self):
        """Wait for the last ``rollout_closed_loop`` / ``rollout_policy`` and return (abort code, detail, env-steps played); the code
        is 0 for a rollout that ran to its end.  Raises ``GqError`` if it was aborted, with the code in the message - the values of
        ``cabi.GQ_CLOSED_ABORT``: ``step_deadline`` (a step wavefront waited past the deadline for an action; detail = its ticket),
        ``policy_deadline`` (a policy wait passed the deadline: missing / stuck policy; detail = the policy lane), ``policy_absent``
        (the policy kernel could not become resident), ``xcd_no_policy`` (an XCD got no policy wavefront; detail = its queue)."""
        st = (C.c_int32 * 4)()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._L.gq_rollout_closed_status(self._hbatch, st, stream), 'gq_rollout_closed')
        return int(st[0]), int(st[1]), int(st[2])

    def reset(self, qpos=None, qvel=None, seed: int | None = None, random: bool = True,
              options: dict[str, Any] | None = None, env_ids=None):
        """Reset (reference ``reset`` :309-406); ``env_ids`` (index tensor / bool mask) restricts it to a subset.
        Returns the observation dict only, like the reference (quirk B7)."""
        if seed is not None:  # reference: np.random.seed(seed) (:338-339); here: re-key the device generators
            self._gen.manual_seed(int(seed))
            self._seed = int(seed)
            self._reset_cfg.seed = self._seed
            self._auto_cfg_struct.seed = self._seed
            self._episode.zero_()
            if getattr(self, '_resample_cfg', None) is not None:
                self._resample_cfg.seed = self._seed
                self._h9[:, 2] = 0; self._h9[:, 5] = 0
                _lib.check(self._L.gq_batch_set_resampling(self._hbatch, C.byref(self._resample_cfg), C.byref(self._reset_cfg),
                                                           self._h9.data_ptr(), self._ext_dist.data_ptr()), 'gq_batch_set_resampling')
        N = self.num_envs
        if env_ids is None:
            mask = self._mask_all
        else:
            idx = torch.as_tensor(env_ids, device=self.device)
            if idx.dtype == torch.bool:
                mask = idx.to(torch.uint8)
            else:
                mask = torch.zeros(N, dtype=torch.uint8, device=self.device)
                mask[idx.long()] = 1
        if qpos is None and qvel is None:
            self._reset_masked(mask, random=random, options=options)
        else:
            qp = torch.as_tensor(qpos, dtype=torch.float64, device=self.device).reshape(-1, 19).expand(N, 19).contiguous()
            qv = torch.as_tensor(qvel, dtype=torch.float32, device=self.device).reshape(-1, 18).expand(N, 18).contiguous()
            self._reset_masked(mask, random=False, options=options, qpos=qp, qvel=qv)
        return self._obs_views

    def _reset_masked(self, mask, random, options, qpos=None, qvel=None):
        """One ``gq_reset`` call = state write (+ lift loop) and the reset's own ``mj_step`` for the masked envs."""
        options = {} if options is None else options
        self._hm_fresh = False
        cfg = self._reset_cfg
        cfg.random = int(bool(random))
        cfg.q_pos_amp = float(options.get('angle_sweep', 20 * math.pi / 180))
        cfg.roll_sweep = float(options.get('roll_sweep', 10 * math.pi / 180))
        cfg.pitch_sweep = float(options.get('pitch_sweep', 10 * math.pi / 180))
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._L.gq_reset(self._hbatch, mask.data_ptr(), None if qpos is None else qpos.data_ptr(),
                                    None if qvel is None else qvel.data_ptr(), C.byref(cfg), self._st, self._out,
                                    self._episode.data_ptr(), self._lift_failed.data_ptr(), stream), 'gq_reset')
        self._launches += 1
        self._note_step()
        self._feet_air.masked_fill_(mask.bool().unsqueeze(1), 0.0)   # a new episode starts with no air time behind it
        if self._policy_hidden is not None:
            self._policy_hidden.masked_fill_(mask.bool().unsqueeze(1), 0.0)   # ... and with no memory
        if self._policy_hist is not None:
            self._policy_hist[1].masked_fill_(mask.bool(), 0)                 # ... of either kind: a control word without VALID is an empty history
        if mask is self._mask_all:  # the reference zeroes mjData.ctrl in reset (:334): torque_ctrl_setpoint reads zero afterwards
            self._ctrl.zero_()
            self._last_action = self._ctrl

    # ------------------------------------------------------------------ command / disturbance sampling
    def _sample_ref_vel(self, mask):
        """Per-env redraw of the velocity command for envs in ``mask`` (reference ``_sample_ref_vel`` :1046-1072)."""
        N, dev, g = self.num_envs, self.device, self._gen
        t = self.base_vel_command_type
        lo, hi = self.base_lin_vel_range
        if 'forward' in t:
            norm = lo + (hi - lo) * torch.rand(N, generator=g, device=dev)
            heading = torch.zeros(N, device=dev)
        elif 'random' in t:
            norm = lo + (hi - lo) * torch.rand(N, generator=g, device=dev)
            heading = (torch.rand(N, generator=g, device=dev) * 2 - 1) * math.pi
        elif 'human' in t:
            norm = torch.zeros(N, device=dev)
            heading = torch.zeros(N, device=dev)
        else:
            raise ValueError(f'Invalid base linear velocity command type: {t}')
        if 'rotate' in t:
            alo, ahi = self.base_ang_vel_range
            yaw_dot = alo + (ahi - alo) * torch.rand(N, generator=g, device=dev)
        else:
            yaw_dot = torch.zeros(N, device=dev)
        new = torch.stack([norm * torch.cos(heading), norm * torch.sin(heading), torch.zeros(N, device=dev), yaw_dot], 1)
        self._cmd.copy_(torch.where(mask.unsqueeze(1), new, self._cmd))
        if 'reset' in t:
            nxt = torch.randint(1000, 3000, (N,), generator=g, device=dev, dtype=torch.int32)
            self._h9[:, 1] = torch.where(mask, nxt, self._h9[:, 1])
            self._h9[:, 0] = torch.where(mask, torch.zeros_like(nxt), self._h9[:, 0])
        self._has_cmd = True

    def _sample_external_disturbances(self, mask):
        """Per-env redraw of the base wrench (reference ``_sample_external_disturbances`` :1074-1139)."""
        N, dev, g = self.num_envs, self.device, self._gen
        kw = self.external_disturbances_kwargs
        cols = []
        for key in ('x', 'y', 'z', 'roll', 'pitch', 'yaw'):
            r = kw.get(key)
            if r is None or len(r) == 0:
                cols.append(torch.zeros(N, device=dev))
            elif len(r) == 1:
                cols.append(torch.full((N,), float(r[0]), device=dev))
            else:
                cols.append(float(r[0]) + (float(r[1]) - float(r[0])) * torch.rand(N, generator=g, device=dev))
        new = torch.stack(cols, 1)
        self._ext_dist.copy_(torch.where(mask.unsqueeze(1), new, self._ext_dist))   # in place: the kernel holds the pointer
        nxt = torch.randint(1000, 3000, (N,), generator=g, device=dev, dtype=torch.int32)
        self._h9[:, 4] = torch.where(mask, nxt, self._h9[:, 4])
        self._h9[:, 3] = torch.where(mask, torch.zeros_like(nxt), self._h9[:, 3])

    # ------------------------------------------------------------------ accessors (reference names)
    @property
    def qpos(self):
        return self._qpos

    @property
    def qvel(self):
        return self._qvel

    @property
    def base_pos(self):
        return self._qpos[:, 0:3]

    @property
    def joint_space_state(self):
        return self._qpos[:, 7:], self._qvel[:, 6:]

    @property
    def torque_ctrl_setpoint(self):
        return self._last_action

    @property
    def simulation_dt(self):
        return self._sim_dt

    @property
    def simulation_time(self):
        return self._time

    @property
    def step_num(self):
        return self._step_num

    @property
    def robot_model(self):
        return self.mjModel

    @property
    def sim_data(self):
        """What the reference's sensors take as ``mj_data`` (reference :1034 returns the MjData): here the batched env itself."""
        return self

    @property
    def lift_failed(self):
        """Per-env flag of the reset RuntimeError condition (reference :387-388)."""
        return self._lift_failed.view(torch.bool)

    @property
    def feet_air_time(self):
        """``[N, 4]`` float32, FL FR RL RR: how long each foot has been in the air, the state of the reward's ``air_time`` term
        (``FootRewardSpec``).  ``rollout_policy(reward=spec)`` with that term on reads and advances it at every physics step, and zeroes
        an env's row at its re-spawn step; ``reset`` zeroes the rows of the envs it resets.  Assigning copies into the same tensor."""
        return self._feet_air

    @feet_air_time.setter
    def feet_air_time(self, value):
        self._feet_air.copy_(torch.as_tensor(value, dtype=torch.float32, device=self.device).reshape(self.num_envs, 4))

    @property
    def policy_hidden(self):
        """``[N, H]`` float32: the hidden state of the ``GruPolicy`` that ``rollout_policy`` runs, or None before the first recurrent call
        (which allocates it as zeros for that policy's ``H``).  The rollout reads and writes it; the policy seat zeroes an env's row when it
        sees the env's termination (the episode rule of ``csrc/gq_policy_gru.h``), ``reset`` zeroes the rows of the envs it resets.
        Assigning a ``[N, H']`` tensor replaces it (a policy with another ``H`` is refused until then); ``state_dict`` carries it."""
        return self._policy_hidden

    @policy_hidden.setter
    def policy_hidden(self, value):
        if value is None:
            self._policy_hidden = None
            return
        v = torch.as_tensor(value, dtype=torch.float32, device=self.device)
        if v.dim() != 2 or v.shape[0] != self.num_envs or not 1 <= v.shape[1] <= 128:
            raise ValueError(f'policy_hidden must be [{self.num_envs}, H] with 1 <= H <= 128, got {tuple(v.shape)}')
        if self._policy_hidden is not None and self._policy_hidden.shape == v.shape:
            self._policy_hidden.copy_(v)
        else:
            self._policy_hidden = v.clone().contiguous()

    @property
    def policy_history(self):
        """``[N, L, F]`` float32, newest first: the frames the ``ObsHistory`` of the ``MlpPolicy`` that ``rollout_policy`` runs would be fed
        next, or None before the first such call (which starts every env with an empty - all zero - history for that policy's ``(L, F)``).
        A copy: the rollout keeps two buffers and a control word per env (``csrc/gq_policy_hist.h``), read here into the law's form.  The
        policy seat empties an env's history when it sees the env's termination (the episode rule), ``reset`` empties those of the envs it
        resets.  Assigning a ``[N, L', F']`` tensor replaces it (a policy with another ``(L, F)`` is refused until then); ``state_dict``
        carries it."""
        if self._policy_hist is None:
            return None
        state, ctl = self._policy_hist
        cur = state[torch.arange(self.num_envs, device=self.device), (ctl & 1).long()]
        return torch.where(((ctl >> 1) & 1).bool().view(-1, 1, 1), cur, torch.zeros_like(cur))

    @policy_history.setter
    def policy_history(self, value):
        if value is None:
            self._policy_hist = None
            return
        v = torch.as_tensor(value, dtype=torch.float32, device=self.device)
        if v.dim() != 3 or v.shape[0] != self.num_envs or v.shape[1] < 1 or v.shape[2] < 1 or v.shape[1] * v.shape[2] >= 256:
            raise ValueError(f'policy_history must be [{self.num_envs}, L, F] with L, F >= 1 and L * F < 256, got {tuple(v.shape)}')
        if self._policy_hist is None or self._policy_hist[0].shape[2:] != v.shape[1:]:
            self._policy_hist = (torch.zeros(self.num_envs, 2, v.shape[1], v.shape[2], dtype=torch.float32, device=self.device),
                                 torch.zeros(self.num_envs, dtype=torch.int32, device=self.device))
        state, ctl = self._policy_hist
        state[:, 0].copy_(v)
        ctl.fill_(2)   # parity 0, VALID

    @property
    def ground_friction_coeff_range(self):
        """``(low, high)`` of the ground friction the resets draw from.  Assigning a scalar or a pair applies from the next reset (the
        auto-resets inside ``step`` included); a range whose lower end is under the solver's floor is refused (``check_ground_friction``)."""
        return self._ground_friction_coeff_range

    @ground_friction_coeff_range.setter
    def ground_friction_coeff_range(self, value):
        rng = _process_range(value)
        check_ground_friction(self.mjModel.cone, self._solver, rng[0], self.robot_name)
        self._ground_friction_coeff_range = rng
        for cfg in (self._reset_cfg, self._auto_cfg_struct):
            cfg.friction_range = (C.c_float * 2)(*map(float, rng))

    def target_base_vel(self):
        """Reference command in the heading frame ``[N,3]`` and yaw rate ``[N]`` (reference :488-499 inputs)."""
        return self._cmd[:, 0:3], self._cmd[:, 3]

    def state_dict(self):
        """Checkpoint: everything needed to resume a rollout bit-for-bit."""
        keys = ['_qpos', '_qvel', '_qacc', '_warm', '_applied', '_time', '_friction', '_cmd', '_step_num', '_episode', '_terminated',
                '_h9', '_ext_dist', '_step_num_prev']
        keys += ['_lift_failed', '_feet_air']
        d = {k: getattr(self, k).clone() for k in keys}
        if self._policy_hidden is not None:
            d['_policy_hidden'] = self._policy_hidden.clone()
        if self._policy_hist is not None:
            d['_policy_history'] = self.policy_history
        d['rng'] = self._gen.get_state()
        # sensor state the kernel reads and writes every step: the IMU bias random walks
        d['sensor_bias'] = [sn.bias_state.clone() if hasattr(sn, 'bias_state') else None for sn in self.sensors]
        return d

    _LEGACY_H9 = {'_steps_after_vel': 0, '_steps_before_vel': 1, '_steps_after_dist': 3, '_steps_before_dist': 4}

    def load_state_dict(self, d):
        self._hm_fresh = False
        if '_friction' in d:   # a checkpoint's per-env ground friction (< 0: the XML's, until the first reset) is held to the solver's floor too
            set_mu = torch.as_tensor(d['_friction'])
            set_mu = set_mu[set_mu >= 0]
            if set_mu.numel():
                check_ground_friction(self.mjModel.cone, self._solver, float(set_mu.min()), self.robot_name)
        for k, v in d.items():
            if k in self._LEGACY_H9:  # checkpoints written before the resampling counters moved into one [N, 6] tensor
                self._h9[:, self._LEGACY_H9[k]].copy_(torch.as_tensor(v, device=self.device).to(torch.int32))
                continue
            if k == 'rng':
                self._gen.set_state(v)
            elif k == '_policy_hidden':
                self.policy_hidden = v
            elif k == '_policy_history':
                self.policy_history = v
            elif k == 'sensor_bias':
                for sn, b in zip(self.sensors, v):
                    if b is not None:
                        sn.bias_state.copy_(b)  # in place: the kernel holds this tensor's pointer
            else:
                getattr(self, k).copy_(v)
        if '_terminated' in d:  # next-step auto-reset: the envs that terminated last step are still waiting for their reset
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(self._L.gq_batch_set_pending(self._hbatch, self._terminated.data_ptr(), stream), 'gq_batch_set_pending')

    def debug_internals(self, n_envs: int, names):
        """Copy solver / dynamics internals of the LAST step for the first ``n_envs`` envs (must be enabled before
        the step with ``enable_debug``)."""
        out = []
        for e in range(n_envs):
            rec = {}
            for nm in names:
                buf = np.zeros(64 * 18, dtype=np.float64)
                n = _lib.check(self._L.gq_debug_get(self._hbatch, e, nm.encode(), buf.ctypes.data, buf.size), 'gq_debug_get')
                rec[nm] = buf[:n].copy()
            out.append(rec)
        return out

    def enable_debug(self, n_envs: int):
        _lib.check(self._L.gq_debug_enable(self._hbatch, int(n_envs)), 'gq_debug_enable')

    def render(self, mode: str = 'human', tint_robot: bool = False, ghost_qpos=None, ghost_alpha=0.5, *, width: int = 320, height: int = 240,
               distance: float = 2.0, azimuth: float = 90.0, elevation: float = -45.0, markers=None):
        """``mode='rgb_array'``: ``[N, H, W, 3]`` uint8 on the env's device, one frame per env (a fresh tensor) from a camera that tracks
        the base: it looks along ``f = (cos el cos az, cos el sin az, sin el)`` (degrees, world axes) from ``base - distance f``, world
        up, 45 degree fovy (``sensors.Camera(rgb=True, track=True)``, cached per argument set).  Every other mode raises: an interactive
        viewer is out of scope of the batched GPU path.

        The reference's arguments: ``tint_robot`` recolours the robot's geoms with its palette (``utils.visual.tint_color``: teal body,
        one colour per leg by body name), on the render camera only; ``ghost_qpos`` (``[19]``, ``[G, 19]`` or ``[N, G, 19]``, G <= 8)
        draws translucent copies of the robot in the robot's colours (tinted or not) at ``ghost_alpha`` (a float, ``[G]`` or ``[N, G]``).
        ``markers`` (``utils.visual.Markers`` or ``[N, K, 16]``) adds spheres, lines and arrows; ``utils.visual.velocity_markers(self)``
        gives the reference's velocity arrows, which are not drawn by default."""
        if mode != 'rgb_array':
            raise NotImplementedError(f'render(mode={mode!r}): only mode="rgb_array" is available (an interactive viewer is out of scope '
                                      'of the batched GPU path)')
        key = (int(width), int(height), float(distance), float(azimuth), float(elevation)) + (('tint',) if tint_robot else ())
        cams = self.__dict__.setdefault('_render_cams', {})
        if key not in cams:
            from .mjcf import mat_to_quat
            from .sensors import Appearance, Camera
            az, el = np.deg2rad(azimuth), np.deg2rad(elevation)
            f = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
            right = np.cross(f, [0.0, 0.0, 1.0])
            if np.linalg.norm(right) < 1e-6:
                raise ValueError(f'render: elevation {elevation} looks straight up or down, the world up is undefined')
            right /= np.linalg.norm(right)
            R = np.stack([right, np.cross(right, f), -f], 1)   # columns: camera x (right), y (up), z (backwards)
            app = None
            if tint_robot:
                from .utils.visual import tinted_geom_mat
                app = Appearance.default(self.mjModel)
                app.geom_mat = tinted_geom_mat(self.mjModel, app.geom_mat)
            cams[key] = Camera(width, height, 30, self.robot_model, self.sim_data, body=1, pos=-distance * f, quat=mat_to_quat(R), fovy=45.0,
                               rgb=True, track=True, appearance=app)
        return cams[key].layered_image(ghost_qpos=ghost_qpos, ghost_alpha=ghost_alpha, markers=markers).contiguous()

    def close(self):
        if getattr(self, '_hbatch', None):
            self._L.gq_batch_destroy(self._hbatch)
            self._hbatch = None
        if getattr(self, '_hmodel', None):
            self._L.gq_model_destroy(self._hmodel)
            self._hmodel = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _save_hyperparameters(self, constructor_params):
        self._init_args = constructor_params
        for k in ['self', '__class__']:
            self._init_args.pop(k, None)

    def get_hyperparameters(self):
        """Constructor arguments (reference :1356-1358)."""
        return copy.copy(self._init_args)

    def __str__(self):
        msg = f'robot={self._init_args["robot"]} terrain={self._init_args["scene"]} task={self.base_vel_command_type} num_envs={self.num_envs}'
        if self.base_vel_command_type != 'human':
            msg += (f' lin_vel_range=({self.base_lin_vel_range[0]:.3f}, {self.base_lin_vel_range[1]:.3f})'
                    f' ang_vel_range=({self.base_ang_vel_range[0]:.3f}, {self.base_ang_vel_range[1]:.3f})'
                    f' lat_friction_range=({self.ground_friction_coeff_range[0]:.1e}, {self.ground_friction_coeff_range[1]:.1e})')
        return msg
