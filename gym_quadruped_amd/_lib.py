"""Loader of the HIP extension ``libgq.so`` (C-ABI of include/gq.h).  There is NO fallback: if the library is
missing or cannot be loaded the product path raises - it never routes through the CPU oracle."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

from .cabi import GQ_ABI_VERSION, GqCamLayers, GqCamShade, GqFootCmd, GqFootReward, GqImuCfg, GqJointCmd, GqLearn, GqMailboxView, GqModelDesc, GqObsOut, GqPolicyGru, GqPolicyHist, GqPolicyMlp, GqPolicyNoise, GqPolicyPd, GqPolicyScan, GqResampleCfg, GqResetCfg, GqState

_LIB = None

# GQ_LIBGQ_PATH: developer override used for A/B timing of two kernel builds inside one GPU session
LIB_PATH = Path(os.environ.get('GQ_LIBGQ_PATH', Path(__file__).parent / 'libgq.so'))

# what gq_struct_sizes reports, in its order: lib() refuses a library whose sizes differ from these mirrors
SIZED_STRUCTS = (GqModelDesc, GqState, GqObsOut, GqResetCfg, GqResampleCfg, GqImuCfg, GqPolicyPd, GqMailboxView)

_P, _v, _i, _f, _i32p = C.POINTER, C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_int32)
_LAUNCH = [GqState, GqObsOut, _P(GqResetCfg), _v, _v]   # runs of parameters that recur in include/gq.h: st, out, auto_reset, episode, lift_failed
_SEQ = [_v, _v, _v]                                     # obs_seq, act_seq, hip_stream
_POLICY = [_v, _i, _P(GqPolicyMlp), _i, _i, C.c_double] + _LAUNCH + _SEQ
_LEARN = _POLICY[:-1] + [_P(GqLearn), _v]
# the three camera calls up to cam_xmat: batch, qpos, stride, body, pos, quat, fovy, width, height, znear, zfar, flags, hull planes, images, camera pose
_CAMERA = [_v, _v, _i, _i, _P(C.c_double), _P(C.c_double), _f, _i, _i, _f, _f, _i, _v, _i32p, _v, _v, _v, _v]

# THE binding's view of include/gq.h, in the header's order: name -> (restype, argtypes).  lib() applies it; EXPORTS is its key list.
ABI = {
    'gq_last_error': (C.c_char_p, []),
    'gq_version': (_i, []),
    'gq_struct_sizes': (_i, [_i32p]),
    'gq_obs_dim': (_i, [_i]),
    'gq_model_create': (_i, [_P(GqModelDesc), _i, _P(_v)]),
    'gq_model_destroy': (_i, [_v]),
    'gq_batch_create': (_i, [_v, _i, _v, _i, _v, _P(_v)]),
    'gq_batch_destroy': (_i, [_v]),
    'gq_batch_obs_dim': (_i, [_v]),
    'gq_batch_set_imu': (_i, [_v, _P(GqImuCfg), _v]),
    'gq_batch_set_heightmap': (_i, [_v, _i, _i, _f, _f, _v]),
    'gq_batch_set_pair_exchange': (_i, [_v, _i]),
    'gq_batch_set_resampling': (_i, [_v, _P(GqResampleCfg), _P(GqResetCfg), _v, _v]),
    'gq_step': (_i, [_v, _v, _v] + _LAUNCH + [_v]),
    'gq_step_range': (_i, [_v, _i, _i, _v] + _LAUNCH + [_v]),
    'gq_rollout': (_i, [_v, _v, _i, _i] + _LAUNCH + [_v, _v]),
    'gq_rollout_closed': (_i, [_v, _i, _i, _P(GqPolicyPd), _i, _i, C.c_double] + _LAUNCH + _SEQ),
    'gq_rollout_closed_status': (_i, [_v, _i32p, _v]),
    'gq_mailbox_get': (_i, [_v, _P(GqMailboxView)]),
    'gq_rollout_policy': (_i, _POLICY),
    'gq_policy_mlp_eval': (_i, [_v, _P(GqPolicyMlp), _v, _i, _i, _v, _v]),
    'gq_rollout_policy_learn': (_i, _LEARN),
    'gq_reward_eval': (_i, [_v, _P(GqLearn), _v, _v, _v, _v, _v, _i, _v, _v]),
    'gq_rollout_policy_learn_feet': (_i, _LEARN[:-1] + [_P(GqFootReward), _v]),
    'gq_reward_eval_feet': (_i, [_v, _P(GqLearn), _P(GqFootReward), _v, _v, _v, _v, _v, _v, _i, _v, _v, _v]),
    'gq_rollout_policy_gru': (_i, _POLICY[:3] + [_P(GqPolicyGru)] + _POLICY[3:-1] + [_P(GqLearn), _P(GqFootReward), _v]),
    'gq_policy_gru_eval': (_i, [_v, _P(GqPolicyMlp), _P(GqPolicyGru), _v, _v, _i, _i, _v, _v, _v]),
    'gq_rollout_policy_scan': (_i, _POLICY[:3] + [_P(GqPolicyGru), _P(GqPolicyScan)] + _POLICY[3:-1] + [_P(GqLearn), _P(GqFootReward), _v]),
    'gq_rollout_policy_hist': (_i, _POLICY[:3] + [_P(GqPolicyScan), _P(GqPolicyHist)] + _POLICY[3:-1] + [_P(GqLearn), _P(GqFootReward), _v]),
    'gq_height_scan_eval': (_i, [_v, _P(GqPolicyScan), _v, _v, _i, _v, _v]),
    'gq_rollout_policy_noise': (_i, _POLICY[:3] + [_P(GqPolicyGru), _P(GqPolicyScan), _P(GqPolicyHist), _P(GqPolicyNoise)] + _POLICY[3:-1] + [_P(GqLearn), _P(GqFootReward), _v]),
    'gq_obs_noise_eval': (_i, [_v, _P(GqPolicyNoise), _i, _i, _i, C.c_uint64, _v, _v, _v, _i, _v, _v]),
    'gq_step_joint_cmd': (_i, [_v, _P(GqJointCmd), _i] + _LAUNCH + _SEQ),
    'gq_step_foot_cmd': (_i, [_v, _P(GqFootCmd), _i] + _LAUNCH + _SEQ),
    'gq_batch_bind': (_i, [_v] + _LAUNCH + [_v]),
    'gq_reset': (_i, [_v, _v, _v, _v, _P(GqResetCfg), GqState, GqObsOut, _v, _v, _v]),
    'gq_batch_set_pending': (_i, [_v, _v, _v]),
    'gq_heightmap': (_i, [_v, _v, _v, _i, _i, _f, _f, _v, _v]),
    'gq_heightmap_strided': (_i, [_v, _v, _i, _v, _i, _i, _i, _f, _f, _v, _v]),
    'gq_jac': (_i, [_v, _v, _i, _v, _v, _v, _v]),
    'gq_ray': (_i, [_v, _v, _v, _i, _v, _v, _v]),
    'gq_camera': (_i, _CAMERA + [_v]),
    'gq_camera_shaded': (_i, _CAMERA + [_P(GqCamShade), _v, _v]),
    'gq_camera_layered': (_i, _CAMERA + [_P(GqCamShade), _v, _P(GqCamLayers), _v]),
    'gq_forward': (_i, [_v, _i, _v, GqState, GqObsOut, _v]),
    'gq_batch_set_outputs': (_i, [_v, _v, _v]),
    'gq_contact_force': (_i, [_v, _i, _v, _v]),
    'gq_full_mass': (_i, [_v, _i, _v, _v]),
    'gq_debug_enable': (_i, [_v, _i]),
    'gq_debug_device_buffer': (_i, [_v, _P(_v), _i32p, _i32p]),
    'gq_debug_stop_stage': (_i, [_v, _i]),
    'gq_debug_field': (_i, [C.c_char_p, _i32p, _i32p]),
    'gq_debug_get': (_i, [_v, _i, C.c_char_p, _v, _i]),
}
EXPORTS = list(ABI)


class GqError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not LIB_PATH.exists():
        raise GqError(f'{LIB_PATH} not found: build the HIP extension first (python -c "import __graft_entry__ as g; '
                      f'g.build()" or make -C gym_quadruped_amd/csrc). There is no CPU fallback.')
    import torch  # noqa: F401  - load torch's HIP runtime first so libgq.so binds to the same one
    L = C.CDLL(str(LIB_PATH))
    # a stale libgq.so (built from an older include/gq.h) would shift every by-value struct argument: refuse it here
    if not hasattr(L, 'gq_struct_sizes') or L.gq_version() != GQ_ABI_VERSION:
        raise GqError(f'{LIB_PATH} implements ABI {L.gq_version()}, this binding expects {GQ_ABI_VERSION}: rebuild the library '
                      f'(make -C gym_quadruped_amd/csrc)')
    sizes = (C.c_int32 * len(SIZED_STRUCTS))()
    L.gq_struct_sizes(sizes)
    mirror = [C.sizeof(t) for t in SIZED_STRUCTS]
    if list(sizes) != mirror:
        raise GqError(f'struct layouts differ between {LIB_PATH} {list(sizes)} and gym_quadruped_amd/cabi.py {mirror}')
    for name, (restype, argtypes) in ABI.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    _LIB = L
    return L


def check(rc, what):
    if rc < 0:
        raise GqError(f'{what} failed ({rc}): {lib().gq_last_error().decode()}')
    return rc
