"""Foot-space actions (gq_step_foot_cmd), the parts that need no GPU: the law of csrc/gq_foot_cmd.h compiled for the host with the
emulator's shim, over the model records gq_host_model.cpp builds (the way tests/simt_emu gets its model: the GqModelDesc goes in through
ctypes, so the host build is a small library of its own rather than a program with a main), held to the fp64 evaluation of
tests/foot_cmd_ref.py; that reference held to a finite difference of the oracle's foot position; the exact reductions; the C ABI.

    python tests/test_foot_cmd_host.py        prints the table of profiles/foot_cmd_law_error.txt (the measured constants)
"""
import ctypes
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
CSRC = ROOT / 'gym_quadruped_amd' / 'csrc'

from foot_cmd_ref import C_BOUND, FootCmdRef  # noqa: E402
from helpers import marshalled  # noqa: E402

ROBOTS = ('mini_cheetah', 'go2', 'hyqreal1', 'b2')
NREC = 10000
REC = 100   # floats per record: q 12, qd 12, qb 4, p_des 12, v_des 12, f_ff 12, kp 12, kd 12, tau_ff 12

LIBRARY = r'''
#include <cstdio>
#include <vector>
#include <gq_foot_cmd.h>
#include "gq_host_model.h"
/* in: n records {q[12], qd[12], qb[4], p_des[12], v_des[12], f_ff[12], kp[12], kd[12], tau_ff[12]} of float32 (foot rows [foot k][xyz],
 * q / qd / tau_ff in hinge order); out: n x 12 torques, hinge order - each foot's leg evaluated by the header's law over the records
 * gq_build_dev_model made of the description, as the kernel's lanes 0-3 do */
extern "C" int foot_law_run(const GqModelDesc* desc, int n, int frame, const float* in, float* out, char* err, int errlen) {
  static GqDevModel M; /* (large) */
  std::vector<float> vx, vy, vz;
  if (gq_build_dev_model(desc, &M, &vx, &vy, &vz, err, (size_t)errlen)) return -1;
  for (int e = 0; e < n; e++) {
    const float* r = in + (size_t)e * 100;
    const float *q = r, *qd = r + 12, *qb = r + 24;
    for (int k = 0; k < 4; k++) {
      const int leg = M.foot_leg[k];
      gq::FootCmd c;
      for (int i = 0; i < 3; i++) {
        c.p_des[i] = r[28 + 3 * k + i]; c.v_des[i] = r[40 + 3 * k + i]; c.f_ff[i] = r[52 + 3 * k + i];
        c.kp[i] = r[64 + 3 * k + i]; c.kd[i] = r[76 + 3 * k + i]; c.tau_ff[i] = r[88 + 3 * leg + i];
      }
      gq::foot_cmd_law(M.link_rec[3 * leg], M.link_rec[3 * leg + 1], M.link_rec[3 * leg + 2], M.foot_pos[k], q + 3 * leg, qd + 3 * leg, qb, c, frame,
                       out + (size_t)e * 12 + 3 * leg);
    }
  }
  return 0;
}
'''


@pytest.fixture(scope='module')
def law(tmp_path_factory):
    """law(mm, records [n, 100] float32, frame) -> torques [n, 12] float32: the header's law built like the emulator (tests/simt_emu/Makefile:
    its gq_device.h shadows the product's on the include path)"""
    d = tmp_path_factory.mktemp('foot_cmd')
    return _build(d)


def _build(d):
    (d / 'law.cpp').write_text(LIBRARY)
    subprocess.run(['g++', '-O2', '-fPIC', '-shared', '-std=c++17', '-ffp-contract=off', '-Wno-unknown-pragmas', '-I', str(ROOT / 'tests' / 'simt_emu'),
                    '-I', str(CSRC), '-I', str(ROOT / 'include'), str(d / 'law.cpp'), str(CSRC / 'gq_host_model.cpp'), '-o', str(d / 'libfootlaw.so'), '-lm'], check=True)
    L = ctypes.CDLL(str(d / 'libfootlaw.so'))

    def run(mm, rec, frame):
        rec = np.ascontiguousarray(rec, dtype=np.float32)
        assert rec.shape[1] == REC
        out = np.zeros((len(rec), 12), np.float32)
        err = ctypes.create_string_buffer(512)
        rc = L.foot_law_run(ctypes.byref(mm.desc), len(rec), int(frame == 'world'), rec.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), err, 512)
        assert rc == 0, err.value.decode()
        return out
    return run


_REFS = {}


def _ref(robot):
    if robot not in _REFS:
        _REFS[robot] = FootCmdRef(marshalled(robot, solver=1))
    return _REFS[robot]


def _records(ref, n, seed):
    """joint angles over each joint's range, qd ~ N(0, 8), quaternions uniform, |f_ff| <= 3 m g, kp <= 2000, kd <= 50, |p_des| <= 1 m,
    |v_des| <= 3, |tau_ff| <= 5"""
    g = np.random.default_rng(seed)
    md = ref.md
    lo = np.array([md.jnt_range[1 + j][0] if md.jnt_limited[1 + j] else -np.pi for j in range(12)])
    hi = np.array([md.jnt_range[1 + j][1] if md.jnt_limited[1 + j] else np.pi for j in range(12)])
    q = g.uniform(lo, hi, (n, 12))
    qd = g.normal(0, 8, (n, 12))
    qb = g.normal(0, 1, (n, 4)); qb /= np.linalg.norm(qb, axis=1, keepdims=True)
    fmax = 3 * ref.mass * 9.81
    u = lambda a: g.uniform(-a, a, (n, 12))
    rec = np.concatenate([q, qd, qb, u(1.0), u(3.0), u(fmax), g.uniform(0, 2000, (n, 12)), g.uniform(0, 50, (n, 12)), u(5.0)], axis=1)
    return rec.astype(np.float32)


def _reference(ref, rec, frame):
    """fp64 torques and scales of the records (the float32 values the law was given, as fp64)"""
    r = rec.astype(np.float64)
    tau, scale = np.zeros((len(r), 12)), np.zeros((len(r), 12))
    for e in range(len(r)):
        qpos = np.r_[0.0, 0.0, 0.5, r[e, 24:28], r[e, 0:12]]
        qvel = np.r_[np.zeros(6), r[e, 12:24]]
        tau[e], scale[e] = ref.torques(qpos, qvel, r[e, 28:40], r[e, 64:76], r[e, 76:88], v_des=r[e, 40:52], f_ff=r[e, 52:64], tau_ff=r[e, 88:100], frame=frame)
    return tau, scale


def _ratio(law, robot, frame, n=NREC):
    ref = _ref(robot)
    rec = _records(ref, n, seed=ROBOTS.index(robot) * 2 + (frame == 'world'))
    got = law(ref.mm, rec, frame).astype(np.float64)
    want, scale = _reference(ref, rec, frame)
    assert np.isfinite(got).all() and (scale > 0).all()
    return float((np.abs(got - want) / (2.0 ** -24 * scale)).max())


@pytest.mark.parametrize('robot', ROBOTS)
def test_reference_law_agrees_with_a_finite_difference_of_the_oracle_foot_position(robot):
    """d p / d q_leg by central differences (1e-6 rad) of the oracle's foot position against the Jacobian the reference uses: 1e-8"""
    ref = _ref(robot)
    rec = _records(ref, 8, seed=40).astype(np.float64)
    h = 1e-6
    for e in range(len(rec)):
        qpos = np.r_[0.3, -0.2, 0.5, rec[e, 24:28], rec[e, 0:12]]
        kin = ref.kinematics(qpos)
        for k in range(4):
            l = ref.leg[k]
            for i in range(3):
                qp, qm = qpos.copy(), qpos.copy()
                qp[7 + 3 * l + i] += h; qm[7 + 3 * l + i] -= h
                fd = (ref.foot_pos(qp, k) - ref.foot_pos(qm, k)) / (2 * h)
                assert np.abs(fd - kin[k][1][:, i]).max() <= 1e-8, (robot, e, k, i)


@pytest.mark.parametrize('frame', ['base', 'world'])
@pytest.mark.parametrize('robot', ROBOTS)
def test_law_of_the_header_is_within_the_rounding_bound_of_the_fp64_reference(law, robot, frame):
    """|tau - tau_ref| <= C 2^-24 scale on 10 000 random records.  Measured by this host build (profiles/foot_cmd_law_error.txt): at most
    18.64 (mini_cheetah, base frame); C_BOUND = 128 is that times 4, rounded up to a power of two."""
    c = _ratio(law, robot, frame)
    print(f'{robot} {frame}: largest |tau - tau_ref| / (2^-24 scale) = {c:.2f} (bound {C_BOUND})')
    assert c <= C_BOUND


@pytest.mark.parametrize('robot', ['mini_cheetah', 'hyqreal1'])
def test_law_reduces_exactly(law, robot):
    ref = _ref(robot)
    rec = _records(ref, 2000, seed=77)
    # no gains, no force: the torques are tau_ff, bit for bit
    r0 = rec.copy()
    r0[:, 52:88] = 0.0
    for frame in ('base', 'world'):
        assert np.array_equal(law(ref.mm, r0, frame).view(np.uint32), r0[:, 88:100].view(np.uint32)), frame
    # world axes with the identity quaternion are the base axes
    r1 = rec.copy()
    r1[:, 24:28] = [1.0, 0.0, 0.0, 0.0]
    assert np.array_equal(law(ref.mm, r1, 'world').view(np.uint32), law(ref.mm, r1, 'base').view(np.uint32))
    # ... and with another one they are not (the comparison above says something)
    assert not np.array_equal(law(ref.mm, rec, 'world'), law(ref.mm, rec, 'base'))


def test_abi_of_the_foot_command_entry_point():
    from gym_quadruped_amd import _lib
    from gym_quadruped_amd.cabi import GqFootCmd, GqObsOut, GqResetCfg, GqState
    assert 'gq_step_foot_cmd' in _lib.EXPORTS                  # layout and export: tests/test_host_and_abi.py, for every struct and symbol
    L = _lib.lib()
    assert L.gq_version() == 660                               # the entry point is additive: the ABI number and the eight pinned sizes stay
    C = ctypes
    assert L.gq_step_foot_cmd.argtypes == [C.c_void_p, C.POINTER(GqFootCmd), C.c_int, GqState, GqObsOut, C.POINTER(GqResetCfg), C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]
    # a stale binding (another struct size) is refused before anything else is looked at
    cmd = GqFootCmd(struct_size=ctypes.sizeof(GqFootCmd) - 8)
    assert L.gq_step_foot_cmd(None, C.byref(cmd), 4, GqState(), GqObsOut(), None, None, None, None, None, None) < 0
    assert b'stale binding' in L.gq_last_error()


if __name__ == '__main__':
    with tempfile.TemporaryDirectory() as tmp:
        run = _build(Path(tmp))
        print('largest |tau - tau_ref| / (2^-24 scale) of csrc/gq_foot_cmd.h, host build (g++ -O2 -ffp-contract=off, the emulator\'s shim), against')
        print(f'tests/foot_cmd_ref.py (fp64, CPU oracle); {NREC} random records per robot and frame (tests/test_foot_cmd_host.py _records)')
        worst = 0.0
        for robot in ROBOTS:
            for frame in ('base', 'world'):
                c = _ratio(run, robot, frame)
                worst = max(worst, c)
                print(f'{robot:14s} {frame:6s} {c:8.3f}')
        print(f'largest: {worst:.3f}; x 4 = {4 * worst:.3f}; rounded up to a power of two: C_BOUND = {2 ** int(np.ceil(np.log2(4 * worst)))}')
