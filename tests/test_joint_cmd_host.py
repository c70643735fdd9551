"""Joint-impedance actions (gq_step_joint_cmd), the parts that need no GPU: the law of csrc/gq_joint_cmd.h compiled for the host with the
emulator's shim and compared bit for bit with the elementwise float32 expression, and the C ABI of the new entry point."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / 'gym_quadruped_amd' / 'csrc'

PROGRAM = r'''
#include <cstdio>
#include <vector>
#include <gq_joint_cmd.h>
/* the same expression WITHOUT the header's pragma: what this build makes of it shows whether the build contracts at all (kept out of
 * line: inlined next to the header's law, its operations would be merged with the guarded ones) */
__attribute__((noinline)) static float law_unguarded(float q_des, float qd_des, float tau_ff, float kp, float kd, float q, float qd) {
  return kp * (q_des - q) + kd * (qd_des - qd) + tau_ff;
}
/* in: n, then n records {q_des, qd_des, tau_ff, kp, kd, q, qd} of float32; out: n torques of the header's law, then n of the twin */
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int n = 0;
  if (fread(&n, sizeof n, 1, f) != 1) return 4;
  std::vector<float> in((size_t)n * 7), out((size_t)n * 2);
  if (fread(in.data(), sizeof(float), in.size(), f) != in.size()) return 5;
  fclose(f);
  for (int i = 0; i < n; i++) {
    const float* r = &in[(size_t)i * 7];
    out[i] = gq::joint_cmd_law(r[0], r[1], r[2], r[3], r[4], r[5], r[6]);
    out[n + i] = law_unguarded(r[0], r[1], r[2], r[3], r[4], r[5], r[6]);
  }
  f = fopen(argv[2], "wb");
  if (!f) return 6;
  fwrite(out.data(), sizeof(float), out.size(), f);
  fclose(f);
  return 0;
}
'''


def _fma_build():
    """(compiler, flags) of a host build that DOES contract a * b + c into a fused multiply-add unless told otherwise: ROCm's clang for a CPU
    with FMA, under the contraction mode hipcc compiles device code with by default (fast-honor-pragmas: fuse across statements, but
    obey the pragmas; plain `fast` lets the backend fuse whatever the pragmas say).  None where that cannot run (no such compiler, or a CPU without the instructions)."""
    clang = next((p for p in ('/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++') if Path(p).exists()), None)
    try:
        has_fma = any(' fma ' in line + ' ' for line in open('/proc/cpuinfo') if line.startswith('flags'))
    except OSError:
        has_fma = False
    return (clang, ['-mfma', '-ffp-contract=fast-honor-pragmas']) if clang and has_fma else None


@pytest.fixture(scope='module')
def law(tmp_path_factory):
    """the header's law as a host program: records [n, 7] float32 -> (torques [n] float32 of the header's law, torques [n] of the same
    expression written without the header's pragma).  Built so that the compiler fuses what it may (clang -mfma -ffp-contract=fast-honor-pragmas):
    only `#pragma clang fp contract(off)` in the header then keeps every operation rounded on its own.  Without such a compiler or
    CPU the build is the emulator's (g++ -ffp-contract=off), which checks the expression but not the pragma."""
    d = tmp_path_factory.mktemp('joint_cmd')
    (d / 'law.cpp').write_text(PROGRAM)
    fma = _fma_build()
    cxx, flags = fma if fma else ('g++', ['-ffp-contract=off', '-Wno-unknown-pragmas'])
    # the emulator's gq_device.h shadows the product's on the include path (tests/simt_emu/Makefile)
    subprocess.run([cxx, '-O2', '-std=c++17', *flags, '-I', str(ROOT / 'tests' / 'simt_emu'), '-I', str(CSRC), str(d / 'law.cpp'), '-o', str(d / 'law')], check=True)

    def run(rec):
        rec = np.ascontiguousarray(rec, dtype=np.float32)
        with open(d / 'in.bin', 'wb') as f:
            f.write(np.int32(len(rec)).tobytes()); f.write(rec.tobytes())
        subprocess.run([str(d / 'law'), str(d / 'in.bin'), str(d / 'out.bin')], check=True)
        out = np.fromfile(d / 'out.bin', dtype=np.float32)
        return out[:len(rec)], out[len(rec):]
    run.contracting = fma is not None
    return run


def _records(n=10000, seed=5):
    """the ranges of the GPU test's commands around a standing posture, and joint states a falling robot reaches"""
    g = np.random.default_rng(seed)
    q_des = g.uniform(-2.5, 2.5, n); qd_des = g.uniform(-1, 1, n); tau_ff = g.uniform(-5, 5, n)
    kp = g.uniform(20, 60, n); kd = g.uniform(0.5, 2, n); q = g.uniform(-3, 3, n); qd = g.normal(0, 8, n)
    return np.stack([q_des, qd_des, tau_ff, kp, kd, q, qd], axis=1).astype(np.float32)


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def test_law_has_the_bits_of_the_elementwise_float32_expression(law):
    r = _records()
    q_des, qd_des, tau_ff, kp, kd, q, qd = r.T
    want = kp * (q_des - q) + kd * (qd_des - qd) + tau_ff      # numpy float32: every operation rounded on its own
    assert want.dtype == np.float32
    got, unguarded = law(r)
    assert np.array_equal(_bits(got), _bits(want))
    if law.contracting:   # this build fuses where nothing forbids it - the twin without the pragma shows it - so the header's pragma is what held
        assert int((_bits(unguarded) != _bits(want)).sum()) >= 1, 'the build does not contract: the comparison above says nothing about the pragma'
    # the same inputs tell a contracted evaluation apart: up + ud with the product kp * e fused into the addition (the product of two
    # float32 is exact in float64; one rounding of the sum to float32)
    e, ud = q_des - q, kd * (qd_des - qd)
    fused = (kp.astype(np.float64) * e.astype(np.float64) + ud.astype(np.float64)).astype(np.float32) + tau_ff
    assert int((_bits(fused) != _bits(want)).sum()) >= 1, 'no input of this set shows a fused multiply-add: the comparison says nothing about contraction'


def test_law_without_velocity_target_and_feed_forward_is_the_pd_law(law):
    r = _records(seed=6)
    r[:, 1] = 0.0; r[:, 2] = 0.0
    q_des, _, _, kp, kd, q, qd = r.T
    want = kp * (q_des - q) - kd * qd                         # pd_law of the closed-loop rollout
    assert np.array_equal(_bits(law(r)[0]), _bits(want))


def test_abi_of_the_joint_command_entry_point():
    from gym_quadruped_amd import _lib
    from gym_quadruped_amd.cabi import GqJointCmd, GqObsOut, GqResetCfg, GqState
    assert 'gq_step_joint_cmd' in _lib.EXPORTS                 # layout and export: tests/test_host_and_abi.py, for every struct and symbol
    L = _lib.lib()
    assert L.gq_version() == 660                               # the entry point is additive: the ABI number and the eight pinned sizes stay
    C = ctypes
    assert L.gq_step_joint_cmd.argtypes == [C.c_void_p, C.POINTER(GqJointCmd), C.c_int, GqState, GqObsOut, C.POINTER(GqResetCfg), C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
    # a stale binding (another struct size) is refused before anything else is looked at
    cmd = GqJointCmd(struct_size=ctypes.sizeof(GqJointCmd) - 8)
    assert L.gq_step_joint_cmd(None, C.byref(cmd), 4, GqState(), GqObsOut(), None, None, None, None, None, None) < 0
    assert b'stale binding' in L.gq_last_error()
