"""The product's device routines one by one on the GPU (tests/device_probe: csrc/gq_device.h's DPP ladders, permutes and transcendental-unit
shortcuts, csrc/gq_step_kernel.h's small math and tree factor / solve, csrc/gq_pairs.h and csrc/gq_convex.h, compiled with the product's flags)
against float64 references: the case tables of tests/device_cases.py and tests/contact_cases.py, which the host emulator is held to as well
(tests/test_device_cases_emulated.py, tests/test_kernel_emulated.py).  The whole-step parity suites see these routines only through
tolerances four orders of magnitude wider than fp32.

Every test adds its measured maxima to a report (the case count, the maximum error, its bound, the worst argument), written when the module is
done to profiles/device_probe_report.txt (GQ_PROBE_REPORT names another file)."""
import os

import pytest

import contact_cases as cc
import device_cases as dc
import hfield_cases as hc
import newton_cases as nc
from helpers import ROOT, probe_lib
from newton_first_step import REPORT_KEY

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    import torch
    assert torch.cuda.is_available()
    return dc.Backend(probe_lib(), 'probe_', device='cuda:0')


@pytest.fixture(scope='module')
def report():
    lines = []
    yield lines
    path = os.environ.get('GQ_PROBE_REPORT', str(ROOT / 'profiles' / 'device_probe_report.txt'))
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        # the first-step lines are tests/test_gpu_parity.py's (newton_first_step.merge_report): kept, whichever module ran first
        kept = [ln for ln in open(path).read().splitlines() if ln.startswith(REPORT_KEY)] if os.path.exists(path) else []
        with open(path, 'w') as fh:
            fh.write('Device probe: the routines called alone on the GPU against float64 references (tests/test_gpu_device_probe.py)\n')
            fh.write('\n'.join(lines + kept) + '\n')
    except OSError:
        pass


def _note(report, lines):
    for line in lines:
        print(line)
        report.append(line)


@pytest.mark.parametrize('name', list(dc.CHECKS) + ['tree'] + list(nc.CHECKS))
def test_device_matches_float64_reference(be, report, name):
    """wave primitives, fast math, small math, Philox, tree factor / solve: see the check of that name in tests/device_cases.py; the Newton
    solver's fused solves, dense step, row laws and elliptic routines: tests/newton_cases.py"""
    check = dc.check_tree if name == 'tree' else (nc.CHECKS[name] if name in nc.CHECKS else dc.CHECKS[name])
    try:
        rows = check(be)
    except AssertionError as e:
        _note(report, [f'{name}: FAILED {str(e)[:600]}'])
        raise
    _note(report, dc.fmt_rows(rows))


def test_pair_routines_on_device_equal_oracle(be, report):
    """capsule_box and box_box, one case per lane, the 1500 cases of the emulated test's table: same counts, tolerances and coverage"""
    cases = cc.pair_cases()
    worst = cc.check_pairs(cases, cc.probe_pairs(be, cases))
    _note(report, [f'capsule_box / box_box        cases {len(cases):>7d}   max error vs fp64 oracle: ' +
                   ', '.join(f'{k} {v[0]:.3g} (trial {v[1]}, tolerance {cc.PAIR_TOL[k]:g})' for k, v in worst.items())])


@pytest.mark.parametrize('robot', [None, 'mini_cheetah', 'hyqreal1', 'go1'])
def test_convex_routine_on_device_equals_oracle(be, report, robot):
    """cvx_pair_wave, one pair per block, the emulated test's four tables: same tolerances and coverage"""
    cases = cc.convex_cases(robot)
    worst = cc.check_convex(cases, cc.probe_convex(be, cases))
    _note(report, [f'cvx_pair_wave {str(robot):<14s} cases {len(cases):>7d}   max error vs fp64 oracle: ' +
                   ', '.join(f'{k} {v[0]:.3g} (trial {v[1]}, tolerance {cc.CVX_TOL[k]:g})' for k, v in worst.items())])


def test_height_field_routines_on_device_equal_oracle(be):
    """closest_on_triangle, hf_triangle_under and sphere_hfield, one case per lane, the emulated test's tables (tests/hfield_cases.py): same
    tolerances and coverage; the worst errors go to profiles/hfield_cases_report.txt"""
    hc.run_backend(be, 'gpu')
