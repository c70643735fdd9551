"""The emulator shim's wave primitives and fast-math stand-ins (tests/simt_emu/gq_device.h) and the kernel's small math compiled against it, held
to the case tables and float64 references of tests/device_cases.py - the same ones tests/test_gpu_device_probe.py holds the hardware to - and
the Newton solver's solves, row laws and elliptic routines (csrc/gq_newton.h) held to those of tests/newton_cases.py."""
import pytest

import device_cases as dc
import newton_cases as nc
from helpers import emu_lib


@pytest.mark.parametrize('name', list(dc.CHECKS))
def test_shim_matches_float64_reference(name):
    for line in dc.fmt_rows(dc.CHECKS[name](dc.Backend(emu_lib(), 'emu_'))):
        print(line)


@pytest.mark.parametrize('name', list(nc.CHECKS))
def test_newton_routines_match_float64_reference(name):
    for line in dc.fmt_rows(nc.CHECKS[name](dc.Backend(emu_lib(), 'emu_'))):
        print(line)
