"""The emulator shim's wave primitives and fast-math stand-ins (tests/simt_emu/gq_device.h) and the kernel's small math compiled against it, held
to the case tables and float64 references of tests/device_cases.py - the same ones tests/test_gpu_device_probe.py holds the hardware to."""
import pytest

import device_cases as dc
from helpers import emu_lib


@pytest.mark.parametrize('name', list(dc.CHECKS))
def test_shim_matches_float64_reference(name):
    for line in dc.fmt_rows(dc.CHECKS[name](dc.Backend(emu_lib(), 'emu_'))):
        print(line)
