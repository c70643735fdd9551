"""TEST INFRASTRUCTURE for the scene-split tests: further host builds with the flags of tests/simt_emu/Makefile (read from `make -n`, so that
they cannot drift from the emulator's own), into a directory of the caller's."""
import ctypes as C
import shlex
import subprocess
from pathlib import Path

import numpy as np

EMU_DIR = Path(__file__).resolve().parent / 'simt_emu'
CSRC = '../../gym_quadruped_amd/csrc'
SCENE_SRC = '../scene_choice.cpp'
# gq::Scene (csrc/gq_step_kernel.h)
SCENE_FLAT, SCENE_FLAT_SELF, SCENE_WORLD_HULL, SCENE_WORLD_PRIM, SCENE_FLAT_SELF_HULL, SCENE_FLAT_SELF_PRIM = range(6)


def emu_compile_line():
    """the emulator Makefile's compile line: [compiler, flags ..., '-o', 'libgq_emu.so', sources ..., libraries]"""
    out = subprocess.run(['make', '-n', '-B', '-C', str(EMU_DIR)], check=True, capture_output=True, text=True).stdout
    return shlex.split(next(l for l in out.splitlines() if ' -shared ' in l))


def build(out_so, extra_flags=(), add_sources=(), only_sources=None):
    """Compile like libgq_emu.so, with extra_flags added: the emulator's sources plus add_sources, or only_sources alone (paths relative
    to tests/simt_emu).  -fno-gnu-unique: a second build loaded into one process keeps its own copies of the inline functions' statics."""
    line = emu_compile_line()
    at = line.index('-o')
    line[at:at + 2] = []
    sources = [a for a in line[1:] if a.endswith('.cpp')]
    libs = [a for a in line[1:] if a.startswith('-l')]
    flags = [a for a in line[1:] if a not in sources and a not in libs]
    sources = list(only_sources) if only_sources is not None else sources + list(add_sources)
    cmd = [line[0], *flags, '-fno-gnu-unique', *extra_flags, '-o', str(out_so), *sources, *libs]
    subprocess.run(cmd, check=True, capture_output=True, cwd=EMU_DIR)
    return C.CDLL(str(out_so))


def build_scene_lib(out_so, extra_flags=()):
    """scene_choice.cpp alone (with the host model builder it calls)"""
    return build(out_so, extra_flags, only_sources=[SCENE_SRC, f'{CSRC}/gq_host_model.cpp'])


def scene_choice(lib, mm):
    """dict(scene, nsp, box pairs, convex pairs, ncvx_self, scene_boxes, scene_self, scene_prim, scene_cvx) of a MarshalledModel"""
    out = np.zeros(9, np.int32)
    err = C.create_string_buffer(512)
    if lib.scene_choice(C.byref(mm.desc), out.ctypes.data_as(C.c_void_p), err, 512) < 0:
        raise RuntimeError(err.value.decode())
    return dict(zip(('scene', 'nsp', 'box', 'cvx', 'ncvx_self', 'boxes', 'self', 'prim', 'has_cvx'), (int(v) for v in out)))
