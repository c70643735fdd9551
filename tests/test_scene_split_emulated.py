"""The flat self-collision scene, split by pair routine (csrc/gq_step_kernel.h Scene), under the host SIMT emulator: robots in
self-colliding poses are stepped through the emulator as it is built - model_scene picks each model's scene, and with it the template
arguments of step_wave - and through a second build of the same sources with -DGQ_SCENE_SPLIT_OFF, in which every model runs the body with
both pair routines, as before the split.  The two must agree to the bit.

What this reaches: for mini_cheetah and hyqreal1 (SCENE_FLAT_SELF_HULL) the body without the exact box routines, PRIM = false - one point per
pair and the ballot form of the append - against the body with them.  For go2 and aliengo (SCENE_FLAT_SELF_PRIM) the body without the convex
block and the pair exchange, CVX = false - the emulator runs the kernels' own driver (csrc/gq_step_driver.h) with CVX from the rule the
launches use (gq_step_kernel.h kernel_cvx), so it instantiates what step_kernel_prim does - against the body with them."""
import numpy as np
import pytest

import helpers
import scene_split_build as ssb
from helpers import dbg, emu_lib, emu_step, marshalled, self_contact_states
from oracle.oracle import Oracle

ROBOTS = {'mini_cheetah': ssb.SCENE_FLAT_SELF_HULL, 'hyqreal1': ssb.SCENE_FLAT_SELF_HULL,
          'go2': ssb.SCENE_FLAT_SELF_PRIM, 'aliengo': ssb.SCENE_FLAT_SELF_PRIM}


@pytest.fixture(scope='module')
def builds(tmp_path_factory):
    """(the emulator with the split off + scene_choice, scene_choice of the tree's own model_scene)"""
    d = tmp_path_factory.mktemp('scene_split')
    off = ssb.build(d / 'libgq_emu_split_off.so', ['-DGQ_SCENE_SPLIT_OFF'], add_sources=[ssb.SCENE_SRC])
    return off, ssb.build_scene_lib(d / 'libscene_choice.so')


def step_with(lib, *args, **kw):
    """helpers.emu_step through another build of the emulator"""
    emu_lib()
    mine, helpers._EMU = helpers._EMU, lib
    try:
        return emu_step(*args, **kw)
    finally:
        helpers._EMU = mine


@pytest.mark.parametrize('robot', list(ROBOTS))
def test_split_scene_steps_like_the_full_kernel(builds, robot):
    off, choice = builds
    n = 8
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-10, noise_floor=0.0)
    assert ssb.scene_choice(choice, mm)['scene'] == ROBOTS[robot] and ssb.scene_choice(off, mm)['scene'] == ssb.SCENE_FLAT_SELF
    o = Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-12))
    rng = np.random.default_rng(7)
    qpos, qvel = self_contact_states(mm.md, n, rng, o, want_cross=True)
    qvel = qvel.astype(np.float32)
    ctrl = (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)
    fric = np.full(n, 0.7, np.float32)
    a = emu_step(mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n, friction=fric)
    b = step_with(off, mm, ctrl, qpos.copy(), qvel.copy(), debug_envs=n, friction=fric)
    for k in ('qpos', 'qvel', 'qacc', 'warm', 'obs', 'terminated', 'invalid'):
        assert np.array_equal(a[k], b[k]), k
    nself = 0
    for e in range(n):
        for f in ('ncon', 'nefc', 'contact_dist', 'contact_geom', 'efc_J', 'efc_aref', 'efc_force', 'qacc'):
            assert np.array_equal(dbg(a['debug'][e], f), dbg(b['debug'][e], f)), (e, f)
        ncon = int(dbg(a['debug'][e], 'ncon')[0])
        # a robot-robot contact names both items: second | (first + 1) << 8 (csrc/gq_boxes.h append_self_contacts)
        nself += int((dbg(a['debug'][e], 'contact_geom')[:ncon].astype(int) >= 256).sum())
    assert nself > 0, 'no robot-robot contact: the self-collision stage was not compared'
    assert not np.array_equal(a['qpos'], qpos)
