"""Which flat self-collision scene a model gets (csrc/gq_step_call.h model_scene; csrc/gq_step_kernel.h Scene): the kernel build is chosen
from the pair table the kernel walks, so a model with a pair for the exact box routines (kinds 1 - 3) always gets a build that has them, and
a model with a pair for the convex routine (kind 4) always gets the convex block.  Host code only: the function is reached through
tests/scene_choice.cpp, built here with the emulator's flags."""
import pytest

import scene_split_build as ssb
from helpers import marshalled

ROBOTS = ['aliengo', 'b2', 'go1', 'go2', 'hyqreal1', 'hyqreal2', 'mini_cheetah', 'spot']
# convex mode (MuJoCo's behaviour), by the robots' colliding geoms: mesh hulls + foot spheres / boxes, capsules, spheres / boxes + cylinders
CONVEX_SCENE = {'mini_cheetah': ssb.SCENE_FLAT_SELF_HULL, 'hyqreal1': ssb.SCENE_FLAT_SELF_HULL, 'spot': ssb.SCENE_FLAT_SELF_HULL,
                'go2': ssb.SCENE_FLAT_SELF_PRIM, 'aliengo': ssb.SCENE_FLAT_SELF_PRIM, 'hyqreal2': ssb.SCENE_FLAT_SELF_PRIM,
                'b2': ssb.SCENE_FLAT_SELF, 'go1': ssb.SCENE_FLAT_SELF}


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
    return ssb.build_scene_lib(tmp_path_factory.mktemp('scene_choice') / 'libscene_choice.so')


@pytest.mark.parametrize('robot', ROBOTS)
@pytest.mark.parametrize('mode', ['convex', 'capsule'])
def test_flat_scene_follows_the_pair_table(lib, robot, mode):
    c = ssb.scene_choice(lib, marshalled(robot, solver=1, self_collision=mode))
    assert c['nsp'] > 0 and c['cvx'] == c['ncvx_self']
    # capsule-proxy mode has no kind 4 pair: never the convex block, whatever the robot is made of
    assert c['scene'] == (CONVEX_SCENE[robot] if mode == 'convex' else ssb.SCENE_FLAT_SELF_PRIM)
    assert (c['cvx'] > 0) == (mode == 'convex' and CONVEX_SCENE[robot] != ssb.SCENE_FLAT_SELF_PRIM)
    # the two rules, from the table itself
    assert c['self'] and not c['boxes']
    if c['box'] > 0:
        assert c['prim'], 'a pair of kind 1 - 3 and a scene without the box routines'
    if c['cvx'] > 0:
        assert c['has_cvx'], 'a pair of kind 4 and a scene without the convex block'
    # ... and nothing is compiled in that the table does not name
    assert c['has_cvx'] == (c['cvx'] > 0)
    assert c['prim'] == (c['box'] > 0 or c['cvx'] == 0)   # (a table of capsule-proxy pairs alone runs the kernel without the convex block)


@pytest.mark.parametrize('robot', ['mini_cheetah', 'go2', 'b2'])
def test_other_scenes_are_as_before(lib, robot):
    from gym_quadruped_amd.robot_cfgs import get_robot_config
    from gym_quadruped_amd.terrain import generate_terrain
    assert ssb.scene_choice(lib, marshalled(robot, solver=1, self_collision=False))['scene'] == ssb.SCENE_FLAT
    scene, lim = generate_terrain('random_boxes', get_robot_config(robot).hip_height)
    c = ssb.scene_choice(lib, marshalled(robot, solver=1, boxes=scene['boxes'], terrain_limits=lim))
    assert c['scene'] == (ssb.SCENE_WORLD_HULL if robot == 'mini_cheetah' else ssb.SCENE_WORLD_PRIM) and c['has_cvx']


def test_split_off_switch_gives_every_model_the_full_kernel(tmp_path):
    off = ssb.build_scene_lib(tmp_path / 'libscene_choice_off.so', ['-DGQ_SCENE_SPLIT_OFF'])
    for robot in ('mini_cheetah', 'go2', 'b2'):
        for mode in ('convex', 'capsule'):
            assert ssb.scene_choice(off, marshalled(robot, solver=1, self_collision=mode))['scene'] == ssb.SCENE_FLAT_SELF
    assert ssb.scene_choice(off, marshalled('go2', solver=1, self_collision=False))['scene'] == ssb.SCENE_FLAT
