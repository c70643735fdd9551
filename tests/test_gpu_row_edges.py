"""Joint-limit rows and low ground friction on the GPU against the fp64 oracle: the cases and checks of tests/row_edge_cases.py that
tests/test_row_edges_emulated.py runs under the host emulator, one launch per case."""
import pytest

import row_edge_cases as rc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('robot', rc.LIMIT_ROBOTS)
def test_joint_limit_rows_match_oracle(robot):
    """test_row_edges_emulated.test_joint_limit_rows_match_oracle at 96 envs"""
    case = rc.limit_case(robot, 96)
    rc.hold_limit_case(case, rc.gpu_case_records(case, 'newton', 100, 1e-8, contacts=True, self_collision=False), 'MI355X')


@pytest.mark.parametrize('robot,solver', rc.FRICTION_CASES)
def test_low_ground_friction_matches_oracle(robot, solver):
    """test_row_edges_emulated.test_low_ground_friction_matches_oracle on the GPU"""
    from gym_quadruped_amd.quadruped_env import PYRAMIDAL_NEWTON_MIN_FRICTION
    case = rc.friction_case(robot, solver)
    rc.hold_friction_case(case, rc.gpu_friction_records(case), 'MI355X', PYRAMIDAL_NEWTON_MIN_FRICTION)


def test_ground_friction_floor_is_refused_on_construction_only_where_it_applies():
    """QuadrupedEnv refuses a friction range under the floor for pyramidal cones with solver='newton'; PGS and elliptic-cone robots take it"""
    from gym_quadruped_amd.quadruped_env import QuadrupedEnv
    with pytest.raises(ValueError, match='floor'):
        QuadrupedEnv('aliengo', ground_friction_coeff=(0.0, 1.0), num_envs=2)
    for robot, kw in (('aliengo', dict(solver='pgs')), ('go2', {})):
        env = QuadrupedEnv(robot, ground_friction_coeff=(0.0, 1.0), num_envs=2, **kw)
        env.reset(random=True)
        env.ground_friction_coeff_range = (0.0, 0.5)
        env.close()
    env = QuadrupedEnv('aliengo', ground_friction_coeff=(0.2, 1.0), num_envs=2)
    env.reset(random=True)
    with pytest.raises(ValueError, match='floor'):
        env.ground_friction_coeff_range = (0.01, 1.0)
    sd = env.state_dict()
    sd['_friction'] = sd['_friction'] * 0.0
    with pytest.raises(ValueError, match='floor'):
        env.load_state_dict(sd)
    env.close()
