"""Joint-limit rows and low ground friction in the UNMODIFIED step kernel under the host SIMT emulator against the fp64 oracle: the cases
and checks of tests/row_edge_cases.py, which tests/test_gpu_row_edges.py runs on the GPU."""
import pytest

import row_edge_cases as rc
from helpers import marshalled


@pytest.mark.parametrize('robot', rc.LIMIT_ROBOTS)
def test_joint_limit_rows_match_oracle(robot):
    """1, 2, 4 or every limited joint 1e-5 .. 0.2 rad past its range on a random side, in flight and on the floor: the row count, the
    +-1 Jacobian entry at the joint's dof, aref and the Newton solution against the oracle converged to 1e-12; a joint 1e-5 inside
    its range gives no row."""
    case = rc.limit_case(robot, 48)
    mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-8, noise_floor=1e-5, self_collision=False)
    rc.hold_limit_case(case, rc.emu_case_records(mm, case, contacts=True), 'emulated')


@pytest.mark.parametrize('robot,solver', rc.FRICTION_CASES)
def test_low_ground_friction_matches_oracle(robot, solver):
    """Ground friction 0 .. 3 with sliding feet.  PGS and the elliptic-cone Newton kernel hold their tolerance set on the whole table; the
    pyramidal-cone Newton kernel holds it from QuadrupedEnv's floor up (DESIGN.md "Known deviations") and stays finite below."""
    from gym_quadruped_amd.quadruped_env import PYRAMIDAL_NEWTON_MIN_FRICTION
    case = rc.friction_case(robot, solver)
    rc.hold_friction_case(case, rc.emu_case_records(case['mm'], case), 'emulated', PYRAMIDAL_NEWTON_MIN_FRICTION)


def test_ground_friction_below_the_floor_is_refused():
    """The refusal is host-side: a pyramidal-cone model under solver='newton' takes no ground friction under the floor, at construction
    (raised before anything touches the device) or later; PGS and elliptic cones take any."""
    from gym_quadruped_amd.quadruped_env import PYRAMIDAL_NEWTON_MIN_FRICTION as floor, QuadrupedEnv, check_ground_friction
    assert floor <= 0.2   # what the suite and the documents already promise
    pyramidal, elliptic = marshalled('aliengo').md.cone, marshalled('go2').md.cone
    assert (pyramidal, elliptic) == (0, 1)
    for lowest in (0.0, 1e-3, 0.99 * floor):
        with pytest.raises(ValueError, match=r"floor .* solver='pgs' .* elliptic"):
            check_ground_friction(pyramidal, 'newton', lowest, 'aliengo')
        check_ground_friction(pyramidal, 'pgs', lowest)
        check_ground_friction(elliptic, 'newton', lowest)
    for lowest in (floor, 0.2, 1.0):
        check_ground_friction(pyramidal, 'newton', lowest)
    for kw in (dict(ground_friction_coeff=(0.0, 1.0)), dict(ground_friction_coeff=0.01), dict(ground_friction_coeff=(0.0, 1.0), scene='perlin')):
        with pytest.raises(ValueError, match='floor'):
            QuadrupedEnv('aliengo', **kw)
        with pytest.raises(ValueError, match='floor'):
            QuadrupedEnv('mini_cheetah', **kw)
