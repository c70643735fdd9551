"""Ground-friction sweep of the step kernel against the fp64 oracle: for every (robot, solver) of tests/row_edge_cases.FRICTION_CASES and
every friction of its table, the qacc error max|dqacc| / max(1, max|qacc|) over the compared envs in contact (n, p50, p99, max) and the
kernel's iteration counts.  The states, the reference (the oracle at iteration cap 300, kept where it agrees with cap 1200) and the row checks
are those of the tests; nothing is asserted about qacc here, so the rows below QuadrupedEnv's floor are on record too.

    python tests/reports/low_friction_sweep.py emu|gpu [out.txt]

profiles/low_friction_sweep.txt holds both backends' tables and the floor read from them.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / 'tests'))
import row_edge_cases as rc  # noqa: E402
import step_parity as sp  # noqa: E402


def main(backend, out=None):
    lines = [f'low-friction sweep, backend {backend}: qacc error max|dqacc| / max(1, max|qacc|) against the oracle (cap 300), compared envs in contact',
             f'{"robot":13s}{"solver":8s}{"friction":>9s}{"n":>4s}{"p50":>10s}{"p99":>10s}{"max":>10s}  kernel niter']
    floor = {}
    for robot, solver in rc.FRICTION_CASES:
        case = rc.friction_case(robot, solver)
        kern = rc.emu_case_records(case['mm'], case) if backend == 'emu' else rc.gpu_friction_records(case)
        md = case['m300'].md
        # the rows (efc_J, efc_aref) are held on the whole table; qacc and what follows from it only reported: a floor above every friction
        by = rc.hold_friction_case(case, kern, backend, floor=np.inf if rc.has_floor(md, solver) else 0.0, tols=sp.pick(rc.friction_tols(md, solver), 'efc_J', 'efc_aref'))
        good = True
        for f in reversed(rc.FRICTIONS):
            err = np.asarray([x[0] for x in by[f]])
            good = good and bool((err < 2e-4).all())
            if good:
                floor[(robot, solver)] = f
            lines.append(f'{robot:13s}{solver:8s}{f:9g}{len(err):4d}{np.median(err):10.1e}{np.percentile(err, 99):10.1e}{err.max():10.1e}  {sorted(x[1] for x in by[f])}')
    lines.append('smallest friction at and above which every compared env holds qacc below(2e-4): ' +
                 ', '.join(f'{r} {s} {f:g}' for (r, s), f in floor.items()))
    text = '\n'.join(lines) + '\n'
    print(text)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(text)


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None)
