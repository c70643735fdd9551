"""How far do the fp64 oracle's own contacts move when its geom poses carry one fp32 rounding?  Every entry of geom_xpos / geom_xmat is
multiplied by 1 +- 2^-23 (Oracle.set_pose_noise) on the draws of the self-collision parity tests, and the movement of dist, normal, tangents
and (determined) point of every contact whose list did not change is recorded.  The tolerances of tests/contact_list.py that the kernel's
fp32 forward kinematics alone can exceed may be set to 4 x these movements and no more (profiles/contact_list_parity.md).  Host only."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / 'tests')]
from helpers import marshalled, self_contact_states   # noqa: E402
from oracle.oracle import Oracle   # noqa: E402


def contacts(o):
    return dict(g=(o.get('contact_geom1').astype(int), o.get('contact_geom').astype(int)), dist=o.get('contact_dist'), frame=o.contact_frame, pos=o.contact_pos,
                gap=o.get('contact_tiegap'), cvx=o.get('contact_cvx').astype(bool))


def main(robots=('mini_cheetah', 'aliengo', 'go2', 'go1', 'hyqreal1', 'b2', 'spot'), n=160, seeds=(1, 2, 3), rel=2.0 ** -23, thr=3e-7):
    keys = ('dist', 'angle_deg', 'normal', 'tangent', 'pos')
    for robot in robots:
        mm = marshalled(robot, solver=1, iterations=100, tolerance=1e-12)
        o = Oracle(mm)
        rng = np.random.default_rng(5)
        hip = float(mm.desc.key_qpos[2])
        cone = mm.md.cone == 1
        qa, va = self_contact_states(mm.md, n // 2, rng, o, z=(0.7 * hip, 1.3 * hip), want_cross=True, cone=cone, max_over=0.08)
        qb, vb = self_contact_states(mm.md, n - n // 2, rng, o, z=(0.7 * hip, 2.5 * hip), want_cross=None, cone=cone, max_over=0.08)
        mv = {(k, c): [] for k in keys for c in (False, True)}
        changed = 0
        for q, v in zip(np.concatenate([qa, qb]), np.concatenate([va, vb])):
            o.set_pose_noise(0.0)
            o.set_state(q, v, np.zeros(18), np.zeros(18), 0.0, 0.8); o.forward(np.zeros(12), stage=1)
            if not o.ncon:
                continue
            a = contacts(o)
            scale = max(1.0, np.abs(a['pos']).max())
            for seed in seeds:
                o.set_pose_noise(rel, seed)
                o.set_state(q, v, np.zeros(18), np.zeros(18), 0.0, 0.8); o.forward(np.zeros(12), stage=1)
                b = contacts(o) if o.ncon else None
                if b is None or len(b['dist']) != len(a['dist']) or any((x != y).any() for x, y in zip(a['g'], b['g'])):
                    changed += 1
                    continue
                for c in range(len(a['dist'])):
                    if a['gap'][c] == 0.0 or b['gap'][c] == 0.0:
                        continue   # capped pairs are not compared
                    k = bool(a['cvx'][c])
                    mv['dist', k].append(abs(a['dist'][c] - b['dist'][c]))
                    mv['angle_deg', k].append(np.degrees(np.arccos(np.clip(a['frame'][c][0] @ b['frame'][c][0], -1, 1))))
                    mv['normal', k].append(np.abs(a['frame'][c][0] - b['frame'][c][0]).max())
                    mv['tangent', k].append(np.abs(a['frame'][c][1:] - b['frame'][c][1:]).max())
                    if a['gap'][c] >= thr and b['gap'][c] >= thr:
                        mv['pos', k].append(np.linalg.norm(a['pos'][c] - b['pos'][c]) / scale)
        for k in (False, True):
            if mv['dist', k]:
                print(f'{robot} {"convex" if k else "primitive"}: {len(mv["dist", k])} contacts; ' +
                      '; '.join(f'{key} p99 {np.percentile(mv[key, k], 99):.2e} max {np.max(mv[key, k]):.2e}' for key in keys if mv[key, k]) + f'; lists changed {changed}')


if __name__ == '__main__':
    main(*([tuple(sys.argv[1:])] if len(sys.argv) > 1 else []))
