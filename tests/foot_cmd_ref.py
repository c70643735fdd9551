"""The foot-space law of gq_step_foot_cmd (include/gq.h) in fp64, one env at a time, from the CPU oracle - derived from the oracle's
world-frame kinematics (mj_kinematics, mj_jac), not from csrc/gq_foot_cmd.h:

    p_w = geom_xpos[foot] - xpos[base]            J_w = jacp(geom_xpos[foot], calf body)[:, the leg's three dof columns]
    A   = xmat[base]                               frame 'base': p = A^T p_w, J = A^T J_w;  frame 'world': p = p_w, J = J_w
    v   = J qd_leg;  F = f_ff + kp (p_des - p) + kd (v_des - v);  tau_leg = J^T F + tau_ff

(the translational Jacobian's columns of the leg's own hinges are a_i x (p - o_i) whatever the base does, and rotating the base
rotates them with it).  ``scale`` is the same expression with every term replaced by its absolute value - the running bound of the sums,
the kinematic chain's included: |p| <= sum of the |segments| of the chain, |J[:, i]| <= |a_i| x that sum below hinge i.
TEST INFRASTRUCTURE: no product code is involved."""
import numpy as np

# |tau - tau_ref| <= C_BOUND 2^-24 scale.  The largest ratio the host build of csrc/gq_foot_cmd.h shows over 10 000 random records per robot
# and frame (tests/test_foot_cmd_host.py, profiles/foot_cmd_law_error.txt) times 4 - the device's sine, cosine, reciprocal square root and
# contraction differ from the host build's by a few ulps - rounded up to a power of two.
C_BOUND = 128   # largest measured: 18.64 (mini_cheetah, base frame)


class FootCmdRef:
    def __init__(self, mm):
        from oracle.oracle import Oracle
        self.mm, self.md = mm, mm.md
        self.o = Oracle(mm)
        self.foot_geom = [int(mm.desc.feet_geomid[k]) for k in range(4)]
        self.calf = [int(self.md.geom_bodyid[g]) for g in self.foot_geom]
        self.leg = [(b - 2) // 3 for b in self.calf]          # kinematic leg (body order) of foot k
        self.mass = float(np.sum(self.md.body_mass))

    def kinematics(self, qpos):
        """per foot k: (p_w [3], J_w [3][3], segs [4][3] world segments base->hip body->thigh->calf->foot, axes [3][3] world, A [3][3])"""
        o = self.o
        o.set_state(np.asarray(qpos, np.float64), np.zeros(18))
        o.forward(stage=1)
        xpos, xmat, gx = o.xpos, o.xmat, o.geom_xpos
        out = []
        for k in range(4):
            b2, l = self.calf[k], self.leg[k]
            pf = gx[self.foot_geom[k]]
            jacp, _ = o.jac(pf, b2)
            chain = [xpos[1], xpos[b2 - 2], xpos[b2 - 1], xpos[b2], pf]
            segs = np.stack([chain[i + 1] - chain[i] for i in range(4)])
            axes = np.stack([xmat[b2 - 2 + i] @ self.md.jnt_axis[1 + 3 * l + i] for i in range(3)])
            jpos = np.stack([xmat[b2 - 2 + i] @ self.md.jnt_pos[1 + 3 * l + i] for i in range(3)])   # anchor offsets (zero for most robots)
            out.append((pf - xpos[1], jacp[:, 6 + 3 * l:9 + 3 * l].copy(), segs, axes, jpos, xmat[1]))
        return out

    def foot_pos(self, qpos, k):
        return self.kinematics(qpos)[k][0]

    def torques(self, qpos, qvel, p_des, kp, kd, v_des=None, f_ff=None, tau_ff=None, frame='base'):
        """one env.  p_des, v_des, f_ff, kp, kd: [12] = [foot k: FL FR RL RR][xyz]; tau_ff: [12] hinge order.  Returns (tau [12], scale [12]), hinge order"""
        z = np.zeros(12)
        p_des, kp, kd = (np.asarray(x, np.float64).reshape(4, 3) for x in (p_des, kp, kd))
        v_des, f_ff = (np.asarray(z if x is None else x, np.float64).reshape(4, 3) for x in (v_des, f_ff))
        tau_ff = np.asarray(z if tau_ff is None else tau_ff, np.float64)
        qvel = np.asarray(qvel, np.float64)
        tau, scale = np.zeros(12), np.zeros(12)
        for k, (p_w, J_w, segs, axes, jpos, A) in enumerate(self.kinematics(qpos)):
            l = self.leg[k]
            T = A.T if frame == 'base' else np.eye(3)
            p, J = T @ p_w, T @ J_w
            qd = qvel[6 + 3 * l:9 + 3 * l]
            v = J @ qd
            F = f_ff[k] + kp[k] * (p_des[k] - p) + kd[k] * (v_des[k] - v)
            tau[3 * l:3 * l + 3] = J.T @ F + tau_ff[3 * l:3 * l + 3]
            # the same with absolute values: chain segments (and anchor offsets) in the law's axes, summed without cancellation
            S = np.abs(segs @ T.T); O = np.abs(jpos @ T.T); Ax = np.abs(axes @ T.T)
            p_abs = S.sum(0)
            J_abs = np.zeros((3, 3))
            for i in range(3):
                r = S[i + 1:].sum(0) + O[i]
                a = Ax[i]
                J_abs[:, i] = [a[1] * r[2] + a[2] * r[1], a[2] * r[0] + a[0] * r[2], a[0] * r[1] + a[1] * r[0]]
            v_abs = J_abs @ np.abs(qd)
            F_abs = np.abs(f_ff[k]) + np.abs(kp[k]) * (np.abs(p_des[k]) + p_abs) + np.abs(kd[k]) * (np.abs(v_des[k]) + v_abs)
            scale[3 * l:3 * l + 3] = J_abs.T @ F_abs + np.abs(tau_ff[3 * l:3 * l + 3])
        return tau, scale
