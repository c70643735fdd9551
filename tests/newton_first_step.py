"""The first Newton step through the product's own kernel, shared by tests/test_kernel_emulated.py (host emulator) and tests/test_gpu_parity.py
(QuadrupedEnv(solver_iterations=1) with enable_debug).  With one iteration allowed, qacc - qacc_smooth is alpha times the kernel's search
direction, so it pins what the whole-step parity tests cannot see - they compare the minimiser, which does not depend on the Hessian: the assembled
Hessian, the middle-zone virtual rows and whichever solve ran (tree-sparse, Sherman-Morrison, dense).  TEST INFRASTRUCTURE.

Per env: the kernel's OWN efc_J, efc_R, efc_aref, qacc_smooth and M (cast to float64: the stages before the solver stay out of the check), the
row types, friction losses and cone parameters of the oracle; g = -J' f(qacc_smooth) and the exact Hessian H = M + J' (d2s/dz2) J in numpy (the
middle-zone block as oracle/gq_oracle.c elliptic_eval documents it); d = qacc - qacc_smooth; alpha = -(g . H d) / (g . g) > 0;
eta = |H d + alpha g|_inf / (|H|_inf |d|_inf + alpha |g|_inf) <= 64 * 2^-24 + 8 eta_ref: at most 64 products are summed per entry of H, and eta_ref
is the largest eta of a float32 numpy Cholesky solve of the same (H, g)."""
from __future__ import annotations

import numpy as np

from helpers import budgeted_states, marshalled, random_states, self_contact_states, tally_note
from step_parity import ParityTally

U24 = 2.0 ** -24
EFC_FRICTION_DOF, EFC_LIMIT_JOINT, EFC_CONTACT_FRICTIONLESS, EFC_CONTACT_PYRAMIDAL, EFC_CONTACT_ELLIPTIC = range(5)   # oracle/gq_oracle.c
NAMES = ['qacc', 'qacc_smooth', 'M', 'nefc', 'ncon', 'efc_J', 'efc_R', 'efc_aref']   # the debug-record fields the check reads


def _elliptic(z, D, mu, fri):
    """cost gradient and Hessian of one elliptic contact at residual z (float64): zone, grad [dim], hess [dim][dim]"""
    dim = len(z)
    U = fri * z[1:]
    T, N = np.sqrt((U * U).sum()), mu * z[0]
    if N >= mu * T or (T <= 0 and N >= 0):
        return 0, np.zeros(dim), np.zeros((dim, dim))
    if mu * N + T <= 0 or (T <= 0 and N < 0):
        return 1, D * z, np.diag(D)
    Dm, q = D[0] / (mu * mu * (1 + mu * mu)), N - mu * T
    u = U / T
    g = np.concatenate([[mu], -mu * fri * u])
    H = Dm * np.outer(g, g)
    H[1:, 1:] += Dm * q * (-mu) * np.outer(fri, fri) * (np.eye(dim - 1) - np.outer(u, u)) / T
    return 2, Dm * q * g, H


def first_step(o, kern):
    """One env, after the oracle has stepped from the same state: dict(eta, eta_ref, alpha, middle, cross, lower) or None when no row is active at
    qacc_smooth (no step to look at).  `cross`: active rows that couple two legs, counted on the float64 side."""
    n = int(kern['nefc'][0])
    J = np.asarray(kern['efc_J'], np.float64).reshape(64, 18)[:n]
    R, aref = np.asarray(kern['efc_R'], np.float64)[:n], np.asarray(kern['efc_aref'], np.float64)[:n]
    qs, qa = np.asarray(kern['qacc_smooth'], np.float64), np.asarray(kern['qacc'], np.float64)
    M = np.asarray(kern['M'], np.float64).reshape(18, 18)
    M = np.tril(M) + np.tril(M, -1).T
    typ, floss = o.get('efc_type').astype(int)[:n], o.get('efc_frictionloss')[:n]
    z, D = J @ qs - aref, 1.0 / R
    s1, W = np.zeros(n), np.zeros((n, n))
    middle = 0
    active = np.zeros(n, bool)
    for i in np.nonzero(typ != EFC_CONTACT_ELLIPTIC)[0]:
        if typ[i] == EFC_FRICTION_DOF:
            if abs(z[i]) < R[i] * floss[i]:   # row_law / row_piece: closed at +-R floss means the border belongs to the LINEAR pieces (y <= -R floss, y >= R floss)
                s1[i], W[i, i] = D[i] * z[i], D[i]
            else:
                s1[i] = np.sign(z[i]) * floss[i]
        elif z[i] < 0:
            s1[i], W[i, i] = D[i] * z[i], D[i]
        active[i] = W[i, i] != 0 and typ[i] != EFC_FRICTION_DOF
    if o.ncon:
        adr, dims = o.get('contact_efc_address').astype(int), o.get('contact_dim').astype(int)
        mus, fr = o.get('contact_mu'), o.get('contact_friction').reshape(-1, 5)
        for c in range(o.ncon):
            a, d = adr[c], dims[c]
            assert a + d <= n, (c, a, d, n)   # an 'ok' env has the oracle's rows: every contact lies within them
            if typ[a] == EFC_CONTACT_ELLIPTIC:
                assert (typ[a:a + d] == EFC_CONTACT_ELLIPTIC).all(), (c, typ[a:a + d])
                zone, g, H = _elliptic(z[a:a + d], D[a:a + d], mus[c], fr[c, :d - 1])
                s1[a:a + d], W[a:a + d, a:a + d] = g, H
                middle += zone == 2
                active[a:a + d] = zone != 0
            else:   # the loop above has taken its rows
                assert typ[a] in (EFC_CONTACT_FRICTIONLESS, EFC_CONTACT_PYRAMIDAL), (c, typ[a])
    g = J.T @ s1
    if not np.abs(g).max() > 0:
        return None
    H = M + J.T @ W @ J
    d = qa - qs
    Hd = H @ d
    alpha = -(g @ Hd) / (g @ g)
    Hn = np.abs(H).sum(1).max()
    eta = np.abs(Hd + alpha * g).max() / (Hn * np.abs(d).max() + abs(alpha) * np.abs(g).max())
    H32, g32 = H.astype(np.float32), g.astype(np.float32)
    L = np.linalg.cholesky(H32)
    x = np.linalg.solve(L.T, np.linalg.solve(L, -g32)).astype(np.float32)
    eta_ref = np.abs(H @ x.astype(np.float64) + g).max() / (Hn * np.abs(x).max() + np.abs(g).max())
    legs = (np.abs(J[:, 6:].reshape(n, 4, 3)).max(2) > 0).sum(1)
    return dict(eta=float(eta), eta_ref=float(eta_ref), alpha=float(alpha), middle=int(middle), cross=int((active & (legs >= 2)).sum()),
                lower=o.primal_cost(qa) < o.primal_cost(o.qacc_smooth))


class FirstStepTally:
    """the per-robot collection: hold() every 'ok' env, finish() asserts the bound and returns the coverage counts"""

    def __init__(self, what, elliptic):
        self.what, self.elliptic, self.res, self.note = what, elliptic, [], None

    def hold(self, e, o, kern):
        r = first_step(o, kern)
        if r is not None:
            r['env'] = e
            self.res.append(r)

    def finish(self):
        assert self.res, self.what
        eta, ref = np.array([r['eta'] for r in self.res]), np.array([r['eta_ref'] for r in self.res])
        bound = 64 * U24 + 8 * ref.max()
        w = int(eta.argmax())
        cov = dict(envs=len(self.res), middle=sum(r['middle'] > 0 for r in self.res), one_cross=sum(r['cross'] == 1 for r in self.res),
                   dense=sum(r['cross'] >= (1 if self.elliptic else 2) for r in self.res))
        self.note = (f'first Newton step {self.what}: {cov["envs"]} envs with a step, max eta {eta.max():.3g} (env {self.res[w]["env"]}), bound {bound:.3g} = 64 * 2^-24 '
                   f'({64 * U24:.3g}) + 8 * float32 Cholesky eta ({ref.max():.3g}); middle-zone envs {cov["middle"]}, one active cross-leg row {cov["one_cross"]}, dense {cov["dense"]}')
        tally_note(self.note)
        bad = [(r['env'], r['alpha']) for r in self.res if not r['alpha'] > 0]
        assert not bad, (self.what, 'alpha <= 0', bad[:8])
        assert eta.max() <= bound, (self.what, 'eta', float(eta.max()), bound, self.res[w])
        up = [r['env'] for r in self.res if not r['lower']]
        assert not up, (self.what, 'the step does not lower the cost', up[:8])
        return cov


# (robot, states): one pyramidal robot, one elliptic robot with condim 3, one with condim 6 on contact-rich floor states; the pyramidal robot and an
# elliptic one on self-contact states, where rows couple two legs
CONFIGS = [('mini_cheetah', 'floor'), ('hyqreal1', 'floor'), ('go1', 'floor'), ('mini_cheetah', 'self'), ('go2', 'self')]
N_ENVS = 64
# Of the 64 envs of a configuration at least half are held: the draws keep the envs over the row budget below 8 % (budgeted_states, max_over), the
# deepest-vertex ties of random states are a few per cent, and an env without an active row at qacc_smooth has no step to look at
MIN_HELD = N_ENVS // 2
FRICTION = 0.8
REPORT_KEY = 'first Newton step'


def merge_report(path, notes):
    """The measured lines of `notes` into the device probe's report: a line replaces the one of the same configuration (the text before the first
    ':'), so a test run alone, or twice, leaves one line per configuration; tests/test_gpu_device_probe.py keeps these lines when it rewrites
    its own."""
    import os
    old = open(path).read().splitlines() if os.path.exists(path) else []
    keys = {n.split(':')[0] for n in notes}
    with open(path, 'w') as fh:
        fh.write('\n'.join([ln for ln in old if ln.split(':')[0] not in keys] + list(notes)) + '\n')


def oracle_for(robot):
    from oracle.oracle import Oracle
    return Oracle(marshalled(robot, solver=1, iterations=100, tolerance=1e-12))


def draw_states(robot, kind, o, n=N_ENVS):
    """(qpos, qvel float32, ctrl float32) of n envs; 'floor': budgeted_states over contact-rich heights, 'self': self_contact_states with a contact
    between two different legs"""
    md = o.mm.md
    cone = md.cone == 1
    hip = float(o.mm.desc.key_qpos[2])
    rng = np.random.default_rng(41 + len(robot) + 7 * (kind == 'self'))
    if kind == 'floor':
        qpos, qvel = budgeted_states(n, lambda k: random_states(md, k, rng, z_range=(0.6 * hip, 1.2 * hip)), o, cone, max_over=0.08)
    else:
        qpos, qvel = self_contact_states(md, n, rng, o, z=(0.7 * hip, 1.3 * hip), want_cross=True, cone=cone, max_over=0.0)
    return qpos, qvel.astype(np.float32), (rng.normal(0, 1, (n, 12)) * 20).astype(np.float32)


def hold_first_step(robot, kind, o, qpos, qvel, ctrl, kern, what, notes=None):
    """Every env that ParityTally.classify calls 'ok' is held to the first-step check; the oracle starts from its own qacc_smooth, where the
    kernel starts.  No row-count mismatch, at least MIN_HELD envs held, and the coverage the configuration is there for.  Returns the coverage counts
    of FirstStepTally.finish(); notes: a list that takes the measured line, passed or failed."""
    cone = o.mm.md.cone == 1
    tally, fs = ParityTally(cone, 3e-7), FirstStepTally(f'{what} {robot} {kind}', cone)
    zero = np.zeros(18)
    for e in range(len(qpos)):
        o.set_state(qpos[e], qvel[e], zero, zero, 0.0, FRICTION)
        o.forward(ctrl[e].astype(np.float64))
        warm = o.qacc_smooth
        o.set_state(qpos[e], qvel[e], warm, zero, 0.0, FRICTION)
        o.step(ctrl[e].astype(np.float64))
        if tally.classify(e, o, int(kern[e]['nefc'][0])) == 'ok':
            fs.hold(e, o, kern[e])
    try:
        cov = fs.finish()
    finally:
        if notes is not None and fs.note:
            notes.append(fs.note)
    tally.finish_count(f'{REPORT_KEY} {what} {robot} {kind}', MIN_HELD)
    assert cov['envs'] >= MIN_HELD, cov
    if kind == 'floor' and cone:
        assert cov['middle'] >= 8, cov
    if kind == 'self':   # pyramidal: one active cross-leg row is the Sherman-Morrison path; two or more, or any on an elliptic robot, the dense path
        assert (cov['dense'] if cone else cov['one_cross']) >= 8, cov
    return cov
