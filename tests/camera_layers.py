"""fp64 numpy restatement of gq_camera_layered's layers (include/gq.h): the marker shapes and the compositor."""
import numpy as np

MAXLAYER = 8


def composite(C0, t0, layers, znear=0.0, maxlayer=MAXLAYER):
    """C0 [3] opaque colour (unclamped), t0 its depth; layers: (t, S [3], a) in layer-index order (ghosts, then markers), t None for no
    hit.  The maxlayer nearest layers with znear <= t < t0 (ties: the higher index is farther), composited far to near."""
    kept = [(t, i, np.asarray(S, np.float64), float(a)) for i, (t, S, a) in enumerate(layers) if t is not None and znear <= t < t0]
    kept.sort(key=lambda x: (x[0], x[1]))
    C = np.asarray(C0, np.float64).copy()
    for t, i, S, a in reversed(kept[:maxlayer]):
        C = a * S + (1.0 - a) * C
    return C


def _basis(u):
    t = np.array([1.0, 0.0, 0.0]) if abs(u[0]) < 0.6 else np.array([0.0, 1.0, 0.0])
    e1 = t - np.dot(t, u) * u
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(u, e1)


def _sphere(o, d, r):
    a, b, c = d @ d, o @ d, o @ o - r * r
    disc = b * b - a * c
    if c <= 0 or disc < 0:
        return None
    return (-b - np.sqrt(disc)) / a


def _interval_cyl(o, d, r, z0, z1):
    """ray interval inside the solid cylinder x^2 + y^2 <= r^2, z0 <= z <= z1"""
    lo, hi = -np.inf, np.inf
    if abs(d[2]) < 1e-300:
        if not z0 <= o[2] <= z1:
            return None
    else:
        a0, a1 = sorted(((z0 - o[2]) / d[2], (z1 - o[2]) / d[2]))
        lo, hi = a0, a1
    a, b, c = d[0] ** 2 + d[1] ** 2, o[0] * d[0] + o[1] * d[1], o[0] ** 2 + o[1] ** 2 - r * r
    if a < 1e-300:
        if c > 0:
            return None
    else:
        disc = b * b - a * c
        if disc < 0:
            return None
        s = np.sqrt(disc)
        lo, hi = max(lo, (-b - s) / a), min(hi, (-b + s) / a)
    return (lo, hi) if lo <= hi else None


def _interval_cone(o, d, rb, zb, zt, n=4000):
    """ray interval inside the solid cone (base radius rb at zb, apex zt), by the convex set's support along the ray: the roots of
    f(t) = x^2 + y^2 - k^2 (zt - z)^2 within the slab, found in fp64 closed form"""
    k2 = (rb / (zt - zb)) ** 2
    lo, hi = -np.inf, np.inf
    if abs(d[2]) < 1e-300:
        if not zb <= o[2] <= zt:
            return None
    else:
        lo, hi = sorted(((zb - o[2]) / d[2], (zt - o[2]) / d[2]))
    hz = zt - o[2]
    a = d[0] ** 2 + d[1] ** 2 - k2 * d[2] ** 2
    b = o[0] * d[0] + o[1] * d[1] + k2 * hz * d[2]
    c = o[0] ** 2 + o[1] ** 2 - k2 * hz * hz
    disc = b * b - a * c
    if abs(a) < 1e-14:
        if abs(b) < 1e-300:
            return (lo, hi) if c <= 0 else None
        r = -0.5 * c / b
        lo, hi = (lo, min(hi, r)) if b > 0 else (max(lo, r), hi)
    elif disc < 0:
        if a > 0:
            return None
    else:
        q0, q1 = sorted(((-b - np.sqrt(disc)) / a, (-b + np.sqrt(disc)) / a))
        if a > 0:
            lo, hi = max(lo, q0), min(hi, q1)
        elif lo <= q0:
            hi = min(hi, q0)
        else:
            lo = max(lo, q1)
    return (lo, hi) if lo <= hi else None


def marker_hit(row, co, dw):
    """(t, unit outward normal [3] world) of one marker row for the ray co + t dw (world), or (None, None)."""
    typ = int(row[0])
    p, ax, size = np.asarray(row[1:4], np.float64), np.asarray(row[4:7], np.float64), np.asarray(row[7:10], np.float64)
    L = np.linalg.norm(ax)
    if typ == 1:
        o = co - p
        t = _sphere(o, dw, size[0])
        return (None, None) if t is None else (t, (o + t * dw) / np.linalg.norm(o + t * dw))
    if typ not in (2, 3) or L == 0:
        return None, None
    u = ax / L
    e1, e2 = _basis(u)
    B = np.stack([e1, e2, u], 1)
    o, d = (co - p) @ B, dw @ B
    best, nl = None, None

    def take(iv, normal_fn):
        nonlocal best, nl
        if iv is not None and iv[0] > 0 and (best is None or iv[0] < best):
            best, nl = iv[0], normal_fn(o + iv[0] * d)
    if typ == 2:
        r = size[0]
        if np.linalg.norm(o - np.clip(o[2], 0, L) * np.array([0, 0, 1.0])) <= r:
            return None, None
        take(_interval_cyl(o, d, r, 0.0, L), lambda q: np.array([q[0], q[1], 0.0]))
        for zc in (0.0, L):
            t = _sphere(o - [0, 0, zc], d, r)
            if t is not None:
                take((t, t), lambda q, zc=zc: q - [0, 0, zc])
    else:
        zb = (1 - size[2]) * L
        k2 = (size[1] / (L - zb)) ** 2
        take(_interval_cyl(o, d, size[0], 0.0, zb), lambda q: np.array([q[0], q[1], 0.0]) if abs(np.hypot(q[0], q[1]) - size[0]) <
             min(abs(q[2]), abs(q[2] - zb)) else np.array([0, 0, np.sign(q[2] - zb / 2)]))
        take(_interval_cone(o, d, size[1], zb, L), lambda q: np.array([q[0], q[1], k2 * (L - q[2])]) if abs(q[2] - zb) > 1e-9 * max(L, 1)
             else np.array([0, 0, -1.0]))
    if best is None:
        return None, None
    n = B @ nl
    return best, n / np.linalg.norm(n)
