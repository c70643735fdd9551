"""fp64 numpy restatement of gq_camera_shaded's shading (include/gq.h), for the RGB camera tests.

The hits come from test_gpu_camera.Caster.  The normal of a hit is found here from the hit point and the geometry (the surface the point
lies on), independently of how the kernel tracks the part of a primitive it entered by; where two surfaces are within a tolerance of the
point (an edge), or the colour changes there (a checker or mark edge, a height-field triangle edge), the pixel is flagged as ambiguous."""
import numpy as np

PART_TOL = 2e-5      # m: a hit this close to another face / part of its primitive has an ambiguous normal
HULL_TOL = 2e-6      # m: ... for a mesh hull's face planes, and only those whose normal differs from the hit's by more than HULL_COS
HULL_COS = 1 - 1e-7  # (scanned hulls carry many small, nearly coplanar facets: their planes pass within microns of a hit)
CHECKER_TOL = 1e-4   # m: ... this close to a checker or mark edge an ambiguous colour
HFIELD_TOL = 1e-5    # m: ... this close to a height-field triangle edge an ambiguous normal


def to_bytes(x):
    return np.floor(255.0 * np.clip(x, 0.0, 1.0) + 0.5).astype(np.int64)


def unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def lights_of(app, Rc):
    """The headlight (world direction of the camera's +z) and the appearance's lights, as dicts in world axes."""
    out = []
    if app.head_active:
        out.append(dict(kind='dir', L=np.asarray(Rc)[:, 2], A=np.asarray(app.head_ambient), D=np.asarray(app.head_diffuse), S=np.asarray(app.head_specular)))
    for lt in app.lights:
        d = unit(np.asarray(lt.dir, np.float64))
        out.append(dict(kind='dir' if lt.directional else 'spot', L=-d, dir=d, pos=np.asarray(lt.pos, np.float64), A=np.asarray(lt.ambient),
                        D=np.asarray(lt.diffuse), S=np.asarray(lt.specular), att=np.asarray(lt.attenuation, np.float64),
                        cos_cut=np.cos(np.deg2rad(lt.cutoff)), expo=float(lt.exponent)))
    return out


def shade(col, mat, n, v, hit, lights):
    """out = emis c + sum_l att spot [A c + D c max(n.L, 0) + (n.L > 0 ? S spec max(n.H, 0)^(128 shin) : 0)], per row; unclamped.
    col [P, 3], mat [P, 3] (specular, shininess, emission), n / v [P, 3] unit (normal, towards the camera), hit [P, 3] world."""
    col, mat, n, v, hit = (np.asarray(a, np.float64).reshape(-1, 3) for a in (col, mat, n, v, hit))
    out = mat[:, 2:3] * col
    for lt in lights:
        if lt['kind'] == 'dir':
            L = np.broadcast_to(lt['L'], n.shape)
            w = np.ones(len(n))
        else:
            q = lt['pos'] - hit
            r = np.linalg.norm(q, axis=1)
            L = q / r[:, None]
            cs = -(L @ lt['dir'])
            with np.errstate(invalid='ignore'):
                spot = np.where(cs >= lt['cos_cut'], np.power(np.maximum(cs, 0.0), lt['expo']), 0.0)
            w = spot / (lt['att'][0] + lt['att'][1] * r + lt['att'][2] * r * r)
        nL = (n * L).sum(1)
        nH = np.maximum((n * unit(L + v)).sum(1), 0.0)
        sp = np.where(nL > 0, mat[:, 0] * np.power(nH, 128.0 * mat[:, 1]), 0.0)
        out = out + w[:, None] * (lt['A'] * col + lt['D'] * col * np.maximum(nL, 0.0)[:, None] + lt['S'] * sp[:, None])
    return out


def background(app, Dw):
    s = 0.5 * (1.0 + unit(Dw)[:, 2])
    bot, top = np.asarray(app.bg_bottom), np.asarray(app.bg_top)
    return bot + (top - bot) * s[:, None]


def checker(app, x, y):
    """(colour [P, 3], ambiguous [P]) of the floor checker at world x / y"""
    sq = app.floor_square
    fx, fy = x / sq, y / sq
    ix, iy = np.floor(fx), np.floor(fy)
    ux, uy = fx - ix, fy - iy
    edge = np.minimum(np.minimum(ux, 1 - ux), np.minimum(uy, 1 - uy)) * sq
    odd = (ix.astype(np.int64) + iy.astype(np.int64)) % 2 == 1
    col = np.where(odd[:, None], np.asarray(app.floor_rgb2), np.asarray(app.floor_rgb1))
    col = np.where((edge < app.floor_mark_w)[:, None], np.asarray(app.floor_mark_rgb), col)
    amb = (edge < CHECKER_TOL) | (np.abs(edge - app.floor_mark_w) < CHECKER_TOL) if app.floor_mark_w > 0 else edge < CHECKER_TOL
    return col, amb


def _second(vals):
    """largest and second-largest of each row"""
    s = np.sort(vals, axis=1)
    return s[:, -1], s[:, -2]


def surface(caster, app, pose, co, Dw, t, seg):
    """Normal (world, unit), base colour, material and ambiguity of every hit (seg >= 0).  t: the oracle's ray parameters."""
    md, ng, nbox = caster.md, caster.ngeom, len(caster.boxes)
    P = len(t)
    hit = co + t[:, None] * Dw
    n, col, mat, amb = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros((P, 3)), np.zeros(P, bool)
    gmat = np.asarray(app.geom_mat, np.float64)
    gx, gm = pose[0], pose[1]
    for g in np.unique(seg[(seg >= 0) & (seg < ng)]):
        sel = seg == g
        p = (hit[sel] - gx[g]) @ gm[g]   # geom frame
        typ, s = int(md.geom_type[g]), md.geom_size[g]
        a = np.zeros(len(p), bool)
        if typ == 2:
            nl = p
        elif typ == 3:
            nl = p - np.stack([0 * p[:, 0], 0 * p[:, 0], np.clip(p[:, 2], -s[1], s[1])], 1)
            a = np.abs(np.abs(p[:, 2]) - s[1]) < PART_TOL
        elif typ == 5:
            ds, dc = np.abs(np.hypot(p[:, 0], p[:, 1]) - s[0]), np.abs(np.abs(p[:, 2]) - s[1])
            cap = dc < ds
            nl = np.where(cap[:, None], np.stack([0 * p[:, 0], 0 * p[:, 0], np.sign(p[:, 2])], 1), np.stack([p[:, 0], p[:, 1], 0 * p[:, 0]], 1))
            a = (ds < PART_TOL) & (dc < PART_TOL)
        elif typ == 6:
            v = np.abs(p) - s
            k = np.argmax(v, 1)
            nl = np.eye(3)[k] * np.sign(p[np.arange(len(p)), k])[:, None]
            a = _second(v)[1] > -PART_TOL
        else:
            cl = int(md.geom_cloudid[g])
            Q = caster.planes[caster.adr[cl]:caster.adr[cl + 1]]
            v = p @ Q[:, :3].T - Q[:, 3]
            k = np.argmax(v, 1)
            nl = Q[k, :3]
            near = v > v[np.arange(len(v)), k][:, None] - HULL_TOL
            a = (near & (nl @ Q[:, :3].T < HULL_COS)).any(1)
        n[sel] = unit(nl) @ gm[g].T
        amb[sel] = a
        col[sel] = gmat[g, :3]
        mat[sel] = gmat[g, 4:7]
    for b, (bx, Rm) in enumerate(zip(caster.boxes, caster.Rb)):
        sel = seg == ng + 1 + b
        if not sel.any():
            continue
        p = (hit[sel] - np.asarray(bx['pos'])) @ Rm
        v = np.abs(p) - np.asarray(bx['size'])
        k = np.argmax(v, 1)
        n[sel] = (np.eye(3)[k] * np.sign(p[np.arange(len(p)), k])[:, None]) @ Rm.T
        amb[sel] = _second(v)[1] > -PART_TOL
        col[sel] = np.asarray(app.box_mat[:3])
        mat[sel] = np.asarray(app.box_mat[4:7])
    ground = (seg == ng) | (seg == ng + 1 + nbox)
    n[seg == ng] = (0.0, 0.0, 1.0)
    sel = seg == ng + 1 + nbox
    if sel.any():
        hf = caster.hf
        data = np.asarray(hf['data'], np.float64) * hf['size'][2]
        sx, sy = hf['size'][0], hf['size'][1]
        pp = np.asarray(hf.get('pos', (0, 0, 0)), np.float64)
        nr, nc = data.shape
        dx, dy = 2 * sx / (nc - 1), 2 * sy / (nr - 1)
        x, y = hit[sel, 0] - pp[0], hit[sel, 1] - pp[1]
        c = np.clip(np.floor((x + sx) / dx).astype(int), 0, nc - 2); r = np.clip(np.floor((y + sy) / dy).astype(int), 0, nr - 2)
        u, w = (x + sx) / dx - c, (y + sy) / dy - r
        upper = u + w > 1
        h00, h10, h01, h11 = data[r, c], data[r, c + 1], data[r + 1, c], data[r + 1, c + 1]
        n0 = np.stack([-(h10 - h00) * dy, -(h01 - h00) * dx, np.full(len(x), dx * dy)], 1)
        n1 = np.stack([(h01 - h11) * dy, (h10 - h11) * dx, np.full(len(x), dx * dy)], 1)
        n[sel] = unit(np.where(upper[:, None], n1, n0))
        tol_u, tol_w = HFIELD_TOL / dx, HFIELD_TOL / dy
        amb[sel] = (np.minimum(u, 1 - u) < tol_u) | (np.minimum(w, 1 - w) < tol_w) | (np.abs(u + w - 1) < tol_u + tol_w)
    if ground.any():
        cc, a = checker(app, hit[ground, 0], hit[ground, 1])
        col[ground] = cc
        amb[ground] |= a
        mat[ground] = (app.floor_specular, app.floor_shininess, app.floor_emission)
    return n, col, mat, amb, hit


def oracle_rgb(caster, app, pose, co, Rc, Dw, znear, zfar):
    """(rgb bytes [P, 3], seg [P], ambiguous [P]) of the rays Dw (world axes, not unit) from co"""
    t, seg = caster.cast(co, Dw, pose, znear, zfar)
    out = background(app, Dw)
    amb = np.zeros(len(t), bool)
    hit = seg >= 0
    if hit.any():
        n, col, mat, a, hp = surface(caster, app, pose, co, Dw[hit], t[hit], seg[hit])
        out[hit] = shade(col, mat, n, -unit(Dw[hit]), hp, lights_of(app, Rc))
        amb[hit] = a
    return to_bytes(out), seg, amb


def seg_band(seg, H, W):
    """the 1-pixel band around a segmentation change: pixels with a 4-neighbour of another id"""
    s = seg.reshape(H, W)
    p = np.pad(s, 1, mode='edge')
    band = np.zeros((H, W), bool)
    for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        band |= p[1 + dr:1 + dr + H, 1 + dc:1 + dc + W] != s
    return band.reshape(-1)


def make_caster(env):
    """test_gpu_camera.Caster (the fp64 hits) with the height-field description surface() reads"""
    from test_gpu_camera import Caster
    c = Caster(env)
    c.hf = env.scene_desc.get('hfield')
    return c
